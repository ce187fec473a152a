"""Synthetic jobs and value sets of the text-format tests (test_text_format_cpu.py, test_gpu_text_format.py): final rows
with their alt identities and raw rows built on the host, and the Python yardstick -- formats.format_final / format_alt /
format_raw with Python's own "{:.2f}".format, a formulation independent of the integer algorithm under test."""
import numpy as np

from stringdecomposer_amd import formats, lib

SPECIAL = [-1.0, 0.0, -0.0, 100.0, 0.125, 0.375, 0.625, 2.5, 2.675, 0.005, 0.015, 99.995, 1e-300, 5e-324, 1099511627775.994]
INTS = [0, -1, 9, 10, 99, 100, 2**31 - 1, -2**31, 2**63 - 1, -2**63]
INTS32 = [0, -1, 9, 10, 99, 100, 2**31 - 1, -2**31]

_cache = {}


def identity_values():
    """Every final_ident_percent(matches, dist) for 0..400 (the arithmetic of sd_final_dev.hpp: a = 0.0; a += m; a /= d + m;
    a * 100), the special values, 300 000 random bit patterns below 2^40 of both signs, and k / 800, k / 200 (binary-exact
    ties and decimal near-ties)."""
    if "values" not in _cache:
        m, d = np.meshgrid(np.arange(401, dtype=np.float64), np.arange(401, dtype=np.float64), indexing="ij")
        keep = (m + d) > 0
        a = np.zeros_like(m) + m
        with np.errstate(invalid="ignore", divide="ignore"):
            a = a / (d + m)
        ident = (a * 100)[keep]
        rng = np.random.default_rng(20240607)
        bits = (rng.integers(0, 2**52, 300000, dtype=np.uint64) | (rng.integers(0, 1023 + 40, 300000, dtype=np.uint64) << np.uint64(52))
                | (rng.integers(0, 2, 300000, dtype=np.uint64) << np.uint64(63)))
        k = np.arange(200000, dtype=np.float64)
        _cache["values"] = np.concatenate([ident, np.array(SPECIAL), bits.view(np.float64), k / 800.0, k / 200.0])
    return _cache["values"]


def final_array(n):
    return np.zeros(n, dtype=lib.final_dtype())


def rows_of_values(vals):
    """vals packed four to a final row of one read and one key -> (FinalRows without alt, read names, keys)"""
    v = np.concatenate([vals, np.zeros((-len(vals)) % 4)]).reshape(-1, 4)
    r = final_array(len(v))
    r["second"], r["homo_best"], r["homo_second"] = -1, -1, -1
    r["ident"], r["second_ident"], r["homo_ident"], r["homo_second_ident"] = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    return lib.FinalRows(r, np.array([0, len(r)], dtype=np.int64), None), ["r"], ["k"]


def read_names(long_name=True):
    """eight reads, their names of the lengths where a 16-byte store begins and ends, one longer than any staging tile"""
    lens = [1, 15, 16, 17, 300, 70000 if long_name else 70, 5, 33]
    return ["".join(chr(97 + (i + j) % 26) for j in range(n)) for i, n in enumerate(lens)]


def row_offsets(n_rows):
    """n_rows over eight reads: none at the front (read 0), in the middle (3) and at the end (7); the long-named read 5
    owns one row as soon as there are two"""
    share = [0] * 8
    left = n_rows
    if n_rows >= 2:
        share[5], left = 1, n_rows - 1
    for x, r in enumerate((1, 2, 4, 6)):
        share[r] = left // 4 + (1 if x < left % 4 else 0)
    return np.concatenate([[0], np.cumsum(share)]).astype(np.int64)


def key_names(n_keys):
    return [("m%d" % (k // 2)) + ("'" if k % 2 else "") + "x" * (k % 19) for k in range(n_keys)]


def final_job(n_rows, n_keys, second_best=True, seed=1, long_name=True):
    """(FinalRows, read names, keys): identities drawn from identity_values(), int64 extremes in start / end, -1 keys, best
    at the first and the last key"""
    rng = np.random.default_rng(seed * 1000 + n_rows * 7 + n_keys)
    vals = identity_values()
    off = row_offsets(n_rows)
    r = final_array(n_rows)
    r["read"] = np.repeat(np.arange(8), np.diff(off))
    ints = np.array(INTS + [12345, 678], dtype=np.int64)
    r["start"] = ints[rng.integers(0, len(ints), n_rows)]
    r["end"] = ints[rng.integers(0, len(ints), n_rows)]
    r["best"] = rng.integers(0, n_keys, n_rows)
    r["best"][0::3] = 0
    r["best"][1::3] = n_keys - 1
    for f in ("second", "homo_best", "homo_second"):
        r[f] = rng.integers(-1, n_keys, n_rows)
    r["second"][::4] = -1
    r["homo_second"][1::4] = -1
    for f in ("ident", "second_ident", "homo_ident", "homo_second_ident"):
        r[f] = vals[rng.integers(0, len(vals), n_rows)]
    r["reliable"] = rng.integers(0, 2, n_rows)
    alt = vals[rng.integers(0, len(vals), n_rows * n_keys)].reshape(n_rows, n_keys) if second_best else None
    return lib.FinalRows(r, off, alt), read_names(long_name), key_names(n_keys)


def raw_job(n_rows, n_tmpl, seed=1, long_name=True):
    """(rows [n, 4] int32, row_off, read names, template names)"""
    rng = np.random.default_rng(seed * 1000 + n_rows * 11 + n_tmpl)
    ints = np.array(INTS32 + [4321, 171], dtype=np.int64)
    rows = np.zeros((n_rows, 4), dtype=np.int32)
    rows[:, 0] = rng.integers(0, n_tmpl, n_rows)
    for c in (1, 2, 3):
        rows[:, c] = ints[rng.integers(0, len(ints), n_rows)]
    return rows, row_offsets(n_rows), read_names(long_name), key_names(n_tmpl)


def python_final(job):
    """(final text, alt text or None) by the pure-Python formatters"""
    fr, names, keys = job
    fin, alt = formats.final_rows(fr, names, keys)
    return formats.format_final(fin).encode(), (None if fr.alt is None else formats.format_alt(alt).encode())


def python_raw(job):
    rows, off, names, tn = job
    out = []
    for r, name in enumerate(names):
        out.extend(formats.raw_rows(name, [(tn[t], s, e, sc) for t, s, e, sc in rows[off[r]:off[r + 1]].tolist()]))
    return formats.format_raw(out).encode()


def python_positions(text, row_off, lines_per_row=1):
    """row_pos / read_pos of a text from its line ends"""
    ends = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1
    starts = np.concatenate([[0], ends]).astype(np.int64)
    row_pos = starts[::lines_per_row] if lines_per_row else starts[:1]
    return row_pos, row_pos[np.asarray(row_off)]
