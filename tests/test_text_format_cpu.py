"""The host twin of the device text formatter (lib.format_final_host / format_raw_host: csrc/sd_text_dev.hpp compiled for
the host) against the pure-Python formatters of formats.py, whose "{:.2f}".format is a formulation independent of the
integer algorithm, and against the committed goldens.  Every comparison is of bytes."""
import gzip
import os
import re

import numpy as np
import pytest

import text_format_cases as tc
from conftest import GOLDEN, ROOT, load_case

from stringdecomposer_amd import formats, lib

FINAL = os.path.join(GOLDEN, "final")
NEW = ["sd_text_tables_create", "sd_text_tables_destroy", "sd_text_final_size_dev", "sd_text_final_write_dev",
       "sd_text_raw_size_dev", "sd_text_raw_write_dev", "sd_text_final_host", "sd_text_raw_host"]


def test_symbols_exported_declared_and_listed():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in lib.EXPORTS and name in declared and hasattr(L, name), name


def test_identities_equal_pythons_format():
    """860 815 values, four to a row: the table of final_ident_percent, the special values, random bit patterns below
    2^40, k / 800 and k / 200"""
    vals = tc.identity_values()
    assert len(vals) == 401 * 401 - 1 + len(tc.SPECIAL) + 700000
    job = tc.rows_of_values(vals)
    got, alt = lib.format_final_host(*job, threads=4)
    assert alt is None
    f2 = "{:.2f}".format
    want = "".join("r\tk\t0\t0\t%s\tNone\t%s\tNone\t%s\tNone\t%s\t?\n" % (f2(a), f2(b), f2(c), f2(d))
                   for a, b, c, d in np.concatenate([vals, np.zeros((-len(vals)) % 4)]).reshape(-1, 4).tolist()).encode()
    if got != want:   # (name the first value that differs)
        g, w = got.split(b"\n"), want.split(b"\n")
        i = next(i for i in range(len(w)) if g[i] != w[i])
        raise AssertionError("row %d: %r, Python: %r" % (i, g[i], w[i]))
    sample = lib.FinalRows(job[0].rows[:5000], np.array([0, 5000]), None)
    assert got.startswith(tc.python_final((sample, job[1], job[2]))[0])      # (the yardstick's own row layout)


def test_unprintable_identities_take_snprintf_on_the_host():
    vals = [float("inf"), float("-inf"), float("nan"), 2.0**40, -(2.0**40), 1e300, 99.5]
    fr, names, keys = tc.rows_of_values(np.array(vals))
    alt = np.array(vals[:len(fr.rows)], dtype=np.float64).reshape(len(fr.rows), 1)
    got, got_alt = lib.format_final_host(lib.FinalRows(fr.rows, fr.row_off, alt), names, keys)
    want = "".join("r\tk\t0\t0\t%s\tNone\t%s\tNone\t%s\tNone\t%s\t?\n" % tuple("%.2f" % v for v in (vals + [0.0])[4 * i:4 * i + 4])
                   for i in range(2))
    assert got == want.encode()
    assert got_alt == "".join("r\tk\t0\t0\t%s\t*\n" % ("%.2f" % v) for v in vals[:2]).encode()


def test_integers_over_the_whole_range():
    r = tc.final_array(len(tc.INTS) ** 2)
    r["start"] = np.repeat(np.array(tc.INTS, dtype=np.int64), len(tc.INTS))
    r["end"] = np.tile(np.array(tc.INTS, dtype=np.int64), len(tc.INTS))
    job = (lib.FinalRows(r, np.array([0, len(r)], dtype=np.int64), np.zeros((len(r), 1))), ["r"], ["k"])
    assert lib.format_final_host(*job) == tc.python_final(job)
    n = len(tc.INTS32)
    rows = np.zeros((n * n, 4), dtype=np.int32)
    rows[:, 1] = np.repeat(np.array(tc.INTS32, dtype=np.int64), n)      # start - previous end and end - start reach +-(2^32 - 1)
    rows[:, 2] = np.tile(np.array(tc.INTS32, dtype=np.int64), n)
    rows[:, 3] = rows[::-1, 1]
    job = (rows, np.array([0, 5, len(rows)], dtype=np.int64), ["r", "s"], ["t"])
    got = lib.format_raw_host(*job)
    assert got == tc.python_raw(job)
    assert b"\t4294967295\n" in got and b"\t-4294967295\n" in got and b"\t-2147483648.000000\t" in got


@pytest.mark.parametrize("n_keys", [1, 2, 24, 260])
@pytest.mark.parametrize("second_best", [False, True])
def test_shapes_equal_the_python_formatters(n_keys, second_best):
    """names of 1 .. 70 000 bytes, reads without rows at the front, in the middle and at the end, key -1, best at the first
    and the last key; the positions are the line starts; four threads give the bytes of one"""
    job = tc.final_job(41, n_keys, second_best)
    fr = job[0]
    assert -1 in fr.rows["second"] and 0 in fr.rows["best"] and n_keys - 1 in fr.rows["best"]
    assert fr.row_off[1] == 0 and fr.row_off[3] == fr.row_off[4] and fr.row_off[7] == fr.row_off[8]
    want = tc.python_final(job)
    (ft, row_pos, read_pos), alt = lib.format_final_host(*job, positions=True)
    assert ft == want[0]
    wp = tc.python_positions(ft, fr.row_off)
    assert np.array_equal(row_pos, wp[0]) and np.array_equal(read_pos, wp[1])
    if second_best:
        assert alt[0] == want[1]
        wp = tc.python_positions(alt[0], fr.row_off, n_keys)
        assert np.array_equal(alt[1], wp[0]) and np.array_equal(alt[2], wp[1])
    else:
        assert alt is None and want[1] is None
    assert lib.format_final_host(*job, threads=4) == want


@pytest.mark.parametrize("n_tmpl", [1, 24])
def test_raw_shapes_equal_the_python_formatter(n_tmpl):
    job = tc.raw_job(41, n_tmpl)
    want = tc.python_raw(job)
    text, row_pos, read_pos = lib.format_raw_host(*job, positions=True)
    assert text == want
    wp = tc.python_positions(text, job[1])
    assert np.array_equal(row_pos, wp[0]) and np.array_equal(read_pos, wp[1])
    assert lib.format_raw_host(*job, threads=4) == want
    structured = np.ascontiguousarray(job[0]).view(lib._rec_dtype()).reshape(-1)
    assert lib.format_raw_host(structured, *job[1:]) == want


def test_no_reads_and_no_rows():
    none = lib.FinalRows(tc.final_array(0), np.zeros(1, dtype=np.int64), np.zeros((0, 3)))
    assert lib.format_final_host(none, [], ["a", "b", "c"]) == (b"", b"")
    assert lib.format_final_host(lib.FinalRows(none.rows, none.row_off, None), [], ["a"]) == (b"", None)
    job = tc.final_job(0, 3)
    (ft, row_pos, read_pos), (at, alt_pos, alt_read_pos) = lib.format_final_host(*job, positions=True)
    assert ft == b"" and at == b"" and row_pos.tolist() == [0] == alt_pos.tolist()
    assert read_pos.tolist() == [0] * 9 == alt_read_pos.tolist()
    assert lib.format_raw_host(np.zeros((0, 4), dtype=np.int32), [0], [], ["t"]) == b""
    assert lib.format_raw_host(*tc.raw_job(0, 2)) == b""
    assert lib.format_raw_host(*tc.raw_job(1, 2)) == tc.python_raw(tc.raw_job(1, 2))


def _refused(call, *a, **kw):
    with pytest.raises(lib.SdError) as e:
        call(*a, **kw)
    assert e.value.code == lib.SD_ERR_PARAM, e.value


def test_bad_arguments_are_refused():
    fr, names, keys = tc.final_job(20, 4, long_name=False)
    for field, value in (("read", 8), ("read", -1), ("best", 4), ("best", -1), ("second", 4), ("homo_best", -2), ("homo_second", 4)):
        rows = fr.rows.copy()
        rows[field][7] = value
        _refused(lib.format_final_host, lib.FinalRows(rows, fr.row_off, fr.alt), names, keys)
    rows = fr.rows.copy()
    rows["read"][7] = 1 if rows["read"][7] != 1 else 2      # a read of the table that does not own the row
    _refused(lib.format_final_host, lib.FinalRows(rows, fr.row_off, fr.alt), names, keys)
    for r, value in ((0, 1), (8, 19), (2, fr.row_off[3] + 1)):    # not from 0, not to n_rows, falling
        off = fr.row_off.copy()
        off[r] = value
        _refused(lib.format_final_host, lib.FinalRows(fr.rows, off, fr.alt), names, keys)
    L = lib.load()                                            # n_keys that is not the table's size: the C entry itself
    t = lib.TextTables(names, keys)
    try:
        import ctypes as C
        err = C.create_string_buffer(256)
        ft, fb = C.c_void_p(), C.c_int64()
        rc = L.sd_text_final_host(t.h, fr.rows.ctypes.data, len(fr.rows), fr.row_off.ctypes.data, None, 3, 1, C.byref(ft),
                                  C.byref(fb), None, None, None, None, None, None, err, 256)
        assert rc == lib.SD_ERR_PARAM and b"n_keys" in err.value and not ft.value
    finally:
        t.close()
    rows, off, rn, tn = tc.raw_job(20, 4, long_name=False)
    for value in (4, -1):
        bad = rows.copy()
        bad[3, 0] = value
        _refused(lib.format_raw_host, bad, off, rn, tn)
    bad = off.copy()
    bad[4] = bad[5] + 1
    _refused(lib.format_raw_host, rows, bad, rn, tn)


def test_device_calls_without_a_device():
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    import ctypes as C
    L = lib.load()
    t = lib.TextTables(["r"], ["k"])
    try:
        err = C.create_string_buffer(256)
        n = C.c_int64()
        p = C.c_void_p(8)
        assert L.sd_text_final_size_dev(t.h, p, 1, p, None, 1, 0, None, p, None, p, None, C.byref(n), C.byref(n), err, 256) == lib.SD_ERR_NO_DEVICE
        assert L.sd_text_final_write_dev(t.h, p, 1, None, 1, 0, None, p, None, p, 8, None, 0, err, 256) == lib.SD_ERR_NO_DEVICE
        assert L.sd_text_raw_size_dev(t.h, p, 1, p, 0, None, p, p, p, C.byref(n), err, 256) == lib.SD_ERR_NO_DEVICE
        assert L.sd_text_raw_write_dev(t.h, p, 1, p, 0, None, p, p, p, 8, err, 256) == lib.SD_ERR_NO_DEVICE
    finally:
        t.close()


# ---- the committed goldens through the host twin -------------------------------------------------------------------

def _rows_from_text(fin, alt):
    """parsed FinalRow / AltRow lists -> (FinalRows, read names, keys)"""
    names = []
    for r in fin:
        if not names or names[-1] != r.read:
            names.append(r.read)
    if alt:
        n_keys = len(alt) // len(fin)
        keys = [a.monomer for a in alt[:n_keys]]
        assert len(alt) == n_keys * len(fin) and len(set(keys)) == n_keys
    else:
        keys = sorted({x for r in fin for x in (r.monomer, r.second_best, r.homo_best, r.homo_second_best)} - {"None"})
    idx = {k: i for i, k in enumerate(keys)}
    idx["None"] = -1
    rows = tc.final_array(len(fin))
    off = np.zeros(len(names) + 1, dtype=np.int64)
    for i, r in enumerate(fin):
        rows[i] = (names.index(r.read), r.start, r.end, idx[r.monomer], idx[r.second_best], idx[r.homo_best], idx[r.homo_second_best],
                   r.identity, r.second_best_identity, r.homo_best_identity, r.homo_second_best_identity, r.reliability == "+")
        off[names.index(r.read) + 1:] = i + 1
    a = np.array([x.identity for x in alt], dtype=np.float64).reshape(len(fin), len(keys)) if alt else None
    return lib.FinalRows(rows, off, a), names, keys


@pytest.mark.parametrize("name", sorted(os.listdir(FINAL)))
def test_final_goldens_through_the_host_twin(name):
    with open(os.path.join(FINAL, name, "final.tsv"), "rb") as f:
        final = f.read()
    gz = os.path.join(FINAL, name, "alt.tsv.gz")
    alt = None
    if os.path.exists(gz):
        with gzip.open(gz, "rb") as f:
            alt = f.read()
    job = _rows_from_text(formats.parse_final(final.decode()), formats.parse_alt(alt.decode()) if alt else None)
    got = lib.format_final_host(*job, threads=2)
    assert got[0] == final
    assert got[1] == alt                    # (None without the file)
    if alt:
        best = [a.monomer for a in formats.parse_alt(got[1].decode()) if a.best]
        assert best == [r.monomer for r in formats.parse_final(final.decode())]


@pytest.mark.parametrize("name", ["td_default", "syn12_ties", "syn64_10kb"])
def test_raw_goldens_through_the_host_twin(name):
    c = load_case(name)
    parsed = formats.parse_raw(c["raw"].decode())
    mn, _, _ = lib.fasta_load(c["monomers"])
    tn = [n.split()[0] for n in mn]
    tn = tn + [n + "'" for n in tn]
    reads = formats.by_read(parsed)
    rows = np.array([(tn.index(r.monomer), r.start, r.end, int(r.score)) for r in parsed], dtype=np.int32).reshape(-1, 4)
    off = np.concatenate([[0], np.cumsum([len(rr) for _, rr in reads])]).astype(np.int64)
    assert lib.format_raw_host(rows, off, [n for n, _ in reads], tn, threads=2) == c["raw"]
