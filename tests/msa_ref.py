"""Test infrastructure of the per-instance rows (--msa): the edlib path of a (block, template) pair
(profile_ref.edlib_path), folded into the pair's own row in Python, from the layout in include/sd_hip.h:

  row of a pair (segment, interleaved template il), forward monomer il >> 1 of length L, (2 L + 1 + 15) & ~15 bytes
    [0, L)       per FORWARD position: 0..4 the read base aligned there (A C G T N), 5 deleted, 7 no instance
    [L, 2L + 1)  per insertion slot 0..L: the read bases inserted before that position, saturating at 255
    padding 0
  a pair against rc(m): position p lands at L-1-p, slot h at L-h, the base complemented
  status 0 = an empty side, 1 = computed"""
import numpy as np

import edlib_ref
import profile_ref
from stringdecomposer_amd import formats

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
DEL, NONE = 5, 7


def pitch(L):
    return (2 * L + 1 + 15) & ~15


def _fast_path(q, t):
    """profile_ref._matrix_path with the rows of the matrix computed by numpy (the same matrix, the same walk)."""
    n, m = len(q), len(t)
    qa = np.frombuffer(q.encode("latin-1"), dtype=np.uint8)
    ta = np.frombuffer(t.encode("latin-1"), dtype=np.uint8)
    D = np.zeros((n + 1, m + 1), dtype=np.int64)
    D[0, :] = np.arange(m + 1)
    ar = np.arange(m + 1)
    for i in range(1, n + 1):
        row = np.empty(m + 1, dtype=np.int64)
        row[0] = i
        row[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (ta != qa[i - 1]))
        D[i] = np.minimum.accumulate(row - ar) + ar    # the left neighbour: D[i, j] = min over k <= j of row[k] + (j - k)
    ops, i, j = [], n, m
    while i > 0 or j > 0:
        if i > 0 and D[i - 1, j] + 1 == D[i, j]:
            ops.append(1)
            i -= 1
        elif j > 0 and D[i, j - 1] + 1 == D[i, j]:
            ops.append(2)
            j -= 1
        else:
            ops.append(0 if D[i - 1, j - 1] == D[i, j] else 3)
            i -= 1
            j -= 1
    return ops[::-1]


def path(q, t):
    if edlib_ref.have_edlib():
        return profile_ref.edlib_path(q, t)
    assert 20 * ((len(q) + 63) // 64) * len(t) + 8 * len(t) < 1 << 20, "a Hirschberg pair needs the reference edlib"
    return _fast_path(q, t)


def row(q, mono, is_rc):
    """(bytes of the row, status) of block q against mono (forward), or against its reverse complement."""
    L = len(mono)
    out = np.zeros(pitch(L), dtype=np.uint8)
    out[:L] = NONE
    if not q or not mono:
        return out, 0
    ops = path(q, profile_ref.rc(mono) if is_rc else mono)
    i = j = 0
    for op in ops:
        if op == 2:
            out[L - 1 - j if is_rc else j] = DEL
            j += 1
            continue
        b = CODE.get(q[i], 4)
        i += 1
        if is_rc and b < 4:
            b = 3 - b
        if op == 1:
            g = L + (L - j if is_rc else j)
            out[g] = min(int(out[g]) + 1, 255)
        else:
            out[L - 1 - j if is_rc else j] = b
            j += 1
    return out, 1


def segments(seq, starts, ends, monos, pair_tmpl):
    """The Python form of sd_msa_segments: (rows, row_at, status)."""
    rows, at, status = [], [0], []
    for s, e, p in zip(starts, ends, pair_tmpl):
        r, st = row(seq[s:e + 1], monos[p >> 1], bool(p & 1))
        rows.append(r)
        at.append(at[-1] + len(r))
        status.append(st)
    return (np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint8), np.asarray(at, dtype=np.int64),
            np.asarray(status, dtype=np.uint8))


def same(msa, ref):
    rows, at, status = ref
    assert (np.asarray(msa.row_at) == at).all()
    assert (np.asarray(msa.status) == status).all()
    assert msa.rows.shape == rows.shape
    bad = np.nonzero(msa.rows != rows)[0]
    assert bad.size == 0, "first differing byte at %d (pair %d)" % (bad[0], np.searchsorted(at, bad[0], side="right") - 1)


def final_rows_of_tsv(final_tsv, read_names, mono_names, final_dtype):
    """The rows of a final_decomposition.tsv as the structured array of a FinalRows (read, start, end, best; keys =
    the interleaved names m0, m0', m1, ...) -> ((rows, row_off, None), keys)."""
    keys = [x for n in mono_names for x in (n, n + "'")]
    kidx = {k: i for i, k in enumerate(keys)}
    ridx = {n: i for i, n in enumerate(read_names)}
    fin = formats.read_final(final_tsv)
    rows = np.zeros(len(fin), dtype=final_dtype)
    for i, r in enumerate(fin):
        rows[i]["read"], rows[i]["start"], rows[i]["end"], rows[i]["best"] = ridx[r.read], r.start, r.end, kidx[r.monomer]
    off = np.searchsorted(rows["read"], np.arange(len(read_names) + 1))
    return (rows, off.astype(np.int64), None), keys


def of_final(final_tsv, reads, names, seqs):
    """The Python rows over the lines of a final_decomposition.tsv: reads = {name: upper-case sequence}."""
    idx = {n: i for i, n in enumerate(names)}
    rows, at, status = [], [0], []
    for r in formats.read_final(final_tsv):
        is_rc = r.monomer.endswith("'")
        m = idx[r.monomer[:-1] if is_rc else r.monomer]
        x, st = row(reads[r.read][max(r.start, 0):r.end + 1], seqs[m], is_rc)
        rows.append(x)
        at.append(at[-1] + len(x))
        status.append(st)
    return np.concatenate(rows), np.asarray(at, dtype=np.int64), np.asarray(status, dtype=np.uint8)
