"""Test infrastructure of the column profiles (--profile): the edlib path of a (block, template) pair, as
edlib.align(query=block, target=template, mode="NW", task="path") returns it, folded into its forward monomer in
Python.  The path comes from the reference's vendored edlib (oracle/_ref/libedlib.so) when present, else from a
full-matrix walk with edlib's priorities (up > left > diagonal) -- the same path for pairs edlib aligns by its block
traceback, i.e. every pair below Hirschberg's split."""
import numpy as np

import edlib_ref
from stringdecomposer_amd import formats

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _matrix_path(q, t):
    n, m = len(q), len(t)
    D = np.zeros((n + 1, m + 1), dtype=np.int32)
    D[:, 0] = np.arange(n + 1)
    D[0, :] = np.arange(m + 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i, j] = min(D[i - 1, j] + 1, D[i, j - 1] + 1, D[i - 1, j - 1] + (q[i - 1] != t[j - 1]))
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


def edlib_path(q, t):
    """edlib's alignment[] of (query q, target t): 0 '=', 1 query base only (insertion), 2 target base only (del), 3 'X'."""
    if edlib_ref.have_edlib():
        ed = edlib_ref._edlib()
        r = ed.edlibAlign(q.encode(), len(q), t.encode(), len(t), edlib_ref._Cfg(-1, 0, 2, None, 0))
        ops = list(bytes(r.alignment[:r.alignmentLength]))
        ed.edlibFreeAlignResult(r)
        return ops
    assert 20 * ((len(q) + 63) // 64) * len(t) + 8 * len(t) < 1 << 20, "a Hirschberg pair needs the reference edlib"
    return _matrix_path(q, t)


def fold(ops, q, L, rc, c):
    """Adds one instance (path ops of block q against the monomer, or against its reverse complement when rc) to c
    ([L + 1, 12] counters of the forward monomer)."""
    i = j = 0
    last = -1
    for op in ops:
        if op == 2:
            c[L - 1 - j if rc else j, 5] += 1
            j += 1
            continue
        b = CODE.get(q[i], 4)
        i += 1
        if rc and b < 4:
            b = 3 - b
        if op == 1:
            g = L - j if rc else j
            if g != last:
                c[g, 6] += 1
                last = g
            c[g, 7 + b] += 1
        else:
            c[L - 1 - j if rc else j, b] += 1
            j += 1


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def profile_segments(seq, starts, ends, monos, pair_tmpl):
    """The Python fold of sd_profile_segments: a list of [L + 1, 12] int64 arrays."""
    out = [np.zeros((len(m) + 1, formats.PROFILE_NCOLS), dtype=np.int64) for m in monos]
    for s, e, p in zip(starts, ends, pair_tmpl):
        q = seq[s:e + 1]
        m = monos[p >> 1]
        if not q or not m:
            continue
        t = rc(m) if p & 1 else m
        fold(edlib_path(q, t), q, len(m), bool(p & 1), out[p >> 1])
    return out


def profile_of_final(final_tsv, reads, names, seqs):
    """The Python fold over the rows of a final_decomposition.tsv: reads = {name: upper-case sequence}."""
    out = [np.zeros((len(m) + 1, formats.PROFILE_NCOLS), dtype=np.int64) for m in seqs]
    idx = {n: i for i, n in enumerate(names)}
    for row in formats.read_final(final_tsv):
        r = row.monomer[:-1] if row.monomer.endswith("'") else row.monomer
        m = idx[r]
        q = reads[row.read][row.start:row.end + 1]
        is_rc = row.monomer.endswith("'")
        if not q:
            continue
        fold(edlib_path(q, rc(seqs[m]) if is_rc else seqs[m]), q, len(seqs[m]), is_rc, out[m])
    return out
