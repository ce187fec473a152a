"""Fixtures of the screen tests (tests/test_screen_cpu.py, tests/test_gpu_screen.py): the Python restatement of the
contract (key of a chunk, regions of a threshold), the kernel cases -- one per instantiation the launch selection can
take -- and the FASTA of the file-job tests.  Everything is a pure function of fixed seeds (synth.Stream is
counter-based and version-stable); references are computed once per process and shared."""
import functools

import numpy as np

import prefilter_cases as pc
from oracle import binding as oracle
from stringdecomposer_amd import synth

PART, OVERLAP = 600, 100          # the kernel cases
F_PART, F_OVERLAP, F_THR = 2000, 200, 40   # the file job


def keys_of(dist):
    """Rule 1: key[c] = (min_j dist(j, c)) << 16 | the smallest j that attains the minimum."""
    d = np.asarray(dist, dtype=np.int64)
    return ((d.min(axis=1) << 16) | d.argmin(axis=1)).astype(np.uint32)   # (argmin: the first minimum)


def regions_of(keys, chunk_read, read_lens, thr, part, overlap):
    """Rules 2 and 3, restated: [(read, start, end_incl, n_chunks, best_key)] in read order, then position order."""
    out = []
    keys = [int(k) for k in keys]
    for r, n in enumerate(read_lens):
        cs = [c for c in range(len(keys)) if chunk_read[c] == r]     # chunk k of the read starts at k * part
        k = 0
        while k < len(cs):
            if keys[cs[k]] >> 16 > thr:
                k += 1
                continue
            a = k
            while k + 1 < len(cs) and keys[cs[k + 1]] >> 16 <= thr:
                k += 1
            out.append((r, a * part, min(n, (k + 1) * part + overlap) - 1, k - a + 1, min(keys[cs[a]:cs[k] + 1])))
            k += 1
    return out


def region_tuples(regions):
    return [(int(g["read"]), int(g["start"]), int(g["end_incl"]), int(g["n_chunks"]), int(g["best_key"])) for g in regions]


def chunk_reads(read_lens, part, overlap):
    return [r for r, n in enumerate(read_lens) for _ in oracle.chunk_plan(n, part, overlap)]


# ---- kernel cases ----------------------------------------------------------------------------------------------------
def _rand(st, n):
    return pc._rand(st, n)


def _reads_for(seed, tm, n_chunks):
    """Reads that make exactly n_chunks chunks at (PART, OVERLAP): mutated copies of templates among random bases, a
    chunk with N, and (n_chunks >= 3) a first read shorter than the shortest template and one shorter than OVERLAP."""
    st = synth.Stream(seed, 7)
    T = len(tm)

    def soup(n):
        parts = []
        while sum(len(x) for x in parts) < n:
            parts.append(pc.mutated(st, tm[int(st.below(1, T)[0])], 0.08) if int(st.below(1, 3)[0]) else _rand(st, 150))
        return bytearray(b"".join(parts)[:n])

    reads = []
    left = n_chunks
    if n_chunks >= 3:
        reads.append(bytes(soup(max(1, min(len(t) for t in tm) - 1))[:PART]))   # shorter than the shortest template
        reads.append(bytes(soup(OVERLAP - 1)))                                  # shorter than the overlap: one chunk
        left -= 2
    # one long read: `left` chunks, the last one short (PART * (left - 1) + OVERLAP + 37 bases)
    n = PART * (left - 1) + OVERLAP + 37 if left > 1 else PART - 11
    r = soup(n)
    for k in (0, 15, 16, 31, 32, len(r) - 1):
        r[k] = ord("N")
    reads.append(bytes(r))
    assert len(pc.chunks_of(reads, PART, OVERLAP)) == n_chunks
    return reads


class KernelCase:
    """A template set with its reads: `kernel` = the instantiation the selection takes (pc.kernel_of), `general` = the
    handle's switch to the general kernel."""

    def __init__(self, name, monomers, n_chunks, general=False, seed=0, exact=True):
        self.name, self._monomers, self.n_chunks, self.general, self.seed, self.exact = name, monomers, n_chunks, general, seed, exact

    @functools.lru_cache(maxsize=None)
    def data(self):
        ms = self._monomers()
        tm = pc.templates(ms)
        reads = _reads_for(self.seed, tm, self.n_chunks)
        return ms, tm, reads

    def kernel(self):
        return pc.kernel_of(self.data()[1], pc.FLAG_FILTER_GENERAL if self.general else 0)

    @functools.lru_cache(maxsize=None)
    def oracle_keys(self):
        """From the oracle's exact infix DP (exact=True cases: few enough pairs for it)."""
        ms, tm, reads = self.data()
        return keys_of(pc.dist_matrix(tm, pc.chunks_of(reads, PART, OVERLAP)))


def _span(seed, n, lo, hi, pal):
    return lambda: pc.make_set(seed, pc.span_lengths(seed, n, lo, hi), pal)


# T = 2 x monomers (make_set adds a palindrome and a duplicate: n + 2 monomers).  T = 2, 24, 66, 300: a chunk's templates
# lie inside a wave, straddle waves, and straddle workgroups; chunk counts 1, 3, 70: one slot, a few, more than a workgroup.
KERNEL_CASES = [
    KernelCase("u3_hi_T24_c70", _span(201, 10, 161, 192, 176), 70, seed=1),
    KernelCase("u3_hi_T24_c3", _span(201, 10, 161, 192, 176), 3, seed=2),
    KernelCase("u3_hi_T24_c1", _span(201, 10, 161, 192, 176), 1, seed=3),
    KernelCase("u3_lo_T24_c70", _span(202, 10, 129, 160, 150), 70, seed=4),
    KernelCase("g3_T24_c70", _span(201, 10, 161, 192, 176), 70, general=True, seed=1),
    KernelCase("u3_hi_T2_c70", lambda: [pc.make_set(203, [171], 171, with_n=False)[0]], 70, seed=5),
    KernelCase("u3_hi_T66_c70", _span(204, 31, 161, 192, 176), 70, seed=6),
    KernelCase("u3_hi_T300_c70", _span(205, 148, 161, 192, 176), 70, seed=7, exact=False),
    KernelCase("g3_T300_c3", _span(205, 148, 161, 192, 176), 3, general=True, seed=8, exact=False),
    KernelCase("g8_T10_c70", _span(206, 3, 300, 500, 400), 70, seed=9),
    KernelCase("g32_T2_c3", lambda: [pc._rand(synth.Stream(207, 1), 2048)], 3, seed=10),
    KernelCase("g32_T2_c70", lambda: [pc._rand(synth.Stream(207, 1), 2048)], 70, seed=11),
]


# ---- the file job ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def file_fixture():
    """(monomer names, monomers, read names, reads): 12 synthetic monomers of ~171 bp and five reads -- a 40-kb read with
    a 15-kb array of mutated monomers (10 % divergence) between random flanks, a read with two arrays, a read that is all
    array, an all-random read, a 150-bp read."""
    mn, ms = synth.make_monomers(12, seed=11)
    ms = [bytes(m) for m in ms]
    st = synth.Stream(4711, 1)

    def array(n):
        parts = []
        while sum(len(x) for x in parts) < n:
            m = ms[int(st.below(1, len(ms))[0])]
            if int(st.below(1, 4)[0]) == 0:
                m = pc.revcomp(m)
            parts.append(pc.mutated(st, m, 0.10))
        return b"".join(parts)[:n]

    reads = [_rand(st, 12500) + array(15000) + _rand(st, 12500),
             _rand(st, 5000) + array(5200) + _rand(st, 9100) + array(3900) + _rand(st, 4300),
             array(9300),
             _rand(st, 13100),
             _rand(st, 150)]
    return list(mn), ms, ["long", "two_arrays", "all_array", "random", "short"], reads


@functools.lru_cache(maxsize=None)
def file_reference():
    """(keys, chunk_read, regions at F_THR) of the file fixture, from the oracle's exact distances."""
    mn, ms, rn, reads = file_fixture()
    tm = pc.templates(ms)
    keys = keys_of(pc.dist_matrix(tm, pc.chunks_of(reads, F_PART, F_OVERLAP)))
    lens = [len(r) for r in reads]
    cr = chunk_reads(lens, F_PART, F_OVERLAP)
    return keys, cr, regions_of(keys, cr, lens, F_THR, F_PART, F_OVERLAP)


def screen_text(regions, read_names, mono_names):
    """<out>_screen.tsv of regions_of()'s tuples."""
    tn = list(mono_names) + [n + "'" for n in mono_names]
    return "".join("%s\t%d\t%d\t%d\t%d\t%s\n" % (read_names[r], s, e, n, k >> 16, tn[k & 0xffff]) for r, s, e, n, k in regions)


def shifted_raw(text, name, base):
    """Raw TSV text of a region's substring -> the parent's rows: the read's name, start and end increased by base."""
    out = []
    for ln in text.decode().split("\n")[:-1]:
        f = ln.split("\t")
        out.append("\t".join([name, f[1], str(int(f[2]) + base), str(int(f[3]) + base)] + f[4:]) + "\n")
    return "".join(out)
