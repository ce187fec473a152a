"""Test infrastructure of the --ed_thr prefilter tests (tests/test_gpu_prefilter.py, tests/test_prefilter_cpu.py,
tests/golden/make_hw_golden.py): monomer sets of given lengths, the `edges` read list built from a template set, and the
reference side -- the oracle's infix-distance matrix, the filtered order computed from it, the thresholds taken from it.
Everything is a pure function of (seed, lengths): synth.Stream is counter-based and version-stable."""
import numpy as np

from oracle import binding as oracle
from stringdecomposer_amd import lib, synth

DROPPED = 0xFFFF
_CODE = np.zeros(256, dtype=np.int64)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i

# the lengths of the committed fixture (tests/golden/hw_dist/pairs.json): every word boundary of the block recurrence
FIXTURE_LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024,
                   1025, 2047, 2048]
FIXTURE_GROUPS = [("le512", 512), ("le1024", 1024), ("le2048", 2048)]   # one set per mask layout (build_peq: 8 / 16 / 32 words)


def revcomp(b):
    return synth.revcomp_bytes(b)


def _rand(st, n):
    return synth._ACGT[st.below(n, 4)].tobytes() if n > 0 else b""


def mutated(st, b, p):
    """b with an error rate of p (60 % substitutions, 20 % insertions, 20 % deletions); an N is read as A."""
    codes = _CODE[np.frombuffer(b.replace(b"N", b"A"), dtype=np.uint8)]
    out = synth._to_ascii(synth.mutate(codes, st, 0.6 * p, 0.2 * p, 0.2 * p))
    return out or b


def make_set(seed, lengths, pal_len, with_n=True):
    """len(lengths) + 2 related monomers (a common ancestor, 15 % substitutions): one of each length, every second one
    with an N, then a reverse-palindromic monomer of pal_len bp (forward == reverse complement; an odd length has an N
    in the middle) at index 1 and a second copy of monomer 0 at the end -- equal distances in every chunk, so that only
    the index decides the rank."""
    st = synth.Stream(seed, 1)
    anc = st.below(max(lengths) + 16, 4)
    ms = []
    for i, L in enumerate(lengths):
        codes = synth.mutate(anc, st, 0.15, 0.02, 0.02)
        while len(codes) < L:
            codes = np.concatenate([codes, st.below(L, 4)])
        m = bytearray(synth._to_ascii(codes[:L]))
        if with_n and i % 2 == 1 and L > 2:
            m[int(st.below(1, L)[0])] = ord("N")
        ms.append(bytes(m))
    half = _rand(st, pal_len // 2)
    pal = half + (b"N" if pal_len & 1 else b"") + revcomp(half)
    assert pal == revcomp(pal) and len(pal) == pal_len
    ms.insert(1, pal)
    ms.append(ms[0])
    return ms


def span_lengths(seed, n, lo, hi):
    """n lengths in [lo, hi], both ends included at least once."""
    st = synth.Stream(seed, 3)
    return [lo, hi] + [lo + int(x) for x in st.below(n - 2, hi - lo + 1)]


def templates(ms):
    """The engine's template list: the monomers, then their reverse complements (main.cpp:364-371)."""
    return list(ms) + [revcomp(m) for m in ms]


def part_size(tm):
    """A part size at which every read of edges() but the last is one chunk."""
    return max(700, 3 * max(len(t) for t in tm) + 8)


OVERLAP = 100


def edges(seed, tm):
    """The read list of the prefilter tests, from the template list tm.  Every read but the last is one chunk at
    part_size(tm); the last is cut into several (chunks that do not start a read)."""
    st = synth.Stream(seed, 2)
    T = len(tm)
    Lmax = max(len(t) for t in tm)
    longest = max(tm, key=len)

    def pick():
        return tm[int(st.below(1, T)[0])]

    def pool(n, p):
        parts = []
        while sum(len(x) for x in parts) < n:
            parts.append(mutated(st, pick(), p))
        return b"".join(parts)

    fl = (Lmax + 3) // 4
    reads = [_rand(st, fl) + longest + _rand(st, fl),          # an exact copy with random flanks, ~1.5 Lmax
             pick(),                                           # an exact copy alone
             (lambda t: t[:-1] if len(t) > 1 else t)(pick()),  # a template without its last base
             _rand(st, 7) + revcomp(pick()) + _rand(st, 5),    # a reverse complement
             _rand(st, fl) + mutated(st, longest, 0.05) + _rand(st, fl),
             pool(3 * Lmax, 0.10)[:3 * Lmax],                  # ~3 Lmax
             mutated(st, pick(), 0.20),
             _rand(st, Lmax + Lmax // 2),                      # unrelated
             b"A" * 65,
             b"N" * 33]
    r = bytearray(_rand(st, 20) + mutated(st, longest, 0.05) + _rand(st, 20))   # N at the word edges of the packed forms
    for k in (0, 15, 16, 31, 32, len(r) - 1):
        r[k] = ord("N")
    reads.append(bytes(r))
    src = pool(400, 0.10)
    for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        o = int(st.below(1, len(src) - n)[0])
        r = bytearray(src[o:o + n])
        if n in (16, 32, 64):
            r[n - 1] = ord("N")
        if n in (17, 33, 65):
            r[0] = ord("N")
        reads.append(bytes(r))
    part = part_size(tm)
    r = bytearray(pool(2 * part + part // 2, 0.08)[:2 * part + part // 2])
    r[part + 31] = ord("N")
    reads.append(bytes(r))
    assert all(len(x) <= part for x in reads[:-1]) and len(reads[-1]) > 2 * part
    return reads


def small_reads(seed, tm, far):
    """Five single chunks of at most 1 500 bases for the large template sets; `far` = a template index beyond the
    part of the set whose masks fit LDS (its exact copy is one of the reads)."""
    st = synth.Stream(seed, 4)
    T = len(tm)
    parts = []
    while sum(len(x) for x in parts) < 1400:
        parts.append(mutated(st, tm[int(st.below(1, T)[0])], 0.08))
    r = bytearray(b"".join(parts)[:1400])
    for k in (0, 15, 16, 31, 32, len(r) - 1):
        r[k] = ord("N")
    return [_rand(st, 9) + tm[far] + _rand(st, 30), mutated(st, tm[T // 2], 0.12), _rand(st, 600), b"N" * 40, bytes(r)]


def chunks_of(reads, part, overlap=OVERLAP):
    """The chunk texts in the order the engine numbers them (main.cpp:70-81)."""
    out = []
    for r in reads:
        out += [r[o:o + n] for o, n in oracle.chunk_plan(len(r), part, overlap)]
    return out


def dist_matrix(tm, chunks):
    """int32 [chunk][template]: the oracle's exact infix DP (sdo_hw_edit_distance)."""
    return np.array([[oracle.hw_edit_distance(t, c) for t in tm] for c in chunks], dtype=np.int32).reshape(len(chunks), len(tm))


def rank_matrix(dist, thr):
    """uint16 [chunk][template]: FilterMonomersForRead (main.cpp:135-149) on the given distances -- sort by (distance,
    index), keep the first and every distance <= thr; a kept template's place in that order, DROPPED for the others."""
    out = np.full(dist.shape, DROPPED, dtype=np.uint16)
    for c, d in enumerate(dist.tolist()):
        order = sorted(range(len(d)), key=lambda j: (d[j], j))
        kept = [order[0]] + [j for j in order[1:] if d[j] <= thr]
        for r, j in enumerate(kept):
            out[c, j] = r
    return out


def mid_threshold(dist):
    """The smallest v >= the median such that v and v + 1 both occur (<= against < then changes the kept set)."""
    vals = set(dist.ravel().tolist())
    med = float(np.median(dist))
    cand = [v for v in sorted(vals) if v >= med and v + 1 in vals]
    assert cand, "no pair of adjacent distances at or above the median"
    return cand[0]


def thresholds(dist):
    """0, the minimum, the mid threshold, the maximum -- from the reference's matrix, never from the device."""
    out = []
    for v in (0, int(dist.min()), mid_threshold(dist), int(dist.max())):
        if v not in out:
            out.append(v)
    return out


def check_reference(dist, tm):
    """A case cannot degenerate: an exact hit, a template with nothing in common with its chunk, many values."""
    assert (dist == 0).any()
    assert (dist == np.array([len(t) for t in tm], dtype=np.int32)[None, :]).any()
    need = 5 if max(len(t) for t in tm) < 40 else 20
    assert len(set(dist.ravel().tolist())) >= need


def fixture_sets(seed=2026):
    """The fixture's template sets: one template of each FIXTURE_LENGTHS, grouped by mask layout, each with its edges
    reads -> [(group name, templates, chunk texts)].  The templates are used as they are (no reverse complements)."""
    st = synth.Stream(seed, 5)
    out, lo = [], 0
    for g, (name, hi) in enumerate(FIXTURE_GROUPS):
        ms = []
        for i, L in enumerate(x for x in FIXTURE_LENGTHS if lo < x <= hi):
            m = bytearray(_rand(st, L))
            if i % 2 == 1:
                m[int(st.below(1, L)[0])] = ord("N")
            ms.append(bytes(m))
        reads = edges(seed + 1 + g, ms)
        out.append((name, ms, chunks_of(reads, part_size(ms))))
        lo = hi
    return out


# ---- the cases of tests/test_gpu_prefilter.py ------------------------------------------------------------------------
FLAG_NO_EDTHR_COMPACT, FLAG_FILTER_GENERAL, KERNEL_GENERIC = lib.FLAG_NO_EDTHR_COMPACT, lib.FLAG_FILTER_GENERAL, lib.KERNEL_GENERIC


def kernel_of(tm, flags=0):
    """The instantiation launch_edthr_filter takes for the template list tm (csrc/sd_filter.hip, sd_engine_create)."""
    W = (max(len(t) for t in tm) + 63) // 64
    words = {(len(t) - 1) >> 6 for t in tm}
    halves = {((len(t) - 1) >> 5) & 1 for t in tm}
    if len(words) == 1 and len(halves) == 1 and W <= 4 and not flags & FLAG_FILTER_GENERAL:
        return "sd_hw_dist_u<%d,%s>" % (W, "hi" if halves.pop() else "lo")
    return "sd_hw_dist<%d>" % (W if W <= 4 else 8 if W <= 8 else 16 if W <= 16 else 32)


def lds_templates(kernel):
    """Templates whose masks the general kernel holds in 64 KB of LDS: the others read theirs from global memory."""
    assert kernel.startswith("sd_hw_dist<")
    return 65536 // (40 * int(kernel[len("sd_hw_dist<"):-1]))


class Case:
    """One monomer set with its reads.  variants: (id, Engine keywords, kernel instantiation, sd_rank_keep form);
    plan: (family, cells) of lib.plan_info / Engine.info() for the set as planned."""

    def __init__(self, name, seed, lengths, pal, plan, variants, reads="edges", mid_only=False, monomers=None):
        self.name, self.seed, self.lengths, self.pal, self.plan = name, seed, lengths, pal, plan
        self.variants, self.reads_kind, self.mid_only, self._monomers = variants, reads, mid_only, monomers
        self._ref = None
        self._rows = {}

    def monomers(self):
        return self._monomers() if self._monomers else make_set(self.seed, self.lengths, self.pal)

    def reference(self):
        """(monomers, templates, reads, part size, chunk texts, oracle distance matrix, thresholds), computed once."""
        if self._ref is None:
            ms = self.monomers()
            tm = templates(ms)
            if self.reads_kind == "edges":
                reads, part = edges(self.seed, tm), part_size(tm)
            else:
                reads, part = small_reads(self.seed, tm, len(tm) - 1), 1500
            chunks = chunks_of(reads, part)
            dist = dist_matrix(tm, chunks)
            check_reference(dist, tm)
            thrs = [mid_threshold(dist)] if self.mid_only else thresholds(dist)
            self._ref = (ms, tm, reads, part, chunks, dist, thrs)
        return self._ref

    def rows(self, oracle_binding, thr):
        """The oracle's raw TSV of the case's reads at ed_thr = thr, computed once per threshold."""
        if thr not in self._rows:
            ms, _, reads, part = self.reference()[:4]
            self._rows[thr] = oracle_binding.decompose(["r%d" % i for i in range(len(reads))], reads,
                                                       ["m%d" % j for j in range(len(ms))], ms, threads=8, part=part,
                                                       overlap=OVERLAP, ed_thr=thr)
        return self._rows[thr]


def _uniform(name, seed, lengths, pal, W, half):
    u = "sd_hw_dist_u<%d,%s>" % (W, half)
    return Case(name, seed, lengths, pal, ("fast", "u16"),
                [("planned", {}, u, "ranked"), ("general", {"flags": FLAG_FILTER_GENERAL}, "sd_hw_dist<%d>" % W, "ranked")])


def _mixed(name, seed, lengths, pal, W, plan):
    g = "sd_hw_dist<%d>" % W
    return Case(name, seed, lengths, pal, plan, [("planned", {}, g, "ranked"), ("generic", {"kernel": KERNEL_GENERIC}, g, "generic")])


def _tiled30():
    """Thirty monomers of ~342 bp, two of them equal and one reverse-palindromic: the tiled multi-wave layout."""
    _, m60 = synth.make_monomers(60, seed=3)
    ms = [m60[2 * j] + m60[2 * j + 1] for j in range(29)]
    ms.insert(1, m60[58] + revcomp(m60[58]))
    ms[-1] = ms[0]
    return ms


CASES = [
    _uniform("u1_lo", 101, [2, 17, 31, 32], 32, 1, "lo"),
    _uniform("u1_hi", 102, [33, 48, 63, 64], 48, 1, "hi"),
    _uniform("u2_lo", 103, [65, 80, 96], 80, 2, "lo"),
    _uniform("u2_hi", 104, [97, 127, 128], 128, 2, "hi"),
    _uniform("u3_lo", 105, [129, 160], 160, 3, "lo"),
    _uniform("u3_hi", 106, [161, 171, 192], 192, 3, "hi"),
    _uniform("u4_lo", 107, [193, 224], 224, 4, "lo"),
    _uniform("u4_hi", 108, [225, 255, 256], 256, 4, "hi"),
    _mixed("g4_mixed", 111, [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256], 64, 4, ("fast", "u16")),
    _mixed("g8_mixed", 112, [1, 64, 257, 320, 511, 512], 320, 8, ("fast", "u16")),
    _mixed("g16_mixed", 113, [65, 513, 700, 1023, 1024], 700, 16, ("fast", "f16/bf8-codes tiled x waves")),
    _mixed("g32_mixed", 114, [128, 1025, 2047, 2048], 2048, 32, ("fast", "int16/int8-codes tiled x waves")),
    # T = 260 on the uniform kernel: the rotating window of 256 templates' masks in LDS
    Case("lds_window_260", 121, span_lengths(121, 128, 161, 192), 176, ("fast", "f16/bf8-codes x waves"),
         [("compacted", {}, "sd_hw_dist_u<3,hi>", "compacted"),
          ("ranked", {"flags": FLAG_NO_EDTHR_COMPACT}, "sd_hw_dist_u<3,hi>", "ranked")]),
    # more templates than 64 KB of LDS hold masks for: lanes on global masks beside lanes on LDS
    Case("masks_w3_560", 131, span_lengths(131, 278, 165, 177), 170, ("fast", "f16/bf8-codes x waves"),
         [("general", {"flags": FLAG_FILTER_GENERAL}, "sd_hw_dist<3>", "compacted")], reads="small"),
    Case("masks_w8_208", 132, span_lengths(132, 102, 260, 330), 300, ("fast", "f16/bf8-codes tiled x waves"),
         [("planned", {}, "sd_hw_dist<8>", "compacted")], reads="small"),
    Case("masks_w16_104", 133, span_lengths(133, 50, 520, 560), 540, ("fast", "f16/bf8-codes tiled x waves"),
         [("planned", {}, "sd_hw_dist<16>", "compacted")], reads="small"),
    Case("masks_w32_52", 134, span_lengths(134, 24, 1030, 1060), 1040, ("fast", "f16/bf8-codes tiled x waves"),
         [("planned", {}, "sd_hw_dist<32>", "compacted")], reads="small"),
    Case("tiled_30x342", 141, None, None, ("fast", "f16/bf8-codes tiled x waves"),
         [("compacted", {}, "sd_hw_dist<8>", "compacted"), ("ranked", {"flags": FLAG_NO_EDTHR_COMPACT}, "sd_hw_dist<8>", "ranked")],
         reads="small", mid_only=True, monomers=_tiled30),
]
MASK_CASES = ("masks_w3_560", "masks_w8_208", "masks_w16_104", "masks_w32_52")


def case_variants():
    return [(c, v) for c in CASES for v in c.variants]
