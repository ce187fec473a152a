"""Cases of the in-stream identity tests (tests/test_ident_cases_cpu.py, tests/test_gpu_ident_routes.py): monomer sets
and reads that put csrc/sd_ident.hip on every route it chooses at run time -- each instantiated word count K, the padding
edges of a top-aligned template, match masks in LDS or in global memory, and the three forms of the selection pass -- with,
per case, the routes it must take (restated here from the sequences alone and asserted at import), an independent
restatement of the pruned homopolymer pass, and the rows of the final decomposition at full precision, recomputed from the
oracle's alignments.

Everything is a pure function of fixed seeds (synth.Stream is counter-based and version-stable); references are computed
once per process and shared."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import binding as oracle
from stringdecomposer_amd import synth

PART, OVERLAP = 5000, 500     # the defaults of the command line: every read below is one chunk
SHORT_MAX = 512               # longer segments go on the long list and past the selection pass
LDS_MASK_BYTES = 60 * 1024    # match masks of a pass stay in LDS up to here
SELECT_BUF = 1024             # candidate slots per wave of the selection pass
FINAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "final")


# ---- what the engine derives from a template set (engine_set_identity, sd_ident_pairs / _dist / _select) -----------------
def words(length):
    """Instantiated word count of templates up to `length` symbols: ceil(L / 64), 5 -> 6 and 7 -> 8."""
    k = (length + 63) // 64
    return 6 if k == 5 else 8 if k == 7 else k


def hpc(seq):
    """Homopolymer compression (bytes)."""
    a = np.frombuffer(seq, dtype=np.uint8)
    return a[np.concatenate([[True], a[1:] != a[:-1]])].tobytes() if len(a) else b""


def revcomp(seq):
    return synth.revcomp_bytes(seq)


def interleaved(names, seqs):
    """m0, m0', m1, m1', ...: the template order of the identity passes and, the names being unique, the key order."""
    return [x for n in names for x in (n, n + "'")], [x for s in seqs for x in (s, revcomp(s))]


def routes(seqs):
    """Route flags of a monomer set: dict(T, taken, K, Kh, mask_bytes, mask_bytes_h, masks, masks_h, select)."""
    T = 2 * len(seqs)
    tmax = max(len(s) for s in seqs)
    hmax = max(len(hpc(s)) for s in seqs)   # (the reverse complement compresses to the same length)
    K, Kh = words(tmax), words(hmax)
    mb, mbh = T * 5 * K * 8, T * 5 * Kh * 8
    # the selection reads a record's words once and keeps them in registers ("two": T <= 128), or reads them twice and
    # collects a wave's candidates in a buffer ("buffered"), or has no buffer ("direct": a record may not fit it)
    select = "two" if T <= 128 else "buffered" if T <= SELECT_BUF else "direct"
    return dict(T=T, taken=tmax <= 512, K=K, Kh=Kh, mask_bytes=mb, mask_bytes_h=mbh,
                masks="lds" if mb <= LDS_MASK_BYTES else "global", masks_h="lds" if mbh <= LDS_MASK_BYTES else "global",
                select=select, pads=sorted({64 * K - len(s) for s in seqs}))


# ---- the cases ------------------------------------------------------------------------------------------------------
def _rand(st, n):
    return synth._ACGT[st.below(n, 4)].tobytes()


def _reads(ms, seed, read_len, n=2):
    rn, rs = synth.make_reads(ms, n, read_len=read_len, seed=seed)
    return list(rn), [bytes(s) for s in rs]


def _with_n(reads, which, at, n):
    """`n` N inserted into read `which` at `at` (the read grows: the block around `at` becomes n symbols longer)."""
    rn, rs = reads
    rs = list(rs)
    rs[which] = rs[which][:at] + b"N" * n + rs[which][at:]
    return rn, rs


def _mono(n, seed, length=171):
    mn, ms = synth.make_monomers(n, seed=seed, length=length)
    return list(mn), [bytes(s) for s in ms]


def _k8_edges(first=512, seed=48):
    """Six monomers from one 500-bp ancestor, cut or extended to exact lengths: with K = 8 the paddings 0, 63 and 447."""
    anc = synth.Stream(seed, 1).below(500, 4)
    out = []
    for j, ln in enumerate([first, 449, 450, 500, 65, 480]):
        m = synth._to_ascii(synth.mutate(anc, synth.Stream(seed, 100 + j), 0.10, 0.005, 0.005))
        m = (m + _rand(synth.Stream(seed, 200 + j), ln))[:ln]
        out.append(m)
    return ["E%d" % j for j in range(6)], out


def _expansions(seed, core_len, n):
    """One compressed sequence of core_len symbols (no two equal neighbours) expanded n times with random run lengths of
    1-3: n monomers that compress to the same template."""
    step = synth.Stream(seed, 1).below(core_len, 3) + 1
    step[0] = 0
    core = np.cumsum(step) % 4
    return [synth._to_ascii(np.repeat(core, synth.Stream(seed, 100 + j).below(core_len, 3) + 1)) for j in range(n)]


def _hpc_ties():
    """Six expansions of one compressed 120-bp sequence and a seventh monomer that is a copy of the first."""
    out = _expansions(43, 120, 6)
    out.append(out[0])
    return ["H%d" % j for j in range(7)], out


class Case:
    """name, monomers() -> (names, seqs), reads() -> (names, seqs), want = the route flags the case exists for."""

    def __init__(self, name, monomers, reads, want, golden=True, strict_prune=True):
        self.name, self._monomers, self._reads, self.want, self.golden, self.strict_prune = name, monomers, reads, want, golden, strict_prune

    @functools.lru_cache(maxsize=None)
    def monomers(self):
        return self._monomers()

    @functools.lru_cache(maxsize=None)
    def reads(self):
        return self._reads(self.monomers()[1])

    @functools.lru_cache(maxsize=None)
    def routes(self):
        return routes(self.monomers()[1])

    def dir(self):
        return os.path.join(FINAL, "ident_" + self.name)

    def __repr__(self):
        return self.name


CASES = [
    Case("k1", lambda: _mono(4, 37, 60), lambda ms: _reads(ms, 37, 1500),
         dict(T=8, K=1, Kh=1, masks="lds", masks_h="lds", select="two")),
    Case("k2", lambda: _mono(5, 45, 120), lambda ms: _with_n(_reads(ms, 45, 2000), 1, 1000, 8),
         dict(T=10, K=2, Kh=2, masks="lds", masks_h="lds", select="two")),
    Case("k4", lambda: _mono(4, 47, 250), lambda ms: _reads(ms, 47, 2500),
         dict(T=8, K=4, Kh=3, masks="lds", masks_h="lds", select="two")),
    Case("k6_round", lambda: _mono(4, 49, 300), lambda ms: _reads(ms, 49, 2500),
         dict(T=8, K=6, Kh=4, masks="lds", masks_h="lds", select="two")),
    Case("k8_round", lambda: _mono(4, 51, 420), lambda ms: _reads(ms, 51, 2500),
         dict(T=8, K=8, Kh=6, masks="lds", masks_h="lds", select="two")),
    Case("k8_edges", _k8_edges, lambda ms: _reads(ms, 48, 2500),
         dict(T=12, K=8, Kh=6, masks="lds", masks_h="lds", select="two", taken=True)),
    Case("k8_513", lambda: _k8_edges(513), lambda ms: _reads(_k8_edges()[1], 48, 2500),
         dict(T=12, taken=False), golden=False),
    # (three reads, so that a row cap of one read cuts the job into three device batches)
    Case("t140", lambda: _mono(70, 35), lambda ms: _with_n(_reads(ms, 35, 1500, n=3), 0, 700, 600),
         dict(T=140, K=3, Kh=3, masks="lds", masks_h="lds", select="buffered")),
    # 470 bp: plain 462-479 (K = 8), compressed 330-373 (K = 6, 62 400 B: just past LDS).  At 500 bp the longest compressed
    # template of every seed tried has 390-400 symbols -- K = 8 again, and K = 6 would read its masks from LDS only
    Case("t260_k8", lambda: _mono(130, 33, 470), lambda ms: _reads(ms, 33, 2500),
         dict(T=260, K=8, Kh=6, mask_bytes=83200, mask_bytes_h=62400, masks="global", masks_h="global", select="buffered")),
    Case("t520", lambda: _mono(260, 39), lambda ms: _reads(ms, 39, 2000),
         dict(T=520, K=3, Kh=3, mask_bytes=62400, masks="global", masks_h="global", select="buffered")),
    Case("t1040", lambda: _mono(520, 31, 100), lambda ms: _reads(ms, 31, 1500),
         dict(T=1040, K=2, Kh=2, mask_bytes=83200, masks="global", masks_h="global", select="direct")),
    Case("hpc_ties", _hpc_ties, lambda ms: _reads(ms, 43, 2000),
         dict(T=14, K=4, Kh=2, masks="lds", masks_h="lds", select="two"), strict_prune=False),
]
# The cases above have a few dozen records each, and the selection runs with thousands of waves: every wave takes at most
# one record, so its buffer never holds two records' candidates and is flushed once, behind the loop.  This case is the one
# that makes waves go through several records: 300 expansions of one 40-symbol compressed sequence -- about half of the 600
# compressed pairs of a record tie for its best, so a wave's buffer of 1024 holds the candidates of two records and must be
# flushed inside the loop before the third -- and reads of ~7000 blocks, in fewer than 256 chunks (one identity slice).  Too
# many pairs for the oracle's alignments of every template: its tests take the rows from the job itself and use that the
# compressed templates are two (test_gpu_ident_routes.py).
WAVE_CASE = Case("t600_waves", lambda: (["X%d" % j for j in range(300)], _expansions(53, 40, 300)),
                 lambda ms: _reads(ms, 53, 4500, n=130),
                 dict(T=600, K=2, Kh=1, masks="lds", masks_h="lds", select="buffered"), golden=False)
BY_NAME = {c.name: c for c in CASES + [WAVE_CASE]}
GOLDEN_CASES = [c for c in CASES if c.golden]


def check_routes(case):
    """A case lies on the routes it exists for (and every read is a single chunk)."""
    r = case.routes()
    for k, v in case.want.items():
        assert r[k] == v, (case.name, k, r[k], v)
    assert all(len(s) < PART for s in case.reads()[1]), case.name
    if case.name == "k6_round":
        assert all((len(s) + 63) // 64 == 5 for s in case.monomers()[1])    # word 0 of every template is padding
    if case.name == "k8_round":
        assert all((len(s) + 63) // 64 == 7 for s in case.monomers()[1])
    if case.name == "k8_edges":
        assert [len(s) for s in case.monomers()[1]] == [512, 449, 450, 500, 65, 480] and {0, 63, 447} <= set(r["pads"])
    if case.name == "k8_513":
        assert [len(s) for s in case.monomers()[1]] == [513, 449, 450, 500, 65, 480]
        assert case.monomers()[1][0][:512] == BY_NAME["k8_edges"].monomers()[1][0] and case.reads() == BY_NAME["k8_edges"].reads()
    if case.name == "t600_waves":
        assert len(case.reads()[1]) < 256 and len(set(case.monomers()[1])) == 300 and len({hpc(s) for s in case.monomers()[1]}) == 1
    if case.name == "hpc_ties":
        ms = case.monomers()[1]
        assert len({hpc(s) for s in ms}) == 1 and len(hpc(ms[0])) == 120 and ms[6] == ms[0] and len(set(ms)) == 6


for _c in CASES + [WAVE_CASE]:   # (0.2 s: a later change to synth cannot silently move a case off its route)
    check_routes(_c)


# ---- the rows of a case, from the oracle --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raw_tsv(name):
    c = BY_NAME[name]
    (rn, rs), (mn, ms) = c.reads(), c.monomers()
    return oracle.decompose(rn, rs, mn, ms, threads=4, part=PART, overlap=OVERLAP)


@functools.lru_cache(maxsize=None)
def raw_rows(name):
    """[(read index, template index in interleaved order, start, end)] of the oracle's raw TSV, in file order."""
    c = BY_NAME[name]
    ridx = {n: i for i, n in enumerate(c.reads()[0])}
    tidx = {n: i for i, n in enumerate(interleaved(*c.monomers())[0])}
    out = []
    for ln in raw_tsv(name).decode().split("\n")[:-1]:
        f = ln.split("\t")
        out.append((ridx[f[0]], tidx[f[1]], int(f[2]), int(f[3])))
    return out


def _segments(name):
    rs = BY_NAME[name].reads()[1]
    return [rs[r][s:e + 1] for r, _, s, e in raw_rows(name)]


def _align(segs, tmpl):
    """-> (d, matches, columns) int64 arrays [rows, T] of the oracle's unit-cost alignments."""
    oracle.lib()
    uniq = list(dict.fromkeys(tmpl))   # (equal templates -- a duplicate monomer, a set that compresses to one -- aligned once)
    with ThreadPoolExecutor(8) as ex:   # (the oracle's C call holds no state and runs without the interpreter lock)
        out = list(ex.map(lambda q: [oracle.nw_identity(q, t) for t in uniq], segs))
    at = {t: k for k, t in enumerate(uniq)}
    out = np.array(out, dtype=np.int64).reshape(len(segs), len(uniq), 3)[:, [at[t] for t in tmpl], :]
    return out[:, :, 0], out[:, :, 1], out[:, :, 2]


def _percent(d, m, cols):
    """The identity as the post-processing computes it: matches / columns, then * 100; 0 for an empty side."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = m.astype(np.float64) / cols
        a = a * 100
    return np.where(d == -1, 0.0, a)


@functools.lru_cache(maxsize=None)
def alignments(name, homo):
    """(d, matches, columns, kept query symbols [rows], template lengths [T]) of every (row, template) pair."""
    tm = interleaved(*BY_NAME[name].monomers())[1]
    segs = _segments(name)
    if homo:
        tm, segs = [hpc(t) for t in tm], [hpc(s) for s in segs]
    d, m, cols = _align(segs, tm)
    return d, m, cols, np.array([len(s) for s in segs], dtype=np.int64), np.array([len(t) for t in tm], dtype=np.int64)


# ---- the pruned homopolymer pass, restated (sd_ident.hip: ident_bounds, sd_ident_select) ---------------------------------
def bounds(d, c, tl):
    """Bounds of a pair's identity from its distance d, its c kept query symbols and tl template symbols.  The number nL of
    template symbols against a gap lies in [max(0, tl - c), (d + tl - c) / 2], and matches / columns =
    (c - d + nL) / (c + nL) grows with nL.  -> (lb, ub, fewest matches)."""
    d, c, tl = np.broadcast_arrays(np.asarray(d, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(tl, dtype=np.int64))
    nlo = np.maximum(0, tl - c)
    nhi = np.maximum(nlo, np.minimum(tl, (d + tl - c) // 2))    # (d >= |tl - c|: the quotient is of a non-negative number)
    m_lb = np.maximum(0, c - d + nlo)
    lb = m_lb.astype(np.float64) / np.maximum(1, c + nlo)
    ub = np.maximum(0, c - d + nhi).astype(np.float64) / np.maximum(1, c + nhi)
    return lb, ub, m_lb


@functools.lru_cache(maxsize=None)
def pruned(name):
    """-> (keep [rows, T] bool, short [rows] bool): the pairs of the compressed pass that go on the candidate list -- upper
    bound >= the row's second largest lower bound (a duplicate of the maximum counts twice) * (1 - 1e-12) -- for the rows of
    at most SHORT_MAX symbols; the longer ones are not selected from (every pair of theirs is aligned in full elsewhere).
    All operands are integers below 65 536, so two bounds are equal as rationals -- and then as correctly rounded doubles --
    or at least 2e-10 apart: the comparison does not depend on rounding."""
    d, _, _, c, tl = alignments(name, True)
    short = np.array([e - s + 1 <= SHORT_MAX for _, _, s, e in raw_rows(name)], dtype=bool)
    return keep_rule(d, c, tl, short), short


def keep_rule(d, c, tl, short):
    """The rule of pruned() on arrays: d [rows, T], c [rows], tl [T], short [rows] -> keep [rows, T]."""
    assert d.min() >= 0 and d.max() < 65536 and c.max() < 65536
    lb, ub, _ = bounds(d, c[:, None], tl[None, :])
    m2 = np.sort(lb, axis=1)[:, -2]
    return (ub >= (m2 * (1.0 - 1e-12))[:, None]) & short[:, None]


def select_trace(cands, T, waves):
    """What the buffer of the selection pass goes through: wave w takes the records w, w + waves, ... in turn, skips the
    long ones (cands[x] < 0), flushes its buffer before a record when the buffer's content and T more entries would not fit,
    and adds the record's candidates.  -> (flushes inside the loop, records added to a buffer that was not empty)."""
    mid = carried = 0
    if T > SELECT_BUF:
        return 0, 0
    for w in range(min(waves, len(cands))):
        nbuf = 0
        for x in range(w, len(cands), waves):
            if cands[x] < 0:
                continue
            if nbuf + T > SELECT_BUF and nbuf:
                mid, nbuf = mid + 1, 0
            carried += nbuf > 0
            nbuf += int(cands[x])
    return mid, carried


def expected_full_pairs(name):
    return int(pruned(name)[0].sum())


# ---- the final rows at full precision (the reference's convert_read: own monomer; first maximum among the others; stable
# sort of the compressed scores) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def final_reference(name):
    """dict(read, start, end, best, second, homo_best, homo_second [rows] int, ident, second_ident, homo_ident,
    homo_second_ident [rows] float64, alt [rows, T] float64) -- key indices in interleaved order (all names are unique)."""
    rows = raw_rows(name)
    d, m, cols, _, _ = alignments(name, False)
    hd, hm, hcols, _, _ = alignments(name, True)
    vals, hvals = _percent(d, m, cols), _percent(hd, hm, hcols)
    n, T = vals.shape
    own = np.array([t for _, t, _, _ in rows], dtype=np.int64)
    second, s2 = np.zeros(n, dtype=np.int64), np.zeros(n)
    for i in range(n):
        sb, sbs = None, -1
        for t in range(T):
            if t != own[i] and (sb is None or sbs < vals[i, t]):
                sb, sbs = t, vals[i, t]
        second[i], s2[i] = sb, sbs
    order = [sorted(range(T), key=lambda t: -hvals[i, t]) for i in range(n)]   # (sorted() is stable)
    h0 = np.array([o[0] for o in order], dtype=np.int64)
    h1 = np.array([o[1] for o in order], dtype=np.int64)
    ar = np.arange(n)
    return dict(read=np.array([r for r, _, _, _ in rows]), start=np.array([s for _, _, s, _ in rows]),
                end=np.array([e for _, _, _, e in rows]), best=own, second=second, homo_best=h0, homo_second=h1,
                ident=vals[ar, own], second_ident=s2, homo_ident=hvals[ar, h0], homo_second_ident=hvals[ar, h1], alt=vals)
