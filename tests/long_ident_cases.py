"""Cases of the identity kernel for monomers of 513 .. 2048 bp (tests/test_long_ident_cases_cpu.py,
tests/test_gpu_long_ident.py): template sets and segment lists that put csrc/sd_nw_long.hip and the long branch of
sd::nw_identity_device (csrc/sd_nw.hip) on every edge they have -- each lanes-per-pair value with K == LPP, template
lengths at the word edges, short templates whose words are all padding, step counts at the 16-step checkpoint edges, the
exact boundary of edlib's Hirschberg split and of the kernel's segment room, waves whose pairs differ maximally in length,
idle pair slots, a second round of pairs in one workgroup -- with, per call, the route it must take and the number of pairs
the driver deals to the device and to host threads.  Those are restated here from lengths alone (not taken from the C++)
and asserted at import; the GPU tests compare them with what lib.nw_route_counts() saw.

Everything is a pure function of fixed seeds (synth.Stream is counter-based and version-stable); the references (the
reference's vendored edlib through edlib_ref.nw) are computed once per process and shared."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import edlib_ref
from stringdecomposer_amd import synth

QCAP = 8192          # symbols of a segment the long kernel has room for (NWL_QCAP); longer ones go to host threads
LONG_MIN = 513       # the long route: longest template (after compression in a homo call) of 513 .. 2048 symbols
COUNT_KEYS = ("long_calls", "long_pairs", "long_host_pairs", "short_calls", "short_pairs", "declined_calls")


# ---- what the driver derives from lengths (nw_identity_device) ----------------------------------------------------------
def splits(q, t):
    """edlib walks a pair by Hirschberg's split once its traceback data would reach 1 MB (edlib.cpp:1186)."""
    return 20 * ((q + 63) // 64) * t + 8 * t >= 1 << 20


def qstar(t):
    """The longest segment that does not split against a template of t symbols."""
    q = 64 * (((1 << 20) - 8 * t - 1) // (20 * t))
    assert not splits(q, t) and splits(q + 1, t)
    return q


def hpc(seq):
    """Homopolymer compression (bytes)."""
    a = np.frombuffer(seq, dtype=np.uint8)
    return a[np.concatenate([[True], a[1:] != a[:-1]])].tobytes() if len(a) else b""


def route(templates, homo):
    """dict(tmax, K, LPP, slots, long, pads) of a call with these (raw) templates."""
    lens = [len(hpc(t)) if homo else len(t) for t in templates]
    tmax = max(lens)
    K = (tmax + 63) // 64
    LPP = 16 if K <= 16 else 32
    return dict(tmax=tmax, K=K, LPP=LPP, slots=2 * 64 // LPP, long=tmax >= LONG_MIN, pads=sorted({64 * K - n for n in lens}))


def deal(seg_lens, templates, pair_tmpl=None):
    """(device pairs, host pairs) of a long call, from the raw lengths: a pair goes to host threads iff its segment is longer
    than QCAP or the pair splits; a pair with an empty side is neither."""
    dev = host = 0
    tl = [len(t) for t in templates]
    for s, q in enumerate(seg_lens):
        for t in (tl if pair_tmpl is None else [tl[int(pair_tmpl[s])]]):
            if q <= 0 or t <= 0:
                continue
            if q > QCAP or splits(q, t):
                host += 1
            else:
                dev += 1
    return dev, host


def expected_counts(seg_lens, templates, homo, pair_tmpl=None):
    """By how much a device call moves each counter of COUNT_KEYS."""
    out = dict.fromkeys(COUNT_KEYS, 0)
    r = route(templates, homo)
    if r["long"]:
        out["long_calls"] = 1
        out["long_pairs"], out["long_host_pairs"] = deal(seg_lens, templates, pair_tmpl)
    elif splits(max(seg_lens), max(len(t) for t in templates)):   # the short route declines the call as a whole
        out["declined_calls"] = 1
    else:
        out["short_calls"] = 1
        out["short_pairs"] = len(seg_lens) * (len(templates) if pair_tmpl is None else 1)
    return out


# ---- the template sets and their segments -------------------------------------------------------------------------------
SETS = {"k9": [513, 576, 1, 64, 65], "k12": [768, 705, 300], "k16": [1024, 961, 960, 512, 63], "k17": [1025, 1088, 2, 600],
        "k24": [1536, 1473, 700], "k32": [2048, 1985, 1984, 130, 1]}
QSTAR = {"k9": 5760, "k12": 4288, "k16": 3200, "k17": 3008, "k24": 2112, "k32": 1600}
# K of the plain and of the compressed call (k9 compresses to 384 bp: the short route)
K_PLAIN = {"k9": 9, "k12": 12, "k16": 16, "k17": 17, "k24": 24, "k32": 32}
K_HOMO = {"k12": 10, "k16": 13, "k17": 13, "k24": 18, "k32": 27}


def content(st, kind, n):
    """n symbols: 0 random ACGT, 1 two letters (A/T), 2 a period-7 tandem repeat, 3 AC repeated, 4 homopolymer runs of 1-8."""
    if kind == 0:
        return synth._ACGT[st.below(n, 4)].tobytes()
    if kind == 1:
        return synth._ACGT[st.below(n, 2) * 3].tobytes()
    if kind == 2:
        return (synth._ACGT[st.below(7, 4)].tobytes() * (n // 7 + 1))[:n]
    if kind == 3:
        return (b"AC" * n)[:n]
    runs = st.below(n, 8) + 1
    return b"".join(bytes([b"ACGT"[i % 4]]) * int(r) for i, r in enumerate(runs))[:n]


def _codes(seq):
    return np.searchsorted(synth._ACGT, np.frombuffer(seq.replace(b"N", b"A"), dtype=np.uint8))


class LongSet:
    """One template set: .templates (the monomers, then their reverse complements), .segs (the segments in increasing
    length, the empty one first), .seq / .starts / .ends (their text), and the pair_tmpl form .pair_order (indices into
    .segs, shortest and longest interleaved) / .pair_tmpl."""

    def __init__(self, name):
        lens = SETS[name]
        self.name, self.lens, self.L0, self.qstar = name, lens, max(lens), QSTAR[name]
        K = (self.L0 + 63) // 64
        st = synth.Stream(900, len(name) + lens[0])
        ms = [content(st, j % 5, ln) for j, ln in enumerate(lens)]
        ms[0] = ms[0][:100] + b"N" + ms[0][101:]
        self.monomers = ms
        self.templates = ms + [synth.revcomp_bytes(m) for m in ms]
        L0 = self.L0
        ql = sorted({1, 2, 15, 16, 17, 64, 65, L0 - 1, L0, L0 + 1, self.qstar, self.qstar + 1, QCAP, QCAP + 1} |
                    {x - K for x in (33, 34, 49) if x - K > 0})
        self.seg_lens = [0] + ql
        segs = [b""]
        for i, n in enumerate(ql, start=1):
            src = ms[i % len(ms)].replace(b"N", b"A")
            base = src * ((n + n // 4 + 16) // len(src) + 2)
            if i % 3 == 0:      # mutated copies of a monomer
                q = synth._to_ascii(synth.mutate(_codes(base[:n + n // 8 + 8]), st, 0.06, 0.03, 0.03))
            elif i % 3 == 1:    # exact copies, rotated by 3
                q = base[3:]
            else:               # low-complexity text
                q = content(st, 1 + i % 4, n)
            segs.append((q + base)[:n])
        assert [len(s) for s in segs] == self.seg_lens
        at = self.seg_lens.index(L0)           # one N in the text as well
        segs[at] = segs[at][:L0 // 2] + b"N" + segs[at][L0 // 2 + 1:]
        self.segs = segs
        self.seq = b"".join(segs)
        off = np.concatenate([[0], np.cumsum(self.seg_lens)])
        self.starts, self.ends = off[:-1].copy(), off[1:] - 1
        self.starts[0], self.ends[0] = 5, 4    # the empty segment: end = start - 1
        # pair_tmpl form: shortest, longest, second shortest, ... so that the consecutive pairs of a wave differ maximally
        # in step count; the segments around L0 and q* against the longest monomer (the exact split boundary), the others
        # against a template that moves with the position
        n = len(segs)
        order = [x for a, b in zip(range(n), range(n - 1, -1, -1)) for x in (a, b)][:n]
        j0, T = lens.index(L0), len(self.templates)
        edge = {L0 - 1, L0, L0 + 1, self.qstar, self.qstar + 1}

        def tmpl_of(order):
            return np.array([(j0 + (p % 2) * len(ms)) if self.seg_lens[s] in edge else (3 * p + 1) % T
                             for p, s in enumerate(order)], dtype=np.int32)

        # neither the list nor its device pairs a multiple of the 4 or 8 pair slots of a workgroup: more 64-symbol segments
        while len(order) % 4 == 0 or deal([self.seg_lens[s] for s in order], self.templates, tmpl_of(order))[0] % 4 == 0:
            order.append(self.seg_lens.index(64))
        self.pair_order = np.array(order)
        self.pair_tmpl = tmpl_of(order)

    def call(self, form):
        """(seq, starts, ends, pair_tmpl or None, segment lengths) of the all-vs-all ("all"), the pair_tmpl ("pair") or the
        single-pair ("one": the q* segment against the longest monomer, the longest pair of the set the device takes) call."""
        if form == "all":
            return self.seq, self.starts, self.ends, None, list(self.seg_lens)
        if form == "pair":
            o = self.pair_order
            return self.seq, self.starts[o], self.ends[o], self.pair_tmpl, [self.seg_lens[s] for s in o]
        assert form == "one"
        s = self.seg_lens.index(self.qstar)
        return self.seq, self.starts[s:s + 1], self.ends[s:s + 1], np.array([self.lens.index(self.L0)], dtype=np.int32), [self.qstar]

    def expected(self, form, homo):
        _, _, _, pt, sl = self.call(form)
        return expected_counts(sl, self.templates, homo, pt)


@functools.lru_cache(maxsize=None)
def long_set(name):
    return LongSet(name)


def _align(segs, tmpl):
    """(dist, matches, columns) int32 [segments, templates] of edlib_ref.nw on every pair."""
    with ThreadPoolExecutor(8) as ex:   # (the C call runs without the interpreter lock)
        out = list(ex.map(lambda q: [edlib_ref.nw(q, t) for t in tmpl], segs))
    out = np.array(out, dtype=np.int32).reshape(len(segs), len(tmpl), 3)
    return out[:, :, 0], out[:, :, 1], out[:, :, 2]


@functools.lru_cache(maxsize=None)
def reference(name, homo):
    """edlib on every (segment, template) pair of a set (or of ROUNDS), all-vs-all; compressed on both sides for homo."""
    c = ROUNDS if name == "rounds" else long_set(name)
    segs, tm = c.segs, c.templates
    if homo:
        segs, tm = [hpc(s) for s in segs], [hpc(t) for t in tm]
    return _align(segs, tm)


def reference_of(name, form, homo):
    """The reference in the shape lib.identity_segments returns for that call."""
    d, m, c = reference(name, homo)
    if form == "all":
        return d, m, c
    s = long_set(name)
    if form == "pair":
        o, t = s.pair_order, s.pair_tmpl
    else:
        o, t = np.array([s.seg_lens.index(s.qstar)]), np.array([s.lens.index(s.L0)])
    return d[o, t], m[o, t], c[o, t]


class Rounds:
    """Set k9 with 300 segments of 1-200 symbols and the 8192 one, all-vs-all: the 8192 segment (against the templates of
    1, 64 and 65 bp it does not split) sizes the LDS room of every pair, one workgroup fits a compute unit, and the launch
    has no more workgroups than compute units -- so with more device pairs than CUs x slots a workgroup takes a second
    round of pairs, in the LDS and checkpoint area of its first."""

    def __init__(self):
        k9 = long_set("k9")
        self.templates = k9.templates
        st = synth.Stream(901, 9)
        lens = [int(x) + 1 for x in st.below(300, 200)] + [QCAP]
        ms = [m.replace(b"N", b"A") for m in k9.monomers if len(m) > 200]
        segs = []
        for i, n in enumerate(lens[:-1]):
            src = ms[i % len(ms)]
            at = int(st.below(1, len(src) - n)[0])
            segs.append(synth._to_ascii(synth.mutate(_codes(src[at:at + n + 40]), st, 0.06, 0.03, 0.03))[:n] if i % 2
                        else content(st, 1 + i % 4, n))
        segs.append(k9.segs[k9.seg_lens.index(QCAP)])
        assert [len(s) for s in segs] == lens
        self.segs, self.seg_lens, self.seq = segs, lens, b"".join(segs)
        off = np.concatenate([[0], np.cumsum(lens)])
        self.starts, self.ends = off[:-1], off[1:] - 1
        self.route = route(self.templates, False)
        self.dev_pairs, self.host_pairs = deal(lens, self.templates)
        lds = self.route["slots"] * (QCAP + 16 * self.route["LPP"] * 16 + 5 * self.route["LPP"] * 8)
        assert 160 * 1024 // lds == 1          # workgroups per CU by LDS (160 KB per CU)

    def rounds(self, n_cu):
        """ceil(device pairs / (grid x slots)) on a device of n_cu compute units."""
        slots = self.route["slots"]
        grid = max(1, min((self.dev_pairs + slots - 1) // slots, n_cu))
        return (self.dev_pairs + grid * slots - 1) // (grid * slots)


ROUNDS = Rounds()
FORMS = ("all", "pair")
CALLS = [(name, homo, form) for name in SETS for homo in (False, True) for form in FORMS]


def check_cases():
    """The cases lie on the edges they exist for."""
    ks, lpp_eq, pads = set(), set(), {}
    for name in SETS:
        s = long_set(name)
        assert s.qstar == qstar(s.L0) and s.seq.count(b"N") == 1 and s.monomers[0].count(b"N") == 1
        assert [len(m) for m in s.monomers] == s.lens and {0, 1, 2, 15, 16, 17, 64, 65, QCAP, QCAP + 1} <= set(s.seg_lens)
        for homo in (False, True):
            r = route(s.templates, homo)
            assert r["K"] == (K_PLAIN[name] if not homo else K_HOMO.get(name, 6)), (name, homo, r)
            assert r["long"] == (not homo or name != "k9") and r["slots"] == (8 if r["K"] <= 16 else 4)
            if not r["long"]:
                continue
            ks.add(r["K"])
            if r["K"] == r["LPP"]:
                lpp_eq.add(r["LPP"])
            pads.setdefault(r["K"], set()).update(r["pads"])
            for form in FORMS:
                e = s.expected(form, homo)
                assert e["long_calls"] == 1 and e["long_pairs"] > 0 and e["long_host_pairs"] > 0, (name, homo, form)
                if form == "pair":   # an idle pair slot in the last round of the launch
                    assert e["long_pairs"] % r["slots"] != 0, (name, homo, form)
            one = s.expected("one", homo)
            assert (one["long_pairs"], one["long_host_pairs"]) == (1, 0)
        # step counts n + K - 1 of the plain call at the edges of the 16-step blocks
        K = K_PLAIN[name]
        assert {n + K - 1 for n in s.seg_lens if n > 0} >= {32, 33, 48}
        # the exact boundaries, in both forms: q* against L0 is the device's, q* + 1 the host's; 8192 / 8193 symbols
        assert not splits(s.qstar, s.L0) and splits(s.qstar + 1, s.L0)
        _, _, _, pt, sl = s.call("pair")
        at = {(q, len(s.templates[t])) for q, t in zip(sl, pt)}
        assert {(s.qstar, s.L0), (s.qstar + 1, s.L0), (s.L0, s.L0)} <= at and len(sl) % 4 != 0
        assert abs(sl[0] - sl[1]) >= QCAP and sl[:4] == [0, QCAP + 1, 1, QCAP]   # neighbours differ maximally in length
        # the compressed k9 call (384 bp: the short route) holds the 8193-symbol segment: declined as a whole
        if name == "k9":
            for form in FORMS:
                assert s.expected(form, True) == dict(dict.fromkeys(COUNT_KEYS, 0), declined_calls=1)
            assert s.expected("one", True) == dict(dict.fromkeys(COUNT_KEYS, 0), short_calls=1, short_pairs=1)
    assert ks == {9, 10, 12, 13, 16, 17, 18, 24, 27, 32}, ks
    assert lpp_eq == {16, 32}
    assert {0, 63} <= pads[9] and max(pads[9]) >= 64 * 8            # 576, 513 and 1 bp with K = 9
    assert 0 in pads[16] and 0 in pads[32] and max(pads[32]) >= 64 * 31
    # (256 compute units: an MI355X; the GPU test asserts the inequality with the count of the device it runs on)
    assert ROUNDS.route["K"] == 9 and ROUNDS.dev_pairs > 256 * ROUNDS.route["slots"] and ROUNDS.host_pairs > 0
    assert ROUNDS.rounds(256) == 2


check_cases()   # (0.3 s: a later change to synth cannot silently move a case off its edge)
