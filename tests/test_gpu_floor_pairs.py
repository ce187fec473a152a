"""The narrow u16 fill with the floor level of a row chosen by the previous and the current read symbol
(sd_fast_fill<..., FLS>, FastPlan::floor_pair): the rows of the default run, of the per-symbol levels
(SD_FILL_SYMBOL_LEVEL=1) and of one level for every row (SD_FILL_ONE_LEVEL=1) all equal the oracle's.

Two sets of 12 monomers of about 170 bp (P = 35, u16 cells): the synthetic benchmark set and one whose lanes meet a base late
or never.  Seven reads of 2-3 kb built to stress the rule: the row maximum growing by the largest table value in every row
(exact copies) and then a change of symbol, two-letter stretches, homopolymer runs, N in front of every base; one chunk per
read by default (rebases at rows 128, 256, ...), and chunks of 410 rows for many rows right behind a row 0."""
import os

import pytest

from stringdecomposer_amd import lib, synth

pytestmark = pytest.mark.gpu

SCORINGS = [(-1, -1, -1, 1), (-2, -3, -4, 2), (-1, -1, -3, 1), (-1, -2, -5, 2), (1, -1, -1, 1)]   # (ins, del, mismatch, match)
_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def _late_base_monomers():
    """Monomers whose lanes meet a base late or never: long homopolymer / two-letter prefixes, a base that is missing
    altogether, an N in the middle of a lane."""
    st = synth.Stream(77, 3)
    rnd = lambda n, alpha=b"ACGT": bytes(alpha[int(x)] for x in st.below(n, len(alpha)))
    ms = [b"A" * 19 + rnd(150), rnd(30, b"AT") + rnd(140), rnd(171, b"ACT"), rnd(20) + b"N" + rnd(150),
          rnd(165), b"ACGT" + rnd(166), rnd(60) + b"C" * 25 + rnd(90), rnd(175), rnd(168), rnd(172),
          rnd(33, b"GC") + rnd(140), rnd(170)]
    return ["m%d" % i for i in range(len(ms))], ms


def _sets():
    return {"synthetic12": synth.make_monomers(12, seed=1), "late_bases": _late_base_monomers()}


def _reads(ms):
    clean = [m.replace(b"N", b"A") for m in ms]
    st = synth.Stream(93, 4)
    two = lambda n, a: bytes(a[int(x)] for x in st.below(n, 2))
    _, rs = synth.make_reads(clean, 2, read_len=2500, seed=23)                       # mutated monomer concatenations
    rs = list(rs)
    rs.append(clean[0] * 7 + b"T" * 60 + clean[5] * 4 + b"G" + clean[2] * 3)          # exact copies, then another symbol
    rs.append((clean[7][::-1].translate(_RC) * 6 + b"C" * 40 + clean[9] * 6)[:2800])  # the same on a reverse complement
    rs.append(b"AC" * 200 + b"GT" * 200 + two(700, b"AG") + b"TA" * 150 + two(600, b"CT") + clean[3])
    rs.append(b"A" * 300 + clean[1] + b"C" * 300 + clean[4] + b"G" * 300 + clean[6] + b"T" * 300 + clean[8] + b"A" * 150)
    n_each = b"".join(b"N" + b + clean[k][:60] + b"NN" + b * 3 + clean[k][60:] for k, b in enumerate([b"A", b"C", b"G", b"T"] * 3))
    rs.append(n_each[:2900])
    assert len(rs) <= 8 and all(2000 <= len(r) <= 3000 for r in rs), [len(r) for r in rs]
    return ["r%d" % i for i in range(len(rs))], rs


def _three_ways(rn, rs, mn, ms, **kw):
    out = {"pair": lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, **kw)}
    for name, var in (("symbol", "SD_FILL_SYMBOL_LEVEL"), ("one", "SD_FILL_ONE_LEVEL")):
        os.environ[var] = "1"
        try:
            out[name] = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, **kw)
        finally:
            del os.environ[var]
    return out


@pytest.mark.parametrize("sc", SCORINGS)
@pytest.mark.parametrize("which", ["synthetic12", "late_bases"])
def test_rows_by_pair_by_symbol_and_one_level_equal_the_oracle(oracle, which, sc):
    mn, ms = _sets()[which]
    rn, rs = _reads(ms)
    info = lib.plan_info(ms, scoring=sc)
    assert (info["family"], info["cells"], info["cells_per_lane"]) == ("fast", "u16", 35), info
    lev = lib.plan_floor_levels(ms, scoring=sc)
    nonneg = min(sc[2], sc[3]) - sc[1] - sc[0] >= 0
    # a negative table value: no floors in place, the one-level kernels run (launch_fast_fill) and the pair levels are off
    assert lev["pair_rule"] == nonneg
    if nonneg:
        assert any(lev["floor_pair"][a][b] < lev["floor_sym"][b] for a in range(4) for b in range(4)), lev   # the rule has work to do
    else:
        assert all(row == lev["floor_sym"] for row in lev["floor_pair"])
    thr = min(16, os.cpu_count() or 1)
    for ed, part, ov in ((-1, 5000, 500), (35, 5000, 500), (-1, 333, 77)):
        exp = oracle.decompose(rn, rs, mn, ms, threads=thr, sc=sc, ed_thr=ed, part=part, overlap=ov)
        got = _three_ways(rn, rs, mn, ms, scoring=sc, ed_thr=ed, part_size=part, overlap=ov)
        for name in ("pair", "symbol", "one"):
            assert got[name] == exp, (which, sc, ed, part, name)
