"""The narrow u16 fill with its slot loop as two runs -- every slot's add, in place in the table registers, then the
maximum chain (sd_fast_fill, SLOT_RUNS): the rows of the fast family equal the oracle's on every kernel that compiles
from that loop and on the u16 kernels that keep the skewed one.

Six template sets: the benchmark's (P = 35, the floors in groups of 4), monomers of about 230 bp (P >= 42, the fl_long
kernels), of about 100 bp (P < 30, sd_fast_u16.hip), five monomers (10 templates: idle planes and idle lanes) of 171 bp
(P = 16) and of 400 bp (P = 35: the two runs again) and a set with a 1-bp template (ONE: a start lane that ends in
slot 0).  At most 8 reads of 300-3000 bp built so that the row maximum grows by the largest table value in every row
(exact copies) and then meets another symbol, with two-letter and homopolymer stretches and an N in front of bases; one
chunk per read (rebases at rows 128 and 256, a checkpoint every 32 rows, the B flush at row 64) and chunks of 333 rows
for many rows right behind a row 0; with and without --ed_thr.

Every (set, scoring) pair below plans u16 cells in the fast family (asserted, never skipped): none had to be dropped."""
import os

import pytest

from stringdecomposer_amd import lib, synth

pytestmark = pytest.mark.gpu

SCORINGS = [(-1, -1, -1, 1), (-2, -3, -4, 2), (-1, -1, -3, 1), (-1, -2, -5, 2), (1, -1, -1, 1)]   # (ins, del, mismatch, match)
_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def _with_one_bp():
    mn, ms = synth.make_monomers(11, seed=4)
    return list(mn) + ["one"], list(ms) + [b"G"]


# name -> (monomers, what plan_info's cells_per_lane must be)
SETS = {
    "bench12": (lambda: synth.make_monomers(12, seed=1), lambda p: p == 35),
    "long230": (lambda: synth.make_monomers(12, seed=5, length=230), lambda p: p >= 42),
    "short100": (lambda: synth.make_monomers(12, seed=7, length=100), lambda p: p < 30),
    "five": (lambda: synth.make_monomers(5, seed=2), lambda p: p < 30),
    "five400": (lambda: synth.make_monomers(5, seed=2, length=400), lambda p: 30 <= p <= 40),
    "one_bp": (_with_one_bp, lambda p: p >= 30),
}


def _reads(ms):
    clean = [m.replace(b"N", b"A") for m in ms if len(m) >= 20]
    k = len(clean)
    st = synth.Stream(31, 4)
    two = lambda n, a: bytes(a[int(x)] for x in st.below(n, 2))
    _, rs = synth.make_reads(clean, 2, read_len=1500, seed=29)                                  # mutated monomer concatenations
    rs = list(rs)
    rs.append((clean[0] * 9)[:700] + b"T" * 60 + (clean[5 % k] * 5)[:500] + b"G" + clean[2] * 2)   # exact copies, then another symbol
    rs.append(((clean[3][::-1].translate(_RC) * 9)[:800] + b"C" * 40 + clean[4] * 3)[:1600])    # the same on a reverse complement
    rs.append(b"AC" * 100 + b"GT" * 100 + two(400, b"AG") + b"TA" * 80 + two(300, b"CT") + clean[3])
    rs.append(b"A" * 150 + clean[1] + b"C" * 150 + clean[4] + b"G" * 150 + clean[2] + b"T" * 150 + clean[0] + b"A" * 70)
    n_each = b"".join(b"N" + b + clean[j % k][:40] + b"NN" + b * 3 + clean[j % k][40:] for j, b in enumerate([b"A", b"C", b"G", b"T"] * 2))
    rs.append(n_each[:1800])
    rs.append((clean[1] * 2)[:150] + b"N" + (clean[2] * 2)[:160])                                         # a short read: fewer than 333 rows
    assert len(rs) <= 8 and all(300 <= len(r) <= 3000 for r in rs), [len(r) for r in rs]
    return ["r%d" % i for i in range(len(rs))], rs


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (make, _) in SETS.items():
        mn, ms = make()
        out[name] = (mn, ms) + _reads(ms)
    return out


@pytest.mark.parametrize("sc", SCORINGS)
@pytest.mark.parametrize("which", list(SETS))
def test_fast_rows_equal_the_oracle(oracle, cases, which, sc):
    mn, ms, rn, rs = cases[which]
    info = lib.plan_info(ms, scoring=sc)
    assert (info["family"], info["cells"]) == ("fast", "u16"), info
    assert SETS[which][1](info["cells_per_lane"]), info
    thr = min(16, os.cpu_count() or 1)
    for ed, part, ov in ((-1, 5000, 500), (35, 5000, 500), (-1, 333, 77), (35, 333, 77)):
        exp = oracle.decompose(rn, rs, mn, ms, threads=thr, sc=sc, ed_thr=ed, part=part, overlap=ov)
        got = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc, ed_thr=ed, part_size=part, overlap=ov)
        assert exp.count(b"\n") >= len(rs)   # (a scoring that rewards insertions gives one row per read)
        assert got == exp, (which, sc, ed, part)
