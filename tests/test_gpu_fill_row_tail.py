"""The row tail of the narrow fill (sd_fast_fill).  In the u16 kernels with floors in place the first crossbar trip of the
carry scan goes out before the next row's table reads, the wave maximum runs while LDS works, the next row's read symbol is
decoded ahead of the slot loop, and the sums of the slots behind the floor groups are made in the tail of the row before
(moved with the cells by a rebase); the other kernels keep their order.  The rows of the fast family equal the oracle's.

* Chunk lengths around every boundary of the row loop -- the 32-row group, the 64-row B flush, the 128-row rebase: one read
  per length, one chunk per read, and chunks of 333 + 77 rows for such lengths behind a row 0; in the default form, the
  DPP scan (SD_FILL_DPP_SCAN=1) and with the crossbar scan kept in a launch's last round (SD_FILL_BPERM_TAIL=1).
* Exact monomer copies (the row maximum grows by the largest table value in every row: large rebase shifts), then another
  symbol and N runs, under three scorings.
* The kernels whose order of work stays: fp16 cells (whose plan takes the 64-row rebase where the scoring asks for it),
  the one-level u16 kernels (also with a negative table value), a 1-bp template, --ed_thr, P = 30 and P = 40."""
import contextlib
import os

import pytest

from stringdecomposer_amd import lib, synth

pytestmark = pytest.mark.gpu

DEFAULT, WIDE, REWARD_INS, NEG_TABLE = (-1, -1, -1, 1), (-2, -3, -4, 2), (1, -1, -1, 1), (-1, -1, -3, 1)   # (ins, del, mismatch, match)
LENGTHS = [1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258, 410]
FORMS = {"default": {}, "dpp_scan": {"SD_FILL_DPP_SCAN": "1"}, "bperm_tail": {"SD_FILL_BPERM_TAIL": "1"}}
SETTINGS = ((5000, 500), (333, 77))   # (part_size, overlap): one chunk per read; many rows right behind a row 0


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _length_reads(ms):
    """One read per length of LENGTHS, cut out of mutated monomer concatenations at different places, and four reads whose
    333-row parts end in chunks of 410, 333 + k and a few rows."""
    _, long_ = synth.make_reads(ms, 3, read_len=2600, seed=41)
    rs = [long_[j % 3][37 * j: 37 * j + n] for j, n in enumerate(LENGTHS)]
    rs += [long_[0][:743], long_[1][:999], long_[2][:1064], long_[0][100:100 + 1397]]
    return ["r%d" % i for i in range(len(rs))], rs


def _copy_reads(ms):
    """Exact copies, then a change of symbol; N runs inside and between the copies."""
    rs = [ms[0] * 4 + b"T" * 40 + ms[5] * 3 + b"G" + ms[2] * 2,
          ms[7] * 3 + b"N" * 5 + ms[7] * 3 + b"C" * 33 + ms[9][:90] + b"NNN" + ms[9][90:] + ms[9] * 2,
          (ms[3] * 9)[:1290],
          ms[1][:64] * 2 + ms[1] * 2 + b"N" + ms[4] * 2]
    assert all(300 <= len(r) <= 1800 for r in rs), [len(r) for r in rs]
    return ["c%d" % i for i in range(len(rs))], rs


class _Oracle:
    """The oracle's rows of a job, computed once and handed out unchanged."""

    def __init__(self, binding):
        self.binding, self.seen = binding, {}

    def rows(self, key, rn, rs, mn, ms, sc, ed, part, ov):
        k = (key, sc, ed, part, ov)
        if k not in self.seen:
            self.seen[k] = self.binding.decompose(rn, rs, mn, ms, threads=min(16, os.cpu_count() or 1), sc=sc, ed_thr=ed, part=part, overlap=ov)
        return self.seen[k]


@pytest.fixture(scope="module")
def expected(oracle):
    return _Oracle(oracle)


@pytest.fixture(scope="module")
def bench12():
    mn, ms = synth.make_monomers(12, seed=1)
    info, lev = lib.plan_info(ms), lib.plan_floor_levels(ms)
    # P = 35, the largest floor group 16, four levels: 18 sums are made ahead
    assert (info["family"], info["cells"], info["cells_per_lane"], info["floor_slots"]) == ("fast", "u16", 35, 16), info
    assert lev["pair_rule"] and len({v for row in lev["floor_pair"] for v in row}) >= 4, lev
    return mn, ms


def _check(expected, key, rn, rs, mn, ms, sc=DEFAULT, ed=-1, settings=SETTINGS):
    for part, ov in settings:
        exp = expected.rows(key, rn, rs, mn, ms, sc, ed, part, ov)
        got = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc, ed_thr=ed, part_size=part, overlap=ov)
        assert exp.count(b"\n") >= len(rs)
        assert got == exp, (key, sc, ed, part, ov)


@pytest.mark.parametrize("form", list(FORMS))
def test_chunk_lengths_around_the_row_loops_boundaries(expected, bench12, form):
    mn, ms = bench12
    rn, rs = _length_reads(ms)
    assert [len(r) for r in rs[:len(LENGTHS)]] == LENGTHS
    with _env(**FORMS[form]):
        _check(expected, "lengths", rn, rs, mn, ms)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("sc", [DEFAULT, WIDE, REWARD_INS])
def test_sums_made_ahead_move_with_a_rebase(expected, bench12, sc, form):
    mn, ms = bench12
    info = lib.plan_info(ms, scoring=sc)
    assert (info["family"], info["cells"], info["cells_per_lane"]) == ("fast", "u16", 35) and info["rebase"] in (64, 128), info
    # floors in place, i.e. the kernels that make sums ahead, where no table value is negative (1,-1,-1,1 has one: mismatch
    # - del - ins = -1, so the one-level kernels run, whose order of adds stays)
    assert lib.plan_floor_levels(ms, scoring=sc)["pair_rule"] == (sc != REWARD_INS)
    rn, rs = _copy_reads(ms)
    with _env(**FORMS[form]):
        _check(expected, "copies", rn, rs, mn, ms, sc=sc)


def _one_bp():
    mn, ms = synth.make_monomers(11, seed=4)
    return list(mn) + ["one"], list(ms) + [b"G"]


# name -> (monomers, cells per lane, scoring, ed_thr, developer switches)
UNCHANGED = {
    "f16": (lambda: synth.make_monomers(12, seed=1), 35, DEFAULT, -1, {"SD_FILL_CELLS": "f16"}),
    "f16_wide_scoring": (lambda: synth.make_monomers(12, seed=1), 35, WIDE, -1, {"SD_FILL_CELLS": "f16"}),   # (rebase 64 where the plan takes it)
    "f16_dpp_scan": (lambda: synth.make_monomers(12, seed=1), 35, DEFAULT, -1, {"SD_FILL_CELLS": "f16", "SD_FILL_DPP_SCAN": "1"}),
    "one_level": (lambda: synth.make_monomers(12, seed=1), 35, DEFAULT, -1, {"SD_FILL_ONE_LEVEL": "1"}),
    "negative_table_value": (lambda: synth.make_monomers(12, seed=1), 35, NEG_TABLE, -1, {}),
    "one_bp": (_one_bp, 35, DEFAULT, -1, {}),
    "one_bp_wide_scoring": (_one_bp, 35, WIDE, -1, {}),
    "ed_thr": (lambda: synth.make_monomers(12, seed=1), 35, DEFAULT, 35, {}),
    "ed_thr_dpp_scan": (lambda: synth.make_monomers(12, seed=1), 35, DEFAULT, 35, {"SD_FILL_DPP_SCAN": "1"}),
    "p30": (lambda: synth.make_monomers(12, seed=6, length=146), 30, DEFAULT, -1, {}),
    "p40": (lambda: synth.make_monomers(12, seed=8, length=194), 40, DEFAULT, -1, {}),
    "p40_wide_scoring": (lambda: synth.make_monomers(12, seed=8, length=194), 40, WIDE, -1, {}),
}


@pytest.mark.parametrize("which", list(UNCHANGED))
def test_other_kernels_of_the_row_loop(expected, which):
    make, p, sc, ed, switches = UNCHANGED[which]
    mn, ms = make()
    info = lib.plan_info(ms, scoring=sc)
    assert (info["family"], info["cells"], info["cells_per_lane"]) == ("fast", "u16", p), info   # (the plan before the switches)
    if which == "negative_table_value":
        assert not lib.plan_floor_levels(ms, scoring=sc)["pair_rule"]   # no floors in place: the one-level kernels
    clean = [m for m in ms if len(m) >= 20]
    rn, rs = _length_reads(clean)
    cn, cs = _copy_reads(clean)
    rn, rs = rn[::3] + cn, rs[::3] + cs   # lengths 1, 31, 34, 65, 128, 255, 258, a 333-row split, and the copies
    with _env(**switches):
        _check(expected, which, rn, rs, mn, ms, sc=sc, ed=ed)
