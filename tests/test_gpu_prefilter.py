"""The --ed_thr prefilter's own numbers (csrc/sd_filter.hip), read back with sd_engine_filter_result: every distance of
sd_hw_dist<W> / sd_hw_dist_u<W, HI> against the oracle's exact infix DP, element for element, and the rank sd_rank_keep
derives from them -- in each of its three forms: rank table, per-lane constants, compacted kept list -- against the
filtered order computed in Python from the oracle's matrix.  The tests of final rows (test_ed_thr_* in test_gpu_parity.py)
see a wrong distance only where it moves a template that wins a row across the threshold.

Cases (tests/prefilter_cases.py: CASES), each with thresholds taken from the oracle's matrix (0, its minimum, a middle
value v with v + 1 present, its maximum), one engine per threshold; every set holds one monomer twice and one
reverse-palindromic monomer, so equal distances occur in every chunk:

  case            distance kernel as planned (second run)                          sd_rank_keep form read back
  u1_lo .. u4_hi  sd_hw_dist_u<1..4, lo|hi>  (FLAG_FILTER_GENERAL: sd_hw_dist<1..4>)  per-lane constants
  g4_mixed        sd_hw_dist<4>, 1 .. 256 bp: short templates stop before the last    per-lane constants
                  word                       (KERNEL_GENERIC: the same kernel)         (rank table)
  g8_mixed        sd_hw_dist<8>, 1 .. 512 bp                  (KERNEL_GENERIC)         per-lane constants (rank table)
  g16_mixed       sd_hw_dist<16>, 65 .. 1024 bp               (KERNEL_GENERIC)         per-lane constants, tiled (rank table)
  g32_mixed       sd_hw_dist<32>, 128 .. 2048 bp              (KERNEL_GENERIC)         per-lane constants, tiled (rank table)
  lds_window_260  sd_hw_dist_u<3, hi>, T = 260: the rotating window of 256 templates'  kept list
                  masks in LDS               (FLAG_NO_EDTHR_COMPACT: the same kernel)  (per-lane constants, 3 waves)
  masks_w3_560    sd_hw_dist<3> by FLAG_FILTER_GENERAL, T = 560 > 546 masks in LDS     kept list
  masks_w8_208    sd_hw_dist<8>,  T = 208 > 204: lanes on global masks beside lanes   kept list, tiled layout
  masks_w16_104   sd_hw_dist<16>, T = 104 > 102     on LDS                             kept list, tiled layout
  masks_w32_52    sd_hw_dist<32>, T = 52 > 51                                          kept list, tiled layout
  tiled_30x342    sd_hw_dist<8>, the middle threshold only   (FLAG_NO_EDTHR_COMPACT)   kept list, tiled (per-lane constants,
                                                                                       every lane of a template, 2 waves)
  fixture         sd_hw_dist<8 / 16 / 32> against the reference's own edlib: tests/golden/hw_dist/pairs.json
  guard trip      u3_hi, lds_window_260, tiled_30x342 with a guard limit any input exceeds: the tables of the repeated run

Found when the file was first run on an MI355X: no mismatch.  That the file can fail was checked on scratch builds: with the
last column left out of `best` in sd_hw_dist, every run of the general kernel and the three fixture sets fail; the same in
sd_hw_dist_u fails the ten uniform runs (smallest pair: a 1-bp chunk against a 2-bp template); the other half of the last
word (HI flipped) fails the high-half sets (u1_hi .. u4_hi, lds_window_260) -- in the low half it is no fault: the rows
behind a template's end match nothing, so row m + 32 has the same minimum over the columns as row m.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import prefilter_cases as pc
from stringdecomposer_amd import lib

pytestmark = pytest.mark.gpu

COMPACTING = ("f16/bf8-codes x waves", "f16/bf8-codes tiled x waves")


def _filter_run(ms, reads, thr, part, **kw):
    """Engine -> load -> run -> fetch -> filter_result: (dist, rank, Engine.info())."""
    e = lib.Engine(ms, ed_thr=thr, part_size=part, overlap=pc.OVERLAP, threads=8, **kw)
    try:
        e.load_reads(reads)
        e.run()
        e.fetch()
        dist, rank = e.filter_result()
        return dist, rank, e.info()
    finally:
        e.close()


def _assert_matrix(got, exp, tm, chunks, what):
    """Element for element; a mismatch is reported with its smallest pair (template length x chunk length)."""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    if len(bad):
        c, j = min(bad.tolist(), key=lambda x: (len(tm[x[1]]) * len(chunks[x[0]]), x))
        pytest.fail("%s: %d of %d entries differ; smallest pair: chunk %d (%d bp) x template %d (%d bp): device %d, reference %d"
                    "\ntemplate %r\nchunk %r" % (what, len(bad), exp.size, c, len(chunks[c]), j, len(tm[j]), int(got[c, j]),
                                                int(exp[c, j]), tm[j][:80], chunks[c][:80]))


def _assert_plan(info, case, kw, form, what):
    """Which family and layout ran, and with it which of sd_rank_keep's forms filter_result decoded."""
    if kw.get("kernel") == lib.KERNEL_GENERIC:
        assert info["family"] == "generic" and form == "generic", (what, info)
        return
    assert (info["family"], info["cells"]) == case.plan, (what, info)
    compacted = info["cells"] in COMPACTING and lib.plan_info(case.reference()[0], ed_thr=0)["waves"] > 1 and \
        not kw.get("flags", 0) & lib.FLAG_NO_EDTHR_COMPACT
    assert form == ("compacted" if compacted else "ranked"), (what, info)


@pytest.mark.parametrize("case,variant", pc.case_variants(), ids=["%s-%s" % (c.name, v[0]) for c, v in pc.case_variants()])
def test_prefilter_distances_and_ranks_vs_exact_dp(oracle, case, variant):
    _, kw, kernel, form = variant
    ms, tm, reads, part, chunks, ref, thrs = case.reference()
    assert pc.kernel_of(tm, kw.get("flags", 0)) == kernel
    if case.name in pc.MASK_CASES:
        assert len(tm) > pc.lds_templates(kernel)
    if case.name == "lds_window_260":
        assert len(tm) >= 256 and (len(chunks) * len(tm)) % 256 != 0
    mn = ["m%d" % j for j in range(len(ms))]
    rn = ["r%d" % i for i in range(len(reads))]
    for thr in thrs:
        what = "%s/%s ed_thr=%d" % (case.name, variant[0], thr)
        t0 = lib.guard_trips()
        dist, rank, info = _filter_run(ms, reads, thr, part, **kw)
        assert info["n_chunks"] == len(chunks), what
        _assert_plan(info, case, kw, form, what)
        assert lib.guard_trips() == t0, what      # the tables are those of the planned layout, not of a repeat
        _assert_matrix(dist, ref, tm, chunks, what + " distances")
        _assert_matrix(rank, pc.rank_matrix(ref, thr), tm, chunks, what + " ranks")
        exp = case.rows(oracle, thr)
        got = lib.decompose(rn, reads, mn, ms, part_size=part, overlap=pc.OVERLAP, ed_thr=thr, threads=8, **kw)
        assert got == exp, what + " rows"


def _fixture():
    with open(os.path.join(GOLDEN, "hw_dist", "pairs.json")) as f:
        return json.load(f)["sets"]


@pytest.mark.parametrize("group", [g for g, _ in pc.FIXTURE_GROUPS])
def test_prefilter_distances_vs_recorded_edlib(group):
    """The device distance of every (template, chunk) pair of the fixture equals what the reference's edlib gave (HW mode,
    k = -1): one template of each length at a word boundary, 1 .. 2048 bp, grouped by mask layout."""
    s = [x for x in _fixture() if x["name"] == group][0]
    tm = [t.encode() for t in s["templates"]]
    chunks = [c.encode() for c in s["chunks"]]
    exp = np.array(s["dist"], dtype=np.int32)
    assert exp.shape == (len(chunks), len(tm))
    dist, _, info = _filter_run(tm, chunks, 0, max(len(c) for c in chunks))
    assert info["n_chunks"] == len(chunks) and info["n_templates"] == 2 * len(tm)
    _assert_matrix(dist[:, :len(tm)], exp, tm, chunks, "fixture " + group)


@pytest.mark.parametrize("name", ["u3_hi", "lds_window_260", "tiled_30x342"])
def test_filter_result_after_a_guard_trip_is_that_of_the_repeated_run(name):
    """A guard limit any input exceeds (sd_params.reserved[2], the test hook): the engine repeats the batch under another
    plan -- integer cells, or the generic family -- and the rows fetched are the repeat's.  So are the tables read back:
    decoded by the form the repeat wrote, equal to the reference."""
    case = [c for c in pc.CASES if c.name == name][0]
    ms, tm, reads, part, chunks, ref, _ = case.reference()
    thr = pc.mid_threshold(ref)
    t0 = lib.guard_trips()
    dist, rank, info = _filter_run(ms, reads, thr, part, f16_guard=40)
    assert lib.guard_trips() > t0
    assert (info["family"], info["cells"]) != case.plan, info
    _assert_matrix(dist, ref, tm, chunks, name + " distances after the repeat")
    _assert_matrix(rank, pc.rank_matrix(ref, thr), tm, chunks, name + " ranks after the repeat")
