"""The --ed_thr prefilter, the parts that need no device: the oracle's infix DP against the reference's own edlib (the
recorded distances of tests/golden/hw_dist/pairs.json, and edlib called live where it was built), the reference side of
tests/test_gpu_prefilter.py (its cases reach the kernels and layouts they are named after, its rank computation), and the
read-back call sd_engine_filter_result (declared, exported, rejects a null engine)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import edlib_ref
import prefilter_cases as pc
from stringdecomposer_amd import lib


@pytest.fixture(scope="module")
def pairs():
    with open(os.path.join(GOLDEN, "hw_dist", "pairs.json")) as f:
        return json.load(f)["sets"]


def test_fixture_holds_every_boundary_length_and_is_what_the_generator_builds(pairs):
    assert [s["name"] for s in pairs] == [g for g, _ in pc.FIXTURE_GROUPS]
    assert sorted(len(t) for s in pairs for t in s["templates"]) == pc.FIXTURE_LENGTHS
    with_n = sum("N" in t for s in pairs for t in s["templates"])
    assert 10 <= with_n <= 15                                     # about half of the 25 templates
    for s, (name, tm, chunks) in zip(pairs, pc.fixture_sets()):
        assert s["templates"] == [t.decode() for t in tm], name
        assert s["chunks"] == [c.decode() for c in chunks], name
        d = np.array(s["dist"])
        assert d.shape == (len(chunks), len(tm))
        # the edges: an exact copy, a template with nothing in common with its chunk, a chunk of one base
        assert (d == 0).any() and (d == np.array([len(t) for t in tm])[None, :]).any(), name
        assert {1, 15, 16, 17, 31, 32, 33, 63, 64, 65} <= {len(c) for c in chunks}, name


def test_oracle_hw_distance_equals_recorded_edlib(oracle, pairs):
    n = 0
    for s in pairs:
        for c, row in zip(s["chunks"], s["dist"]):
            for t, d in zip(s["templates"], row):
                assert oracle.hw_edit_distance(t, c) == d, (s["name"], len(t), len(c), t[:60], c[:60])
                n += 1
    assert n >= 25 * 20


def test_edlib_ref_hw_equals_oracle_and_fixture(oracle, pairs):
    """edlib_ref.hw: the reference's edlib called live where oracle/_ref/libedlib.so exists (else the oracle itself)."""
    assert edlib_ref.hw(b"ACGT", b"TTACGTTT") == 0
    assert edlib_ref.hw(b"ACGT", b"NNNN") == 4
    assert edlib_ref.hw(b"ANGT", b"CCANGTCC") == 0                # N against N is a match
    assert edlib_ref.hw(b"ACGT", b"A") == 3
    for s in pairs:
        for c, row in list(zip(s["chunks"], s["dist"]))[::3]:
            for t, d in zip(s["templates"], row):
                assert edlib_ref.hw(t, c) == d == oracle.hw_edit_distance(t, c), (s["name"], len(t), len(c))


def test_rank_matrix_is_the_reference_filter():
    """main.cpp:135-149 on small hand-made rows: ties go to the smaller index, the first is kept whatever its distance."""
    D = pc.DROPPED
    d = np.array([[3, 1, 1, 5], [7, 7, 7, 7], [2, 9, 0, 2]], dtype=np.int32)
    assert pc.rank_matrix(d, 0).tolist() == [[D, 0, D, D], [0, D, D, D], [D, D, 0, D]]
    assert pc.rank_matrix(d, 1).tolist() == [[D, 0, 1, D], [0, D, D, D], [D, D, 0, D]]
    assert pc.rank_matrix(d, 2).tolist() == [[D, 0, 1, D], [0, D, D, D], [1, D, 0, 2]]
    assert pc.rank_matrix(d, 7).tolist() == [[2, 0, 1, 3], [0, 1, 2, 3], [1, D, 0, 2]]
    assert pc.mid_threshold(np.array([[0, 1, 5, 6, 9, 10, 20]])) == 9   # the median 6 has no 7 beside it
    assert pc.thresholds(np.array([[0, 1, 5, 6, 9, 10, 20]])) == [0, 9, 20]


@pytest.mark.parametrize("case", pc.CASES, ids=[c.name for c in pc.CASES])
def test_cases_reach_their_kernels_and_layouts(oracle, case):
    """Every case of the GPU file, on the host: its reference matrix does not degenerate (an exact hit, a full-length
    distance, many values, adjacent values around the middle threshold), its lengths select the instantiation it is named
    after, and the layout plan is the one its rank form belongs to -- a change of the plan shows here first."""
    ms, tm, reads, part, chunks, dist, thrs = case.reference()
    assert len(chunks) <= 40 and len(tm) == 2 * len(ms)
    assert tm[0] == tm[len(ms) - 1] and tm[1] == tm[len(ms) + 1]          # the monomer held twice, the palindrome
    assert any(len(set(row)) < len(row) for row in dist.tolist())         # ties that only the index resolves
    for thr in thrs:
        kept = (pc.rank_matrix(dist, thr) != pc.DROPPED).sum(axis=1)
        assert kept.min() >= 1
    if not case.mid_only:
        assert thrs[0] == 0 and thrs[-1] == dist.max() and len(thrs) >= 3
        v = thrs[-2]
        assert (dist == v).any() and (dist == v + 1).any() and v >= np.median(dist)
    if case.reads_kind == "edges":
        assert {1, 15, 16, 17, 31, 32, 33, 63, 64, 65} <= {len(c) for c in chunks}
        assert len(chunks) > len(reads)                                   # chunks that do not start a read
    pi = lib.plan_info(ms, ed_thr=thrs[-1], part_size=part, overlap=pc.OVERLAP)
    assert (pi["family"], pi["cells"]) == case.plan
    for _, kw, kernel, form in case.variants:
        assert pc.kernel_of(tm, kw.get("flags", 0)) == kernel
        if form == "compacted":
            assert pi["waves"] > 1 and pi["cells"].startswith("f16/bf8-codes") and not kw.get("flags", 0) & lib.FLAG_NO_EDTHR_COMPACT
    if case.name in pc.MASK_CASES:
        assert all(len(tm) > pc.lds_templates(k) for _, _, k, _ in case.variants)


def test_filter_result_declared_exported_and_callable():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert "sd_engine_filter_result" in set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", hdr))
    assert "sd_engine_filter_result" in lib.EXPORTS
    assert callable(L.sd_engine_filter_result)
    assert callable(lib.Engine.filter_result)


def test_filter_result_of_a_null_engine_is_a_param_error():
    L = lib.load()
    err = C.create_string_buffer(256)
    dist = (C.c_int32 * 4)(7, 7, 7, 7)
    rank = (C.c_uint16 * 4)(9, 9, 9, 9)
    n, t = C.c_int64(-5), C.c_int32(-5)
    assert L.sd_engine_filter_result(None, dist, rank, 4, C.byref(n), C.byref(t), err, 256) == lib.SD_ERR_PARAM
    assert L.sd_engine_filter_result(None, None, None, 0, None, None, None, 0) == lib.SD_ERR_PARAM
    assert list(dist) == [7] * 4 and list(rank) == [9] * 4 and (n.value, t.value) == (-5, -5)   # nothing touched
