"""Identity against lag (--lags) without a device: the host form (sd_lag_segments) against the Python fold of
tests/lag_ref.py, the period rule, the two file formats, and the refusals that need no GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lag_cases
import lag_ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
NEW = ["sd_lag_segments", "sd_lag_segments_dev", "sd_lag_final_dev", "sd_lag_final_host", "sd_lag_identities", "sd_lag_periods",
       "sd_lag_kernel_bench"]


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.LAG_DMAX == 255


@pytest.mark.parametrize("D", [1, 3, 255])
def test_host_form_equals_the_reference_fold(D):
    """groups of 0, 1, 2, D, D + 1 and 3 D rows; the pool holds segments with N, an exact duplicate, 1-bp segments, a
    513-bp and a 1025-bp segment and a byte outside ACGTN"""
    pool = lag_cases.pool(extra_byte="R")
    sizes = [0, 1, 2, D, D + 1, 3 * D]
    groups = lag_cases.pooled_groups(sizes, pool, seed=D)
    flat = [s for g in groups for s in g]
    if D == 255:   # every special row is drawn somewhere (the small cases: see the next test)
        assert {513, 1025, 1} <= {len(s) for s in flat} and any("N" in s for s in flat) and any("R" in s for s in flat)
        assert any(a == b for g in groups for a, b in zip(g, g[1:]))
    text, st, en, off = lag_cases.layout(groups, seed=D)
    got = lib.lag_segments(text, st, en, off, D, threads=4)
    assert got.dist.shape == got.matches.shape == (len(st), D) and got.sums.shape == (len(sizes), D, 3)
    lag_ref.same(got, lag_ref.segments(text, st, en, off, D))
    # what a group of n rows must look like: row x has partners at lags 1 .. n - 1 - x only
    for g, n in enumerate(sizes):
        for x in range(n):
            have = min(D, n - 1 - x)
            row = got.dist[off[g] + x]
            assert (row[:have] >= 0).all() and (row[have:] == -1).all() and not got.matches[off[g] + x][have:].any()
        assert [int(v) for v in got.sums[g, :, 0]] == [max(0, n - d) for d in range(1, D + 1)]
    assert (got.dist != -2).all()
    # one thread, the same bytes
    one = lib.lag_segments(text, st, en, off, D, threads=1)
    assert (one.dist == got.dist).all() and (one.matches == got.matches).all() and (one.sums == got.sums).all()


def test_the_special_rows_as_query_and_as_target():
    """each special segment next to an ordinary one, in both roles, at D = 2; an empty segment has no alignment"""
    pool = lag_cases.pool(extra_byte="R")
    unit = pool[0]
    special = [s for s in pool if len(s) in (1, 9, 513, 1025) or "N" in s or "R" in s] + [""]
    groups = [[unit, s, unit, s, s] for s in special]
    text, st, en, off = lag_cases.layout(groups, seed=5)
    got = lib.lag_segments(text, st, en, off, 2, threads=4)
    ref = lag_ref.segments(text, st, en, off, 2)
    lag_ref.same(got, ref)
    g = len(special) - 1   # the empty segment: dist -1 although the partner exists, and no pair counted
    assert got.dist[off[g]].tolist() == [-1, 0] and got.dist[off[g] + 1].tolist() == [-1, -1]
    assert got.sums[g, :, 0].tolist() == [0, 1]
    # identical neighbours: distance 0, every column a match
    i = off[0] + 3
    assert got.dist[i][0] == 0 and got.matches[i][0] == len(special[0])


def test_no_pair_across_a_group_boundary():
    pool = lag_cases.pool()
    rows = lag_cases.pooled_groups([12], pool, seed=3)[0]
    D = 4
    one = lag_cases.layout([rows], seed=1)
    cut = lag_cases.layout([rows[:5], rows[5:6], [], rows[6:]], seed=1)
    assert one[:3] == cut[:3]   # the same text and segments, other groups
    a = lib.lag_segments(*one, D)
    b = lib.lag_segments(*cut, D)
    lag_ref.same(b, lag_ref.segments(*cut, D))
    for first, n in ((0, 5), (5, 1), (6, 6)):
        for x in range(n):
            have = min(D, n - 1 - x)
            assert (b.dist[first + x][:have] == a.dist[first + x][:have]).all()
            assert (b.dist[first + x][have:] == -1).all() and (a.dist[first + x][:min(D, 11 - first - x)] >= 0).all()
    assert b.sums[:, :, 0].tolist() == [[4, 3, 2, 1], [0, 0, 0, 0], [0, 0, 0, 0], [5, 4, 3, 2]]
    # group offsets that do not cover the segments are refused
    for off in ([0, 5], [1, 12], [0, 7, 5, 12]):
        with pytest.raises(lib.SdError) as e:
            lib.lag_segments(one[0], one[1], one[2], off, D)
        assert e.value.code == lib.SD_ERR_PARAM


def test_period_rule():
    assert formats.lag_period([[0, 0, 0]] * 4) == 0 == lag_ref.period([[0, 0, 0]] * 4)
    cases = [
        ([[3, 50, 100], [2, 100, 200], [1, 1, 2]], 1),                     # an exact tie: the smallest lag
        ([[3, 50, 100], [0, 0, 0], [1, 51, 100]], 3),
        ([[0, 0, 0], [2, 99, 100], [1, 99, 100]], 2),                      # lags without pairs do not count
        ([[5, 10 ** 17, 3 * 10 ** 17], [5, 10 ** 17 + 1, 3 * 10 ** 17]], 2),   # doubles cannot tell these apart
        ([[5, 10 ** 17 + 1, 3 * 10 ** 17], [5, 10 ** 17, 3 * 10 ** 17]], 1),
        ([[1, 2 ** 62 - 1, 2 ** 62], [1, 2 ** 62 - 2, 2 ** 62 - 1]], 1),       # (2^62 - 1)^2 > 2^62 (2^62 - 2): 128-bit products
    ]
    a, b = cases[3][0]
    assert float(a[1]) / float(a[2]) >= float(b[1]) / float(b[2])   # in floating point lag 1 would keep the tie
    for sums, want in cases:
        assert lag_ref.period(sums) == want
        assert formats.lag_period(sums) == want
        period, pooled = lib.lag_periods(np.asarray([sums], dtype=np.int64))
        assert period.tolist() == [want]
        assert pooled[0].tolist() == [lag_ref.identity(c - m, m) if n else -1.0 for n, m, c in sums]
    assert formats.lag_period(np.asarray([c[0][:2] for c in cases[:2]], dtype=np.int64)) == [1, 1]


def test_identities_are_the_identity_columns_arithmetic():
    d = np.asarray([[-1, 0, 3, 17, 1, -2]], dtype=np.int32)
    m = np.asarray([[0, 171, 168, 154, 2, 0]], dtype=np.int32)
    got = lib.lag_identities(d, m)[0].tolist()
    assert got == [lag_ref.identity(a, b) for a, b in zip(d[0].tolist(), m[0].tolist())]
    assert got[0] == -1.0 and got[1] == 100.0 and got[5] == -1.0 and got[4] == 2 / 3 * 100


def test_formats_round_trip(tmp_path):
    pool = lag_cases.pool()
    groups = lag_cases.pooled_groups([7, 1, 0, 4], pool, seed=8)
    text, st, en, off = lag_cases.layout(groups, seed=8)
    lags = lib.lag_segments(text, st, en, off, 3)
    names = ["read_%d" % g for g in range(4) for _ in groups[g]]
    ident = lib.lag_identities(lags.dist, lags.matches).tolist()
    period, pooled = lib.lag_periods(lags.sums)
    rows = [formats.LagRow(n, s, e, tuple(v)) for n, s, e, v in zip(names, st, en, ident)]
    per = [formats.PeriodRow("read_%d" % g, len(groups[g]), int(period[g]), tuple(pooled[g].tolist())) for g in range(4)]
    assert [p.period for p in per] == formats.lag_period(lags.sums) and per[2].period == 0
    a, b = str(tmp_path / "x_lags.tsv"), str(tmp_path / "x_period.tsv")
    formats.write_lags(a, rows)
    formats.write_periods(b, per)
    ta, tb = open(a).read(), open(b).read()
    assert ta.count("\n") == len(st) and tb.count("\n") == 4
    assert ta.splitlines()[6].endswith("\t-1.00\t-1.00\t-1.00") and tb.splitlines()[2] == "read_2\t0\t0\t-1.00\t-1.00\t-1.00"
    ra, rb = formats.read_lags(a), formats.read_periods(b)
    assert [(r.read, r.start, r.end) for r in ra] == [(r.read, r.start, r.end) for r in rows]
    assert [(p.read, p.rows, p.period) for p in rb] == [(p.read, p.rows, p.period) for p in per]
    assert formats.format_lags(ra) == ta and formats.format_periods(rb) == tb   # text -> rows -> the same text
    assert all(abs(x - y) <= 0.005 for r, q in zip(ra, rows) for x, y in zip(r.identities, q.identities))
    with open(a, "a") as f:
        f.write("read_9\t1\t2\t50.00\n")
    with pytest.raises(formats.FormatError):
        formats.read_lags(a)


@pytest.mark.parametrize("D", [0, 256, -1])
def test_d_out_of_range_is_refused(D):
    import ctypes as C
    for call in (lambda: lib.lag_segments("ACGT", [0], [3], [0, 1], D),
                 lambda: lib.lag_segments("ACGT", [0], [3], [0, 1], D, device=0),
                 lambda: lib.final_lags_host((np.zeros(0, dtype=lib.final_dtype()), None, None), [], D)):
        with pytest.raises(lib.SdError) as e:
            call()
        assert e.value.code == lib.SD_ERR_PARAM
    # the C entries themselves, before any device work (no device is needed to be refused)
    L = lib.load()
    z = np.zeros(8, dtype=np.int64)
    err = C.create_string_buffer(256)
    p = z.ctypes.data
    assert L.sd_lag_segments(b"ACGT", 4, p, p, 1, p, 1, D, 1, p, p, p) == lib.SD_ERR_PARAM
    assert L.sd_lag_segments_dev(b"ACGT", 4, p, p, 1, p, 1, D, 0, 1, p, p, p) == lib.SD_ERR_PARAM
    assert L.sd_lag_final_host(p, 0, b"ACGT", p, p, 0, D, 1, p, p, p) == lib.SD_ERR_PARAM
    assert L.sd_lag_final_dev(p, 0, p, p, p, 0, D, 0, None, p, p, p, (C.c_int64 * 3)(), err, 256) == lib.SD_ERR_PARAM
    assert b"D = " in err.value


@pytest.mark.parametrize("extra,word", [(["--lags", "4", "--records"], "--records"), (["--lags", "0"], "1 .. 255"),
                                        (["--lags", "256"], "1 .. 255")])
def test_cli_refusals_before_device_work(tmp_path, extra, word):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no device could be used: none is needed
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), os.path.join(TD, "read.fa"),
                        os.path.join(TD, "DXZ1_star_monomers.fa"), "-o", str(tmp_path / "out")] + extra,
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 2, p.stderr
    assert "--lags" in p.stderr and word in p.stderr
    assert not os.path.exists(str(tmp_path / "out" / "final_decomposition_raw.tsv"))


def test_final_lags_host_on_a_golden_final_tsv():
    """The rows of the reference's final TSV of tests/golden/test_data as final rows: segments clamped as the selection
    measured them, partners by the rows' read index."""
    fin = formats.read_final(os.path.join(TD, "final_decomposition_fc89af8.tsv"))[:60]
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    seq = rs[0].upper()
    rows = np.zeros(len(fin) + 2, dtype=lib.final_dtype())
    for i, r in enumerate(fin):
        rows[i]["read"], rows[i]["start"], rows[i]["end"] = 1, r.start, r.end
    rows[len(fin)]["read"], rows[len(fin)]["start"], rows[len(fin)]["end"] = 2, -5, 30             # clamped at 0
    rows[len(fin) + 1]["read"], rows[len(fin) + 1]["start"], rows[len(fin) + 1]["end"] = 2, 90, 400   # clamped at the read's end
    reads = [b"ACGT", seq, seq[:100]]
    got = lib.final_lags_host((rows, None, None), reads, 5, threads=4)
    text = b"".join(reads)
    base = [0, 4, 4 + len(seq)]
    st = [base[1] + r.start for r in fin] + [base[2], base[2] + 90]
    en = [base[1] + r.end for r in fin] + [base[2] + 30, base[2] + 99]
    ref = lag_ref.segments(text, st, en, [0, 0, len(fin), len(fin) + 2], 5)
    lag_ref.same(got, ref)
    assert got.sums[0].sum() == 0 and got.sums[1, 0, 0] == len(fin) - 1 and got.sums[2, :, 0].tolist() == [1, 0, 0, 0, 0]
