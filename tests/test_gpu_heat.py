"""The binned all-against-all identities (--heatmap) on the device: the wave-per-(target, strip) kernel
(sd_heat_segments_dev) against the host form at the edges of strips, groups and bins and at every word class, the pairs it
hands to the host, its reduction on known sums, the device-resident chain (Stream(device_final=True) on DeviceReads ->
lib.final_heat_device) and the command line's file."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import heat_ref
import lag_cases
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8


def _dev_equals_host(text, st, en, off, B, W):
    dev = lib.heat_segments(text, st, en, off, B, W, device=0, threads=THREADS)
    host = lib.heat_segments(text, st, en, off, B, W, threads=THREADS)
    assert dev.cell_off.tolist() == host.cell_off.tolist() and dev.nb.tolist() == host.nb.tolist()
    bad = np.argwhere(dev.sums != host.sums)
    assert bad.size == 0, "first differing cell %d: %s on the device, %s on the host" % (
        bad[0][0], dev.sums[bad[0][0]].tolist(), host.sums[bad[0][0]].tolist())
    assert dev.classes == heat_ref.classes(text, st, en, off, W)
    return dev


@pytest.fixture(scope="module")
def edge_job():
    """groups of 1, 2, 63, 64, 65, 66, 129 and 130 rows: groups start in the middle of a strip's range and of a bin; short
    rows of the pool only (the long ones: test_rows_handed_to_the_host)"""
    pool = [s for s in lag_cases.pool() if len(s) <= 100]
    groups = lag_cases.pooled_groups([1, 2, 63, 64, 65, 66, 129, 130], pool, seed=7)
    return lag_cases.layout(groups, seed=7)


@pytest.mark.parametrize("B", [1, 3, 64, 100])
@pytest.mark.parametrize("W", [0, 1, 63, 64, 65])
def test_strip_and_group_edges(edge_job, B, W):
    text, st, en, off = edge_job
    dev = _dev_equals_host(text, st, en, off, B, W)
    assert dev.classes[0] == heat_ref.layout(off, B, W)[3] and dev.classes[1:] == (0, 0)
    if (B, W) == (3, 65):
        heat_ref.same(dev, heat_ref.segments(text, st, en, off, B, W))


@pytest.mark.parametrize("tl", [1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512])
def test_every_word_class(tl):
    """targets of tl bases (every word class, both sides of each boundary), some with N, and queries of S - 1, S, S + 1,
    2 S + 1, tl and 1024 bases, each row against its three predecessors; the 1024-bp rows as targets go to the host"""
    text, st, en, off = lag_cases.layout(lag_cases.length_case(tl), seed=tl)
    dev = _dev_equals_host(text, st, en, off, 3, 3)
    ln = [e - s + 1 for s, e in zip(st, en)]
    mine = sum(1 for y in range(len(ln)) for x in range(max(0, y - 3), y) if ln[y] == tl and ln[x] <= 1024)
    assert dev.classes[0] >= mine > 250   # no case passes on the host form alone
    if tl in (1, 193, 512):
        heat_ref.same(dev, heat_ref.segments(text, st, en, off, 3, 3))


def test_rows_handed_to_the_host():
    """513-bp and 1025-bp rows and an empty segment among ordinary rows"""
    pool = lag_cases.pool()
    groups = lag_cases.pooled_groups([70, 1, 45], pool, seed=11)
    groups[0][7] = ""
    flat = [s for g in groups for s in g]
    assert {513, 1025} <= {len(s) for s in flat}
    text, st, en, off = lag_cases.layout(groups, seed=11)
    for B, W in ((4, 0), (1, 66)):
        dev = _dev_equals_host(text, st, en, off, B, W)
        assert dev.classes[0] > 0 and dev.classes[1] > 0 and dev.classes[2] > 0
    heat_ref.same(dev, heat_ref.segments(text, st, en, off, 1, 66))
    # a byte outside ACGTN: every pair is the host's, the same bytes
    groups = lag_cases.pooled_groups([30], lag_cases.pool(extra_byte="R"), seed=12)
    groups[0][5] = pool[0][:10] + "R" + pool[0][11:]
    text, st, en, off = lag_cases.layout(groups, seed=12)
    dev = lib.heat_segments(text, st, en, off, 4, 0, device=0, threads=THREADS)
    assert (dev.sums == lib.heat_segments(text, st, en, off, 4, 0, threads=THREADS).sums).all() and dev.classes[0] == 0


def test_reduction_on_identical_rows():
    """130 identical rows of L bases: every pair is (0, L), so a cell holds its pair count times L"""
    L, n = 47, 130
    row = lag_cases.rand_seq(random.Random(5), L)
    text, st, en, off = lag_cases.layout([[row] * n], seed=5, gap=0)
    dev = lib.heat_segments(text, st, en, off, 64, 0, device=0)
    assert dev.nb.tolist() == [3] and dev.classes == (n * (n - 1) // 2, 0, 0)
    size = [64, 64, 2]
    for I in range(3):
        for J in range(I, 3):
            pairs = size[I] * (size[I] - 1) // 2 if I == J else size[I] * size[J]
            assert dev.cell(0, I, J) == (pairs, pairs * L, pairs * L)
    one = lib.heat_segments(text, st, en, off, 1, 0, device=0)
    want = np.zeros((n * (n + 1) // 2, 3), dtype=np.int64)
    for x in range(n):
        for y in range(x + 1, n):
            want[one.index(0, x, y)] = (1, L, L)
    assert (one.sums == want).all()


def test_scan_of_more_than_a_tile_of_targets_in_two_classes():
    """one group of 300 rows of 60 and of 200 bp: the strip counts of 299 targets are scanned over two tiles of 256, in the
    order of two word classes with a bound between them; every cell against the host form of the same call"""
    r = random.Random(31)
    short, long_ = lag_cases.rand_seq(r, 60), lag_cases.rand_seq(r, 200)
    rows = [lag_cases.fit(r, lag_cases.mutate(r, b), len(b)) for b in (long_ if r.random() < 0.4 else short for _ in range(300))]
    assert {lag_cases.words(len(s)) for s in rows} == {1, 4}
    text, st, en, off = lag_cases.layout([rows], seed=31)
    dev = lib.heat_segments(text, st, en, off, 16, 0, device=0, threads=THREADS)
    host = lib.heat_segments(text, st, en, off, 16, 0, threads=THREADS, which=0)
    assert dev.classes == (300 * 299 // 2, 0, 0)
    assert dev.sums.shape == host.sums.shape and (dev.sums == host.sums).all()
    assert int(dev.sums[:, 0].sum()) == 300 * 299 // 2


# ---- the device-resident form ------------------------------------------------------------------------------------------

def _device_reads(rs):
    data = torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).to("cuda:0")
    return lib.DeviceReads(data, [len(s) for s in rs])


def test_the_device_resident_chain():
    """Stream(final=True, device_final=True) over the test read and the DXZ1 monomers -> final_heat_device on a caller's
    stream: torch tensors on the device, equal to final_heat_host less its which = 1 part, the same classes"""
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    mn, ms, _ = lib.fasta_load(os.path.join(TD, "DXZ1_star_monomers.fa"))
    rs = [s.upper() for s in rs]
    dr = _device_reads(rs)
    stream = lib.Stream([s.upper() for s in ms], final=True, mono_names=mn, threads=THREADS, device_final=True)
    try:
        stream.submit(dr)
        dfr = stream.collect_final_device()
    finally:
        stream.close()
    fr = dfr.to_host()
    assert dfr.n_rows == len(fr.rows) > 100
    side = torch.cuda.Stream(device=dfr.rows.device)
    for B, W in ((16, 0), (1, 70)):
        dh = lib.final_heat_device(dfr, dr, B, W, stream=side)
        assert dh.sums.is_cuda and dh.sums.dtype == torch.int64 and dh.cell_off.is_cuda and dh.nb.is_cuda
        with torch.cuda.stream(side):
            got = dh.sums.to("cpu", non_blocking=False)
        side.synchronize()
        every = lib.final_heat_host(fr, rs, B, W, threads=THREADS)
        left = lib.final_heat_host(fr, rs, B, W, threads=THREADS, which=1)
        assert (got.numpy() == every.sums - left.sums).all()
        assert dh.classes == every.classes and dh.classes[0] == int(got[:, 0].sum()) > 1000
        assert dh.cell_off.cpu().numpy().tolist() == every.cell_off.tolist() and dh.nb.cpu().numpy().tolist() == every.nb.tolist()
        assert (dh.to_host(B, W).sums == got.numpy()).all()
    # sums the caller sized for another layout are refused before anything is written
    import ctypes as C
    err = C.create_string_buffer(512)
    cls = (C.c_int64 * 3)()
    guard = torch.full((8, 3), 77, dtype=torch.int64, device="cuda:0")
    rc = lib.load().sd_heat_final_dev(C.c_void_p(dfr.rows.data_ptr()), dfr.n_rows, C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, 16, 0, 0, 0,
                                      None, C.c_void_p(guard.data_ptr()), 8, cls, err, 512)
    torch.cuda.synchronize()
    assert rc == lib.SD_ERR_PARAM and b"cells" in err.value and (guard == 77).all()


# ---- the command line --------------------------------------------------------------------------------------------------

def _cli(out, extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), os.path.join(TD, "read.fa"),
                        os.path.join(TD, "DXZ1_star_monomers.fa"), "-o", out, "-t", str(THREADS)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return p


TSVS = ("final_decomposition.tsv", "final_decomposition_alt.tsv", "final_decomposition_raw.tsv")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plain"))
    _cli(out, [])
    return {f: open(os.path.join(out, f), "rb").read() for f in TSVS}


def _reads():
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    return {n.split()[0]: s.decode().upper() for n, s in zip(rn, rs)}


def test_cli_heatmap(tmp_path, plain_run):
    out = str(tmp_path / "heat")
    _cli(out, ["--heatmap", "4"])
    for f in TSVS:
        assert open(os.path.join(out, f), "rb").read() == plain_run[f], f
    fin = formats.read_final(os.path.join(out, "final_decomposition.tsv"))
    assert len(fin) > 100
    text = open(os.path.join(out, "final_decomposition_heatmap.tsv")).read()
    assert text == heat_ref.text_of_final(fin, _reads(), 4)
    rows = formats.read_heatmap(os.path.join(out, "final_decomposition_heatmap.tsv"))
    nb = (len(fin) + 3) // 4
    alone = 1 if len(fin) % 4 == 1 else 0   # a last bin of one row: its diagonal cell has no pair and no line
    assert len(rows) == nb * (nb + 1) // 2 - alone and sum(r.pairs for r in rows) == len(fin) * (len(fin) - 1) // 2
    assert rows[0].start_i == fin[0].start and rows[0].end_i == fin[3].end and rows[-1].end_j == fin[-1].end
    assert "final_decomposition_heatmap.tsv" in open(os.path.join(out, "stringdecomposer.log")).read()


def test_cli_refusal_for_size_keeps_the_decomposition(tmp_path, plain_run):
    """a read over the cap on pairs: named with its rows, the pairs and the cap; the three TSVs are complete"""
    out = str(tmp_path / "cap")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), os.path.join(TD, "read.fa"),
                        os.path.join(TD, "DXZ1_star_monomers.fa"), "-o", out, "-t", str(THREADS), "--heatmap", "4",
                        "--heatmap-max-pairs", "1000"], capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    for f in TSVS:
        assert open(os.path.join(out, f), "rb").read() == plain_run[f], f
    fin = formats.read_final(os.path.join(out, "final_decomposition.tsv"))
    line = [x for x in p.stderr.splitlines() if x.startswith("--heatmap failed: ")]
    assert len(line) == 1
    for word in ("read " + fin[0].read, "%d rows" % len(fin), "%d pairs" % (len(fin) * (len(fin) - 1) // 2), "the cap is 1000"):
        assert word in line[0], line[0]
    assert "the decomposition is in" in open(os.path.join(out, "stringdecomposer.log")).read()
    assert not os.path.exists(os.path.join(out, "final_decomposition_heatmap.tsv"))   # refused before the file is opened


def test_cli_heatmap_of_single_rows_agrees_with_lags(tmp_path, plain_run):
    out = str(tmp_path / "both")
    _cli(out, ["--heatmap", "1,8", "--lags", "8"])
    for f in TSVS:
        assert open(os.path.join(out, f), "rb").read() == plain_run[f], f
    fin = formats.read_final(os.path.join(out, "final_decomposition.tsv"))
    text = open(os.path.join(out, "final_decomposition_heatmap.tsv")).read()
    assert text == heat_ref.text_of_final(fin, _reads(), 1, 8)
    lags = formats.read_lags(os.path.join(out, "final_decomposition_lags.tsv"))
    rows = formats.read_heatmap(os.path.join(out, "final_decomposition_heatmap.tsv"))
    first = {}
    for i, r in enumerate(fin):
        first.setdefault(r.read, i)
    seen = 0
    for r in rows:   # every line is one pair: row bin_i against row bin_j of its read, bin_j - bin_i <= 8
        x, d = first[r.read] + r.bin_i, r.bin_j - r.bin_i
        assert r.pairs == 1 and 1 <= d <= 8
        assert (r.start_i, r.end_i, r.start_j, r.end_j) == (fin[x].start, fin[x].end, fin[x + d].start, fin[x + d].end)
        assert "%.2f" % r.identity == "%.2f" % lags[x].identities[d - 1]
        seen += 1
    assert seen == sum(1 for l in lags for v in l.identities if v >= 0) > 1000
