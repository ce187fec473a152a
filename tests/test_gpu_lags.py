"""Identity against lag (--lags) on the device: the lane kernel (sd_lag_segments_dev) against the host form at every word
class and on both sides of each boundary, the pairs it hands to the host, the sums reduced on the device, the
device-resident chain (Stream(device_final=True) on DeviceReads -> lib.final_lags_device) and the command line's two files."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import lag_cases
import lag_ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8


def _same(a, b):
    bad = np.argwhere(a.dist != b.dist)
    assert bad.size == 0, "first differing distance at segment %d, lag %d: %d != %d" % (
        bad[0][0], bad[0][1] + 1, a.dist[tuple(bad[0])], b.dist[tuple(bad[0])])
    bad = np.argwhere(a.matches != b.matches)
    assert bad.size == 0, "first differing match count at segment %d, lag %d" % (bad[0][0], bad[0][1] + 1)
    assert (a.sums == b.sums).all()


def _dev_equals_host(text, st, en, off, D):
    dev = lib.lag_segments(text, st, en, off, D, device=0, threads=THREADS)
    host = lib.lag_segments(text, st, en, off, D, threads=THREADS)
    _same(dev, host)
    assert (dev.dist != -2).all()
    return host


def _sums_of(dist, matches, group_of, n_groups):
    """the sums recomputed from dist / matches (pairs with dist >= 0)"""
    D = dist.shape[1]
    out = np.zeros((n_groups, D, 3), dtype=np.int64)
    for s in range(dist.shape[0]):
        ok = dist[s] >= 0
        out[group_of[s], ok, 0] += 1
        out[group_of[s], ok, 1] += matches[s][ok]
        out[group_of[s], ok, 2] += dist[s][ok].astype(np.int64) + matches[s][ok]
    return out


@pytest.mark.parametrize("tl", [1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512])
def test_kernel_equals_host_on_lengths(tl):
    """100 pairs with a target of tl bases (every word class, both sides of each boundary) and queries of S - 1, S, S + 1,
    2 S + 1, tl and 1024 bases; 99 more with those as targets: more than one wave and a partial wave in a class"""
    text, st, en, off = lag_cases.layout(lag_cases.length_case(tl), seed=tl)
    host = _dev_equals_host(text, st, en, off, 1)
    assert (host.dist[:-1] >= 0).all() and host.dist[-1][0] == -1 and host.sums[0, 0, 0] == len(st) - 1
    if tl in (1, 193, 512):   # and the host against the reference fold, where the pairs differ most from the CPU tests'
        lag_ref.same(host, lag_ref.segments(text, st, en, off, 1))


def test_targets_of_n_only():
    text, st, en, off = lag_cases.layout(lag_cases.length_case(171, target=lambda i: "N" * 171), seed=1)
    host = _dev_equals_host(text, st, en, off, 1)
    assert (host.dist[0:-1:2, 0] >= 0).all()
    assert int(host.matches[2, 0]) == 0 and int(host.dist[2, 0]) == 171   # (query 1 holds no N: every column a mismatch or a gap)


@pytest.mark.parametrize("tl", [64, 130, 512])
def test_targets_that_differ_in_the_last_base_only(tl):
    """the last base of a target is bit 63 of the last word, whatever the length: the top alignment of the masks"""
    import random
    common = lag_cases.rand_seq(random.Random(tl), tl - 1)
    groups = lag_cases.length_case(tl, target=lambda i: common + "ACGT"[i % 4], seed=3)
    rows = groups[0]
    for i in range(0, len(rows), 16):   # some queries are the common part plus one base: the last column decides
        rows[i] = common + "ACGT"[(i // 16) % 4]
    text, st, en, off = lag_cases.layout(groups, seed=tl)
    host = _dev_equals_host(text, st, en, off, 1)
    d = [int(host.dist[i][0]) for i in range(0, len(rows), 16)]
    assert set(d) == {0, 1}


def test_lags_over_several_groups_and_classes():
    """D = 7 over groups of 0 .. 40 rows drawn from segments of every word class: the grouping by class, several reads in
    one workgroup's table of sums"""
    import random
    r = random.Random(4)
    units = [lag_cases.rand_seq(r, n) for n in (30, 100, 171, 250, 330, 500)]
    sizes = [0, 1, 2, 7, 8, 21, 40, 3, 33]
    groups = [[lag_cases.mutate(r, r.choice(units), 0.1, "ACGTN") for _ in range(n)] for n in sizes]
    text, st, en, off = lag_cases.layout(groups, seed=4)
    host = _dev_equals_host(text, st, en, off, 7)
    group_of = [g for g, n in enumerate(sizes) for _ in range(n)]
    assert (host.sums == _sums_of(host.dist, host.matches, group_of, len(sizes))).all()


def test_pairs_handed_to_the_host_give_the_same_bytes():
    """a 513-bp target, a 1025-bp query and an empty segment among ordinary rows; then a text with a byte outside ACGTN"""
    pool = lag_cases.pool()
    groups = lag_cases.pooled_groups([60, 1, 45], pool, seed=11)
    groups[0][7] = ""
    flat = [s for g in groups for s in g]
    assert {513, 1025} <= {len(s) for s in flat}
    text, st, en, off = lag_cases.layout(groups, seed=11)
    host = _dev_equals_host(text, st, en, off, 3)
    lag_ref.same(host, lag_ref.segments(text, st, en, off, 3))
    groups = lag_cases.pooled_groups([30], lag_cases.pool(extra_byte="R"), seed=12)
    groups[0][5] = pool[0][:10] + "R" + pool[0][11:]
    text, st, en, off = lag_cases.layout(groups, seed=12)
    _dev_equals_host(text, st, en, off, 3)


# ---- the device-resident form ------------------------------------------------------------------------------------------

def _device_reads(rs):
    data = torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).to("cuda:0")
    return lib.DeviceReads(data, [len(s) for s in rs])


def _rows_on_device(rows, n_reads):
    t = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(len(rows), -1).copy()).to("cuda:0")
    counts = np.bincount(rows["read"], minlength=n_reads)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to("cuda:0")
    return lib.DeviceFinalRows(t, off, None, len(rows))


def test_final_rows_with_pairs_left_out():
    """Hand-made final rows over three reads: ordinary blocks, a 513-bp and a 1025-bp block, rows clamped at the read's
    ends.  The pairs outside the kernel's limits come out as -2 and are counted; every other entry equals the host twin's,
    and the sums are those of the entries that were computed."""
    import random
    r = random.Random(6)
    unit = lag_cases.rand_seq(r, 171)
    lens = [171] * 9 + [513] + [171] * 6 + [1025] + [171] * 8
    reads, rows = [], []
    for read, blocks in enumerate((lens, [171] * 3, lens[5:20])):
        seq, at = "", 0
        for n in blocks:
            seq += lag_cases.fit(r, lag_cases.mutate(r, unit * 7, 0.08), n)
            rows.append((read, at, at + n - 1))
            at += n
        reads.append(seq.encode())
    rows[0] = (0, -4, 170)                      # clamped at 0
    rows[-1] = (2, rows[-1][1], rows[-1][2] + 50)   # clamped at the read's end
    arr = np.zeros(len(rows), dtype=lib.final_dtype())
    for i, (read, s, e) in enumerate(rows):
        arr[i]["read"], arr[i]["start"], arr[i]["end"] = read, s, e
    D = 4
    host = lib.final_lags_host((arr, None, None), reads, D, threads=THREADS)
    dl = lib.final_lags_device(_rows_on_device(arr, 3), _device_reads(reads), D)
    got = dl.to_host()
    left = got.dist == -2
    assert dl.classes[2] == int(left.sum()) > 0 and sum(dl.classes) == len(rows) * D
    assert dl.classes[0] == int((host.dist == -1).sum()) and not got.matches[left].any()
    # exactly the pairs with a 513-bp target or a 1025-bp query
    seg = [min(e + 1, len(reads[rd])) - max(s, 0) for rd, s, e in rows]
    want = np.zeros_like(left)
    for x, (rd, _, _) in enumerate(rows):
        for d in range(1, D + 1):
            if x + d < len(rows) and rows[x + d][0] == rd:
                want[x][d - 1] = seg[x + d] > 512 or seg[x] > 1024
    assert (left == want).all()
    assert (got.dist[~left] == host.dist[~left]).all() and (got.matches[~left] == host.matches[~left]).all()
    assert (got.sums == _sums_of(got.dist, got.matches, [x[0] for x in rows], 3)).all()
    assert (host.sums == _sums_of(host.dist, host.matches, [x[0] for x in rows], 3)).all()


def test_the_chain_on_a_side_stream():
    """Stream(final=True, device_final=True) on DeviceReads -> final_lags_device on a caller's stream: equals the host twin
    on the collected rows, and the reference fold over their segments"""
    mn, ms = synth.make_monomers(6, seed=31)
    rn, rs = synth.make_reads(ms, 3, read_len=3000, seed=31)
    dr = _device_reads(rs)
    st = lib.Stream(ms, final=True, mono_names=mn, threads=THREADS, device_final=True)
    try:
        st.submit(dr)
        dfr = st.collect_final_device()
    finally:
        st.close()
    fr = dfr.to_host()
    assert dfr.n_rows == len(fr.rows) > 30
    D = 5
    side = torch.cuda.Stream(device=dfr.rows.device)
    dl = lib.final_lags_device(dfr, dr, D, stream=side)
    assert dl.dist.is_cuda and dl.dist.dtype == torch.int32 and dl.matches.dtype == torch.int32 and dl.sums.dtype == torch.int64
    with torch.cuda.stream(side):   # ordered on the side stream: a copy enqueued there, and that stream alone waited for
        got = [x.to("cpu", non_blocking=False) for x in (dl.dist, dl.matches, dl.sums)]
    side.synchronize()
    got = formats.Lags(got[0].numpy(), got[1].numpy(), got[2].numpy())
    host = lib.final_lags_host(fr, rs, D, threads=THREADS)
    _same(got, host)
    assert dl.classes[2] == 0 and sum(dl.classes) == dfr.n_rows * D and dl.classes[1] == int((host.dist >= 0).sum())
    text = b"".join(rs)
    base = np.cumsum([0] + [len(s) for s in rs])
    s0 = [int(base[r] + max(s, 0)) for r, s in zip(fr.rows["read"], fr.rows["start"])]
    e0 = [int(base[r] + min(e, len(rs[r]) - 1)) for r, e in zip(fr.rows["read"], fr.rows["end"])]
    lag_ref.same(host, lag_ref.segments(text, s0, e0, [int(x) for x in fr.row_off], D))
    assert formats.lag_period(host.sums) == lib.lag_periods(host.sums)[0].tolist()


def test_foreign_pointers_are_refused():
    import ctypes as C
    L = lib.load()
    arr = np.zeros(4, dtype=lib.final_dtype())
    arr["end"] = 9
    reads = [b"ACGTACGTACGTACGT"]
    dfr, dr = _rows_on_device(arr, 1), _device_reads(reads)
    D = 2
    dist = torch.full((4, D), 77, dtype=torch.int32, device="cuda:0")
    matches = torch.full((4, D), 77, dtype=torch.int32, device="cuda:0")
    sums = torch.zeros((1, D, 3), dtype=torch.int64, device="cuda:0")
    host = np.zeros(64, dtype=np.int64)
    err = C.create_string_buffer(1024)
    cls = (C.c_int64 * 3)()
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    h = C.c_void_p(host.ctypes.data)
    call = lambda rows, text, d, m, s: L.sd_lag_final_dev(rows, 4, text, dr.c_off, dr.c_lens, 1, D, 0, None, d, m, s, cls, err, 1024)   # noqa: E731
    assert call(h, C.c_void_p(dr.ptr), p(dist), p(matches), p(sums)) == lib.SD_ERR_PARAM
    assert call(p(dfr.rows), h, p(dist), p(matches), p(sums)) == lib.SD_ERR_PARAM
    assert call(p(dfr.rows), C.c_void_p(dr.ptr), h, p(matches), p(sums)) == lib.SD_ERR_PARAM
    assert call(p(dfr.rows), C.c_void_p(dr.ptr), p(dist), p(matches), h) == lib.SD_ERR_PARAM
    if torch.cuda.device_count() > 1:
        far = torch.zeros((4, D), dtype=torch.int32, device="cuda:1")
        assert call(p(dfr.rows), C.c_void_p(dr.ptr), p(far), p(matches), p(sums)) == lib.SD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (dist == 77).all() and (matches == 77).all()
    assert call(p(dfr.rows), C.c_void_p(dr.ptr), p(dist), p(matches), p(sums)) == lib.SD_OK
    torch.cuda.synchronize()
    assert dist.cpu().numpy().tolist() == [[0, 0], [0, 0], [0, -1], [-1, -1]]   # (four times the same ten bases)
    assert matches.cpu().numpy().tolist() == [[10, 10], [10, 10], [10, 0], [0, 0]]
    assert list(cls) == [3, 5, 0] and sums.cpu().numpy().tolist() == [[[3, 30, 30], [2, 20, 20]]]


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


@pytest.mark.parametrize("extra", [[], ["--screen", "2048"]], ids=["plain", "behind_screen"])
def test_cli_lags(tmp_path, plain_run, extra):
    out = str(tmp_path / "lags")
    _cli(out, ["--lags", "4"] + extra)
    for f in TSVS:
        assert open(os.path.join(out, f), "rb").read() == plain_run[f], f
    fin = formats.read_final(os.path.join(out, "final_decomposition.tsv"))
    assert len(fin) > 100
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    reads = {n.split()[0]: s.decode().upper() for n, s in zip(rn, rs)}
    lag_text, per_text = lag_ref.files_of_final(fin, reads, 4)
    assert open(os.path.join(out, "final_decomposition_lags.tsv")).read() == lag_text
    assert open(os.path.join(out, "final_decomposition_period.tsv")).read() == per_text
    rows = formats.read_lags(os.path.join(out, "final_decomposition_lags.tsv"))
    assert [(r.read, r.start, r.end) for r in rows] == [(r.read, r.start, r.end) for r in fin]
    assert all(len(r.identities) == 4 for r in rows) and rows[-1].identities == (-1.0,) * 4
    per = formats.read_periods(os.path.join(out, "final_decomposition_period.tsv"))
    assert sum(p.rows for p in per) == len(fin) and all(1 <= p.period <= 4 for p in per if p.rows > 1)
    assert "final_decomposition_lags.tsv" in open(os.path.join(out, "stringdecomposer.log")).read()
