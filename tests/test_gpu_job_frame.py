"""The per-device work areas of the analyses (csrc/sd_job_dev.hpp: DevWork) reused while the previous call's kernels may
still be in flight, growing and shrinking between calls: device-resident calls in a row on one stream, nothing waited for
in between, every call with outputs of its own, all compared with the host forms at the end."""
import os
import random

import numpy as np
import pytest
import torch   # before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import lag_cases
from conftest import GOLDEN
from stringdecomposer_amd import lib

pytestmark = pytest.mark.gpu
# Loaded here, before torch initialises the device (test_gpu_autocorr.py and test_gpu_dotplot.py load it at import too, for
# their INFO).  Every unit of the library registers the removal of its code objects with atexit when it is loaded, and exit
# handlers run in reverse order.  This test's first device call is torch's: loaded only then, behind an initialised runtime,
# the library's removals ran at exit ahead of the runtime's own tear-down, and a process of this file alone -- a cached
# pipeline's streams and torch's side stream still open -- passed and never ended.  Loaded first, it ends.
lib.load()
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8


def _device_reads(rs):
    data = torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).to("cuda:0")
    return lib.DeviceReads(data, [len(s) for s in rs])


def test_calls_in_a_row_on_one_stream():
    rng = random.Random(59)
    small = [lag_cases.rand_seq(rng, 300).encode()]
    large = [lag_cases.rand_seq(rng, 5000).encode() for _ in range(3)]
    jobs = [small, large, small]
    side = torch.cuda.Stream(device="cuda:0")
    reads = [_device_reads(rs) for rs in jobs]
    # the final rows of the test read, for the two analyses on rows
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
    lag_d, heat_bw = (1, 8, 1), ((64, 0), (1, 70), (64, 0))

    torch.cuda.synchronize()
    # ---- from here to the synchronise below the host waits for nothing of its own
    ac = [lib.autocorr_device(r, 4, 64, stream=side) for r in reads]
    dp = [lib.dotplot_device(r, 4, 64, stream=side) for r in reads]
    lags = [lib.final_lags_device(dfr, dr, D, stream=side) for D in lag_d]
    heat = [lib.final_heat_device(dfr, dr, B, W, stream=side) for B, W in heat_bw]
    side.synchronize()

    for job, a, d in zip(jobs, ac, dp):
        want = lib.autocorr(job, 4, 64, threads=THREADS)
        assert (a.counts.cpu().numpy() == want.counts).all() and a.win_off.cpu().numpy().tolist() == want.win_off.tolist()
        want = lib.dotplot(job, 4, 64, threads=THREADS)
        assert (d.kmers.cpu().numpy() == want.kmers).all() and (d.shared.cpu().numpy() == want.shared).all()
        assert d.kmers_rc is None and d.shared_rc is None
    assert (ac[0].counts == ac[2].counts).all() and (dp[0].kmers == dp[2].kmers).all() and (dp[0].shared == dp[2].shared).all()

    read_of = fr.rows["read"]
    got = [x.to_host() for x in lags]
    for D, dl, g in zip(lag_d, lags, got):
        host = lib.final_lags_host(fr, rs, D, threads=THREADS)
        left = g.dist == -2   # the pairs the lane kernel does not take: not in the device's sums
        assert dl.classes[2] == int(left.sum()) and sum(dl.classes) == dfr.n_rows * D
        assert (g.dist[~left] == host.dist[~left]).all() and (g.matches[~left] == host.matches[~left]).all()
        want = host.sums.copy()
        for x, d in np.argwhere(left & (host.dist >= 0)):
            want[read_of[x], d] -= (1, host.matches[x, d], host.dist[x, d] + host.matches[x, d])
        assert (g.sums == want).all()
    assert (got[0].dist == got[2].dist).all() and (got[0].matches == got[2].matches).all() and (got[0].sums == got[2].sums).all()

    sums = [h.sums.cpu().numpy() for h in heat]
    for (B, W), dh, s in zip(heat_bw, heat, sums):
        every = lib.final_heat_host(fr, rs, B, W, threads=THREADS)
        left = lib.final_heat_host(fr, rs, B, W, threads=THREADS, which=1)
        assert (s == every.sums - left.sums).all() and dh.classes == every.classes
    assert (sums[0] == sums[2]).all() and heat[0].classes[0] > 1000
