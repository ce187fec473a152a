#!/usr/bin/env python3
"""The wall time of one whole device-form call of each analysis -- lib.lag_segments, lib.heat_segments, lib.autocorr,
lib.dotplot, lib.split_rows with device=0 -- at the default shapes of lags_bench.py, heat_bench.py, autocorr_bench.py,
dotplot_bench.py and split_bench.py: a host clock around a call that ends in a synchronise, the median of 5 after 2
warm-ups, one JSON line.  The kernels are what those benches time; this is the frame around them (argument checks,
work area, uploads, stream, the copy back).  The device-resident calls -- lib.final_lags_device, lib.final_heat_device,
lib.autocorr_device, lib.motif_device (the built-in cenpb, E = 1, on the autocorr reads), lib.dotplot_device -- follow at the
same shapes, inputs already on the device, each call followed by a synchronise: there the Python frame is most of the host
time.  SD_HIP_LIB selects the library, so two builds are compared by running fresh processes in turn
(profiles/analysis_call_timing.md); two versions of the Python layer, by running this file from a checkout of each.

usage: [SD_HIP_LIB=path/to/libsd_hip.so] python tools/analysis_call_timing.py [--reps 5] [--warmup 2] [--device 0]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import autocorr_bench   # noqa: E402
import dotplot_bench   # noqa: E402
import heat_bench   # noqa: E402
import lags_bench   # noqa: E402
import split_bench   # noqa: E402
from stringdecomposer_amd import lib   # noqa: E402


def device_job(text, starts, ends, off, dev):
    """a rows job of the benches as a job in device memory: every group a read, its rows final rows -> (DeviceFinalRows,
    DeviceReads)"""
    import numpy as np
    import torch
    starts, ends, off = (np.asarray(x, dtype=np.int64) for x in (starts, ends, off))
    n = len(starts)
    read_off = starts[off[:-1]]
    read_len = ends[off[1:] - 1] + 1 - read_off
    rows = np.zeros(n, dtype=lib.final_dtype())
    rows["read"] = np.repeat(np.arange(len(read_off)), np.diff(off))
    rows["start"], rows["end"] = starts - read_off[rows["read"]], ends - read_off[rows["read"]]
    to = lambda a: torch.from_numpy(a).to("cuda:%d" % dev)   # noqa: E731
    dfr = lib.DeviceFinalRows(to(rows.view(np.uint8).reshape(n, -1)), to(off), None, n)
    return dfr, lib.DeviceReads(to(np.frombuffer(text, dtype=np.uint8).copy()), read_len.tolist(), offsets=read_off.tolist())


def device_reads(reads, dev):
    import numpy as np
    import torch
    flat = torch.from_numpy(np.frombuffer(b"".join(reads), dtype=np.uint8).copy()).to("cuda:%d" % dev)
    return lib.DeviceReads(flat, [len(s) for s in reads])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    dev = a.device
    lag_job = lags_bench.make_rows(290000, 171, 2000, seed=5)
    heat_job = heat_bench.make_rows(1024 * 256, 171, 256, seed=5)
    reads = autocorr_bench.make_reads(1000, 50000, seed=5)
    array = dotplot_bench.make_array(5000000)
    sym = split_bench.make_rows(290000, 171, 12, 30, seed=5)
    R = lib.split_radius(15, 171)
    calls = {"lags": lambda: lib.lag_segments(*lag_job, 8, device=dev),
             "heatmap": lambda: lib.heat_segments(*heat_job, 32, 0, device=dev),
             "autocorr": lambda: lib.autocorr(reads, 8, 4096, 0, device=dev),
             "dotplot": lambda: lib.dotplot([array], 21, 2000, 0, 1, False, device=dev),
             "split": lambda: lib.split_rows(sym, R, 64, 8, 16, device=dev)}
    import torch
    lag_dfr, lag_dr = device_job(*lag_job, dev)
    heat_dfr, heat_dr = device_job(*heat_job, dev)
    d_reads, d_array = device_reads(reads, dev), device_reads([array], dev)
    resident = {"lags_device": lambda: lib.final_lags_device(lag_dfr, lag_dr, 8),
                "heatmap_device": lambda: lib.final_heat_device(heat_dfr, heat_dr, 32, 0),
                "autocorr_device": lambda: lib.autocorr_device(d_reads, 8, 4096, 0),
                "motif_device": lambda: lib.motif_device(d_reads, ["cenpb"], 1),
                "dotplot_device": lambda: lib.dotplot_device(d_array, 21, 2000, 0, 1, False)}
    out = {"lib": lib.LIB_PATH, "reps": a.reps, "warmup": a.warmup}
    for name, call in list(calls.items()) + list(resident.items()):
        ms = []
        for it in range(a.warmup + a.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            call()
            if name in resident:
                torch.cuda.synchronize(dev)
            if it >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms"] = round(statistics.median(ms), 3)
        out[name + "_all"] = [round(x, 3) for x in ms]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
