#!/usr/bin/env python3
"""The wall time of one whole device-form call of each analysis -- lib.lag_segments, lib.heat_segments, lib.autocorr,
lib.dotplot, lib.split_rows with device=0 -- at the default shapes of lags_bench.py, heat_bench.py, autocorr_bench.py,
dotplot_bench.py and split_bench.py: a host clock around a call that ends in a synchronise, the median of 5 after 2
warm-ups, one JSON line.  The kernels are what those benches time; this is the frame around them (argument checks,
work area, uploads, stream, the copy back).  SD_HIP_LIB selects the library, so two builds are compared by running fresh
processes in turn (profiles/analysis_call_timing.md).

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
    out = {"lib": lib.LIB_PATH, "reps": a.reps, "warmup": a.warmup}
    for name, call in calls.items():
        ms = []
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            call()
            if it >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms"] = round(statistics.median(ms), 3)
        out[name + "_all"] = [round(x, 3) for x in ms]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
