#!/usr/bin/env python3
"""The kernels of --split (sd_split_prep: symbol rows -> bit planes; sd_split_assign: a lane per row against the centres in
LDS; the modes: scan, group, count, centres) on planted rows -- `classes` centres that differ in 20 % of the columns, rows
with 5 % noise, a few junk rows -- each stage between two HIP events on the final centres of one whole split
(sd_split_kernel_bench); medians, minima and maxima over `rounds` calls of `reps` repetitions, the wall time of the whole
call on the device, and with --host T that of the host form on T threads; one JSON line.

usage: python tools/split_bench.py [--rows 290000] [-L 171] [--classes 12] [-P 15] [--rounds 3] [--reps 5] [--host 16]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib   # noqa: E402


def make_rows(n, L, classes, junk, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, L)
    cen = np.tile(base, (classes, 1))
    m = rng.random((classes, L)) < 0.20
    cen[m] = (cen[m] + rng.integers(1, 4, int(m.sum()))) % 4
    sym = cen[rng.integers(0, classes, n)]
    e = rng.random((n, L)) < 0.05
    sym[e] = rng.integers(0, 6, int(e.sum()))
    sym[rng.choice(n, junk, replace=False)] = rng.integers(0, 6, (junk, L))
    return np.ascontiguousarray(sym, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=290000)
    ap.add_argument("-L", type=int, default=171)
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--junk", type=int, default=30)
    ap.add_argument("-P", type=int, default=15)
    ap.add_argument("-K", type=int, default=64)
    ap.add_argument("--min-size", type=int, default=8)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host", type=int, default=0, metavar="T", help="also time sd_split_host on T threads")
    a = ap.parse_args()
    sym = make_rows(a.rows, a.L, a.classes, a.junk, seed=5)
    R = lib.split_radius(a.P, a.L)
    ms = {"prep_ms": [], "assign_ms": [], "modes_ms": []}
    info = None
    for _ in range(a.rounds):
        info = lib.split_kernel_bench(sym, R, a.K, a.min_size, a.iters, device=a.device, warmup=a.warmup, reps=a.reps)
        for key in ms:
            ms[key] += info[key]
    wall = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        dev = lib.split_rows(sym, R, a.K, a.min_size, a.iters, device=a.device)
        wall.append((time.perf_counter() - t0) * 1e3)
    med = {key: statistics.median(v) for key, v in ms.items()}
    out = {"rows": a.rows, "L": a.L, "classes": a.classes, "junk": a.junk, "R": R, "K": a.K, "min_size": a.min_size, "iters_cap": a.iters,
           "k": info["k"], "rounds": info["rounds"], "lloyd_iterations": info["iters"], "assign_launches": info["launches"],
           "prep_ms": med["prep_ms"], "assign_ms": med["assign_ms"], "modes_ms": med["modes_ms"],
           "min_max": {key: [min(v), max(v)] for key, v in ms.items()},
           "row_centre_distances_per_s": a.rows * info["k"] / (med["assign_ms"] / 1e3),
           "device_call_ms": statistics.median(wall), "device_call_ms_all": [round(x, 2) for x in wall],
           "all": {key: [round(x, 4) for x in v] for key, v in ms.items()}}
    if a.host > 0:
        t0 = time.perf_counter()
        host = lib.split_rows(sym, R, a.K, a.min_size, a.iters, threads=a.host)
        out["host_threads"] = a.host
        out["host_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_equals_device"] = bool(np.array_equal(host.assign, dev.assign) and np.array_equal(host.centres, dev.centres)
                                         and np.array_equal(host.d1, dev.d1) and np.array_equal(host.d2, dev.d2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
