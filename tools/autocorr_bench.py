#!/usr/bin/env python3
"""The kernels of --autocorr (sd_autocorr_prep: byte text -> bit planes; sd_autocorr_pairs: a workgroup per tile of a
window and block of 256 lags) on synthetic reads -- noisy tandem arrays of a 171-bp unit -- each stage between two HIP
events (sd_autocorr_kernel_bench), `rounds` calls of warmup + reps repetitions each; medians, minima and maxima over all
repetitions, base-lag products per second, one JSON line.  With --host T: also the wall time of sd_autocorr_host on T
threads, once.

usage: python tools/autocorr_bench.py [--reads 1000] [--length 50000] [-k 8] [-D 4096] [--window 0] [--rounds 3] [--reps 5]
       python tools/autocorr_bench.py --reads 1 --length 50000000 --window 100000
       python tools/autocorr_bench.py --reads 64 -D 65536"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib   # noqa: E402


def make_reads(n_reads, length, seed, unit_len=171):
    """copies of one unit with 5 % substitutions and 1 % N, cut into reads"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    total = n_reads * length
    text = np.tile(acgt[rng.integers(0, 4, unit_len)], total // unit_len + 1)[:total].copy()
    x = rng.random(total)
    sub = x < 0.05
    text[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    text[(x >= 0.05) & (x < 0.06)] = ord("N")
    flat = text.tobytes()
    return [flat[i * length:(i + 1) * length] for i in range(n_reads)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--length", type=int, default=50000)
    ap.add_argument("-k", type=int, default=8)
    ap.add_argument("-D", type=int, default=4096)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host", type=int, default=0, metavar="T", help="also time sd_autocorr_host on T threads")
    a = ap.parse_args()
    reads = make_reads(a.reads, a.length, seed=5)
    ms = {"prep_ms": [], "pairs_ms": []}
    info = None
    for _ in range(a.rounds):
        info = lib.autocorr_kernel_bench(reads, a.k, a.D, a.window, device=a.device, warmup=a.warmup, reps=a.reps)
        for key in ms:
            ms[key] += info[key]
    products = sum(max(0, min(a.D, len(s) - a.k)) * len(s) for s in reads)   # lags above n - k are not launched
    med = {key: statistics.median(v) for key, v in ms.items()}
    out = {"reads": a.reads, "length": a.length, "k": a.k, "D": a.D, "window": a.window, "launches": info["launches"],
           "workgroups": info["workgroups"], "cells": info["cells"], "plane_words": info["words"], "base_lag_products": products,
           "prep_ms": med["prep_ms"], "pairs_ms": med["pairs_ms"],
           "prep_ms_min_max": [min(ms["prep_ms"]), max(ms["prep_ms"])], "pairs_ms_min_max": [min(ms["pairs_ms"]), max(ms["pairs_ms"])],
           "products_per_s": products / (med["pairs_ms"] / 1e3), "word_steps_per_s": products / 64 / (med["pairs_ms"] / 1e3),
           "all": {key: [round(x, 4) for x in v] for key, v in ms.items()}}
    if a.host > 0:
        t0 = time.perf_counter()
        lib.autocorr(reads, a.k, a.D, a.window, threads=a.host)
        out["host_threads"] = a.host
        out["host_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
