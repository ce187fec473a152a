#!/usr/bin/env python3
"""The kernels of --dotplot (count, sets, pairs: csrc/sd_dotplot.hip) on one synthetic tandem array -- twelve 171-bp
monomers of stringdecomposer_amd/synth.py repeated to `--length` bases, every copy mutated by 2 % -- each pass between two
HIP events (sd_dotplot_kernel_bench), `rounds` calls of warmup + reps repetitions each; medians, minima and maxima over
all repetitions, pair-elements per second, one JSON line per setting (with and without the reverse strand).  The whole
device call (sd_dotplot_dev: upload, kernels, download) is timed by the wall clock; with --host T also sd_dotplot_host on T
threads, once, and its integers are compared with the device's.

usage: python tools/dotplot_bench.py [--length 5000000] [-k 21] [-W 2000] [-B 0] [-M 1] [--rounds 3] [--reps 5] [--host 16]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib, synth   # noqa: E402


def make_array(length, seed=5):
    """one read: the twelve monomers in their order, over and over, substitutions only, 2 % per copy"""
    _, ms = synth.make_monomers(12, seed=seed)
    _, rs = synth.make_reads(ms, 1, read_len=length, seed=seed, psub=0.02, pins=0.0, pdel=0.0)
    return rs[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--length", type=int, default=5000000)
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("-W", type=int, default=2000)
    ap.add_argument("-B", type=int, default=0)
    ap.add_argument("-M", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host", type=int, default=0, metavar="T", help="also time sd_dotplot_host on T threads and compare the integers")
    ap.add_argument("--strands", default="1,2", help="1 = forward only, 2 = with the reverse strand (by default both, one line each)")
    a = ap.parse_args()
    read = make_array(a.length)
    for strands in [int(x) for x in a.strands.split(",")]:
        rc = strands == 2
        ms = {"count_ms": [], "sets_ms": [], "pairs_ms": []}
        info = None
        for _ in range(a.rounds):
            info = lib.dotplot_kernel_bench([read], a.k, a.W, a.B, a.M, rc, device=a.device, warmup=a.warmup, reps=a.reps)
            for key in ms:
                ms[key] += info[key]
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            dev = lib.dotplot([read], a.k, a.W, a.B, a.M, rc, device=a.device)
            wall.append((time.perf_counter() - t0) * 1e3)
        # pair-elements: every cell looks the elements of S_j (and R_j) up in S_i
        nw = dev.n_windows(0)
        elems = 0
        for i in range(nw):
            j0 = dev.first(i)
            elems += int(dev.kmers[j0:i + 1].sum()) + (int(dev.kmers_rc[j0:i + 1].sum()) if rc else 0)
        probes = elems * max(1.0, float(np.log2(max(2.0, float(dev.kmers.mean())))))
        med = {key: statistics.median(v) for key, v in ms.items()}
        out = {"length": a.length, "k": a.k, "W": a.W, "B": a.B, "M": a.M, "rc": rc, "windows": info["windows"], "cells": info["cells"],
               "selected": info["selected"], "largest_set": info["largest"], "launches": info["launches"], "workgroups": info["workgroups"],
               "pair_elements": elems, "count_ms": med["count_ms"], "sets_ms": med["sets_ms"], "pairs_ms": med["pairs_ms"],
               "min_max": {key: [min(v), max(v)] for key, v in ms.items()},
               "elements_per_s": elems / (med["pairs_ms"] / 1e3), "lds_probes_per_s": probes / (med["pairs_ms"] / 1e3),
               "device_call_ms": statistics.median(wall), "device_call_ms_all": [round(x, 2) for x in wall],
               "all": {key: [round(x, 4) for x in v] for key, v in ms.items()}}
        if a.host > 0:
            t0 = time.perf_counter()
            host = lib.dotplot([read], a.k, a.W, a.B, a.M, rc, threads=a.host)
            out["host_threads"] = a.host
            out["host_ms"] = (time.perf_counter() - t0) * 1e3
            out["equal"] = bool((host.kmers == dev.kmers).all() and (host.shared == dev.shared).all() and
                                (not rc or ((host.kmers_rc == dev.kmers_rc).all() and (host.shared_rc == dev.shared_rc).all())))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
