#!/usr/bin/env python3
"""The kernels of --motif (sd_autocorr_prep: byte text -> bit planes; sd_motif_size: the hits of every (tile, pattern-strand)
item counted, scanned; sd_motif_write: the records) on synthetic reads -- noisy tandem arrays of a 171-bp unit that holds a
CENP-B box -- each stage between two HIP events (sd_motif_kernel_bench), `rounds` calls of warmup + reps repetitions each;
medians, minima and maxima over all repetitions, base x pattern-strand products per second, the wall time of the whole call
on host memory (sd_motif_dev) and of the device-resident call (sd_motif_reads_size_dev + _write_dev), one JSON line.  With
--host T: also the wall time of sd_motif_host on T threads, `rounds` times.  With --edits K: the same figures for the kernels
of --motif-edits (sd_motif_edit_size, sd_motif_edit_write) at a budget of K edits, -E ignored; a product is then one step of
the bit-vector column, warm-up not counted.

usage: python tools/motif_bench.py [--reads 1000] [--length 50000] [--motifs 0] [-E 1] [--rounds 3] [--reps 5]
       python tools/motif_bench.py --reads 1 --length 50000000
       python tools/motif_bench.py --reads 100 --motifs 512 -E 0
       python tools/motif_bench.py --edits 1 --host 16"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch   # before the library is loaded: one HIP runtime in the process

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib   # noqa: E402


def make_reads(n_reads, length, seed, unit_len=171):
    """copies of one unit with a CENP-B box in it, 5 % substitutions and 1 % N, cut into reads"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    total = n_reads * length
    unit = acgt[rng.integers(0, 4, unit_len)]
    unit[40:57] = np.frombuffer(b"CTTCGTTGGAAACGGGA", dtype=np.uint8)
    text = np.tile(unit, total // unit_len + 1)[:total].copy()
    x = rng.random(total)
    sub = x < 0.05
    text[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    text[(x >= 0.05) & (x < 0.06)] = ord("N")
    flat = text.tobytes()
    return [flat[i * length:(i + 1) * length] for i in range(n_reads)]


def make_motifs(n, seed):
    """cenpb alone (n = 0), or n random motifs of 17 codes, 9 of them constrained like the box's"""
    if n <= 0:
        return ["cenpb"]
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        p = ["N"] * 17
        for j in rng.choice(17, 9, replace=False):
            p[j] = "ACGT"[rng.integers(0, 4)]
        out.append(("m%d" % i, "".join(p)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--length", type=int, default=50000)
    ap.add_argument("--motifs", type=int, default=0, help="random motifs of 17 codes (by default 0: cenpb alone)")
    ap.add_argument("-E", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--edits", type=int, default=None, metavar="K", help="time the kernels of --motif-edits at K edits instead")
    ap.add_argument("--host", type=int, default=0, metavar="T", help="also time sd_motif_host on T threads")
    a = ap.parse_args()
    reads = make_reads(a.reads, a.length, seed=5)
    motifs = make_motifs(a.motifs, seed=6)
    edits = a.edits is not None
    budget = a.edits if edits else a.E
    kernel_bench, whole, resident = ((lib.motif_edits_kernel_bench, lib.motif_edits, lib.motif_edits_device) if edits else
                                     (lib.motif_kernel_bench, lib.motif, lib.motif_device))
    strands = len(lib.motif_compile(motifs, 0 if edits else a.E)[2])
    ms = {"prep_ms": [], "size_ms": [], "write_ms": []}
    info = None
    for _ in range(a.rounds):
        info = kernel_bench(reads, motifs, budget, device=a.device, warmup=a.warmup, reps=a.reps)
        for key in ms:
            ms[key] += info[key]
    products = sum(len(s) for s in reads) * strands
    med = {key: statistics.median(v) for key, v in ms.items()}
    out = {"reads": a.reads, "length": a.length, "motifs": len(motifs), "pattern_strands": strands, "edits" if edits else "E": budget, "write_launches": info["launches"],
           "items": info["items"], "hits": info["hits"], "plane_words": info["words"], "base_strand_products": products}
    for key in ms:
        out[key] = med[key]
        out[key + "_min_max"] = [min(ms[key]), max(ms[key])]
    out["products_per_s_size"] = products / (med["size_ms"] / 1e3)
    out["products_per_s_size_write"] = products / ((med["size_ms"] + med["write_ms"]) / 1e3)
    call = []
    for _ in range(a.rounds + 1):   # the whole call on host memory: upload, the three stages, hits and per back (the first is a warm-up)
        t0 = time.perf_counter()
        whole(reads, motifs, budget, device=a.device)
        call.append((time.perf_counter() - t0) * 1e3)
    out["call_ms"] = statistics.median(call[1:])
    out["call_ms_min_max"] = [min(call[1:]), max(call[1:])]
    flat = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    dr = lib.DeviceReads(torch.from_numpy(flat).to("cuda:%d" % a.device), [len(s) for s in reads])
    torch.cuda.synchronize()
    res = []
    for _ in range(a.rounds + 1):   # the device-resident call: reads in HBM, hits left in HBM
        t0 = time.perf_counter()
        resident(dr, motifs, budget)
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0) * 1e3)
    out["resident_ms"] = statistics.median(res[1:])
    out["resident_ms_min_max"] = [min(res[1:]), max(res[1:])]
    out["all"] = {key: [round(x, 4) for x in v] for key, v in ms.items()}
    if a.host > 0:
        host = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            whole(reads, motifs, budget, threads=a.host)
            host.append((time.perf_counter() - t0) * 1e3)
        out["host_threads"] = a.host
        out["host_ms"] = statistics.median(host)
        out["host_ms_min_max"] = [min(host), max(host)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
