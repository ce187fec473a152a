#!/usr/bin/env python3
"""The pair kernel of the cyclic pass (sd_cyclic_pairs: every query against every target written twice, on both strands) on
synthetic seed monomers -- `seqs` sequences of `length` bases planted from `families` unrelated random sequences, each at a
random rotation, on a random strand, with up to 6 % edits -- all pairs in one call, its launches between two HIP events
(sd_cyclic_kernel_bench), `rounds` calls of warmup + reps repetitions each; medians, minima and maxima over all
repetitions, word steps (columns x words x pairs) per second, the wall time of the whole call on host memory
(sd_cyclic_pairs_dev) and of the merge at P = 85 (sd_cyclic_merge_dev), one JSON line.  With --host T: also the wall time of
the host forms on T threads; --host-queries Q times the host pairs on the first Q queries against all targets and says so
(a call of 1 000 x 2 054 bp takes the host minutes).  With --variants: per class of one to four words, the column in 64-bit
words beside the column in 32-bit halves, alternating in one process.  Sequences of more than 2 048 bases run on the team
kernel (sd_cyclic_pairs_long, timed by sd_cyclic_long_kernel_bench): its word steps count pad words and ramp steps, and
useful_word_steps (columns x the query's own words x pairs) stands beside them.  --long K,L forces every query into the
class of K words x L lanes, short ones included; --long-classes times the classes of equal capacity beside each other
(4 x 16 and 2 x 32 at 4 096 bp, 4 x 32 and 2 x 64 at 8 192 bp), alternating in one process.

usage: python tools/cyclic_bench.py [--seqs 1000] [--length 171] [--rounds 3] [--reps 5] [--host 16]
       python tools/cyclic_bench.py --length 2054 --host 16 --host-queries 50
       python tools/cyclic_bench.py --merge-only --length 2048 --block 1024 --host 16 --host-merge-reps 1
       python tools/cyclic_bench.py --variants
       python tools/cyclic_bench.py --length 2054 --host 16 --host-queries 50      (the team kernel: 3 words x 16 lanes)
       python tools/cyclic_bench.py --length 4096 --host 16 --host-queries 20
       python tools/cyclic_bench.py --seqs 200 --length 16384 --host 16 --host-queries 4
       python tools/cyclic_bench.py --length 4096 --long 2,32
       python tools/cyclic_bench.py --long-classes

The merges are timed --merge-reps times (by default 5) after one warm-up call; --merge-only times nothing else."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch   # noqa: F401  before the library is loaded: one HIP runtime in the process

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib   # noqa: E402

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def make_seqs(n, length, families, seed):
    rng = random.Random(seed)
    fam = ["".join(rng.choice("ACGT") for _ in range(length)) for _ in range(families)]
    out = []
    for _ in range(n):
        s = fam[rng.randrange(families)]
        r = rng.randrange(length)
        s = s[r:] + s[:r]
        if rng.randrange(2):
            s = "".join(COMP[c] for c in reversed(s))
        s = list(s)
        for _ in range(rng.randrange(length * 6 // 100 + 1)):   # substitutions only: every sequence keeps the length
            s[rng.randrange(length)] = rng.choice("ACGT")
        out.append("".join(s))
    return out


def wall(fn, rounds):
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def spread(out, key, ms):
    out[key] = statistics.median(ms)
    out[key + "_min_max"] = [min(ms), max(ms)]


def kernel(seqs, a, variant=0, team=None):
    """team: None = the lane kernel, (K, L) = the team kernel in that class, (0, 0) = in the library's classes"""
    ms, info = [], None
    for _ in range(a.rounds):
        if team is None:
            info = lib.cyclic_kernel_bench(seqs, device=a.device, warmup=a.warmup, reps=a.reps, variant=variant)
        else:
            info = lib.cyclic_long_kernel_bench(seqs, device=a.device, K=team[0], L=team[1], warmup=a.warmup, reps=a.reps)
        ms += info["pairs_ms"]
    return ms, info


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seqs", type=int, default=1000)
    ap.add_argument("--length", type=int, default=171)
    ap.add_argument("--families", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host", type=int, default=0, metavar="T", help="also time the host forms on T threads")
    ap.add_argument("--host-queries", dest="host_queries", type=int, default=0, metavar="Q",
                    help="time the host pairs on the first Q queries only (by default 0: all)")
    ap.add_argument("--block", type=int, default=None, help="the merge's block (by default the library's)")
    ap.add_argument("--merge-reps", dest="merge_reps", type=int, default=5, help="timed merges after one warm-up (by default 5)")
    ap.add_argument("--host-merge-reps", dest="host_merge_reps", type=int, default=0, help="timed host merges (by default as --merge-reps)")
    ap.add_argument("--merge-only", dest="merge_only", action="store_true", help="time the merges only")
    ap.add_argument("--variants", action="store_true", help="per class of 1 .. 4 words: 64-bit words beside 32-bit halves")
    ap.add_argument("--long", default=None, metavar="K,L", help="time the team kernel with every query forced into the class of K words x L lanes")
    ap.add_argument("--long-classes", dest="long_classes", action="store_true", help="the team kernel's classes of equal capacity beside each other")
    a = ap.parse_args()
    if a.long_classes:
        for length, pair in ((4096, ((4, 16), (2, 32))), (8192, ((4, 32), (2, 64)))):
            seqs = make_seqs(a.seqs, length, a.families, seed=length)
            out = {"seqs": a.seqs, "length": length, "words": (length + 63) // 64}
            for _ in range(2):   # alternating
                for c in pair:
                    out.setdefault("%dx%d_ms_all" % c, []).extend(kernel(seqs, a, team=c)[0])
            for c in pair:
                spread(out, "%dx%d_ms" % c, out.pop("%dx%d_ms_all" % c))
            print(json.dumps(out), flush=True)
        return
    if a.variants:
        for length in (64, 128, 171, 192, 256):
            seqs = make_seqs(a.seqs, length, a.families, seed=length)
            out = {"seqs": a.seqs, "length": length, "words": (length + 63) // 64}
            for _ in range(2):   # alternating: words, halves, words, halves
                for name, v in (("words_ms", 1), ("halves_ms", 2)):
                    out.setdefault(name + "_all", []).extend(kernel(seqs, a, v)[0])
            for name in ("words_ms", "halves_ms"):
                spread(out, name, out.pop(name + "_all"))
            print(json.dumps(out), flush=True)
        return
    seqs = make_seqs(a.seqs, a.length, a.families, seed=5)
    out = {"seqs": a.seqs, "length": a.length, "pairs": a.seqs * a.seqs}
    team = tuple(int(x) for x in a.long.split(",")) if a.long else (0, 0) if a.length > lib.CYCLIC_QMAX else None
    if team is not None:
        out["kernel"] = "team"
        out["class"] = list(team if a.long else lib.cyclic_team_class(a.length) or (0, 0))
    if not a.merge_only:
        ms, info = kernel(seqs, a, team=team)
        out.update(device_pairs=info["pairs"], launches=info["launches"], workgroups=info["workgroups"], word_steps=info["steps"])
        if info["pairs"]:
            spread(out, "pairs_ms", ms)
            out["word_steps_per_s"] = info["steps"] / (out["pairs_ms"] / 1e3)
            # the steps a pair needs whatever the geometry: the query's own words over the strands' columns
            out["useful_word_steps"] = info["pairs"] * 2 * (2 * a.length - 1) * ((a.length + 63) // 64)
            out["useful_word_steps_per_s"] = out["useful_word_steps"] / (out["pairs_ms"] / 1e3)
            # (with no pair inside the device's limits the call is the host form: --host times that)
            spread(out, "call_ms", wall(lambda: lib.cyclic_pairs(seqs, device=a.device, threads=max(a.host, 1)), a.rounds + 1)[1:])
    out["block"], out["merge_reps"] = a.block or lib.cyclic_info()["block"], a.merge_reps
    before = lib.cyclic_info()["launches"] + lib.cyclic_long_info()["launches"]
    out["clusters"] = lib.cyclic_merge(seqs, None, 85, block=a.block, device=a.device, threads=max(a.host, 1)).n_clusters   # (the warm-up)
    out["merge_launches"] = lib.cyclic_info()["launches"] + lib.cyclic_long_info()["launches"] - before
    spread(out, "merge_ms", wall(lambda: lib.cyclic_merge(seqs, None, 85, block=a.block, device=a.device, threads=max(a.host, 1)), a.merge_reps))
    if a.host > 0:
        if not a.merge_only:
            q = list(range(min(a.host_queries, a.seqs) if a.host_queries > 0 else a.seqs))
            out["host_threads"], out["host_queries"] = a.host, len(q)
            spread(out, "host_pairs_ms", wall(lambda: lib.cyclic_pairs(seqs, q, None, threads=a.host), 1 if len(q) * a.length > 50000 else a.rounds))
            out["host_pairs_ms_all_queries"] = out["host_pairs_ms"] * a.seqs / len(q)
        spread(out, "host_merge_ms", wall(lambda: lib.cyclic_merge(seqs, None, 85, block=a.block, threads=a.host), a.host_merge_reps or a.merge_reps))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
