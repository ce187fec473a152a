#!/usr/bin/env python3
"""The pair kernel of --heatmap (sd_heat_pairs: a wave per target and strip of 64 queries, the target's masks built once
per wave) against the lane kernel of --lags (sd_lag_pairs: every lane builds its own target's masks) on the SAME pairs, in
one process: groups of 256 rows of a 171-bp repeat (mutated copies of one unit), all against all -- --heatmap 32 with no
distance limit is --lags 255 on such groups.  Every stage runs between two HIP events (sd_heat_kernel_bench,
sd_lag_kernel_bench); the two benches alternate, `rounds` times each; medians over all repetitions, one JSON line.
With --array N: one group of N rows instead (an array-sized read), the heatmap kernel alone.

usage: python tools/heat_bench.py [--groups 1024] [--rows 256] [--length 171] [--bin 32] [--rounds 3] [--reps 5] [--warmup 2]
       python tools/heat_bench.py --array 16384 --bin 64"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib   # noqa: E402


def make_rows(n_rows, length, per_group, seed):
    """n_rows copies of one unit of `length` bases, each with ~8 % edits (3 % substitutions, 2.5 % deletions, 2.5 %
    insertions), back to back; groups of per_group rows -> (text, starts, ends, group_off)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    unit = acgt[rng.integers(0, 4, length)]
    src = np.tile(unit, n_rows)
    x = rng.random(len(src))
    sub = x < 0.03
    src[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    cnt = np.ones(len(src), dtype=np.int64)
    cnt[(x >= 0.03) & (x < 0.055)] = 0
    cnt[(x >= 0.055) & (x < 0.08)] = 2
    text = np.repeat(src, cnt)
    ins = np.repeat(cnt == 2, cnt) & (np.concatenate([[0], np.diff(np.repeat(np.arange(len(src)), cnt))]) == 0)
    text[ins] = acgt[rng.integers(0, 4, int(ins.sum()))]
    at = np.concatenate([[0], np.cumsum(cnt)])
    bounds = at[np.arange(0, n_rows + 1) * length]
    starts, ends = bounds[:-1], bounds[1:] - 1
    off = list(range(0, n_rows, per_group)) + [n_rows]
    return text.tobytes(), starts, ends, off


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=256, help="rows per group (at most 256: --lags reaches 255 rows)")
    ap.add_argument("--array", type=int, default=0, help="one group of this many rows; no --lags comparison")
    ap.add_argument("--length", type=int, default=171)
    ap.add_argument("--bin", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if not a.array and not 2 <= a.rows <= 256:
        ap.error("--rows is 2 .. 256")
    n_rows, per = (a.array, a.array) if a.array else (a.groups * a.rows, a.rows)
    text, st, en, off = make_rows(n_rows, a.length, per, seed=5)
    heat = {k: [] for k in ("group_ms", "pairs_ms", "walk_ms")}
    lags = {k: [] for k in ("group_ms", "pairs_ms", "walk_ms", "ident_ms")}
    hinfo = linfo = None
    for _ in range(a.rounds):   # alternating, so that a drift of the box touches both alike
        hinfo = lib.heat_kernel_bench(text, st, en, off, a.bin, 0, device=a.device, warmup=a.warmup, reps=a.reps)
        for k in heat:
            heat[k] += hinfo[k]
        if not a.array:
            linfo = lib.lag_kernel_bench(text, st, en, off, a.rows - 1, device=a.device, warmup=a.warmup, reps=a.reps)
            for k in lags:
                lags[k] += linfo[k]
    mp = hinfo["pairs"] / 1e6
    hm = {k: statistics.median(v) for k, v in heat.items()}
    out = {"rows": n_rows, "rows_per_group": per, "length": a.length, "mean_block": float(np.mean(en - st + 1)), "bin": a.bin,
           "pairs": hinfo["pairs"], "host_pairs": hinfo["host_pairs"], "K": hinfo["K"], "items": hinfo["items"], "cells": hinfo["cells"],
           "grid": hinfo["grid"], "ck_slots": hinfo["ck_slots"],
           "heat_group_ms": hm["group_ms"], "heat_pairs_ms": hm["pairs_ms"], "heat_walk_ms": hm["walk_ms"],
           "heat_pairs_ms_per_mpair": hm["pairs_ms"] / mp, "heat_walk_ms_per_mpair": hm["walk_ms"] / mp,
           "heat_pairs_per_s": hinfo["pairs"] / (hm["pairs_ms"] / 1e3),
           "heat_build_and_sink_share": (hm["pairs_ms"] - hm["walk_ms"]) / hm["pairs_ms"],
           "heat_all": {k: [round(x, 4) for x in v] for k, v in heat.items()}}
    if linfo:
        lm = {k: statistics.median(v) for k, v in lags.items()}
        assert linfo["pairs"] == hinfo["pairs"], (linfo["pairs"], hinfo["pairs"])   # the same pairs
        out.update({"lag_group_ms": lm["group_ms"], "lag_pairs_ms": lm["pairs_ms"], "lag_walk_ms": lm["walk_ms"], "lag_ident_ms": lm["ident_ms"],
                    "lag_pairs_ms_per_mpair": lm["pairs_ms"] / mp, "lag_walk_ms_per_mpair": lm["walk_ms"] / mp,
                    "lag_ident_ms_per_mpair": lm["ident_ms"] / mp, "lag_grid": linfo["grid"],
                    "heat_to_lag_pairs": hm["pairs_ms"] / lm["pairs_ms"], "heat_to_lag_walk": hm["pairs_ms"] / lm["walk_ms"],
                    "lag_all": {k: [round(x, 4) for x in v] for k, v in lags.items()}})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
