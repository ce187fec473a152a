#!/usr/bin/env python3
"""The lane kernel of --lags (sd_lag_pairs) on the rows of a C2-sized job: 290 000 blocks of a 171-bp repeat (mutated
copies of a 12-monomer higher-order repeat, back to back in reads of 2 000 blocks) at D = 8, against the light identity
kernel (sd_nw_pairs) on as many pairs of the same queries in the same process.  Every stage runs between two HIP events
(sd_lag_kernel_bench): the grouping (plan + scan + scatter), the lane kernels with their reduction, the lane kernels
without it, the yardstick; medians of 5 after 2 warm-ups, one JSON line.

usage: python tools/lags_bench.py [--rows 290000] [--length 171] [--lags 8] [--reps 5] [--warmup 2] [--device 0]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib, synth   # noqa: E402


def make_rows(n_rows, length, per_read, seed):
    """n_rows blocks: the monomers of a 12-mer in turn, each with ~8 % edits (3 % substitutions, 2.5 % deletions, 2.5 %
    insertions), back to back; reads of per_read blocks -> (text, starts, ends, group_off)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    _, ms = synth.make_monomers(12, seed=seed, length=length)
    unit = np.concatenate([np.frombuffer(m, dtype=np.uint8) for m in ms])
    src = np.tile(unit, (n_rows + 11) // 12)[:n_rows * length].copy()
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
    off = list(range(0, n_rows, per_read)) + [n_rows]
    return text.tobytes(), starts, ends, off


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=290000)
    ap.add_argument("--length", type=int, default=171)
    ap.add_argument("--lags", type=int, default=8)
    ap.add_argument("--per-read", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    text, st, en, off = make_rows(a.rows, a.length, a.per_read, seed=5)
    b = lib.lag_kernel_bench(text, st, en, off, a.lags, device=a.device, warmup=a.warmup, reps=a.reps)
    med = {k: statistics.median(b[k]) for k in ("group_ms", "pairs_ms", "walk_ms", "ident_ms")}
    mp = b["pairs"] / 1e6
    out = {"rows": a.rows, "lags": a.lags, "length": a.length, "mean_block": float(np.mean(en - st + 1)),
           "pairs": b["pairs"], "host_pairs": b["host_pairs"], "K": b["K"], "K_pairs": b["K_pairs"], "grid": b["grid"],
           "ck_slots": b["ck_slots"], "ident_grid": b["ident_grid"], "ident_ck_slots": b["ident_ck_slots"],
           "group_ms": med["group_ms"], "pairs_ms": med["pairs_ms"], "walk_ms": med["walk_ms"], "ident_ms": med["ident_ms"],
           "reduction_ms": med["pairs_ms"] - med["walk_ms"],
           "pairs_ms_per_mpair": med["pairs_ms"] / mp, "walk_ms_per_mpair": med["walk_ms"] / mp,
           "group_ms_per_mpair": med["group_ms"] / mp, "ident_ms_per_mpair": med["ident_ms"] / mp,
           "ratio_to_ident": med["pairs_ms"] / med["ident_ms"],
           "all": {k: [round(x, 4) for x in b[k]] for k in ("group_ms", "pairs_ms", "walk_ms", "ident_ms")}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
