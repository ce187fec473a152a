#!/usr/bin/env python3
"""The row kernel of --msa (sd_nw_msa) against the profile kernel (sd_nw_profile) on the same pairs: 290 000 mutated
instances of a 12 x 171-bp set (about what 50 Mbp of reads yield), both orientations.  Both kernels run in turn in one
process, each launch between two HIP events (sd_msa_kernel_bench); the medians of 5 after 2 warm-ups, one JSON line.

usage: python tools/msa_bench.py [--pairs 290000] [--monomers 12] [--length 171] [--reps 5] [--warmup 2] [--device 0]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib, synth   # noqa: E402

_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def make_pairs(monos, n, seed):
    """n blocks: a monomer or its reverse complement between flanks of 0..20 random bases, with ~8 % edits (3 %
    substitutions, 2.5 % deletions, 2.5 % insertions), cut from one text -> (text, starts, ends, pair_tmpl)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    tmpl = []
    for m in monos:
        tmpl += [np.frombuffer(m, dtype=np.uint8), np.frombuffer(m[::-1].translate(_RC), dtype=np.uint8)]
    pt = rng.integers(0, len(tmpl), n)
    flank = rng.integers(0, 21, (n, 2))
    src_len = np.array([len(tmpl[p]) for p in pt]) + flank.sum(axis=1)
    src = acgt[rng.integers(0, 4, int(src_len.sum()))]          # the flanks keep these bases
    at = np.concatenate([[0], np.cumsum(src_len)])
    for i, p in enumerate(pt):
        a = at[i] + flank[i, 0]
        src[a:a + len(tmpl[p])] = tmpl[p]
    x = rng.random(len(src))
    sub = x < 0.03
    src[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    cnt = np.ones(len(src), dtype=np.int64)
    cnt[(x >= 0.03) & (x < 0.055)] = 0
    ins = (x >= 0.055) & (x < 0.08)
    cnt[ins] = 2
    cnt[at[:-1]] = np.maximum(cnt[at[:-1]], 1)                  # (no empty block)
    ends = np.cumsum(cnt)
    out = np.repeat(src, cnt)
    extra = ends[ins] - 1                                       # the second copy of a doubled base: the inserted one
    out[extra] = acgt[rng.integers(0, 4, len(extra))]
    blk = np.add.reduceat(cnt, at[:-1])
    st = np.concatenate([[0], np.cumsum(blk)[:-1]])
    return out.tobytes(), st, st + blk - 1, pt.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=290000)
    ap.add_argument("--monomers", type=int, default=12)
    ap.add_argument("--length", type=int, default=171)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    mn, ms = synth.make_monomers(a.monomers, seed=7, length=a.length)
    seq, st, en, pt = make_pairs(ms, a.pairs, seed=a.pairs)
    r = lib.msa_kernel_bench(seq, st, en, ms, pt, device=a.device, warmup=a.warmup, reps=a.reps)
    r["msa_ms_median"] = statistics.median(r["msa_ms"])
    r["profile_ms_median"] = statistics.median(r["profile_ms"])
    r["ratio"] = r["msa_ms_median"] / r["profile_ms_median"]
    r["text_bytes"] = len(seq)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
