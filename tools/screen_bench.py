#!/usr/bin/env python3
"""--screen measured three ways on one device, one JSON line:

  kernel      the screen's launch (key fill + distance kernel with the key sink) beside the distance kernel of --ed_thr
              alone on the same batch -- C2's shape, 1 000 reads of 50 kb against 24 templates -- alternating in one
              process, each launch between two HIP events (sd_screen_kernel_bench)
  chromosome  one synthetic sequence (--mb, default 50 Mb) with --fraction (2 %) of its length in arrays of mutated
              monomers: the plain file job and the job with --screen 40, alternating in this process: wall time, the
              device time per phase, bases decomposed
  satellite   C2's reads with a threshold every chunk passes against the plain job: what asking costs when nothing can be
              skipped

Warm-up runs first, then --reps (default 5) timed ones; medians with minimum and maximum.

usage: python tools/screen_bench.py [--reps 5] [--warmup 2] [--mb 50] [--fraction 0.02] [--threads 16] [--device 0]
                                    [--only kernel|chromosome|satellite]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stringdecomposer_amd import lib, synth   # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def chromosome(monos, n_bases, fraction, seed):
    """Random bases with `fraction` of the length in ten arrays of mutated monomers (synth.make_reads), evenly spaced."""
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n_bases)]
    n_arr = 10
    alen = max(1000, int(n_bases * fraction / n_arr))
    _, arrays = synth.make_reads(monos, n_arr, read_len=alen, seed=seed)
    for i, a in enumerate(arrays):
        at = (2 * i + 1) * n_bases // (2 * n_arr) - len(a) // 2
        seq[at:at + len(a)] = np.frombuffer(a, dtype=np.uint8)
    return seq.tobytes()


def file_jobs(reads_fa, mono_fa, d, variants, warmup, reps, threads, device):
    """variants: {name: run_files keywords}; the jobs alternate.  -> per variant wall / phase times."""
    out = {k: {"wall_ms": [], "screen_ms": [], "screen_kernel_ms": [], "fill_ms": [], "trace_ms": [], "ident_ms": []} for k in variants}
    for r in range(-warmup, reps):
        for name, kw in variants.items():
            o = [os.path.join(d, "%s_%s.tsv" % (name, x)) for x in ("raw", "final", "alt", "screen")]
            t0 = time.perf_counter()
            lib.run_files(reads_fa, mono_fa, o[0], o[1], o[2], threads=threads, device=device,
                          screen_tsv_out=o[3] if kw.get("screen") is not None else None, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            if r < 0:
                continue
            s = lib.last_run_stats()
            v = out[name]
            v["wall_ms"].append(wall)
            v["fill_ms"].append(s["fill_ms"]); v["trace_ms"].append(s["trace_ms"]); v["ident_ms"].append(s["ident_ms"])
            v["screen_ms"].append(s.get("screen_ms", 0.0)); v["screen_kernel_ms"].append(s.get("screen_kernel_ms", 0.0))
            if kw.get("screen") is not None:
                v["counts"] = lib.last_run_screen()
            v["raw_bytes"] = os.path.getsize(o[0])
    return {k: {m: (spread(x) if isinstance(x, list) else x) for m, x in v.items()} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mb", type=float, default=50.0)
    ap.add_argument("--fraction", type=float, default=0.02)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--only", choices=["kernel", "chromosome", "satellite"], default=None)
    a = ap.parse_args()
    mn, ms = synth.make_monomers(12, seed=1)
    res = {}
    c2 = None
    if a.only in (None, "kernel", "satellite"):
        c2 = synth.make_reads(ms, 1000, read_len=50000, seed=1)
    if a.only in (None, "kernel"):
        s = lib.Screener(ms, device=a.device)
        k = s.chunks(c2[1])
        sc_ms, d_ms = s.kernel_bench(a.warmup, a.reps)
        res["kernel"] = {"kernel": s.kernel(), "chunks": len(k.key), "templates": 2 * len(ms), "screen_ms": spread(sc_ms),
                         "edthr_dist_ms": spread(d_ms), "ratio": statistics.median(sc_ms) / statistics.median(d_ms)}
        s.close()
    with tempfile.TemporaryDirectory() as d:
        mono_fa = os.path.join(d, "m.fa")
        synth.write_fasta(mono_fa, mn, ms)
        if a.only in (None, "chromosome"):
            fa = os.path.join(d, "chr.fa")
            synth.write_fasta(fa, ["chr"], [chromosome(ms, int(a.mb * 1e6), a.fraction, 5)], width=80)
            res["chromosome"] = file_jobs(fa, mono_fa, d, {"plain": {}, "screen40": {"screen": 40}}, a.warmup, a.reps, a.threads, a.device)
            res["chromosome"]["input"] = {"bases": int(a.mb * 1e6), "array_fraction": a.fraction}
        if a.only in (None, "satellite"):
            fa = os.path.join(d, "c2.fa")
            synth.write_fasta(fa, c2[0], c2[1], width=80)
            res["satellite"] = file_jobs(fa, mono_fa, d, {"plain": {}, "screen_all": {"screen": 2048}}, a.warmup, a.reps, a.threads, a.device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
