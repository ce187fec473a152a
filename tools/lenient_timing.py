#!/usr/bin/env python3
"""Timing of the lenient mode (developer tool; the numbers of profiles/lenient_timing.md).

  python tools/lenient_timing.py job [--root DIR] [--lower] [--reps 5] [--threads 16]
      The file job of bench.py's C2 shape (1000 reads x 50 kb, 12 monomers) through lib.run_files: FASTA in, three
      TSVs out.  One warm-up run, then --reps timed runs; prints one JSON line with the wall ms of each.  --root DIR
      imports the package of another checkout (the parent commit, built there), so that two trees can be compared on
      the same machine by alternating processes.  --lower: the all-lower-case copy of the reads, with lenient=True.
  python tools/lenient_timing.py kernel [--mb 50]
      sd_normalize_dev (out of place, then in place) and the device packer on the same --mb MB of reads in device memory,
      three times each; meant to run under `rocprofv3 --kernel-trace --stats`, which gives the kernels' times."""
import argparse
import json
import os
import sys
import tempfile
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["job", "kernel"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--lower", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--mb", type=int, default=50)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from stringdecomposer_amd import lib, synth
    mn, ms = synth.make_monomers(12, seed=1)
    if a.mode == "job":
        rn, rs = synth.make_reads(ms, 1000, read_len=50000, seed=1)
        d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        rfa, mfa = os.path.join(d, "r.fa"), os.path.join(d, "m.fa")
        with open(rfa, "wb") as f:
            for n, s in zip(rn, rs):
                s = bytes(s)
                f.write(b">" + n.encode() + b"\n" + (s.lower() if a.lower else s) + b"\n")
        synth.write_fasta(mfa, mn, ms)
        o = [os.path.join(d, x) for x in ("raw.tsv", "final.tsv", "alt.tsv")]
        kw = dict(threads=a.threads)
        if a.lower:
            kw["lenient"] = True
        ms_ = []
        for i in range(a.reps + 1):
            t0 = time.perf_counter()
            lib.run_files(rfa, mfa, o[0], o[1], o[2], **kw)
            ms_.append((time.perf_counter() - t0) * 1e3)
        out = {"root": os.path.abspath(a.root), "lower": a.lower, "warmup_ms": round(ms_[0], 2),
               "ms": [round(x, 2) for x in ms_[1:]], "median_ms": round(sorted(ms_[1:])[len(ms_[1:]) // 2], 2),
               "min_ms": round(min(ms_[1:]), 2), "max_ms": round(max(ms_[1:]), 2), "raw_bytes": os.path.getsize(o[0])}
        if hasattr(lib, "last_run_input_stats"):
            out["input"] = lib.last_run_input_stats()
        print(json.dumps(out), flush=True)
        for x in o + [rfa, mfa]:
            os.remove(x)
        os.rmdir(d)
        return
    import numpy as np
    import torch
    n_reads = a.mb * 20
    rn, rs = synth.make_reads(ms, 50, read_len=50000, seed=1)
    text = b"".join(bytes(s) for s in rs).lower() * (n_reads // 50)
    lens = [50000] * n_reads
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    out = torch.empty_like(t)
    stats = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    for _ in range(3):
        lib.normalize_device(t, lens, out=out, stats=stats)
    for _ in range(3):
        lib.normalize_device(t, lens, stats=stats)
    torch.cuda.synchronize()
    off = np.arange(0, len(text), 5000, dtype=np.int64)
    ln = np.minimum(5500, len(text) - off).astype(np.int32)
    for _ in range(3):
        lib.pack_bases_device(t, off, ln)
    torch.cuda.synchronize()
    print(json.dumps({"bytes": len(text), "stats": stats.tolist()}), flush=True)


if __name__ == "__main__":
    main()
