#!/usr/bin/env python3
"""Time of Stream(final=True) on the C4 shape (64 monomers x 256 reads x 50 kb, --second-best) next to lib.run_files on
the same reads, in one process on one GPU.  Prints one JSON line.

  stream_final_ms     one job at a time: submit + collect of the final rows and the _alt matrix (no text)
  stream_final_imap_ms  per job, `--jobs` jobs pipelined through imap(depth=2)
  stream_raw_ms       the same job through the raw stream (the DP rows only), for the cost of the identities
  run_files_ms        sd_run_files: FASTA on tmpfs -> the three TSV files (what bench.py --config c4-second-best times)

The stream's final text is checked once against the run_files output (final TSV byte for byte).  Steps of the three
paths alternate, medians are reported.

usage: python tools/stream_final_bench.py [--steps 5] [--jobs 4] [--reads 256] [--threads 16]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stringdecomposer_amd import formats, lib, main as sdmain, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--reads", type=int, default=256)
    ap.add_argument("--monomers", type=int, default=64)
    ap.add_argument("--read-len", type=int, default=50000)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    mn, ms = synth.make_monomers(args.monomers, seed=1)
    rn, rs = synth.make_reads(ms, args.reads, read_len=args.read_len, seed=1)
    bp = sum(len(x) for x in rs)
    coef = sdmain._lr_coef()
    kw = dict(threads=args.threads, device=0)
    rset = lib.ReadSet(rs)
    d = tempfile.mkdtemp(prefix="sd_stream_final_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        rf, mf = os.path.join(d, "reads.fa"), os.path.join(d, "monomers.fa")
        synth.write_fasta(rf, rn, rs, width=80)
        synth.write_fasta(mf, mn, ms)
        outs = [os.path.join(d, x) for x in ("raw.tsv", "final.tsv", "alt.tsv")]

        def run_files():
            for x in outs:
                if os.path.exists(x):
                    os.unlink(x)
            t0 = time.perf_counter()
            lib.run_files(rf, mf, *outs, second_best=True, lr_coef=coef, **kw)
            return time.perf_counter() - t0

        fin_st = lib.Stream(ms, final=True, mono_names=mn, second_best=True, lr_coef=coef, **kw)
        raw_st = lib.Stream(ms, **kw)

        def one(st):
            t0 = time.perf_counter()
            st.submit(rset)
            out = st.collect()
            return time.perf_counter() - t0, out

        def piped():
            t0 = time.perf_counter()
            for _ in fin_st.imap([rset] * args.jobs, depth=2):
                pass
            return (time.perf_counter() - t0) / args.jobs

        # warm-up (all three engines of each stream -- consecutive jobs go to consecutive engines --, pinned blocks, the
        # cached pipeline of run_files) and the parity check
        run_files()
        _, fr = one(fin_st)
        for _ in range(3):
            one(raw_st)
        piped()
        fin, _ = formats.final_rows((fr.rows, fr.row_off, None), rn, fin_st.keys())
        with open(outs[1], "rb") as f:
            parity = formats.format_final(fin).encode() == f.read()
        t = {"stream_final": [], "stream_final_imap": [], "stream_raw": [], "run_files": []}
        s0 = fin_st.stats()
        for _ in range(args.steps):
            t["stream_final"].append(one(fin_st)[0])
            t["stream_final_imap"].append(piped())
            t["stream_raw"].append(one(raw_st)[0])
            t["run_files"].append(run_files())
        s1 = fin_st.stats()
        jobs = s1["jobs"] - s0["jobs"]
        res = {"workload": "C4 shape: %d monomers x %d reads x %d bp, --second-best" % (args.monomers, args.reads, args.read_len),
               "bp": bp, "threads": args.threads, "steps": args.steps, "final_text_equals_run_files": parity,
               "final_rows": int(len(fr.rows)), "alt_shape": list(fr.alt.shape),
               "stream_ident_pairs_per_job": (s1["ident_pairs"] - s0["ident_pairs"]) / jobs,
               "stream_fallback_blocks": s1["fallback_blocks"] - s0["fallback_blocks"],
               "stream_ident_ms_per_job": (s1["ident_ms"] - s0["ident_ms"]) / jobs}
        for k, v in t.items():
            m = statistics.median(v)
            res[k + "_ms"] = round(m * 1e3, 2)
            res[k + "_ms_all"] = [round(x * 1e3, 2) for x in v]
            res[k + "_mbp_per_s"] = round(bp / m / 1e6, 1)
        fin_st.close()
        raw_st.close()
        print(json.dumps(res))
        return 0 if parity else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
