#!/usr/bin/env python3
"""Wall time of the command line with and without --profile (developer tool): a C2-shaped read set (default 1 000 reads
x 50 kb = 50 Mbp, 12 monomers, -t 16), every run a fresh process, the two configurations interleaved.  Prints one line
per run with the library's own time for the profile pass ("[sd timing] column profiles"), then the medians, and checks
that the three TSV files are byte-identical with and without the flag.
usage: python tools/profile_cli_timing.py [--reads N] [--repeat R] [--second-best] [--out DIR]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stringdecomposer_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--read-len", type=int, default=50000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--second-best", action="store_true")
    ap.add_argument("--out", default=None, help="directory for the inputs and outputs (default: a temporary one)")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    d = a.out or tempfile.mkdtemp()
    os.makedirs(d, exist_ok=True)
    mn, ms = synth.make_monomers(12, seed=1)
    rn, rs = synth.make_reads(ms, a.reads, read_len=a.read_len, seed=1)
    rfa, mfa = os.path.join(d, "r.fa"), os.path.join(d, "m.fa")
    synth.write_fasta(rfa, rn, rs, width=80)
    synth.write_fasta(mfa, mn, ms)
    extra = ["--second-best"] if a.second_best else []
    times = {"no flag": [], "--profile": []}
    outs = {}
    for trial in range(a.repeat):
        for cfg in ("no flag", "--profile"):
            o = os.path.join(d, "out_" + ("plain" if cfg == "no flag" else "profile"))
            args = [sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), rfa, mfa, "-o", o, "-t", str(a.threads)]
            args += extra + (["--profile"] if cfg == "--profile" else [])
            t0 = time.perf_counter()
            p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.timeout,
                               env=dict(os.environ, SD_TIMING="1"))
            dt = time.perf_counter() - t0
            if p.returncode != 0:
                sys.stdout.write(p.stdout.decode(errors="replace")[-4000:])
                raise SystemExit("%s: exit status %d" % (cfg, p.returncode))
            prof = [x for x in p.stdout.decode().splitlines() if "column profiles" in x]
            times[cfg].append(dt)
            print("run %d %-9s %.3f s  %s" % (trial, cfg, dt, " | ".join(x.replace("[sd timing] ", "").strip() for x in prof)),
                  flush=True)
            outs[cfg] = o
    for cfg, v in times.items():
        print("%-9s median %.3f s  min %.3f s  runs %s" % (cfg, statistics.median(v), min(v), " ".join("%.3f" % x for x in v)))
    for f in ("final_decomposition_raw.tsv", "final_decomposition.tsv", "final_decomposition_alt.tsv"):
        same = open(os.path.join(outs["no flag"], f), "rb").read() == open(os.path.join(outs["--profile"], f), "rb").read()
        print("%s identical with and without --profile: %s" % (f, same))


if __name__ == "__main__":
    main()
