#!/usr/bin/env python3
"""Wall time of the command line on a C3-shaped read set (reads x 50 kb, 12 monomers, -b 5000) with one pipeline and
with several in the process (--gpus N / --devices LIST); every run is a fresh process, as a user runs it.

    python tools/multi_device_cli_timing.py --reads 2000 --repeat 3 --lists 0 0,0 --gpus 1 2 4 8

Prints one JSON line per configuration: median / min / all wall seconds (the configurations run interleaved)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=50000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--lists", nargs="*", default=["0", "0,0"], help="--devices lists to time")
    ap.add_argument("--gpus", nargs="*", type=int, default=[], help="--gpus values to time (those above the device count are skipped)")
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    from stringdecomposer_amd import lib, synth
    ndev = lib.device_count()
    with tempfile.TemporaryDirectory() as d:
        mn, ms = synth.make_monomers(12, seed=1)
        rn, rs = synth.make_reads(ms, a.reads, read_len=a.read_len, seed=1)
        rfa, mfa = os.path.join(d, "r.fa"), os.path.join(d, "m.fa")
        synth.write_fasta(rfa, rn, rs, width=80)
        synth.write_fasta(mfa, mn, ms)
        del rs
        runs = [("none", [])] + [("--devices " + x, ["--devices", x]) for x in a.lists]
        runs += [("--gpus %d" % g, ["--gpus", str(g)]) for g in a.gpus if g <= ndev]
        secs_of = {tag: [] for tag, _ in runs}
        for r in range(a.repeat):   # (interleaved: every round runs each configuration once)
            for tag, extra in runs:
                out = os.path.join(d, "o")
                t0 = time.perf_counter()
                p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), rfa, mfa, "-o", out,
                                    "-t", str(a.threads), "-b", "5000"] + extra,
                                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=a.timeout)
                secs_of[tag].append(time.perf_counter() - t0)
                if p.returncode != 0:
                    print(json.dumps({"run": tag, "rc": p.returncode, "stderr": p.stderr.decode()[-500:]}), flush=True)
                    return 1
        for tag, secs in secs_of.items():
            print(json.dumps({"run": tag, "bp": a.reads * a.read_len, "devices_visible": ndev, "median_s": statistics.median(secs),
                              "min_s": min(secs), "all_s": [round(x, 3) for x in secs]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
