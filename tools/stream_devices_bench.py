#!/usr/bin/env python3
"""Time of Stream(devices=[...]) next to the plain stream on the same GPUs.  Two workloads:

  c2   the C2 shape of bench.py (12 monomers x 1000 reads x 50 kb), raw rows
  c4   the C4 shape (64 monomers x 256 reads x 50 kb), final=True, second_best=True

For every workload, the plain stream and one stream per device list given (e.g. `--devices 0 0,0`) take turns, each
run in a fresh child process (with several streams alive in one process, the one created first ran C4 4-5 ms per job
faster than an identical one created after it): `--runs` rounds, each stream once per round.  A run warms up, then
times `--steps` steps of `--jobs` jobs through imap (default depth).  Per stream it reports the median over the runs
of each run's median ms per job, the run medians, Mbp/s, and per run and entry the batches dealt and the device busy ms of the timed steps
(sd_stream_device_stats).  The outputs of every run are checked against the plain stream's (raw: the row count of every
job; final: sha256 of the typed rows and the _alt matrix).  Prints one JSON line.

usage: python tools/stream_devices_bench.py [--devices 0 0,0] [--config c2 c4] [--runs 3] [--steps 5] [--jobs 6]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stringdecomposer_amd import lib, main as sdmain, synth  # noqa: E402

SHAPES = {"c2": dict(monomers=12, reads=1000, final=False), "c4": dict(monomers=64, reads=256, final=True)}


def run_one(name, devices, args):
    """One stream (devices None: the plain stream) on one workload, in this process: warm-up, then `--steps` steps of
    `--jobs` jobs through imap.  Returns ms per job of every step, per-entry stats of the timed steps and a digest of
    the outputs of the last step (raw: the row count of every job; final: sha256 of the typed rows and _alt)."""
    sh = SHAPES[name]
    mn, ms = synth.make_monomers(sh["monomers"], seed=1)
    _, rs = synth.make_reads(ms, sh["reads"], read_len=args.read_len, seed=1)
    rset = lib.ReadSet(rs)
    kw = dict(threads=args.threads, device=0)
    if sh["final"]:
        kw.update(final=True, mono_names=mn, second_best=True, lr_coef=sdmain._lr_coef())
    st = lib.Stream(ms, devices=devices, **kw)
    try:
        def step():
            t0 = time.perf_counter()
            out = list(st.imap([rset] * args.jobs))
            return (time.perf_counter() - t0) / args.jobs, out

        for _ in range(2):   # warm-up: every engine of every entry gets its buffers
            step()
        d0 = st.device_stats()
        times = []
        for _ in range(args.steps):
            t, out = step()
            times.append(t)
        d1 = st.device_stats()
        if sh["final"]:
            h = hashlib.sha256()
            for fr in out:
                h.update(fr.rows.tobytes())
                h.update(fr.alt.tobytes())
            digest = h.hexdigest()
        else:
            digest = [int(n) for n in out]
        return {"bp": rset.bp, "ms": [round(t * 1e3, 3) for t in times], "digest": digest,
                "entries": [{"device": y["device"], "batches": y["batches"] - x["batches"],
                             "busy_ms": round(y["busy_ms"] - x["busy_ms"], 1)} for x, y in zip(d0, d1)]}
    finally:
        st.close()


def run_config(name, args):
    """The plain stream and every device list, each in a fresh child process, `--runs` rounds in turn."""
    lists = ["plain"] + args.devices
    runs = {d: [] for d in lists}
    for _ in range(args.runs):
        for d in lists:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", name, d, "--steps", str(args.steps),
                   "--jobs", str(args.jobs), "--read-len", str(args.read_len), "--threads", str(args.threads)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.child_timeout, check=True)
            runs[d].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    sh = SHAPES[name]
    ref = runs["plain"][0]["digest"]
    parity = [all(x["digest"] == ref for x in runs[d]) for d in lists]
    res = {"workload": "%s: %d monomers x %d reads x %d bp%s" % (name, sh["monomers"], sh["reads"], args.read_len,
                                                                ", final, --second-best" if sh["final"] else ""),
           "bp": runs["plain"][0]["bp"], "jobs_per_step": args.jobs, "steps": args.steps, "runs": args.runs,
           "outputs_equal_plain_stream": dict(zip(lists, parity)), "streams": []}
    for d in lists:
        med = [statistics.median(x["ms"]) for x in runs[d]]   # one median per run (process)
        m = statistics.median(med)
        res["streams"].append({"devices": d, "ms_per_job": round(m, 2), "ms_per_job_runs": [round(x, 2) for x in med],
                               "mbp_per_s": round(res["bp"] / m / 1e3, 1), "entries": [x["entries"] for x in runs[d]]})
    return res, all(parity)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", nargs="+", default=["0", "0,0"], help="device lists, each comma-separated")
    ap.add_argument("--config", nargs="+", default=["c2", "c4"], choices=sorted(SHAPES))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=6)
    ap.add_argument("--read-len", type=int, default=50000)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--runs", type=int, default=3, help="child processes per stream and workload")
    ap.add_argument("--child-timeout", type=float, default=600)
    ap.add_argument("--one", nargs=2, metavar=("CONFIG", "DEVICES"), help=argparse.SUPPRESS)   # (a child's job)
    args = ap.parse_args()
    if args.one:
        name, d = args.one
        print(json.dumps(run_one(name, None if d == "plain" else [int(x) for x in d.split(",")], args)))
        return 0
    out, ok = {"threads": args.threads, "configs": []}, True
    for c in args.config:
        r, good = run_config(c, args)
        out["configs"].append(r)
        ok = ok and good
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
