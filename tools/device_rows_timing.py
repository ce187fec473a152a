#!/usr/bin/env python3
"""Step time and host CPU of the C2 shape (1 000 reads x 50 kb, 12 monomers, default scoring, bench.py's generator)
through lib.Stream.imap with ONE resident lib.DeviceReads as input, the rows returned in host memory or left on the
device (Stream(device_rows=True), imap(device=True)).

  python tools/device_rows_timing.py --rows host|device [--steps 20] [--warmup 5] [--threads N] [--depth D]

One timing run per process: prints ONE JSON line {"rows_form", "ms_per_step", "host_cpu_ms_per_step", "rows",
"stats_per_step"}.  Run it several times (each under its own timeout) for the spread; --rows host also runs on a commit
without device rows.  The assembly kernels' own time: one run under `rocprofv3 --kernel-trace --stats -- python
tools/device_rows_timing.py --rows device` (kernels sd_rows_* and sd_seam_*).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import stringdecomposer_amd  # noqa: E402

stringdecomposer_amd.prefer_queue_thread_dispatch()   # as bench.py, before any HIP call

from stringdecomposer_amd import lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=("host", "device"), required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--read-len", type=int, default=50000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--depth", type=int, default=-1, help="jobs outstanding before the oldest is collected (default: imap's)")
    args = ap.parse_args()
    import torch
    threads = args.threads if args.threads > 0 else max(1, min(32, len(os.sched_getaffinity(0))))
    mn, ms = synth.make_monomers(12, seed=args.seed)
    rn, rs = synth.make_reads(ms, args.reads, read_len=args.read_len, seed=args.seed)
    keep = torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    job = lib.DeviceReads(keep, [len(s) for s in rs], stream=0)
    dev = args.rows == "device"
    st = lib.Stream(ms, threads=threads, device_rows=True) if dev else lib.Stream(ms, threads=threads)

    def run(k):
        n = 0
        kw = {} if args.depth < 0 else {"depth": args.depth}
        for out in (st.imap([job] * k, device=True, **kw) if dev else st.imap([job] * k, **kw)):
            n = out.n_rows if dev else out
        return n

    rows = run(args.warmup)
    s0 = st.stats()
    c0, t0 = time.process_time(), time.perf_counter()
    assert run(args.steps) == rows
    if dev:
        torch.cuda.synchronize()   # (the last scatter is on torch's stream)
    t1, c1 = time.perf_counter(), time.process_time()
    s1 = st.stats()
    st.close()
    per = {k: round((s1[k] - s0[k]) / args.steps, 4) for k in
           ("fill_ms", "trace_ms", "compact_ms", "run_ms", "host_pack_ms", "host_wait_ms", "host_assemble_ms", "submit_ms",
            "collect_ms")}
    print(json.dumps({"rows_form": args.rows, "steps": args.steps, "warmup": args.warmup, "host_threads": threads, "depth": args.depth,
                      "ms_per_step": round((t1 - t0) * 1e3 / args.steps, 3),
                      "host_cpu_ms_per_step": round((c1 - c0) * 1e3 / args.steps, 3), "rows": int(rows),
                      "stats_per_step": per}))
    del keep


if __name__ == "__main__":
    main()
