#!/usr/bin/env python3
"""Time per job and host CPU per job of a final-mode stream, two ways:

  --mode host     lib.Stream(final=True): reads submitted from host memory, the final rows collected into host memory
  --mode device   ONE resident lib.DeviceReads -> lib.Stream(final=True, device_final=True) -> imap(device=True): the
                  final rows selected on the device (csrc/sd_final_dev.hip) and left there as torch tensors

for two shapes (bench.py's generators):

  --shape c2      1 000 reads x 50 kb, 12 monomers, light mode
  --shape c4      256 reads x 50 kb, 64 monomers, --second-best

  python tools/device_final_timing.py --shape c2|c4 --mode host|device [--steps 12] [--warmup 4] [--threads N] [--depth D]

One timing run per process: prints ONE JSON line.  Run it several times (each under its own timeout) for the spread;
--mode host also runs on a commit without device-final streams, which is the baseline.  The selection kernels' own
time: one run under `rocprofv3 --kernel-trace --stats -- python tools/device_final_timing.py --shape c4 --mode device`
(kernels sd_final_*).
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

SHAPES = {"c2": dict(monomers=12, reads=1000, second_best=False), "c4": dict(monomers=64, reads=256, second_best=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--mode", choices=("host", "device"), required=True)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--read-len", type=int, default=50000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--depth", type=int, default=2, help="jobs outstanding before the oldest is collected")
    args = ap.parse_args()
    shape = SHAPES[args.shape]
    threads = args.threads if args.threads > 0 else max(1, min(32, len(os.sched_getaffinity(0))))
    mn, ms = synth.make_monomers(shape["monomers"], seed=args.seed)
    rn, rs = synth.make_reads(ms, shape["reads"], read_len=args.read_len, seed=args.seed)
    dev = args.mode == "device"
    kw = dict(final=True, mono_names=mn, second_best=shape["second_best"], threads=threads)
    if dev:
        import torch
        keep = torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        job = lib.DeviceReads(keep, [len(s) for s in rs], stream=0)
        st = lib.Stream(ms, device_final=True, **kw)
    else:
        job = lib.ReadSet(rs)
        st = lib.Stream(ms, **kw)

    def run(k):
        n = 0
        for out in st.imap([job] * k, depth=args.depth, device=dev):
            n = out.n_rows if dev else len(out.rows)
        return n

    rows = run(args.warmup)
    s0 = st.stats()
    c0, t0 = time.process_time(), time.perf_counter()
    assert run(args.steps) == rows
    if dev:
        torch.cuda.synchronize()   # (the last copy is on torch's stream)
    t1, c1 = time.perf_counter(), time.process_time()
    s1 = st.stats()
    st.close()
    per = {k: round((s1[k] - s0[k]) / args.steps, 4) for k in
           ("fill_ms", "trace_ms", "compact_ms", "run_ms", "ident_ms", "host_pack_ms", "host_wait_ms", "host_assemble_ms",
            "submit_ms", "collect_ms")}
    print(json.dumps({"shape": args.shape, "mode": args.mode, "steps": args.steps, "warmup": args.warmup, "host_threads": threads,
                      "depth": args.depth, "ms_per_job": round((t1 - t0) * 1e3 / args.steps, 3),
                      "host_cpu_ms_per_job": round((c1 - c0) * 1e3 / args.steps, 3), "rows": int(rows),
                      "fallback_blocks": int(s1["fallback_blocks"]), "stats_per_job": per}))


if __name__ == "__main__":
    main()
