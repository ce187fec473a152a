#!/usr/bin/env python3
"""Wall time from submit to the end of profile() of a final-mode stream that also profiles, two ways, for ONE resident
lib.DeviceReads of 200 reads x 50 kb against 12 monomers (bench.py's generators):

  --mode host     lib.Stream(final=True, profile=True): rows and profile through the host (the reads come down for the
                  profile pass and go up again: csrc/sd_nw.hip, nw_profile_device)
  --mode device   lib.Stream(final=True, device_final=True, device_profile=True): rows selected and profiles folded on
                  the device (csrc/sd_final_prof_dev.hip), the rows left there as torch tensors

  python tools/device_profile_timing.py --mode host|device [--steps 8] [--warmup 3] [--threads N]

Every job is timed on its own: submit, collect, profile(reset=True).  One timing run per process: prints ONE JSON line.
--mode host also runs on a commit without device profiles, which is the baseline.  The fold kernel's own time: one run
under `rocprofv3 --kernel-trace --stats -- python tools/device_profile_timing.py --mode ...` (kernel sd_nw_profile).
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

from stringdecomposer_amd import formats, lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("host", "device"), required=True)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=200)
    ap.add_argument("--read-len", type=int, default=50000)
    ap.add_argument("--monomers", type=int, default=12)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch
    threads = args.threads if args.threads > 0 else max(1, min(32, len(os.sched_getaffinity(0))))
    mn, ms = synth.make_monomers(args.monomers, seed=args.seed)
    rn, rs = synth.make_reads(ms, args.reads, read_len=args.read_len, seed=args.seed)
    keep = torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    job = lib.DeviceReads(keep, [len(s) for s in rs], stream=0)
    dev = args.mode == "device"
    kw = dict(final=True, mono_names=mn, threads=threads)
    st = lib.Stream(ms, device_final=True, device_profile=True, **kw) if dev else lib.Stream(ms, profile=True, **kw)

    def one():
        t0 = time.perf_counter()
        st.submit(job)
        rows = st.collect_final_device().n_rows if dev else len(st.collect().rows)
        prof = st.profile(reset=True)
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, rows, sum(formats.profile_instances(c) for c in prof.counts)

    for _ in range(args.warmup):
        one()
    s0 = st.stats()
    runs = [one() for _ in range(args.steps)]
    s1 = st.stats()
    st.close()
    assert all(r[1] == r[2] == runs[0][1] for r in runs), "every kept row is one instance"
    ms_job = sorted(r[0] for r in runs)
    out = {"mode": args.mode, "steps": args.steps, "warmup": args.warmup, "host_threads": threads, "reads": args.reads,
           "read_len": args.read_len, "rows": int(runs[0][1]), "ms_per_job_sorted": [round(x, 3) for x in ms_job],
           "ms_per_job_median": round(ms_job[len(ms_job) // 2], 3), "fallback_blocks": int(s1["fallback_blocks"]),
           "bases_per_job": sum(len(s) for s in rs)}
    for k in ("profile_pairs_device", "profile_pairs_host", "profile_text_to_host", "profile_ms"):
        if k in s1:
            out[k + "_per_job"] = round((s1[k] - s0[k]) / args.steps, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
