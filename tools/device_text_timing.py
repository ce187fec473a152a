#!/usr/bin/env python3
"""Where the text of a C4-shaped --second-best job is cheapest to make (profiles/device_text_timing.md).

One job of 256 reads x 50 kb against 64 monomers goes through lib.Stream(final=True, device_final=True, second_best=True);
its DeviceFinalRows are then formatted

  device   lib.format_final_device with one lib.TextTables: the size call (length pass, scan, 32 bytes to the host) and the
           write call, timed with device events around each and with a host clock around both ending in a synchronise
  copy     the two texts to pinned host memory (torch, non_blocking, then a synchronise)
  host     lib.format_final_host(threads=16) on the same rows in host memory
  python   formats.final_rows + format_final + format_alt on every 100th row, scaled by 100

  python tools/device_text_timing.py [--reps 7] [--threads 16] [--kernels-only]

Prints ONE JSON line.  --kernels-only: two device formats and nothing else, for a run of its own under
`rocprofv3 --kernel-trace --stats` (kernels sd_text_*).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import stringdecomposer_amd  # noqa: E402

stringdecomposer_amd.prefer_queue_thread_dispatch()   # as bench.py, before any HIP call

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stringdecomposer_amd import formats, lib, synth  # noqa: E402


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reads", type=int, default=256)
    ap.add_argument("--read-len", type=int, default=50000)
    ap.add_argument("--monomers", type=int, default=64)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    mn, ms = synth.make_monomers(args.monomers, seed=1)
    rn, rs = synth.make_reads(ms, args.reads, read_len=args.read_len, seed=1)
    st = lib.Stream(ms, final=True, mono_names=mn, second_best=True, device_final=True, threads=args.threads)
    st.submit(rs)
    dfr = st.collect_final_device()
    keys = st.keys()
    torch.cuda.synchronize()
    tables = lib.TextTables(rn, keys)
    L = lib.load()
    n, nr, nk = dfr.n_rows, len(rn), len(keys)
    dev = dfr.rows.device
    pos = [torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev),
           torch.empty(nr + 1, dtype=torch.int64, device=dev), torch.empty(nr + 1, dtype=torch.int64, device=dev)]
    err = C.create_string_buffer(1024)
    fb, ab = C.c_int64(), C.c_int64()
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    s = torch.cuda.current_stream(dev)

    def size():
        rc = L.sd_text_final_size_dev(tables.h, p(dfr.rows), n, p(dfr.row_off), p(dfr.alt), nk, 0, C.c_void_p(s.cuda_stream),
                                      p(pos[0]), p(pos[1]), p(pos[2]), p(pos[3]), C.byref(fb), C.byref(ab), err, 1024)
        assert rc == 0, err.value

    size()
    ft = torch.empty(fb.value, dtype=torch.uint8, device=dev)
    at = torch.empty(ab.value, dtype=torch.uint8, device=dev)

    def write():
        rc = L.sd_text_final_write_dev(tables.h, p(dfr.rows), n, p(dfr.alt), nk, 0, C.c_void_p(s.cuda_stream), p(pos[0]), p(pos[1]),
                                       p(ft), fb.value, p(at), ab.value, err, 1024)
        assert rc == 0, err.value

    write()
    torch.cuda.synchronize()
    if args.kernels_only:
        size()
        write()
        torch.cuda.synchronize()
        print(json.dumps({"rows": n, "keys": nk, "final_bytes": fb.value, "alt_bytes": ab.value}))
        return
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_size, t_write, t_both, t_copy = [], [], [], []
    h_ft = torch.empty(fb.value, dtype=torch.uint8, pin_memory=True)
    h_at = torch.empty(ab.value, dtype=torch.uint8, pin_memory=True)
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        size()
        ev[1].record()
        write()
        ev[2].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        h_ft.copy_(ft, non_blocking=True)
        h_at.copy_(at, non_blocking=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_size.append(ev[0].elapsed_time(ev[1]))
        t_write.append(ev[1].elapsed_time(ev[2]))
        t_both.append((t1 - t0) * 1e3)
        t_copy.append((t2 - t1) * 1e3)
    fr = dfr.to_host()
    t_host = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        host = lib.format_final_host(fr, rn, keys, threads=args.threads)
        t_host.append((time.perf_counter() - t0) * 1e3)
    assert h_ft.numpy().tobytes() == host[0] and h_at.numpy().tobytes() == host[1], "device text differs from the host twin"
    sample = lib.FinalRows(fr.rows[::100], None, fr.alt[::100])
    t0 = time.perf_counter()
    fin, alt = formats.final_rows(sample, rn, keys)
    py = (formats.format_final(fin), formats.format_alt(alt))
    t_py = (time.perf_counter() - t0) * 1e3 * (n / max(1, len(sample.rows)))
    tables.close()
    st.close()
    out = {"rows": n, "keys": nk, "final_bytes": fb.value, "alt_bytes": ab.value, "threads": args.threads,
           "size_call_ms": [round(x, 3) for x in sorted(t_size[1:])], "write_call_ms": [round(x, 3) for x in sorted(t_write[1:])],
           "device_both_host_clock_ms": [round(x, 3) for x in sorted(t_both[1:])], "copy_to_pinned_ms": [round(x, 3) for x in sorted(t_copy[1:])],
           "host_twin_ms": [round(x, 2) for x in sorted(t_host[1:])], "python_1pct_scaled_ms": round(t_py, 0),
           "python_sample_bytes": len(py[0]) + len(py[1]),
           "write_GBps": round((fb.value + ab.value) / med(t_write[1:]) / 1e6, 1),
           "copy_GBps": round((fb.value + ab.value) / med(t_copy[1:]) / 1e6, 1),
           "device_plus_copy_ms": round(med(t_both[1:]) + med(t_copy[1:]), 3), "host_twin_median_ms": round(med(t_host[1:]), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
