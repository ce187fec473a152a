#!/usr/bin/env python3
"""Start-term floors per row of the narrow u16 fill on the benchmark's read set, computed on the host (no GPU):
the levels by read symbol (SD_FILL_SYMBOL_LEVEL=1, the form before the pair rule) against the levels by previous and
current symbol, with the four level groups the kernel has (FL, FL - 4, FL - 8, FL - 12 slots).

usage: python tools/floors_per_row.py [reads [read_len [monomers [seed]]]]     (default: 1000 50000 12 1 = C2)

A chunk's row 0 runs no floor (it is computed by another formula) but is a row of the launch, so it counts in the
denominator like every row; row 1 takes the per-symbol level in both forms; a row behind an N does too."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from stringdecomposer_amd import lib, synth   # noqa: E402

FL_LEVELS = (12, 16, 20, 24, 28)   # FlLevels of sd_fast.hpp (P = 30..40)
STEP = 4


def group_floors(fl, need):
    """Floors a row applies when it needs the first `need` slots: the smallest of fl, fl - 4, fl - 8, fl - 12 (>= 1) covering it."""
    lv = 0
    while lv < 3 and fl - (lv + 1) * STEP >= max(1, need):
        lv += 1
    return max(1, fl - lv * STEP)


def main():
    a = [int(x) for x in sys.argv[1:]] + [None] * 4
    n_reads, read_len, n_mono, seed = a[0] or 1000, a[1] or 50000, a[2] or 12, a[3] or 1
    _, ms = synth.make_monomers(n_mono, seed=seed)
    info = lib.plan_info(ms)
    lev = lib.plan_floor_levels(ms)
    P, fs = info["cells_per_lane"], info["floor_slots"]
    fl = next((c for c in FL_LEVELS if fs <= c and c + 2 < P), None)
    if fl is None or info["cells"] != "u16" or not 30 <= P <= 40:
        sys.exit("this set does not run sd_fast_fill<P, ., u16, FL, ., 4> with P = 30..40: %r" % (info,))
    sym = np.array([group_floors(fl, lev["floor_sym"][b]) for b in range(5)], dtype=np.int64)
    pair = np.array([[group_floors(fl, lev["floor_pair"][p][b]) for b in range(5)] for p in range(5)], dtype=np.int64)
    exact_sym = np.array(lev["floor_sym"], dtype=np.int64)
    exact_pair = np.array(lev["floor_pair"], dtype=np.int64)
    code = np.full(256, 4, dtype=np.int64)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = k
    rows = n_sym = n_pair = x_sym = x_pair = 0
    for lo in range(0, n_reads, 50):
        _, rs = synth.make_reads(ms, min(50, n_reads - lo), read_len=read_len, seed=seed, first_index=lo)
        for r in rs:
            c = code[np.frombuffer(r, dtype=np.uint8)]
            for off, n in lib.chunk_plan(len(r)):
                cc = c[off:off + n]
                rows += n
                if n < 2:
                    continue
                cur, prev = cc[1:], cc[:-1].copy()
                prev[0] = 4                                  # row 1: the per-symbol level
                n_sym += int(sym[cur].sum())
                n_pair += int(pair[prev, cur].sum())
                x_sym += int(exact_sym[cur].sum())
                x_pair += int(exact_pair[prev, cur].sum())
    print("P = %d, FL = %d, floor_sym %s, pair rule %s" % (P, fl, lev["floor_sym"], lev["pair_rule"]))
    print("rows %d" % rows)
    print("floors per row, groups of %d slots:  by symbol %.3f   by pair %.3f   difference %.3f" % (STEP, n_sym / rows, n_pair / rows, (n_sym - n_pair) / rows))
    print("floors per row, exact levels:       by symbol %.3f   by pair %.3f" % (x_sym / rows, x_pair / rows))


if __name__ == "__main__":
    main()
