#!/usr/bin/env python3
"""Infix ("HW") edit distances as the REFERENCE's own edlib gives them (oracle/_ref/libedlib.so, built from the reference
sources by oracle/Makefile; called as MonomerEditDistance does, main.cpp:129: k = -1, EDLIB_MODE_HW, EDLIB_TASK_DISTANCE)
for one template of each length at a word boundary of the prefilter's block recurrence -- 1, 2, 31 ... 2047, 2048 bp, every
second one with an N -- against every chunk of the `edges` read list of its set (tests/prefilter_cases.py).  The --ed_thr
prefilter kernels (tests/test_gpu_prefilter.py) and the oracle's sdo_hw_edit_distance (tests/test_prefilter_cpu.py) are
held against these numbers where no edlib exists.
Run where the reference library was built:
    python tests/golden/make_hw_golden.py
Writes tests/golden/hw_dist/pairs.json: per set the templates, the chunk texts and dist[chunk][template].  Data only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edlib_ref  # noqa: E402
import prefilter_cases as pc  # noqa: E402

assert edlib_ref.have_edlib(), "build oracle/_ref/libedlib.so first (make -C oracle ref)"
PATH = os.path.join(ROOT, "tests", "golden", "hw_dist", "pairs.json")
sets = []
for name, tm, chunks in pc.fixture_sets():
    dist = [[edlib_ref.hw(t, c) for t in tm] for c in chunks]
    assert all(d >= 0 for row in dist for d in row)
    sets.append({"name": name, "templates": [t.decode() for t in tm], "chunks": [c.decode() for c in chunks], "dist": dist})
    print(name, len(tm), "templates x", len(chunks), "chunks", flush=True)
out = {"made_by": "tests/golden/make_hw_golden.py: edlibAlign(template, chunk, k=-1, EDLIB_MODE_HW, EDLIB_TASK_DISTANCE) of the "
                  "reference's edlib.cpp compiled by oracle/Makefile; sequences from tests/prefilter_cases.fixture_sets()",
       "sets": sets}
os.makedirs(os.path.dirname(PATH), exist_ok=True)
with open(PATH, "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
