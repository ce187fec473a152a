"""The team kernel of cyclic pairs on the device (sd_cyclic_pairs_long<K, L>: queries of 2 049 to 16 384 bp, a query across
L lanes): every class forced onto the shapes of tests/cyclic_long_cases.py against the host form, byte for byte; the routing
of one call among the lane kernel, the team kernel and the host; teams and waves that are not full, with guard words behind
the arrays; planted rotations at 2 054 bp; the merge of planted families of 2 054-bp seeds and their dimers; two launches
from short sequences; the files of bin/sd-merge."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch   # noqa: F401  before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import cyclic_long_cases as cases
import cyclic_ref as ref
from stringdecomposer_amd import cyclic, formats, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = cases.THREADS


def lane_launches():
    return lib.cyclic_info()["launches"]


def team_launches():
    return lib.cyclic_long_info()["launches"]


def both(seqs, q=None, t=None):
    """(device, host, launches of the lane kernel, launches of the team kernel), the arrays equal byte for byte"""
    lane, team = lane_launches(), team_launches()
    d = lib.cyclic_pairs(seqs, q, t, device=0, threads=THREADS)
    lane, team = lane_launches() - lane, team_launches() - team
    h = lib.cyclic_pairs(seqs, q, t, threads=THREADS)
    cases.same_arrays(d, h)
    assert d.phase.tobytes() == h.phase.tobytes()
    return d, h, lane, team


def same_merge(a, b):
    return a.n_clusters == b.n_clusters and all(x.tobytes() == y.tobytes() for x, y in zip(a[:6], b[:6]))


@pytest.mark.parametrize("K,L", cases.CLASSES)
def test_forced_classes(K, L):
    seqs, q, t = cases.case(K, L)
    lane, team = lane_launches(), team_launches()
    got = lib.cyclic_long_kernel_bench(seqs, q, t, device=0, K=K, L=L, warmup=0, reps=1, arrays=True)
    assert team_launches() - team == got["launches"] >= 1 and lane_launches() == lane
    assert got["pairs"] == len(q) * len(t)
    cases.same_arrays(got, cases.host_arrays(K, L))


def test_routing():
    rng = random.Random(52)
    ql, tl = [100, 2048, 2049, 2054, 4000, 16384, 16385], [1, 171, 2054, 65535, 65536]
    seqs = [ref.rnd(rng, n) for n in ql + tl]
    seqs[3] = ref.edited(rng, ref.rotated(seqs[len(ql) + 2], 700, 1), 6)[:2054].ljust(2054, "A")
    assert [len(s) for s in seqs] == ql + tl
    q, t = list(range(len(ql))), list(range(len(ql), len(seqs)))
    d, _, lane, team = both(seqs, q, t)
    assert lane == 2      # the classes of the 100- and the 2 048-bp query
    assert team >= 3      # 2 049 and 2 054 bp share a class; 4 000 and 16 384 bp have their own
    assert d.dist[3, 2] <= 6 + 1 and d.strand[3, 2] == 1
    lane, team = lane_launches(), team_launches()
    lib.cyclic_pairs(seqs, [6], t, device=0, threads=THREADS)   # only the query beyond the limit: all on the host
    assert (lane_launches(), team_launches()) == (lane, team)


@pytest.mark.parametrize("m", [1, 3, 5])
@pytest.mark.parametrize("k", [1, 3])
def test_partial_teams_and_waves_leave_the_guard_bytes(m, k):
    """2 054 bp is L = 16: four teams to a wave, so 1, 3 and 5 queries leave teams empty, 1 and 3 targets leave waves idle"""
    assert lib.cyclic_team_class(2054) == (3, 16)
    rng = random.Random(60 + 10 * m + k)
    seqs = [ref.rnd(rng, 2054) for _ in range(m)] + [ref.rnd(rng, n) for n in (2054, 171, 300)[:k]]
    text, ro, rl = lib._reads_text(seqs)
    qi, ti = np.arange(m, dtype=np.int32), np.arange(m, m + k, dtype=np.int32)
    G = 64
    out = [np.full(m * k + G, 0x5A5A5A5A, dtype=np.int32), np.full(m * k + G, 0x5A5A5A5A, dtype=np.int32), np.full(m * k + G, 0x5A, dtype=np.uint8)]
    err = C.create_string_buffer(512)
    lane, team = lane_launches(), team_launches()
    rc = lib.load().sd_cyclic_pairs_dev(text, ro.ctypes.data, rl.ctypes.data, len(rl), qi.ctypes.data, ti.ctypes.data, m, k, 0, 1,
                                        out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, err, 512)
    assert rc == lib.SD_OK, err.value
    assert team_launches() == team + 1 and lane_launches() == lane
    h = lib.cyclic_pairs(seqs, qi, ti, threads=THREADS)
    for got, want in zip(out, (h.dist, h.end, h.strand)):
        assert got[:m * k].tobytes() == want.tobytes()
        assert (got[m * k:] == (0x5A if got.dtype == np.uint8 else 0x5A5A5A5A)).all()


def test_planted_rotations_at_2054():
    """whole queries, not cut to the lane kernel's 2 048 bp"""
    c, planted = ref.planted(20 + 2054, 2054)
    qs = [q for q, _, _, _ in planted]
    assert min(len(q) for q in qs) > lib.CYCLIC_QMAX
    d, _, lane, team = both([c] + qs, list(range(1, len(qs) + 1)), [0])
    assert lane == 0 and team >= 1
    for i, (q, r, strand, e) in enumerate(planted):
        if e == 0:
            assert (d.dist[i, 0], d.phase[i, 0], d.strand[i, 0]) == (0, r, strand), (r, strand)
        else:
            assert d.dist[i, 0] <= e and d.strand[i, 0] == strand


def test_merge_of_2054_bp_seeds_and_their_dimers():
    names, seqs, label = cases.merge_seeds()
    assert len(seqs) == 28 and sorted({len(s) // 1000 for s in seqs}) == [2, 4] and min(len(s) for s in seqs) > lib.CYCLIC_QMAX
    lane, team = lane_launches(), team_launches()
    d = lib.cyclic_merge(seqs, None, 85, device=0, threads=THREADS)
    assert team_launches() > team and lane_launches() == lane
    h = lib.cyclic_merge(seqs, None, 85, threads=THREADS)
    assert same_merge(d, h) and d.n_clusters == 4 and ref.same_partition(d.cluster.tolist(), label)
    dimers = {int(c) for c, f in zip(d.cluster, label) if f == 3}
    assert len(dimers) == 1 and dimers.isdisjoint(int(c) for c, f in zip(d.cluster, label) if f != 3)
    assert same_merge(lib.cyclic_merge(seqs, None, 85, block=7, device=0, threads=THREADS), h)


def test_two_launches_of_the_team_kernel():
    """more word steps than a launch takes, from short sequences: the class of 4 words x 64 lanes forced onto queries of 64
    bases against targets of 100 -- a pair is 2 (2 x 100 - 1 + 63) steps of 256 words, pad and ramp counted"""
    work = lib.cyclic_info()["launch_work"]
    per_pair = 2 * (2 * 100 - 1 + 63) * 256
    m = 256
    k = int(1.3 * work / (per_pair * m)) + 1
    assert m * k <= lib.cyclic_info()["pairs_max"] and m * ((k + 7) // 8) >= 2 * lib.CYCLIC_LAUNCH_WG_MIN
    rng = random.Random(53)
    seqs = [ref.rnd(rng, 64) for _ in range(m)] + [ref.rnd(rng, 100) for _ in range(k)]
    q, t = list(range(m)), list(range(m, m + k))
    team = team_launches()
    got = lib.cyclic_long_kernel_bench(seqs, q, t, device=0, K=4, L=64, warmup=0, reps=1, arrays=True)
    assert team_launches() - team == got["launches"] == 2 and got["steps"] == per_pair * m * k
    cases.same_arrays(got, lib.cyclic_pairs(seqs, q, t, threads=THREADS))


def test_command_line(tmp_path):
    from stringdecomposer_amd import synth
    names, seqs, label = cases.merge_seeds()
    fa = str(tmp_path / "seeds.fa")
    synth.write_fasta(fa, names, [s.encode() for s in seqs], width=80)
    out, host = str(tmp_path / "out"), str(tmp_path / "host")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "sd-merge"), fa, "-o", out, "--merge", "85", "-t", "4"], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    os.makedirs(host)
    hn, hs = cyclic.read_fasta(fa)
    m = cyclic.merge_files(hn, hs, 85, os.path.join(host, "merged.fa"), os.path.join(host, "merge.tsv"), threads=THREADS)   # the host form
    assert m.n_clusters == 4
    for fn in ("merged.fa", "merge.tsv"):
        got = open(os.path.join(out, "final_decomposition_" + fn), "rb").read()
        assert got == open(os.path.join(host, fn), "rb").read() and len(got) > 0, fn
    rows = formats.read_merge(os.path.join(out, "final_decomposition_merge.tsv"))
    assert len(rows) == 28 and ref.same_partition([r.cluster for r in rows], label)
