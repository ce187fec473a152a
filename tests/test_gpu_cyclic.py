"""Cyclic pairs and the merge of seed monomers on the device: the pair kernel (sd_cyclic_pairs_dev, sd_cyclic_merge_dev)
against the host form, byte for byte on all three arrays, at every word class and last-word bit, at the device's limits,
over several launches, in waves and workgroups that are not full; a thinned subset against the naive table of
tests/cyclic_ref.py; planted rotations; the merge of planted families; the command line's files."""
import argparse
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch   # noqa: F401  before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import cyclic_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import autocorr, cyclic, formats, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 16
QL = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 171, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]
TL = [1, 2, 64, 171, 2048, 3000]


def launches():
    return lib.cyclic_info()["launches"]


def both(seqs, q=None, t=None):
    """(device, host, launches of the device call), the three arrays equal byte for byte"""
    before = launches()
    d = lib.cyclic_pairs(seqs, q, t, device=0, threads=THREADS)
    n = launches() - before
    h = lib.cyclic_pairs(seqs, q, t, threads=THREADS)
    for name in ("dist", "end", "strand", "phase"):
        a, b = getattr(d, name), getattr(h, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    return d, h, n


def same_merge(a, b):
    return a.n_clusters == b.n_clusters and all(x.tobytes() == y.tobytes() for x, y in zip(a[:6], b[:6]))


def test_word_classes_and_last_word_bits():
    rng = random.Random(41)
    seqs = [ref.rnd(rng, n) for n in QL + TL]
    # related sequences among them, so that distances are not all near the query's length
    seqs[QL.index(171)] = ref.edited(rng, ref.rotated(seqs[len(QL) + TL.index(171)], 100, 1), 5)[:171]
    seqs[QL.index(2047)] = ref.edited(rng, ref.rotated(seqs[len(QL) + TL.index(2048)], 1500, 0), 9)[:2047]
    seqs[QL.index(1025)] = ref.edited(rng, seqs[len(QL) + TL.index(3000)][700:1725], 6)[:1025]
    d, _, n = both(seqs)   # everything against everything, in one call
    assert n >= 10         # a launch per word class at least
    # the thinned subset against the table: every query length once, both strands, 8 pairs with a 2 048-bp query or target
    nq = len(QL)
    subset = [(a, nq + (a % 4)) for a in range(nq)]                                   # targets of 1, 2, 64, 171
    subset += [(a, nq + 4 + (a % 2)) for a in range(0, nq - 1, 2)]                    # targets of 2 048 and 3 000
    subset += [(a, b) for a in (5, 11, 14, 20) for b in (3, 8, 12, 17)]               # queries as targets
    subset += [(a, nq + 2) for a in range(1, nq, 3)]                                  # the target of one word
    subset += [(nq - 1, nq + 3), (nq - 1, nq + 4), (QL.index(171), nq + 3), (QL.index(2047), nq + 4), (QL.index(1025), nq + 5)]
    assert len(set(subset)) >= 60 and sum(1 for a, _ in set(subset) if QL[a] == 2048) <= 12
    strands = set()
    for a, b in sorted(set(subset)):
        want = ref.pair(seqs[a], seqs[b])
        assert (int(d.dist[a, b]), int(d.end[a, b]), int(d.strand[a, b]), int(d.phase[a, b])) == want, (len(seqs[a]), len(seqs[b]))
        strands.add(want[2])
    assert strands == {0, 1}
    assert d.dist[QL.index(171), nq + 3] <= 5 and d.strand[QL.index(171), nq + 3] == 1


@pytest.mark.parametrize("variant", [1, 2])
def test_both_forms_of_the_column_up_to_four_words(variant):
    """the classes of one to four words have the column in 64-bit words and in 32-bit halves; the library launches one of
    them, the bench entry either: both give the host's arrays"""
    rng = random.Random(45)
    lens = [n for n in QL if n <= 257] + [300]
    seqs = [ref.rnd(rng, n) for n in lens] + [ref.rnd(rng, n) for n in (1, 64, 171, 300)]
    seqs[lens.index(171)] = ref.edited(rng, ref.rotated(seqs[-2], 77, 1), 4)[:171]
    seqs[lens.index(257)] = ref.edited(rng, ref.rotated(seqs[-1], 130, 0), 7)[:257]
    before = launches()
    got = lib.cyclic_kernel_bench(seqs, device=0, warmup=0, reps=1, variant=variant, arrays=True)
    assert launches() - before == got["launches"] >= 4
    h = lib.cyclic_pairs(seqs, threads=THREADS)
    for name in ("dist", "end", "strand"):
        assert got[name].tobytes() == getattr(h, name).tobytes(), name


def test_mixed_limits_in_one_call():
    rng = random.Random(42)
    lens = [100, 2049, 171, 4000, 2048, 65536, 65535, 300]
    seqs = [ref.rnd(rng, n) for n in lens]
    seqs[0] = ref.rotated(seqs[7], 200, 1)[:100]
    _, _, n = both(seqs, [0, 1, 2, 3, 4], [5, 2, 6, 7, 0])
    assert n >= 3   # the in-limit queries (100, 171 and 2 048 bp: three classes) ran on the device
    before = launches()
    lib.cyclic_pairs(seqs, [1, 3], [0, 2, 7], device=0)     # no query in the limit: all on the host
    lib.cyclic_pairs(seqs, [0, 2], [5], device=0, threads=THREADS)   # no target in the limit
    assert launches() == before


@pytest.mark.parametrize("n", [171, 2054])
def test_planted_rotations(n):
    c, cases = ref.planted(20 + n, n)
    qs = [q for q, _, _, _ in cases]
    if n == 2054:   # (queries of more than 2 048 bp are the host's: the device takes them cut to its limit, phase r as before)
        cut = [(q[:2048], r, s, e) for q, r, s, e in cases]
        d, _, k = both([c] + [q for q, _, _, _ in cut], list(range(1, len(cut) + 1)), [0])
        assert k >= 1
        for i, (q, r, strand, e) in enumerate(cut):
            assert d.dist[i, 0] <= e and d.strand[i, 0] == strand and (e > 0 or (d.dist[i, 0] == 0 and d.phase[i, 0] == (r + 2048) % n))
    d, _, k = both([c] + qs, list(range(1, len(qs) + 1)), [0])
    assert k >= 1 if n == 171 else k == 0
    for i, (q, r, strand, e) in enumerate(cases):
        if e == 0:
            assert (d.dist[i, 0], d.phase[i, 0], d.strand[i, 0]) == (0, r, strand), (r, strand)
        else:
            assert d.dist[i, 0] <= e and d.strand[i, 0] == strand


def test_several_launches():
    """more word steps than a launch takes, from short sequences: queries of one word against targets of 100 bases"""
    work = lib.cyclic_info()["launch_work"]
    cols = 2 * (2 * 100 - 1)
    m = 4000
    k = int(1.3 * work / (cols * m)) + 1
    assert m * k <= lib.cyclic_info()["pairs_max"]
    rng = random.Random(43)
    seqs = [ref.rnd(rng, 64) for _ in range(m)] + [ref.rnd(rng, 100) for _ in range(k)]
    _, _, n = both(seqs, list(range(m)), list(range(m, m + k)))
    assert n == 2


@pytest.mark.parametrize("m,k", [(1, 1), (63, 1), (65, 3)])
def test_partial_waves_leave_the_guard_bytes(m, k):
    rng = random.Random(44 + m)
    seqs = [ref.rnd(rng, rng.choice((40, 64, 65, 171))) for _ in range(m + k)]
    text, ro, rl = lib._reads_text(seqs)
    qi, ti = np.arange(m, dtype=np.int32), np.arange(m, m + k, dtype=np.int32)
    G = 64
    out = [np.full(m * k + G, 0x5A5A5A5A, dtype=np.int32), np.full(m * k + G, 0x5A5A5A5A, dtype=np.int32), np.full(m * k + G, 0x5A, dtype=np.uint8)]
    err = C.create_string_buffer(512)
    before = launches()
    rc = lib.load().sd_cyclic_pairs_dev(text, ro.ctypes.data, rl.ctypes.data, len(rl), qi.ctypes.data, ti.ctypes.data, m, k, 0, 1,
                                        out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, err, 512)
    assert rc == lib.SD_OK, err.value
    assert launches() > before
    h = lib.cyclic_pairs(seqs, qi, ti)
    for got, want in zip(out, (h.dist, h.end, h.strand)):
        assert got[:m * k].tobytes() == want.tobytes()
        assert (got[m * k:] == (0x5A if got.dtype == np.uint8 else 0x5A5A5A5A)).all()


def test_merge_device_against_host():
    seqs, label, fam = ref.families(31)
    before = launches()
    d = lib.cyclic_merge(seqs, None, 85, device=0, threads=THREADS)
    assert launches() > before
    h = lib.cyclic_merge(seqs, None, 85, threads=THREADS)
    assert same_merge(d, h) and d.n_clusters == 3 and ref.same_partition(d.cluster.tolist(), label)
    assert same_merge(lib.cyclic_merge(seqs, None, 85, block=16, device=0, threads=THREADS), d)
    rng = random.Random(1)
    w = [rng.randrange(3) for _ in seqs]
    assert same_merge(lib.cyclic_merge(seqs, w, 95, block=7, device=0, threads=THREADS), lib.cyclic_merge(seqs, w, 95, threads=THREADS))


def _args(reads, **kw):
    d = dict(sequences=reads, lenient=False, threads="4", autocorr="8", autocorr_window=0, autocorr_min_lag=1, autocorr_peaks="8,8",
             autocorr_spectrum=False, autocorr_seeds=1, autocorr_merge=85, autocorr_merge_min_size=1)
    d.update(kw)
    return argparse.Namespace(**d)


def _run(prog, args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


def test_command_line(tmp_path):
    from stringdecomposer_amd import synth
    names, reads, label = ref.array_reads(4)
    fa = str(tmp_path / "reads.fa")
    synth.write_fasta(fa, names, [s.encode() for s in reads], width=80)
    out, host, out2 = (str(tmp_path / d) for d in ("out", "host", "out2"))
    p = _run("sd-autocorr", [fa, "-o", out, "-t", "4", "--autocorr", "8", "--autocorr-seeds", "1", "--autocorr-merge", "85"])
    os.makedirs(host)
    saved = autocorr.write(_args(fa), host, "final_decomposition", None)   # the host form of the whole pass
    assert len(saved) == 4 and "_autocorr_merge.tsv" in p.stderr
    for fn in saved[1:]:
        got = os.path.join(out, os.path.basename(fn))
        assert open(got, "rb").read() == open(fn, "rb").read() and os.path.getsize(fn) > 0, fn
    rows = formats.read_merge(os.path.join(out, "final_decomposition_autocorr_merge.tsv"))
    assert len(rows) == 12 and {r.cluster for r in rows} == {"M1", "M2"}
    by_read = {r.seed.split("/")[0]: r.cluster for r in rows}
    assert ref.same_partition([by_read[n] for n in names], label)
    merged = open(os.path.join(out, "final_decomposition_autocorr_merged.fa")).read().split("\n")
    assert len(merged) == 5 and merged[0].startswith(">M1 period=") and " seeds=6 " in merged[0] and " seeds=6 " in merged[2]
    periods = sorted(int(merged[i].split()[1][7:]) for i in (0, 2))
    assert periods == [171, 340] and [len(merged[i]) for i in (1, 3)] == [int(merged[i].split()[1][7:]) for i in (0, 2)]
    assert [r.length for r in rows] == [(171, 340)[a] for a in label]   # --autocorr finds the planted period on every read
    seeds = os.path.join(out, "final_decomposition_autocorr_seeds.fa")
    _run("sd-merge", [seeds, "-o", out2, "--merge", "85", "-t", "4"])
    rows2 = formats.read_merge(os.path.join(out2, "final_decomposition_merge.tsv"))
    assert rows2 == rows
    assert open(os.path.join(out2, "final_decomposition_merged.fa")).read() == "\n".join(merged)
    # and in this process: the device ran the seeds' pairs
    sn, ss = cyclic.read_fasta(seeds)
    before = launches()
    m = lib.cyclic_merge(ss, [cyclic.weight_of(n) for n in sn], 85, device=0)
    assert launches() > before and ["M%d" % (c + 1) for c in m.cluster] == [r.cluster for r in rows]


def test_command_line_on_the_real_read(tmp_path):
    out = str(tmp_path / "out")
    _run("sd-autocorr", [os.path.join(TD, "read.fa"), "-o", out, "--autocorr-seeds", "1", "--autocorr-merge", "85"])
    rows = formats.read_merge(os.path.join(out, "final_decomposition_autocorr_merge.tsv"))
    assert len(rows) == 1 and rows[0][1:] == (2054, "M1", rows[0].seed, 0, "100.00", "+", 0)
    merged = open(os.path.join(out, "final_decomposition_autocorr_merged.fa")).read().split("\n")
    assert len(merged) == 3 and merged[0].startswith(">M1 period=2054 seeds=1 ") and len(merged[1]) == 2054
    seed = open(os.path.join(out, "final_decomposition_autocorr_seeds.fa")).read().split("\n")[1]
    assert lib.cyclic_canon(seed)[0] == merged[1]
