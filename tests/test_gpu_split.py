"""The subfamilies of a monomer's instances (--split) on the device: the kernels of csrc/sd_split.hip (sd_split_dev) against
the host form, element for element, at the edges of plane words and wave sizes and with one, two and 64 subfamilies allowed;
the host path of a monomer above 512 bp; and the command line's three files."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import split_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8


def same_split(a, b, what):
    assert a.centres.shape == b.centres.shape, "%s: %d centres against %d" % (what, len(a.centres), len(b.centres))
    for name in ("centres", "assign", "d1", "d2", "sizes"):
        x, y = getattr(a, name), getattr(b, name)
        bad = np.argwhere(np.asarray(x) != np.asarray(y))
        assert bad.size == 0, "%s: %s differs in %d places, the first at %s: %d against %d" % (
            what, name, len(bad), bad[0].tolist(), np.asarray(x)[tuple(bad[0])], np.asarray(y)[tuple(bad[0])])
    assert (a.rounds, a.iters) == (b.rounds, b.iters), what


def rows_for(L, n, seed):
    """planted classes with junk rows, N and deletions among the noise; fewer classes than rows"""
    rng = np.random.default_rng(seed)
    classes = max(1, min(5, n // 12))
    junk = 0 if n < 8 else max(1, n // 30)
    per = max(1, (n - junk) // classes)
    sym, _ = ref.planted(rng, classes, per, L, 0.3, 0.04, junk=n - classes * per)
    assert sym.shape == (n, L)
    return sym


@pytest.mark.parametrize("L", [1, 63, 64, 65, 171, 512])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_device_equals_host(L, n):
    sym = rows_for(L, n, 1000 * L + n)
    R = lib.split_radius(12, L)
    for K in (1, 2, 64):
        before = lib.split_info()["launches"]
        dev = lib.split_rows(sym, R, K=K, min_size=4, max_iter=6, device=0)
        launched = lib.split_info()["launches"] - before
        host = lib.split_rows(sym, R, K=K, min_size=4, max_iter=6, threads=THREADS)
        same_split(dev, host, "L %d n %d K %d" % (L, n, K))
        assert launched >= 1 + dev.rounds + dev.iters, "the assign kernel ran %d times for %d rounds and %d iterations" % (
            launched, dev.rounds, dev.iters)
        assert len(dev.centres) <= K and int(dev.sizes.sum()) == n


def test_device_equals_reference():
    """a thinned subset against the numpy restatement itself"""
    for L, n in ((65, 130), (171, 300)):
        sym = rows_for(L, n, 7 * L + n)
        R = lib.split_radius(12, L)
        dev = lib.split_rows(sym, R, K=64, min_size=4, max_iter=6, device=0)
        exp = ref.split(sym, R, 64, 4, 6)
        same_split(dev, formats.Split(exp["centres"], exp["assign"], exp["d1"], exp["d2"], exp["sizes"], exp["rounds"], exp["iters"]),
                   "L %d n %d" % (L, n))
        assert len(dev.centres) > 2


def test_long_monomer_takes_the_host_path():
    sym = rows_for(513, 120, 513)
    before = lib.split_info()["launches"]
    dev = lib.split_rows(sym, 60, K=8, min_size=4, max_iter=6, device=0)
    assert lib.split_info()["launches"] == before, "a monomer of 513 bp is above the kernels' 512"
    same_split(dev, lib.split_rows(sym, 60, K=8, min_size=4, max_iter=6, threads=THREADS), "L 513")
    assert len(dev.centres) > 1


def run_cli(out_dir, monomers, *extra):
    cmd = [sys.executable, "-m", "stringdecomposer_amd.main", os.path.join(TD, "read.fa"), monomers, "-o", out_dir, "-t", "4"] + list(extra)
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=150)


def test_command_line(tmp_path):
    mono = os.path.join(TD, "DXZ1_star_monomers.fa")
    plain, split = str(tmp_path / "plain"), str(tmp_path / "split")
    r = run_cli(plain, mono)
    assert r.returncode == 0, r.stderr
    r = run_cli(split, mono, "--split", "12")
    assert r.returncode == 0, r.stderr
    for f in ("final_decomposition.tsv", "final_decomposition_raw.tsv", "final_decomposition_alt.tsv"):
        a, b = os.path.join(plain, f), os.path.join(split, f)
        if os.path.exists(a) or os.path.exists(b):
            assert open(a, "rb").read() == open(b, "rb").read(), f
    final = formats.read_final(os.path.join(split, "final_decomposition.tsv"))
    rows = formats.read_split(os.path.join(split, "final_decomposition_split.tsv"))
    assert len(rows) == len(final) > 0
    for f, s in zip(final, rows):
        assert (f.read, f.start, f.end, f.monomer) == (s.read, s.start, s.end, s.monomer)
        assert s.subfamily == "*" or s.subfamily.rsplit(".", 1)[0] == f.monomer.rstrip("'")
    summary = formats.read_split_summary(os.path.join(split, "final_decomposition_split_summary.tsv"))
    names = lib.fasta_load(mono)[0]
    assert {x.monomer for x in summary} <= set(names)
    for x in summary:
        mine = [s for s in rows if s.subfamily == x.subfamily]
        assert x.size == len(mine) and x.sum_d1 == sum(s.d1 for s in mine) and x.max_d1 == max([s.d1 for s in mine] or [0])
    fa = os.path.join(split, "final_decomposition_split_monomers.fa")
    sn, ss, _ = lib.fasta_load(fa)
    assert len(sn) >= len(names) and {n.rsplit(".", 1)[0] for n in sn} == set(names)
    again = str(tmp_path / "again")
    r = run_cli(again, fa)
    assert r.returncode == 0, r.stderr
    second = formats.read_final(os.path.join(again, "final_decomposition.tsv"))
    assert len(second) > 0 and {x.monomer.rstrip("'") for x in second} <= set(sn)
