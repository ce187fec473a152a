"""The windowed k-mer identity (--dotplot) on the device: the count, set and pair kernels (sd_dotplot_dev) against the host form,
element for element, at the edges of k, windows, tiles, the set cap, the pair kernel's stretches and launches, a thinned
subset against the set restatement of tests/dotplot_ref.py, the device-resident form on DeviceReads, and the command line's
file."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import dotplot_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib
from test_dotplot_cpu import grid_reads, layout, mixed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8
INFO = lib.dotplot_info()
JSEG, CAP = INFO["jseg"], INFO["set_max"]


def same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        bad = np.flatnonzero(np.asarray(a) != np.asarray(b))
        assert bad.size == 0, "%s: %d elements differ, the first: [%d] = %d on the device, %d on the host" % (
            what, len(bad), bad[0], a[bad[0]], b[bad[0]])


def dev_equals_host(text, off, lens, k, W, B=0, M=1, rc=True, min_launches=1):
    """the device form equals the host form element for element, and the pair kernel was launched for it"""
    before = lib.dotplot_info()["launches"]
    dev = lib.dotplot_text(text, off, lens, k, W, B, M, rc, device=0)
    launched = lib.dotplot_info()["launches"] - before
    host = lib.dotplot_text(text, off, lens, k, W, B, M, rc, threads=THREADS)
    assert dev.win_off.tolist() == host.win_off.tolist() and dev.cell_off.tolist() == host.cell_off.tolist()
    what = "k %d W %d B %d M %d rc %d" % (k, W, B, M, rc)
    for name in ("kmers", "kmers_rc", "shared", "shared_rc"):
        same(getattr(dev, name), getattr(host, name), what + " " + name)
    assert launched >= min_launches, "the pair kernel was launched %d times" % launched
    return dev


def one(s, k, W, **kw):
    return dev_equals_host(s, [0], [len(s)], k, W, **kw)


def equals_reference_at(dev, reads, k, W, B, M, keep):
    kmers, kmers_rc, shared, shared_rc, win_off, cell_off = ref.dotplot(reads, k, W, B, M, keep)
    have = shared >= 0
    assert dev.win_off.tolist() == win_off and dev.cell_off.tolist() == cell_off and have.any()
    assert dev.kmers.tolist() == kmers.tolist() and (dev.shared[have] == shared[have]).all()
    if dev.rc:
        assert dev.kmers_rc.tolist() == kmers_rc.tolist() and (dev.shared_rc[have] == shared_rc[have]).all()


@pytest.mark.parametrize("W", [64, 65, 4096])
@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_the_grid_of_lengths_k_m_and_b(k, W):
    """reads of 0, 1, k - 1, k, k + 1, W - 1, W, W + 1, 2 W + k - 1 and 9 W + 5 bases in one call, offsets with gaps and not
    ascending; M in {1, 2, 7, 1009}, B in {0, 1, 2, nw}, both strands and one"""
    rng = random.Random(1000 * W + k)
    reads = grid_reads(rng, k, W)
    text, off, lens = layout(reads, rng)
    assert off != sorted(off)
    nw = max(ref.n_windows(n, W) for n in lens)
    total = 0
    for M in (1, 2, 7, 1009):
        for B in (0, 1, 2, nw):
            for rc in (True, False):
                dev = dev_equals_host(text, off, lens, k, W, B, M, rc)
                total += int(dev.shared.sum())
                if W < 4096 and (M, B, rc) in ((1, 0, True), (7, 2, True), (2, 1, False)):
                    equals_reference_at(dev, reads, k, W, B, M, lambda r, i, j: (r + i + 2 * j) % 3 == 0)
    assert total > 1000


def test_one_repeated_base_and_windows_without_a_kmer():
    s = "A" * 300
    dev = one(s, 5, 64)
    assert dev.kmers.tolist() == [1] * 5 and dev.shared.tolist() == [1] * 15 and dev.kmers_rc.tolist() == [1] * 5 and dev.shared_rc.sum() == 0
    rng = random.Random(4)
    s = "N" * 200 + mixed(rng, 330) + "N" * 64 + "ACGT"   # windows of N alone, and a last window shorter than k
    dev = one(s, 6, 64)
    assert dev.kmers[:3].tolist() == [0, 0, 0] and dev.kmers[-1] == 0 and dev.kmers.sum() > 100
    m = dev.matrix(0)
    assert (m[:, :3][m[:, :3] >= 0] == 0).all() and m[2, 2] == 0 and m[5, 4] > 0
    dev = one(mixed(rng, 500), 16, 64, M=1 << 20)   # nothing is selected anywhere
    assert dev.kmers.sum() == 0 and dev.kmers_rc.sum() == 0 and dev.shared.sum() == 0 and dev.shared_rc.sum() == 0


def distinct_bases(n, k, seed):
    """n + k - 1 bases whose n k-mers are distinct, forward and reverse alike: from the next seed until they are"""
    while True:
        rng = random.Random(seed)
        s = "".join(rng.choice("ACGT") for _ in range(n + k - 1))
        fr = [ref.codes(s[i:i + k]) for i in range(n)]
        if len({f for f, _ in fr}) == n and len({r for _, r in fr}) == n:
            return s
        seed += 1


def test_a_window_at_the_set_cap_and_one_over_it():
    s = distinct_bases(CAP, 16, 77)
    dev = one(s, 16, CAP)   # window 0: exactly 4096 selected positions; window 1: 15 bases, no 16-mer
    assert dev.kmers.tolist() == [CAP, 0] and dev.kmers_rc.tolist() == [CAP, 0] and dev.shared.tolist() == [CAP, 0, 0]
    assert sorted(ref.window_sets(s, 16, CAP, 1)[0][0]) == sorted({ref.codes(s[i:i + 16])[0] for i in range(CAP)})
    twice = s[:CAP] + s   # both windows hold the same 4096 16-mers but for the 15 across the seam
    dev = one(twice, 16, CAP)
    assert dev.kmers[:2].tolist() == [CAP, CAP] and dev.shared[1] == CAP - 15
    s = distinct_bases(CAP + 1, 16, 78)
    msgs = []
    for device in (None, 0):
        with pytest.raises(lib.SdError) as x:
            lib.dotplot(["ACGT", s], 16, CAP + 1, rc=True, device=device)
        assert x.value.code == lib.SD_ERR_PARAM
        msgs.append(x.value.msg.split(": ", 1)[1])
    assert msgs[0] == msgs[1] and "read 1 window 0 has 4097 selected forward k-mers, the cap is 4096" in msgs[0] and "larger M" in msgs[0]
    assert one(s, 16, CAP + 1, M=2).kmers.max() < CAP   # and the call after a refusal is served


def test_a_read_and_its_reverse_complement():
    rng = random.Random(3)
    half = "".join(rng.choice("ACGT") for _ in range(10 * 64))
    dev = one(half + ref.revcomp(half), 12, 64)
    m, mr = dev.matrix(0), dev.matrix(0, rc=True)
    for w in range(10):   # window 19 - w holds the reverse complements of the 12-mers that lie wholly inside window w
        assert mr[19 - w, w] == 64 - 11 and m[19 - w, w] == 0
    equals_reference_at(dev, [half + ref.revcomp(half)], 12, 64, 0, 1, None)


def test_an_even_k_palindrome():
    """ACGT is its own reverse complement: forward and reverse code are one number, S and R of a window hold it alike"""
    assert ref.codes("ACGT")[0] == ref.codes("ACGT")[1] and ref.codes("AATT")[0] == ref.codes("AATT")[1]
    s = "ACGT" * 50 + "AATT" * 30 + "ACGTAATT" * 20
    for k, M in ((4, 1), (4, 3), (8, 1), (2, 1)):
        dev = one(s, k, 64, M=M)
        equals_reference_at(dev, [s], k, 64, 0, M, None)
    dev = one(s, 4, 64)
    m, mr = dev.matrix(0), dev.matrix(0, rc=True)   # windows 0 .. 2 are ACGT alone: four 4-mers, on either strand the same four
    assert dev.kmers[:3].tolist() == dev.kmers_rc[:3].tolist() == [4, 4, 4] and (m[:3, :3] == mr[:3, :3]).all() and m[2, 0] == 4


@pytest.mark.parametrize("nw", [JSEG - 1, JSEG, JSEG + 1, 2 * JSEG + 1])
def test_rows_around_the_pair_kernels_stretches(nw):
    rng = random.Random(nw)
    reads = [mixed(rng, 16 * nw - 3, 7), mixed(rng, 16 * 5)]
    text, off, lens = layout(reads, rng)
    for B in (0, JSEG - 1, JSEG, JSEG + 1):
        dev = dev_equals_host(text, off, lens, 4, 16, B)
    assert dev.n_windows(0) == nw and dev.shared.sum() > 1000
    equals_reference_at(dev, reads, 4, 16, JSEG + 1, 1, lambda r, i, j: (i + j) % 5 == 0)


@pytest.mark.parametrize("W", [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1000])
def test_sets_around_the_pair_kernels_steps(W):
    """a lane looks several keys up per step, 64 apart, and the rest of a set in halving steps: sets of one key fewer, as many
    and one more than every such step holds"""
    rng = random.Random(W)
    s = "".join(rng.choice("ACGT") for _ in range(5 * W + 40))
    dev = one(s, 14, W)
    assert dev.kmers[:5].tolist() == [W] * 5 and dev.shared.sum() > 5 * W   # (random 14-mers: all distinct)
    equals_reference_at(dev, [s], 14, W, 0, 1, None)


def test_a_call_of_several_launches():
    """rows x the largest set x strands above the bound of one launch: every launch writes its own rows"""
    rng = np.random.default_rng(4)
    W, k, nw = 64, 8, 2100
    n = W * nw
    codes = np.tile(rng.integers(0, 4, 171), n // 171 + 1)[:n]
    noise = rng.random(n) < 0.02
    codes[noise] = rng.integers(0, 4, int(noise.sum()))
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes().decode()
    assert nw * (nw + 1) // 2 * W * 2 > INFO["launch_work"]
    dev = one(s, k, W, min_launches=2)
    assert dev.shared.sum() > 10 * len(dev.shared)
    rows = {0, 1, 999, 1000, nw - 1}
    equals_reference_at(dev, [s], k, W, 0, 1, lambda r, i, j: i in rows and j % 97 in (0, 5))


def test_the_device_resident_form():
    """dotplot_device on a DeviceReads of padded rows, on a caller's stream"""
    rng = random.Random(12)
    reads = [mixed(rng, n) for n in (300, 0, 1089, 64, 1000)]
    width = max(len(s) for s in reads) + 13
    rows = np.frombuffer(("".join(s + "A" * (width - len(s)) for s in reads)).encode(), dtype=np.uint8).reshape(len(reads), width)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        data = torch.from_numpy(rows.copy()).to("cuda:0", non_blocking=False)
        dr = lib.DeviceReads(data, [len(s) for s in reads])
    for k, W, B, M, rc in ((5, 64, 0, 1, True), (8, 100, 3, 2, False)):
        host = lib.dotplot(reads, k, W, B, M, rc, threads=THREADS)
        before = lib.dotplot_info()["launches"]
        dd = lib.dotplot_device(dr, k, W, B, M, rc, stream=side)
        assert lib.dotplot_info()["launches"] > before
        assert dd.kmers.is_cuda and dd.kmers.dtype == torch.int32 and dd.shared.is_cuda and dd.win_off.is_cuda and dd.cell_off.is_cuda
        assert (dd.kmers_rc is None) == (not rc) and (dd.shared_rc is None) == (not rc)
        side.synchronize()
        back = dd.to_host(dr.read_lens, k, W, B, M)
        for name in ("kmers", "kmers_rc", "shared", "shared_rc", "win_off", "cell_off"):
            same(getattr(back, name), getattr(host, name), name)
        fresh = lib.dotplot(dr, k, W, B, M, rc)   # torch's own buffers, the current stream
        same(fresh.shared, host.shared, "shared")
    assert host.shared.sum() > 1000
    up = lib.dotplot_device(reads, 5, 64, rc=True).to_host([len(s) for s in reads], 5, 64)   # a list of reads is uploaded first
    same(up.shared_rc, lib.dotplot(reads, 5, 64, rc=True).shared_rc, "shared_rc")


# ---- the command line --------------------------------------------------------------------------------------------------

OPTS = ["--dotplot", "2054,20", "--dotplot-k", "16", "--dotplot-rc", "--dotplot-min", "50"]
TSVS = ("final_decomposition.tsv", "final_decomposition_alt.tsv", "final_decomposition_raw.tsv")
OURS = "final_decomposition_dotplot.tsv"


def _run(prog, out, extra):
    args = [os.path.join(TD, "read.fa")] + ([os.path.join(TD, "DXZ1_star_monomers.fa")] if prog == "stringdecomposer" else [])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog)] + args + ["-o", out, "-t", str(THREADS)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return p


def test_cli_files(tmp_path):
    plain, with_flag, alone = (str(tmp_path / d) for d in ("plain", "flag", "alone"))
    _run("stringdecomposer", plain, [])
    _run("stringdecomposer", with_flag, OPTS)
    _run("sd-dotplot", alone, OPTS)
    for f in TSVS:   # the decomposition does not change
        assert open(os.path.join(with_flag, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
        assert not os.path.exists(os.path.join(alone, f))
    assert os.path.getsize(os.path.join(with_flag, TSVS[0])) > 0 and not os.path.exists(os.path.join(plain, OURS))
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    names = [n.split()[0] for n in rn]
    want = formats.format_dotplot(formats.dotplot_rows(lib.dotplot(rs, 16, 2054, 20, 1, True, threads=THREADS), names, 50))
    assert open(os.path.join(with_flag, OURS)).read() == want == open(os.path.join(alone, OURS)).read()
    rows = formats.read_dotplot(os.path.join(alone, OURS))
    assert len(rows) > 300 and all(r.start_i - r.start_j <= 20 * 2054 for r in rows) and all(max(r.identity, r.identity_rc) >= 50 for r in rows)
    assert OURS in open(os.path.join(with_flag, "stringdecomposer.log")).read()
