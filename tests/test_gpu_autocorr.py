"""The k-mer autocorrelation (--autocorr) on the device: the plane and pair kernels (sd_autocorr_dev) against the host form,
element for element, at the edges of words, tiles, lag blocks, windows and launches, a thinned subset against the numpy
restatement of tests/autocorr_ref.py, the device-resident form on DeviceReads, and the command line's files."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import autocorr_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8
INFO = lib.autocorr_info()
TB, LB = INFO["tile"], INFO["lags"]


def mixed(rng, n):
    """random ACGT with about 2 % N and a stretch of a noisy short-period array, so that every k finds hits"""
    s = [rng.choice("ACGT") if rng.random() >= 0.02 else "N" for _ in range(n)]
    if n >= 40:
        unit = [rng.choice("ACGT") for _ in range(rng.choice((5, 7, 11)))]
        a = rng.randrange(n // 4)
        for i in range(a, a + n // 2):
            if rng.random() >= 0.03:
                s[i] = unit[(i - a) % len(unit)]
    return "".join(s)


def layout(reads, rng):
    """the reads in one buffer in a shuffled order with gaps of bases that would match if they were read"""
    order = list(range(len(reads)))
    rng.shuffle(order)
    off, parts, at = [0] * len(reads), [], 0
    for r in order:
        gap = "".join(rng.choice("ACGT") for _ in range(rng.randrange(0, 9)))
        parts += [gap, reads[r]]
        off[r] = at + len(gap)
        at += len(gap) + len(reads[r])
    return "".join(parts) + "ACGT", off, [len(s) for s in reads]


def dev_equals_host(text, off, lens, k, D, W, min_launches=1):
    """the device form equals the host form element for element, and the pair kernel was launched for it"""
    before = lib.autocorr_info()["launches"]
    dev = lib.autocorr_text(text, off, lens, k, D, W, device=0)
    launched = lib.autocorr_info()["launches"] - before
    host = lib.autocorr_text(text, off, lens, k, D, W, threads=THREADS)
    assert dev.win_off.tolist() == host.win_off.tolist() and dev.counts.shape == host.counts.shape
    bad = np.argwhere(dev.counts != host.counts)
    assert bad.size == 0, "k %d D %d W %d: %d cells differ, the first: window %d lag %d: %d on the device, %d on the host" % (
        k, D, W, len(bad), bad[0][0], bad[0][1] + 1, dev.counts[tuple(bad[0])], host.counts[tuple(bad[0])])
    assert launched >= min_launches, "the pair kernel was launched %d times" % launched
    return dev


def equals_reference_at(dev, reads, k, D, W, lags):
    want, off = ref.spectra(reads, k, D, W, lags=[d for d in lags if d <= D])
    assert dev.win_off.tolist() == off.tolist()
    keep = want >= 0
    assert keep.any() and (dev.counts[keep] == want[keep]).all()


@pytest.mark.parametrize("k,W", [(3, 0), (8, 0), (3, TB)])
def test_read_lengths_around_words_and_tiles(k, W):
    """reads of 0, 1, k, k + 1, 63, 64, 65, TB - 1, TB, TB + 1 and 2 TB + k - 1 bases in one call, offsets with gaps and not
    ascending"""
    rng = random.Random(10 + k)
    reads = [mixed(rng, n) for n in (0, 1, k, k + 1, 63, 64, 65, TB - 1, TB, TB + 1, 2 * TB + k - 1)]
    text, off, lens = layout(reads, rng)
    assert off != sorted(off)
    D = LB + 44
    dev = dev_equals_host(text, off, lens, k, D, W)
    equals_reference_at(dev, reads, k, D, W, [1, 2, 5, 63, 64, 65, LB - 1, LB, LB + 1, D])
    assert dev.counts.sum() > 1000


@pytest.mark.parametrize("D", [1, 63, 64, 65, LB - 1, LB, LB + 1, 2 * LB + 1, 1500])
def test_lags_around_words_and_lag_blocks(D):
    """D below, at and above a word and a workgroup's block of lags; 1500 exceeds both reads"""
    rng = random.Random(D)
    reads = [mixed(rng, 2 * LB + 200), mixed(rng, 100)]
    text, off, lens = layout(reads, rng)
    dev = dev_equals_host(text, off, lens, 3, D, 0)
    equals_reference_at(dev, reads, 3, D, 0, sorted({1, D // 2 + 1, max(1, D - 1), D}))
    if D > max(lens):
        assert dev.counts[:, max(lens) - 3:].sum() == 0   # lags above n - k count nothing


def planted_runs(rng, lag=70):
    """A read in which, for every o in 33 .. 63, the 32 bases from 512 j + 64 + o on recur exactly `lag` bases on with a
    mismatch on either side (a 32-run across a word boundary), and the 31 / 30 / 1 / 0 bases from 512 j + 300 + o on
    likewise (runs of exactly k - 1 for k = 32, 31, 2, 1 that must not count)"""
    n = 31 * 512 + 200
    s = [rng.choice("ACGT") for _ in range(n)]
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    plants = []
    for j, o in enumerate(range(33, 64)):
        for p, L in ((512 * j + 64 + o, 32), (512 * j + 300 + o, (31, 30, 1, 0)[j % 4])):
            s[p + lag:p + lag + L] = s[p:p + L]
            s[p + lag - 1] = other[s[p - 1]]
            s[p + lag + L] = other[s[p + L]]
            plants.append((p, L))
    return "".join(s), plants


@pytest.mark.parametrize("k", [1, 2, 31, 32])
def test_k_at_its_ends_and_runs_across_words(k):
    rng = random.Random(32)
    s, plants = planted_runs(rng)
    h = ref.hits(s, k, 70)
    for p, L in plants:   # the plants are what they claim: L - k + 1 hits from p on, none before or behind
        assert h[p:p + max(0, L - k + 1)].all() and not h[p - 1] and not h[p + max(0, L - k + 1)]
        assert L != 32 or (p % 64 >= 33 and (p + 31) // 64 == p // 64 + 1)
    assert {L for _, L in plants} == {32, 31, 30, 1, 0}
    dev = dev_equals_host(s, [0], [len(s)], k, 128, 0)
    equals_reference_at(dev, [s], k, 128, 0, [1, 69, 70, 71, 128])
    assert dev.counts[0, 69] == int(h.sum()) >= sum(max(0, L - k + 1) for _, L in plants)


def test_n_at_word_ends_read_ends_and_behind_a_read():
    rng = random.Random(6)
    unit = "ACGTTGCA"
    a = list(unit * 40)   # 320 bases of an exact array: every N shows in many lags
    for i in (0, 63, 64, 127, 128, 191, 319):   # the first and last base of words, the last base of the read
        a[i] = "N"
    a = "".join(a)
    b = unit * 30         # its neighbour in the buffer begins with an N, directly behind the end of a clean read c
    c = unit * 16
    text = a + c + "N" + b[1:] + "N" + unit * 4
    off, lens = [0, len(a) + len(c), len(a)], [len(a), len(b), len(c)]
    reads = [a, "N" + b[1:], c]
    assert [text[o:o + n] for o, n in zip(off, lens)] == reads and text[off[2] + lens[2]] == "N"
    for k in (1, 4, 9):
        dev = dev_equals_host(text, off, lens, k, 200, 0)
        want, _ = ref.spectra(reads, k, 200, 0)
        assert (dev.counts == want).all()
    clean = lib.autocorr_text(unit * 40, [0], [320], 4, 200, device=0)
    assert (clean.counts[0] > dev_equals_host(text, off, lens, 4, 200, 0).counts[0])[7::8].all()   # the Ns cost hits at every multiple of 8


@pytest.mark.parametrize("W", [1, 63, 64, 65, TB, TB + 1])
def test_windows_around_words_and_tiles(W):
    rng = random.Random(W)
    reads = [mixed(rng, 2 * TB + 77), mixed(rng, 130), "", mixed(rng, TB + 1)]
    text, off, lens = layout(reads, rng)
    D = 70
    dev = dev_equals_host(text, off, lens, 4, D, W)
    whole = lib.autocorr_text(text, off, lens, 4, D, 0, device=0)
    for r in range(len(reads)):
        assert (dev.spectrum(r) == whole.counts[r]).all()   # the windows of a read sum to its spectrum
    equals_reference_at(dev, reads, 4, D, W, [1, 7, 64, 70])
    assert dev.counts.shape[0] == sum(ref.n_windows(n, W) for n in lens)


def test_a_call_of_several_launches():
    """n x D above the bound of one launch: the launches accumulate into the same counters; a planted period, so the counts
    are large"""
    rng = np.random.default_rng(4)
    period, D = 171, 4097
    n = INFO["launch_work"] // D + 2 * TB
    unit = rng.integers(0, 4, period)
    codes = np.tile(unit, n // period + 1)[:n]
    noise = rng.random(n) < 0.02
    codes[noise] = rng.integers(0, 4, int(noise.sum()))
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes()
    assert n * D > INFO["launch_work"]
    dev = dev_equals_host(s, [0], [n], 8, D, 0, min_launches=2)
    equals_reference_at(dev, [s], 8, D, 0, [1, 170, 171, 172, 342, 4096, 4097])
    lag = lib.autocorr_peaks(dev.counts, 2, 8, D // period)[0][0]   # (every copy is as noisy as every other: the multiples count alike)
    assert dev.counts[0, period - 1] > n // 2 and sorted(lag.tolist()) == [period * m for m in range(1, D // period + 1)]


def test_the_device_resident_form():
    """autocorr_device on a DeviceReads of padded rows, on a caller's stream, into a stale counts buffer"""
    rng = random.Random(12)
    reads = [mixed(rng, n) for n in (300, 0, TB + 65, 64, 1000)]
    width = max(len(s) for s in reads) + 13
    rows = np.frombuffer(("".join(s + "A" * (width - len(s)) for s in reads)).encode(), dtype=np.uint8).reshape(len(reads), width)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        data = torch.from_numpy(rows.copy()).to("cuda:0", non_blocking=False)
        dr = lib.DeviceReads(data, [len(s) for s in reads])
    for k, D, W in ((4, LB + 3, 0), (6, 90, 500)):
        host = lib.autocorr(reads, k, D, W, threads=THREADS)
        with torch.cuda.stream(side):
            stale = torch.full(host.counts.shape, 77, dtype=torch.int64, device="cuda:0")
        before = lib.autocorr_info()["launches"]
        da = lib.autocorr_device(dr, k, D, W, stream=side, counts=stale)
        assert lib.autocorr_info()["launches"] > before
        assert da.counts.is_cuda and da.counts.dtype == torch.int64 and da.win_off.is_cuda and da.counts.data_ptr() == stale.data_ptr()
        side.synchronize()
        assert (da.counts.cpu().numpy() == host.counts).all() and da.win_off.cpu().numpy().tolist() == host.win_off.tolist()
        back = da.to_host(k, dr.read_lens, W)
        assert (back.counts == host.counts).all() and back.win_end.tolist() == host.win_end.tolist()
        fresh = lib.autocorr(dr, k, D, W)   # torch's own buffer, the current stream
        assert (fresh.counts == host.counts).all()
    assert host.counts.sum() > 1000
    # host memory in the place of device memory is refused
    err = C.create_string_buffer(512)
    hostbuf = np.zeros(1000, dtype=np.int64)
    rc = lib.load().sd_autocorr_reads_dev(C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, 4, 8, 0, 0, None, C.c_void_p(hostbuf.ctypes.data), err, 512)
    assert rc == lib.SD_ERR_PARAM and b"not in device memory" in err.value


# ---- the command line --------------------------------------------------------------------------------------------------

OPTS = ["--autocorr", "8,2200", "--autocorr-window", "30000", "--autocorr-spectrum", "--autocorr-seeds", "100"]
TSVS = ("final_decomposition.tsv", "final_decomposition_alt.tsv", "final_decomposition_raw.tsv")
OURS = ("final_decomposition_autocorr.tsv", "final_decomposition_autocorr_spectrum.tsv", "final_decomposition_autocorr_seeds.fa")


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
    _run("sd-autocorr", alone, OPTS)
    for f in TSVS:   # the decomposition does not change
        assert open(os.path.join(with_flag, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
        assert not os.path.exists(os.path.join(alone, f))
    for f in OURS:   # the launcher of the pass alone writes the same files
        assert open(os.path.join(alone, f), "rb").read() == open(os.path.join(with_flag, f), "rb").read(), f
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    reads, names = [s.decode() for s in rs], [n.split()[0] for n in rn]
    spec = [ref.spectrum(s, 8, 2200, 30000) for s in reads]   # the reference, once for the three files
    rows = formats.read_autocorr(os.path.join(with_flag, OURS[0]))
    assert formats.format_autocorr(rows) == open(os.path.join(with_flag, OURS[0])).read() == ref.summary_text(reads, names, 8, 2200, 30000, 1, 8, 8, spec)
    assert len(rows) == 4 and all(2030 <= r.period <= 2060 for r in rows)
    srows = formats.read_autocorr_spectrum(os.path.join(with_flag, OURS[1]))
    assert formats.format_autocorr_spectrum(srows) == open(os.path.join(with_flag, OURS[1])).read() == ref.spectrum_text(reads, names, 8, 2200, 30000, spec)
    seeds = ref.seeds(reads, names, 8, 2200, 1, 8, 100, [a.sum(axis=0) for a in spec])   # (the windows sum to the read: tested above)
    assert open(os.path.join(with_flag, OURS[2])).read() == "".join(">%s\n%s\n" % x for x in seeds) and len(seeds) == 1
    assert "final_decomposition_autocorr.tsv" in open(os.path.join(with_flag, "stringdecomposer.log")).read()
