"""The k-mer autocorrelation (--autocorr) without a device: the host form (sd_autocorr_host) against the numpy restatement of
tests/autocorr_ref.py, the closed forms, the peak and seed rules, the refusals, the two file formats, the command line's
refusals that need no GPU, and the period of a real read."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import autocorr_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
NEW = ["sd_autocorr_layout", "sd_autocorr_host", "sd_autocorr_dev", "sd_autocorr_reads_dev", "sd_autocorr_positions",
       "sd_autocorr_peaks", "sd_autocorr_seed", "sd_autocorr_info", "sd_autocorr_kernel_bench"]


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.AUTOCORR_KMAX == 32 and re.search(r"#define SD_AUTOCORR_KMAX 32\b", header)
    assert lib.AUTOCORR_DMAX == 1 << 20 and "#define SD_AUTOCORR_DMAX (1 << 20)" in header
    assert lib.AUTOCORR_CELLS_MAX == 1 << 27 and "#define SD_AUTOCORR_CELLS_MAX ((int64_t)1 << 27)" in header
    info = lib.autocorr_info()
    assert info["tile"] > 0 and info["tile"] % 64 == 0 and info["lags"] > 0 and info["launch_work"] >= info["tile"] * info["lags"]


def noisy(rng, n):
    """random ACGT with about 2 % N, and (where there is room) one R, two lower-case bytes and one '-' that match nothing"""
    s = [rng.choice("ACGT") if rng.random() >= 0.02 else "N" for _ in range(n)]
    for ch in "Rac-":
        if n >= 8:
            s[rng.randrange(n)] = ch
    return "".join(s)


def low_complexity(rng, n):
    """few distinct k-mers, so that long k still finds hits: copies of a short unit with a little noise"""
    unit = "".join(rng.choice("ACGT") for _ in range(11))
    s = list((unit * (n // 11 + 1))[:n])
    for i in range(n):
        if rng.random() < 0.01:
            s[i] = rng.choice("ACGTN")
    return "".join(s)


@pytest.mark.parametrize("k", [1, 2, 8, 31, 32])
def test_host_form_equals_the_reference(k):
    """reads of 0, k, k + 1, 63, 64, 65 and 129 bases and a longer one, D below and above n, every window length"""
    rng = random.Random(100 + k)
    n = 200
    reads = [noisy(rng, m) for m in (0, k, k + 1, 63, 64, 65, 129)] + [low_complexity(rng, m) for m in (k + 1, 64, 129, n)]
    for D in (40, n + 7):
        for W in (0, 1, 50, 64, 100, n, n + 1):
            got = lib.autocorr(reads, k, D, W, threads=3)
            want, off = ref.spectra(reads, k, D, W)
            assert got.win_off.tolist() == off.tolist() and got.counts.shape == want.shape and got.counts.dtype == np.int64
            bad = np.argwhere(got.counts != want)
            assert bad.size == 0, "k %d D %d W %d: window %d lag %d: %d, the reference has %d" % (
                k, D, W, bad[0][0], bad[0][1] + 1, got.counts[tuple(bad[0])], want[tuple(bad[0])])
            assert got.win_start.tolist() == [ref.window(len(s), w, W)[0] for s in reads for w in range(ref.n_windows(len(s), W))]
            assert got.win_end.tolist() == [ref.window(len(s), w, W)[1] for s in reads for w in range(ref.n_windows(len(s), W))]
    assert want.sum() > 0 and any(c in r for r in reads for c in "NRa-")


def test_bytes_outside_acgt_match_nothing():
    for ch in "NRacgtn-":
        assert lib.autocorr([ch * 40], 1, 10).counts.sum() == 0, ch
    assert lib.autocorr(["A" * 40], 1, 10).counts[0].tolist() == [40 - d for d in range(1, 11)]


def test_gaps_padding_and_any_order_of_offsets():
    rng = random.Random(5)
    reads = [noisy(rng, m) for m in (70, 0, 129, 33)]
    text = "TTTT" + reads[2] + "ACGTACGT" + reads[0] + reads[3] + "GG"   # padding that would match if it were read
    off = [4 + 129 + 8, 0, 4, 4 + 129 + 8 + 70]
    got = lib.autocorr_text(text, off, [len(s) for s in reads], 2, 80, 50, threads=2)
    assert (got.counts == ref.spectra(reads, 2, 80, 50)[0]).all()


def planted(rng, period=37, copies=40, flank=300):
    unit = "".join(rng.choice("ACGT") for _ in range(period))
    return "".join(rng.choice("ACGT") for _ in range(flank)) + unit * copies + "".join(rng.choice("ACGT") for _ in range(flank))


def test_a_planted_tandem_array_shows_its_period():
    s = planted(random.Random(1))
    ac = lib.autocorr([s], 8, 512)
    assert ac.counts[0, 36] >= 39 * 37 - 8 + 1
    lag, cnt = lib.autocorr_peaks(ac.counts, 1, 8, 4)
    assert lag[0, 0] == 37 and cnt[0, 0] == ac.counts[0, 36]
    assert (ac.counts == ref.spectra([s], 8, 512)[0]).all()


@pytest.mark.parametrize("W", [1, 50, 64, 100, 1000])
def test_windows_sum_to_the_whole_read(W):
    rng = random.Random(W)
    reads = [planted(rng, 23, 12, 100), noisy(rng, 333), ""]
    whole = lib.autocorr(reads, 4, 300, 0, threads=2)
    cut = lib.autocorr(reads, 4, 300, W, threads=2)
    for r in range(len(reads)):
        assert (cut.spectrum(r) == whole.counts[r]).all()
    assert whole.counts.sum() > 0


@pytest.mark.parametrize("k,D,W", [(1, 30, 0), (8, 70, 16), (32, 64, 1), (5, 100, 64)])
def test_positions_equal_a_count(k, D, W):
    lens = [0, 1, k, k + 1, 40, 65]
    got = lib.autocorr_positions(lens, k, D, W)
    want = np.concatenate([ref.positions(n, k, D, W) for n in lens], axis=0)
    assert got.shape == want.shape and (got == want).all()
    reads = ["A" * n for n in lens]   # every position that can be a hit is one
    assert (lib.autocorr(reads, k, D, W).counts == got).all()


def _peaks(A, lo, R, P):
    lag, cnt = lib.autocorr_peaks(np.asarray(A, dtype=np.int64), lo, R, P)
    return [(int(a), int(b)) for a, b in zip(lag[0], cnt[0])]


def test_peak_rule():
    #    lag 1  2  3  4  5  6  7  8  9 10 11 12
    A = [0, 5, 5, 5, 1, 0, 7, 2, 7, 0, 3, 3]
    for lo, R, P in [(1, 1, 8), (1, 0, 8), (1, 2, 8), (1, 20, 3), (8, 1, 8), (8, 3, 2), (12, 5, 4), (1, 1, 2), (3, 1, 5)]:
        want = ref.peaks(A, lo, R, P)
        assert _peaks(A, lo, R, P) == want + [(0, 0)] * (P - len(want)), (lo, R, P)
    assert _peaks(A, 1, 1, 8)[:5] == [(7, 7), (9, 7), (2, 5), (11, 3), (0, 0)]     # the plateaus 2-4 and 11-12 go to their smaller lags
    assert _peaks(A, 1, 2, 8)[:3] == [(7, 7), (2, 5), (0, 0)]                      # lag 9 ties with 7 inside its radius: the smaller lag wins
    assert _peaks(A, 1, 0, 3) == [(7, 7), (9, 7), (2, 5)]                          # R = 0: every positive lag, by count then lag
    assert _peaks(A, 8, 1, 8)[0] == (9, 7)                                         # LO cuts the best lag away, and lag 7 no longer shadows 9
    assert _peaks([0] * 9, 1, 2, 3) == [(0, 0)] * 3                                # an all-zero spectrum: period 0
    assert _peaks(A, 1, 20, 3) == [(7, 7), (0, 0), (0, 0)]                         # fewer than P peaks
    rng = random.Random(3)
    for _ in range(30):
        B = [rng.choice([0, 0, 1, 2, 3, 9]) for _ in range(rng.randrange(1, 40))]
        lo, R, P = rng.randrange(1, len(B) + 1), rng.randrange(0, 6), rng.randrange(1, 6)
        want = ref.peaks(B, lo, R, P)
        assert _peaks(B, lo, R, P) == want + [(0, 0)] * (P - len(want))
    with pytest.raises(lib.SdError):
        lib.autocorr_peaks(np.zeros((1, 4), dtype=np.int64), 0, 1, 1)


def test_seeds_follow_the_rule():
    rng = random.Random(8)
    unit = "".join(rng.choice("ACGT") for _ in range(29))
    clean = planted(rng, 29, 30, 200)
    # two arrays of the same unit, the first shorter: the longest run lies in the second; the third read's unit holds an N,
    # so its runs of hits are shorter than the period and the period's worth of bases from a run's start reaches the next N
    two = "".join(rng.choice("ACGT") for _ in range(90)) + unit * 6 + "".join(rng.choice("ACGT") for _ in range(150)) + unit * 9
    unit_n = "".join(rng.choice("ACGT") for _ in range(15)) + "N" + "".join(rng.choice("ACGT") for _ in range(15))
    dirty = "".join(rng.choice("ACGT") for _ in range(50)) + unit_n * 20 + "".join(rng.choice("ACGT") for _ in range(50))
    reads = [clean, two, dirty, "ACGT" * 3, noisy(rng, 300)]
    names = ["r%d" % i for i in range(len(reads))]
    for r in reads[:3]:
        for p in (29, 31, 58):
            assert lib.autocorr_seed(r, 6, p) == ref.seed(r, 6, p)
    assert lib.autocorr_seed("ACGTTGCA", 4, 3) == (-1, 0) == ref.seed("ACGTTGCA", 4, 3)
    ac = lib.autocorr(reads, 6, 128)
    got = lib.autocorr_seeds(reads, names, ac, 5, 20)
    assert got == ref.seeds(reads, names, 6, 128, 5, 8, 20)
    assert [n.split("/")[0] for n, _ in got] == ["r0", "r1"]   # r2: its seed holds the N and is dropped; r3, r4: no period with 20 hits
    s, run = ref.seed(reads[2], 6, 31)
    assert ref.period(ac.spectrum(2), 5, 8)[0] == 31 and "N" in reads[2][s:s + 31]
    name, seq = got[1]
    m = re.fullmatch(r"r1/(\d+)_(\d+) period=29 count=\d+", name)
    s = int(m.group(1))
    assert int(m.group(2)) == s + 29 and two[s:s + 29] == seq and s >= 90 + 29 * 6 + 150 - 29   # in the second, longer array


def _host_rc(reads, k, D, W, counts_len=16):
    text = "".join(reads).encode() or b"N"
    ro = np.cumsum([0] + [len(s) for s in reads[:-1]]).astype(np.int64)
    rl = np.asarray([len(s) for s in reads], dtype=np.int64)
    counts = np.full(counts_len, 77, dtype=np.int64)
    err = C.create_string_buffer(512)
    rc = lib.load().sd_autocorr_host(text, ro.ctypes.data, rl.ctypes.data, len(reads), k, D, W, 1, counts.ctypes.data, err, 512)
    return rc, err.value.decode(), counts


@pytest.mark.parametrize("k,D,W,reads,words", [(0, 8, 0, ["ACGT"], ["k = 0", "32"]), (33, 8, 0, ["ACGT"], ["k = 33", "32"]),
                                               (4, 0, 0, ["ACGT"], ["D = 0", "1048576"]),
                                               (4, (1 << 20) + 1, 0, ["ACGT"], ["D = 1048577", "1048576"]),
                                               (4, 8, -1, ["ACGT"], ["W = -1"]),
                                               (4, 1 << 20, 1, ["A" * 129], ["129 windows", "1048576", str(1 << 27)])])
def test_refusals_carry_the_numbers(k, D, W, reads, words):
    rc, msg, counts = _host_rc(reads, k, D, W)
    assert rc == lib.SD_ERR_PARAM and all(w in msg for w in words), msg
    assert (counts == 77).all()   # nothing was written
    # the device form refuses before any device work: the same answer on a machine without a device
    err = C.create_string_buffer(512)
    rl = np.asarray([len(s) for s in reads], dtype=np.int64)
    ro = np.zeros(len(reads), dtype=np.int64)
    for fn, extra in ((lib.load().sd_autocorr_dev, (0, 1)), (lib.load().sd_autocorr_reads_dev, (0, None))):
        rc = fn(b"N", ro.ctypes.data, rl.ctypes.data, len(reads), k, D, W, *extra, counts.ctypes.data, err, 512)
        assert rc == lib.SD_ERR_PARAM and all(w in err.value.decode() for w in words)
    with pytest.raises(lib.SdError) as e:
        lib.autocorr(reads, k, D, W)
    assert e.value.code == lib.SD_ERR_PARAM


def test_the_cap_itself_is_allowed():
    rc, msg, _ = _host_rc(["A" * 2], 1, 8, 1, counts_len=16)   # 2 windows x 8 lags
    assert rc == lib.SD_OK, msg
    win_off, start, end, windows = lib.autocorr_layout([0, 5, 128, 129], 64)
    assert win_off.tolist() == [0, 1, 2, 4, 7] and windows == 7 and start.tolist() == [0, 0, 0, 64, 0, 64, 128] and end.tolist() == [0, 5, 64, 128, 64, 128, 129]


def test_formats_round_trip_byte_for_byte(tmp_path):
    rng = random.Random(2)
    reads = [planted(rng, 19, 10, 40), noisy(rng, 90), "ACGT"]
    names = ["read/1", "b", "c"]
    lens = [len(s) for s in reads]
    ac = lib.autocorr(reads, 5, 60, 100)
    rows = lib.autocorr_rows(ac, names, lens, 2, 3, 4)
    text = formats.format_autocorr(rows)
    assert text == ref.summary_text(reads, names, 5, 60, 100, 2, 4, 3)
    p = str(tmp_path / "x_autocorr.tsv")
    formats.write_autocorr(p, rows)
    assert open(p).read() == text and formats.read_autocorr(p) == rows and formats.format_autocorr(formats.read_autocorr(p)) == text
    assert any(not r.peaks for r in rows) and any(len(r.peaks) == 4 for r in rows)
    srows = lib.autocorr_spectrum_rows(ac, names, lens)
    stext = formats.format_autocorr_spectrum(srows)
    assert stext == ref.spectrum_text(reads, names, 5, 60, 100) and len(srows) > 5
    q = str(tmp_path / "x_autocorr_spectrum.tsv")
    formats.write_autocorr_spectrum(q, srows)
    assert formats.read_autocorr_spectrum(q) == srows and formats.format_autocorr_spectrum(formats.read_autocorr_spectrum(q)) == stext
    for path, bad in ((p, "r\t1\t2\n"), (p, "r\t0\t9\t5\t3\t1\t4\t3-1\n"), (q, "r\t1\t2\t3\n")):
        with open(path, "a") as f:
            f.write(bad)
        with pytest.raises(formats.FormatError):
            (formats.read_autocorr if path == p else formats.read_autocorr_spectrum)(path)


NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no device could be used: none is needed


@pytest.mark.parametrize("extra,env,word", [(["--autocorr", "8"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, "WORLD_SIZE=2"),
                                            (["--autocorr", "0"], {}, "1 <= K <= 32"),
                                            (["--autocorr", "33"], {}, "1 <= K <= 32"),
                                            (["--autocorr", "8,0"], {}, "1 <= D <= 1048576"),
                                            (["--autocorr", "8,1048577"], {}, "1 <= D <= 1048576"),
                                            (["--autocorr", "8,x"], {}, "1 <= K"),
                                            (["--autocorr", "8", "--autocorr-window", "-5"], {}, "--autocorr-window -5"),
                                            (["--autocorr", "8,100", "--autocorr-min-lag", "0"], {}, "1 .. D = 100"),
                                            (["--autocorr", "8,100", "--autocorr-min-lag", "101"], {}, "1 .. D = 100"),
                                            (["--autocorr", "8", "--autocorr-peaks", "2000"], {}, "0 <= P <= 1024"),
                                            (["--autocorr", "8", "--autocorr-peaks", "4,-1"], {}, "0 <= R"),
                                            (["--autocorr", "8", "--autocorr-seeds", "-1"], {}, "--autocorr-seeds -1")])
@pytest.mark.parametrize("prog", ["stringdecomposer", "sd-autocorr"])
def test_cli_refusals_before_device_work(tmp_path, prog, extra, env, word):
    env = dict(os.environ, **NO_DEVICE, **env)
    args = [os.path.join(TD, "read.fa")] + ([os.path.join(TD, "DXZ1_star_monomers.fa")] if prog == "stringdecomposer" else [])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog)] + args + ["-o", str(tmp_path / "out")] + extra,
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 2, p.stderr
    assert p.stderr.count("\n") == 1 and p.stderr.startswith(prog + ": --autocorr") and word in p.stderr
    assert not os.path.exists(str(tmp_path / "out" / "final_decomposition_raw.tsv"))
    assert not os.path.exists(str(tmp_path / "out" / "final_decomposition_autocorr.tsv"))


def test_sd_autocorr_help_needs_no_device():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "sd-autocorr"), "--help"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stderr
    for opt in ("--autocorr K[,D]", "--autocorr-window", "--autocorr-min-lag", "--autocorr-peaks", "--autocorr-spectrum", "--autocorr-seeds",
                "--lenient", "--device"):
        assert opt in p.stdout, opt
    assert "monomers" not in p.stdout.split("options:")[0].split("positional arguments:")[-1]


def test_a_real_read_shows_its_higher_order_repeat():
    """the first 20 000 bases of the DXZ1 read at k = 8: equal to the reference, and the period is the 12-mer HOR (about 2 054 bp)"""
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    s = rs[0][:20000].decode().upper()
    ac = lib.autocorr([s], 8, 2200, threads=4)
    assert (ac.counts == ref.spectra([s], 8, 2200)[0]).all()
    lag, cnt = lib.autocorr_peaks(ac.counts, 1, 8, 8)
    assert 2049 <= lag[0, 0] <= 2059 and cnt[0, 0] == ac.counts[0, lag[0, 0] - 1] > 100
    assert lag[0, 0] == ref.period(ac.counts[0], 1, 8)[0]
