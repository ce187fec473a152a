"""The windowed k-mer identity (--dotplot) without a device: the host form (sd_dotplot_host) against the set restatement of
tests/dotplot_ref.py element for element, the hash, the layout, the refusals and their numbers, the text and its
identities, --dotplot-min in integers, the command line's refusals, and the DXZ1 test read."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import dotplot_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
HEADER = os.path.join(ROOT, "include", "sd_hip.h")
SYMBOLS = ("sd_dotplot_layout", "sd_dotplot_host", "sd_dotplot_dev", "sd_dotplot_reads_dev", "sd_dotplot_info", "sd_dotplot_hash",
           "sd_dotplot_kernel_bench")


def test_symbols_exported_and_declared():
    L, text = lib.load(), open(HEADER).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and re.search(r"\b%s\(" % s, text), s
    for name in ("KMAX", "WMAX", "MMAX", "BMAX", "CELLS_MAX", "SET_MAX"):
        m = re.search(r"#define SD_DOTPLOT_%s (.+)" % name, text)
        assert m and eval(m.group(1).replace("(int64_t)", "")) == getattr(lib, "DOTPLOT_" + name), name


def mixed(rng, n, unit_len=None):
    """random ACGT with about 2 % N and a stretch of a noisy short-period array, so that windows share k-mers"""
    s = [rng.choice("ACGT") if rng.random() >= 0.02 else "N" for _ in range(n)]
    if n >= 40:
        unit = [rng.choice("ACGT") for _ in range(unit_len or rng.choice((23, 37, 41)))]
        a = rng.randrange(n // 4)
        for i in range(a, a + n // 2):
            if rng.random() >= 0.03:
                s[i] = unit[(i - a) % len(unit)]
    return "".join(s)


def layout(reads, rng):
    """the reads in one buffer in a shuffled order with gaps of bases that would count if they were read"""
    order = list(range(len(reads)))
    rng.shuffle(order)
    off, parts, at = [0] * len(reads), [], 0
    for r in order:
        gap = "".join(rng.choice("ACGT") for _ in range(rng.randrange(0, 9)))
        parts += [gap, reads[r]]
        off[r] = at + len(gap)
        at += len(gap) + len(reads[r])
    return "".join(parts) + "ACGT", off, [len(s) for s in reads]


def grid_reads(rng, k, W):
    return [mixed(rng, n) for n in (0, 1, k - 1, k, k + 1, W - 1, W, W + 1, 2 * W + k - 1, 9 * W + 5)]


def equals_reference(dp, reads, k, W, B, M, rc, keep=None):
    kmers, kmers_rc, shared, shared_rc, win_off, cell_off = ref.dotplot(reads, k, W, B, M, keep)
    assert dp.win_off.tolist() == win_off and dp.cell_off.tolist() == cell_off
    assert dp.kmers.tolist() == kmers.tolist()
    have = shared >= 0
    assert have.any() and (dp.shared[have] == shared[have]).all()
    if rc:
        assert dp.kmers_rc.tolist() == kmers_rc.tolist() and (dp.shared_rc[have] == shared_rc[have]).all()
    else:
        assert dp.kmers_rc is None and dp.shared_rc is None


@pytest.mark.parametrize("k", [1, 2, 16, 31, 32])
def test_host_form_equals_the_reference(k):
    """k at its ends; M in {1, 2, 7, 1009}; B in {0, 1, 2, nw}; both strands and one; reads of 0, 1, k - 1, k, k + 1, W - 1, W,
    W + 1, 2 W + k - 1 bases and a longer one, laid out shuffled with gaps"""
    W = 41
    rng = random.Random(100 + k)
    reads = grid_reads(rng, k, W)
    text, off, lens = layout(reads, rng)
    assert off != sorted(off)
    nw = max(ref.n_windows(n, W) for n in lens)
    seen = 0
    for M in (1, 2, 7, 1009):
        for B in (0, 1, 2, nw):
            for rc in (True, False):
                dp = lib.dotplot_text(text, off, lens, k, W, B, M, rc, threads=3)
                equals_reference(dp, reads, k, W, B, M, rc)
                seen += int(dp.shared.sum())
    assert seen > 1000


def test_selection_thins_the_sets_by_about_m():
    rng = random.Random(5)
    s = "".join(rng.choice("ACGT") for _ in range(40000))
    for M in (7, 1009):
        dp = lib.dotplot([s], 16, 4000, M=M, rc=True, threads=2)
        equals_reference(dp, [s], 16, 4000, 0, M, True)
        assert 0.6 * 40000 / M < dp.kmers.sum() < 1.5 * 40000 / M and 0.6 * 40000 / M < dp.kmers_rc.sum() < 1.5 * 40000 / M


def test_the_hash_is_the_splitmix64_finaliser():
    assert ref.h(0) == 0xE220A8397B1DCDAF   # the first output of splitmix64 seeded with 0
    for x in (0, 1, (1 << 64) - 1, 0x0123456789ABCDEF):
        assert lib.dotplot_hash(x) == ref.h(x), x


@pytest.mark.parametrize("B", [0, 1, 3, 1000])
def test_layout_equals_the_reference(B):
    lens = [0, 1, 99, 100, 101, 1234, 0, 5000]
    win_off, cell_off, windows, cells = lib.dotplot_layout(lens, 100, B)
    w, c = ref.layout(lens, 100, B)
    assert win_off.tolist() == w and cell_off.tolist() == c and windows == w[-1] and cells == c[-1]


def test_cell_and_matrix_follow_the_order_of_the_cells():
    rng = random.Random(8)
    reads = [mixed(rng, 700), mixed(rng, 330)]
    for B in (0, 2):
        dp = lib.dotplot(reads, 5, 64, B, rc=True)
        at = 0
        for r in range(2):
            m, mr = dp.matrix(r), dp.matrix(r, rc=True)
            for i in range(dp.n_windows(r)):
                for j in range(i + 1):
                    if j < ref.row_first(i, B):
                        assert m[i, j] == -1
                        with pytest.raises(IndexError):
                            dp.cell(r, i, j)
                        continue
                    assert dp.cell(r, i, j) == at and m[i, j] == dp.shared[at] and mr[i, j] == dp.shared_rc[at]
                    at += 1
        assert at == len(dp.shared)


def test_reverse_strand_shows_an_inversion_the_forward_strand_does_not():
    rng = random.Random(3)
    half = "".join(rng.choice("ACGT") for _ in range(640))
    s = half + ref.revcomp(half)
    dp = lib.dotplot([s], 12, 64, rc=True)
    m, mr = dp.matrix(0), dp.matrix(0, rc=True)
    for w in range(10):   # window 19 - w holds the reverse complements of the 12-mers that lie wholly inside window w
        assert mr[19 - w, w] == 64 - 11 and m[19 - w, w] == 0


def c_call(fn, reads, k, W, B, M, rc, *more):
    text = "".join(reads).encode() or b"N"
    lens = np.array([len(s) for s in reads], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64) if len(reads) else np.zeros(0, dtype=np.int64)
    out = np.zeros(16, dtype=np.int32)
    err = C.create_string_buffer(512)
    e = fn(text, off.ctypes.data, lens.ctypes.data, len(reads), k, W, B, M, rc, *more, out.ctypes.data, out.ctypes.data, out.ctypes.data,
           out.ctypes.data, err, 512)
    return e, err.value.decode()


@pytest.mark.parametrize("k,W,B,M,words", [(0, 10, 0, 1, ("k = 0", "1 .. 32")), (33, 10, 0, 1, ("k = 33", "1 .. 32")),
                                           (4, 0, 0, 1, ("W = 0", "1 .. 1073741824")), (4, (1 << 30) + 1, 0, 1, ("W = 1073741825", "1 .. 1073741824")),
                                           (4, 10, 0, 0, ("M = 0", "1 .. 1048576")), (4, 10, 0, (1 << 20) + 1, ("M = 1048577", "1 .. 1048576")),
                                           (4, 10, -1, 1, ("B = -1", "1073741824")), (4, 10, (1 << 30) + 1, 1, ("B = 1073741825", "1073741824"))])
def test_refusals_carry_the_numbers(k, W, B, M, words):
    e, msg = c_call(lib.load().sd_dotplot_host, ["ACGT" * 10], k, W, B, M, 1, 1)
    assert e == lib.SD_ERR_PARAM and all(w in msg for w in words), msg
    with pytest.raises(lib.SdError) as x:
        lib.dotplot(["ACGT" * 10], k, W, B, M)
    assert x.value.code == lib.SD_ERR_PARAM and words[0].replace(" = ", " = ") in x.value.msg


def test_the_cap_on_cells_is_refused_with_the_numbers():
    n = 16384   # windows of one base: 16 384 x 16 385 / 2 cells, one row more than the cap holds
    assert n * (n + 1) // 2 > lib.DOTPLOT_CELLS_MAX >= (n - 1) * n // 2
    e, msg = c_call(lib.load().sd_dotplot_host, ["A" * n], 1, 1, 0, 1, 0, 1)
    assert e == lib.SD_ERR_PARAM and str(n * (n + 1) // 2) in msg and str(lib.DOTPLOT_CELLS_MAX) in msg and "16384 windows" in msg
    with pytest.raises(lib.SdError) as x:
        lib.dotplot(["A" * n], 1, 1)
    assert str(n * (n + 1) // 2) in x.value.msg and str(lib.DOTPLOT_CELLS_MAX) in x.value.msg
    assert lib.dotplot(["A" * n], 1, 1, B=3).kmers.tolist() == [1] * n   # a band brings it back under the cap


def test_a_window_over_the_set_cap_is_refused_by_name():
    rng = random.Random(2)
    small = "".join(rng.choice("ACGT") for _ in range(300))
    big = "".join(rng.choice("ACGT") for _ in range(2 * 4200))
    with pytest.raises(lib.SdError) as x:
        lib.dotplot([small, big], 16, 4200, threads=2)
    assert x.value.code == lib.SD_ERR_PARAM
    for word in ("read 1 window 0", "4200 selected forward", "cap is 4096", "larger M"):
        assert word in x.value.msg, x.value.msg
    with pytest.raises(lib.SdError) as x:   # the last window holds 4200 - 15 forward k-mers, and as many reverse ones
        lib.dotplot([small, big[:4200]], 16, 4200, rc=True)
    assert "read 1 window 0" in x.value.msg and "4185 selected forward" in x.value.msg
    assert lib.dotplot([small, big], 16, 4200, M=2).kmers.max() <= 4096   # the advice works


def test_formats_round_trip_and_identities(tmp_path):
    rng = random.Random(7)
    reads = [mixed(rng, 900), mixed(rng, 0), mixed(rng, 400)]
    names = ["r0", "r1", "r2"]
    for k, rc in ((5, True), (16, False), (32, True)):
        dp = lib.dotplot(reads, k, 100, rc=rc, threads=2)
        rows = formats.dotplot_rows(dp, names)
        text = formats.format_dotplot(rows)
        fn = str(tmp_path / ("d%d.tsv" % k))
        formats.write_dotplot(fn, rows)
        back = formats.read_dotplot(fn)
        assert open(fn).read() == text == formats.format_dotplot(back) and len(back) == len(rows) > 10
        assert all(len(line.split("\t")) == (12 if rc else 9) for line in text.splitlines())
        kmers, kmers_rc, shared, shared_rc, win_off, cell_off = ref.dotplot(reads, k, 100)
        want = []   # the reference's lines: (read, i, j) -> the floats
        for r in range(3):
            at = cell_off[r]
            for i in range(win_off[r + 1] - win_off[r]):
                for j in range(i + 1):
                    s, s2 = int(shared[at]), int(shared_rc[at]) if rc else 0
                    at += 1
                    if s or s2:
                        ki, kj, kr = (int(x) for x in (kmers[win_off[r] + i], kmers[win_off[r] + j], kmers_rc[win_off[r] + j]))
                        want.append((names[r], i * 100, j * 100, ki, kj, s, ref.identity(s, ki, kj, k), kr, s2, ref.identity(s2, ki, kr, k) if rc else 0))
        assert len(want) == len(back)
        for row, w in zip(back, want):
            assert (row.read, row.start_i, row.start_j, row.kmers_i, row.kmers_j, row.shared) == w[:6]
            assert abs(row.identity - w[6]) <= 0.005 + 1e-9   # half a unit of the printed digit
            if rc:
                assert (row.kmers_rc_j, row.shared_rc) == w[7:9] and abs(row.identity_rc - w[9]) <= 0.005 + 1e-9
        assert [(r.read, r.start_i, r.start_j) for r in back] == sorted((r.read, r.start_i, r.start_j) for r in back)
        n = [len(s) for s in reads]
        assert all(r.end_i == min(n[names.index(r.read)], r.start_i + 100) and r.end_j == min(n[names.index(r.read)], r.start_j + 100) for r in back)
    with pytest.raises(formats.FormatError):
        open(fn, "a").write("r0\t1\t2\n")
        formats.read_dotplot(fn)


def test_dotplot_min_decides_in_integers():
    """shared = min is 100 percent; one k-mer fewer is not, although it prints as 100.00 at k = 32"""
    assert formats.dotplot_reaches(4096, 4096, 5000, 32, 100) and "%.2f" % formats.dotplot_identity(4096, 4096, 5000, 32) == "100.00"
    assert not formats.dotplot_reaches(4095, 4096, 5000, 32, 100) and "%.2f" % formats.dotplot_identity(4095, 4096, 5000, 32) == "100.00"
    assert formats.dotplot_reaches(1, 2, 2, 1, 50) and not formats.dotplot_reaches(1, 3, 3, 1, 34) and formats.dotplot_reaches(1, 3, 3, 1, 33)
    assert formats.dotplot_reaches(0, 5, 5, 3, 0) and not formats.dotplot_reaches(0, 5, 5, 3, 1)
    for k in (1, 7, 21, 32):   # against exact rationals
        for s, m in ((3, 7), (999, 1000), (1, 4096), (2047, 2048)):
            for P in range(0, 101, 5):
                assert formats.dotplot_reaches(s, m, m + 1, k, P) == (s * 100 ** k >= P ** k * m)
    s = "ACGTTGCATTAGGCAT" * 8 + "ACGTTGCATTAGGCAT"[:8] + "GGGGGGGGCCCCCCCCTTTTTTTTAAAAAAAACGCGCGCGATATATAT" * 2
    dp = lib.dotplot([s], 4, 32)
    rows = formats.dotplot_rows(dp, ["r"], 100)
    full = formats.dotplot_rows(dp, ["r"])
    assert 0 < len(rows) < len(full)
    assert [r for r in full if r.shared == min(r.kmers_i, r.kmers_j)] == rows


NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no device could be used: none is needed


@pytest.mark.parametrize("extra,env,word", [(["--dotplot", "2000"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, "WORLD_SIZE=2"),
                                            (["--dotplot", "0"], {}, "1 <= W <= 1073741824"),
                                            (["--dotplot", "1073741825"], {}, "1 <= W <= 1073741824"),
                                            (["--dotplot", "2000,x"], {}, "1 <= W"),
                                            (["--dotplot", "2000,1073741825"], {}, "0 <= B <= 1073741824"),
                                            (["--dotplot", "2000", "--dotplot-k", "0"], {}, "--dotplot-k 0"),
                                            (["--dotplot", "2000", "--dotplot-k", "33"], {}, "1 .. 32"),
                                            (["--dotplot", "2000", "--dotplot-mod", "0"], {}, "--dotplot-mod 0"),
                                            (["--dotplot", "2000", "--dotplot-mod", "1048577"], {}, "1 .. 1048576"),
                                            (["--dotplot", "2000", "--dotplot-min", "101"], {}, "0 .. 100")])
@pytest.mark.parametrize("prog", ["stringdecomposer", "sd-dotplot"])
def test_cli_refusals_before_device_work(tmp_path, prog, extra, env, word):
    env = dict(os.environ, **NO_DEVICE, **env)
    args = [os.path.join(TD, "read.fa")] + ([os.path.join(TD, "DXZ1_star_monomers.fa")] if prog == "stringdecomposer" else [])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog)] + args + ["-o", str(tmp_path / "out")] + extra,
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 2, p.stderr
    assert p.stderr.count("\n") == 1 and p.stderr.startswith(prog + ": --dotplot") and word in p.stderr
    assert not os.path.exists(str(tmp_path / "out" / "final_decomposition_raw.tsv"))
    assert not os.path.exists(str(tmp_path / "out" / "final_decomposition_dotplot.tsv"))


def test_sd_dotplot_help_needs_no_device():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "sd-dotplot"), "--help"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0, p.stderr
    for opt in ("--dotplot W[,B]", "--dotplot-k", "--dotplot-mod", "--dotplot-rc", "--dotplot-min", "--lenient", "--device"):
        assert opt in p.stdout, opt
    assert "monomers" not in p.stdout.split("options:")[0].split("positional arguments:")[-1]


def test_a_real_read_shows_its_array_and_no_inversion():
    """the DXZ1 read at k = 16, W = 2054 (its higher-order repeat), M = 1: 47 windows of 369 .. 2038 distinct 16-mers; every
    off-diagonal cell among windows 0 .. 11 prints an identity between 90 and 96; no reverse-strand identity reaches 80"""
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    dp = lib.dotplot([rs[0]], 16, 2054, rc=True, threads=4)
    assert dp.n_windows(0) == 47 and int(dp.kmers.min()) == 369 and int(dp.kmers.max()) == 2038
    rows = formats.read_dotplot_text(formats.format_dotplot(formats.dotplot_rows(dp, ["read"])))
    near = [r for r in rows if r.start_j < r.start_i < 12 * 2054]
    assert len(near) == 66 and all(90 <= r.identity <= 96 for r in near), (min(r.identity for r in near), max(r.identity for r in near))
    assert 0 < max(r.identity_rc for r in rows) < 80
