"""CPU checks of the screen (--screen): the host keys (sd_screen_chunks_host) against the oracle's exact infix distances
reduced by the key rule, the regions (sd_screen_regions) against a Python restatement of the region rule, the helpers
that carry regions through an unchanged Stream (region_reads, rows_from_regions), the region file's format, and the
refusals that come before any work on a GPU.  No device compute happens here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import prefilter_cases as pc
import screen_cases as sc
from stringdecomposer_amd import formats, lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- keys ------------------------------------------------------------------------------------------------------------
def _host_keys(ms, reads, part, overlap):
    k = lib.screen_chunks_host(ms, reads, part, overlap)
    lens = [len(r) for r in reads]
    assert k.chunk_read.tolist() == sc.chunk_reads(lens, part, overlap)
    plan = [x for n in lens for x in pc.oracle.chunk_plan(n, part, overlap)]
    assert list(zip(k.chunk_off.tolist(), k.chunk_len.tolist())) == plan
    return k.key


def test_host_keys_equal_the_distance_matrix_reduced():
    """A duplicated and a reverse-palindromic template (ties go to the smaller index), templates and reads with N, a
    read shorter than the shortest template, a read shorter than the overlap, a read whose last chunk is short."""
    ms = pc.make_set(301, [40, 57, 63, 64, 65, 90], 48)
    tm = pc.templates(ms)
    st = synth.Stream(302, 1)
    long_read = bytearray(b"".join(pc.mutated(st, tm[int(st.below(1, len(tm))[0])], 0.1) for _ in range(14))[:2 * 300 + 50 + 17])
    long_read[5] = long_read[331] = ord("N")
    reads = [bytes(long_read), pc._rand(st, 39), pc._rand(st, 49), ms[1], ms[0], b"N" * 70, pc.mutated(st, tm[3], 0.2)]
    part, overlap = 300, 50
    chunks = pc.chunks_of(reads, part, overlap)
    assert len(chunks[2]) == 67 and len(reads[1]) < min(len(t) for t in tm) and len(reads[2]) < overlap
    dist = pc.dist_matrix(tm, chunks)
    exp = sc.keys_of(dist)
    got = _host_keys(ms, reads, part, overlap)
    assert got.dtype == np.uint32 and got.tolist() == exp.tolist()
    # the ties are real: the palindrome (index 1) equals its reverse complement, monomer 0 its copy at the end
    n = len(ms)
    assert (dist[:, 1] == dist[:, n + 1]).all() and (dist[:, 0] == dist[:, n - 1]).all()
    c_pal, c_dup = len(chunks) - 4, len(chunks) - 3      # the reads that are ms[1] and ms[0] themselves
    assert got[c_pal] == 1 and got[c_dup] == 0           # distance 0, the smaller index of the tie
    assert (exp >> 16).max() > (exp >> 16).min() and len(set((exp & 0xffff).tolist())) > 3


@pytest.mark.parametrize("case", [c for c in sc.KERNEL_CASES if c.exact and c.n_chunks <= 3], ids=lambda c: c.name)
def test_host_keys_of_the_kernel_cases(case):
    ms, tm, reads = case.data()
    assert _host_keys(ms, reads, sc.PART, sc.OVERLAP).tolist() == case.oracle_keys().tolist()


def test_host_keys_refusals():
    with pytest.raises(lib.SdError) as e:
        lib.screen_chunks_host([b"ACGT"], [b""], 100, 10)
    assert e.value.code == lib.SD_ERR_EMPTY
    with pytest.raises(lib.SdError) as e:
        lib.screen_chunks_host([b"ACGT"], [b"ACGX"], 100, 10)
    assert e.value.code == lib.SD_ERR_SYMBOL
    with pytest.raises(lib.SdError) as e:
        lib.screen_chunks_host([b"A" * 2049], [b"ACGT"], 100, 10)
    assert e.value.code == lib.SD_ERR_UNSUPPORTED
    if lib.device_count() < 1:                 # an entry point that needs a device says so without one
        with pytest.raises(lib.SdError) as e:
            lib.Screener([b"ACGT"])
        assert e.value.code == lib.SD_ERR_NO_DEVICE


# ---- regions ---------------------------------------------------------------------------------------------------------
def _regions(keys, lens, thr, part, overlap):
    cr = np.array(sc.chunk_reads(lens, part, overlap), dtype=np.int32)
    k = lib.ScreenKeys(cr, None, None, np.asarray(keys, dtype=np.uint32))
    return sc.region_tuples(lib.screen_regions(k, lens, thr, part, overlap)), cr


def test_regions_against_the_restated_rule():
    rng = np.random.default_rng(5)
    seen = {"all": 0, "none": 0, "single": 0, "alternating": 0, "clipped": 0}
    for trial in range(500):
        part = int(rng.integers(2, 9))
        overlap = int(rng.integers(0, part))
        n_reads = int(rng.integers(1, 5))
        lens = [int(rng.integers(1, 6 * part)) for _ in range(n_reads)]
        if trial % 7 == 0:
            lens[0] = int(rng.integers(1, part + 1))          # a single-chunk read
        n = len(sc.chunk_reads(lens, part, overlap))
        mode = trial % 5
        d = {0: rng.integers(0, 9, n), 1: np.zeros(n, dtype=np.int64), 2: np.full(n, 8), 3: np.arange(n) % 2 * 8,
             4: rng.integers(3, 6, n)}[mode]
        keys = (d.astype(np.uint32) << 16) | rng.integers(0, 24, n).astype(np.uint32)
        thr = 4
        got, cr = _regions(keys, lens, thr, part, overlap)
        exp = sc.regions_of(keys, cr.tolist(), lens, thr, part, overlap)
        assert got == exp, (trial, part, overlap, lens, keys.tolist())
        # the properties the rule implies, stated on their own
        for a, b in zip(got, got[1:]):
            assert (a[0], a[2]) < (b[0], b[1])                               # read order, position order, no overlap
        assert sum(x[3] for x in got) == int((d <= thr).sum())               # every passing chunk in exactly one region
        for r, s, e, k, best in got:
            first = cr.tolist().index(r) + s // part                         # the region's first chunk in the table
            assert s % part == 0 and e < lens[r] and best == min(int(x) for x in keys[first:first + k])
        seen["all"] += mode == 1 and all(s == 0 and e == lens[r] - 1 for r, s, e, _, _ in got) and len(got) == n_reads
        seen["none"] += mode == 2 and not got
        seen["single"] += any(len(pc.oracle.chunk_plan(x, part, overlap)) == 1 for x in lens)
        seen["alternating"] += mode == 3 and n > 2 and all(x[3] == 1 for x in got)
        seen["clipped"] += any((e + 1 - s) < k * part + overlap for _, s, e, k, _ in got)
    assert all(v > 20 for v in seen.values()), seen


def test_regions_clip_at_the_read_end_and_keep_the_smallest_key():
    # 5 chunks of part 10 / overlap 3 in a read of 47 bases: chunks at 0, 10, 20, 30, 40 (7 bases)
    keys = [(9 << 16) | 1, (2 << 16) | 7, (1 << 16) | 3, (9 << 16) | 0, (4 << 16) | 5]
    got, _ = _regions(keys, [47], 4, 10, 3)
    assert got == [(0, 10, 32, 2, (1 << 16) | 3), (0, 40, 46, 1, (4 << 16) | 5)]
    got, _ = _regions(keys, [47], 9, 10, 3)
    assert got == [(0, 0, 46, 5, (1 << 16) | 3)]               # everything passes: the whole read, clipped at its end
    got, _ = _regions(keys, [47], 0, 10, 3)
    assert got == []


def test_regions_refusals():
    k = lib.ScreenKeys(np.zeros(1, dtype=np.int32), None, None, np.zeros(1, dtype=np.uint32))
    for part, overlap, thr in ((10, 10, 3), (10, 11, 3), (10, 3, -1)):
        with pytest.raises(lib.SdError) as e:
            lib.screen_regions(k, [5], thr, part, overlap)
        assert e.value.code == lib.SD_ERR_PARAM
    with pytest.raises(lib.SdError) as e:
        lib.screen_regions(k, [5], 3, 10, 10)
    assert "overlap" in e.value.msg


# ---- helpers and formats ---------------------------------------------------------------------------------------------
def test_region_reads_and_rows_from_regions_round_trip():
    reads = [b"ACGTACGTACGTAAAC", b"TTTTGGGGCCCCAAAATTTT", b"ACGT"]
    regions = np.zeros(3, dtype=lib.screen_region_dtype())
    regions["read"], regions["start"], regions["end_incl"] = [0, 1, 1], [4, 0, 12], [11, 7, 19]
    sub = lib.region_reads(reads, regions)
    assert [bytes(x) for x in sub] == [reads[0][4:12], reads[1][0:8], reads[1][12:20]]
    assert all(isinstance(x, memoryview) for x in sub)                    # slices, not copies
    assert [s for s in lib.ReadSet(sub).seqs] == [bytes(x) for x in sub]  # ... that a read set takes
    # rows of the three regions (tmpl, start, end, score), local coordinates
    rows = np.array([[0, 0, 3, 4], [1, 4, 7, 4], [2, 1, 6, 5], [0, 0, 2, 3], [1, 3, 7, 5]], dtype=np.int32)
    row_off = np.array([0, 2, 3, 5], dtype=np.int64)
    out, off = lib.rows_from_regions(rows, row_off, regions, len(reads))
    assert out.tolist() == [[0, 4, 7, 4], [1, 8, 11, 4], [2, 1, 6, 5], [0, 12, 14, 3], [1, 15, 19, 5]]
    assert off.tolist() == [0, 2, 5, 5] and rows[0, 1] == 0               # per parent read; the input is untouched
    # the shifted rows cut the parents where the local rows cut the regions
    for g in range(3):
        for x in range(row_off[g], row_off[g + 1]):
            parent = reads[int(regions["read"][g])]
            assert parent[out[x, 1]:out[x, 2] + 1] == bytes(sub[g])[rows[x, 1]:rows[x, 2] + 1]
    # structured rows (final rows): positions shifted, the read index mapped back
    fr = np.zeros(5, dtype=lib.final_dtype())
    fr["read"], fr["start"], fr["end"] = [0, 0, 1, 2, 2], rows[:, 1], rows[:, 2]
    out, off = lib.rows_from_regions(fr, row_off, regions, len(reads))
    assert out["read"].tolist() == [0, 0, 1, 1, 1] and out["start"].tolist() == [4, 8, 1, 12, 15] and off.tolist() == [0, 2, 5, 5]
    # no region at all
    out, off = lib.rows_from_regions(rows[:0], np.zeros(1, dtype=np.int64), regions[:0], 3)
    assert len(out) == 0 and off.tolist() == [0, 0, 0, 0]
    with pytest.raises(lib.SdError):
        lib.rows_from_regions(rows, row_off[:-1], regions, 3)


def test_screen_file_round_trip(tmp_path):
    rows = [formats.ScreenRow("chr1 description", 0, 10199, 5, 17, "m3"), formats.ScreenRow("chr1 description", 40000, 47199, 3, 0, "m11'"),
            formats.ScreenRow("r2", 2000, 2149, 1, 40, "A'")]
    text = "chr1 description\t0\t10199\t5\t17\tm3\nchr1 description\t40000\t47199\t3\t0\tm11'\nr2\t2000\t2149\t1\t40\tA'\n"
    assert formats.format_screen(rows) == text and formats.parse_screen(text) == rows
    fn = tmp_path / "x_screen.tsv"
    formats.write_screen(str(fn), rows)
    assert fn.read_bytes() == text.encode() and formats.read_screen(str(fn)) == rows
    formats.write_screen(str(fn), [])
    assert fn.read_bytes() == b"" and formats.read_screen(str(fn)) == []
    fn.write_text("r\t0\t9\t1\t3\n")
    with pytest.raises(formats.FormatError):
        formats.read_screen(str(fn))
    regions = np.zeros(2, dtype=lib.screen_region_dtype())
    regions["read"], regions["start"], regions["end_incl"], regions["n_chunks"] = [0, 1], [0, 2000], [10199, 2149], [5, 1]
    regions["best_key"] = [(17 << 16) | 1, (40 << 16) | 2]
    assert formats.screen_rows(regions, ["c", "r2"], ["A", "m3"]) == [formats.ScreenRow("c", 0, 10199, 5, 17, "m3"),
                                                                     formats.ScreenRow("r2", 2000, 2149, 1, 40, "A'")]


# ---- refusals before any GPU work ------------------------------------------------------------------------------------
def _cli(args, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer")] + args, env=env,
                          capture_output=True, text=True, timeout=120)


def test_cli_screen_refusals_come_before_any_work(tmp_path):
    m = tmp_path / "m.fa"
    m.write_text(">x\nACGTACGT\n")
    r = tmp_path / "r.fa"
    r.write_text(">r\nACGTACGT\n")
    out = tmp_path / "out"
    base = [str(r), str(m), "-o", str(out)]
    p = _cli(base + ["--screen", "40"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    err = p.stderr.strip().splitlines()
    assert p.returncode == 2 and len(err) == 1 and "torch.distributed" in err[0] and "--screen" in err[0]
    p = _cli(base + ["--screen", "-1"])
    err = p.stderr.strip().splitlines()
    assert p.returncode == 2 and len(err) == 1 and "--screen -1" in err[0]
    p = _cli(base + ["--screen", "40", "--records"])
    err = p.stderr.strip().splitlines()
    assert p.returncode == 2 and len(err) == 1 and "the record stream holds whole reads" in err[0]
    p = _cli(base + ["--screen", "40", "-b", "500", "-v", "500"])
    err = p.stderr.strip().splitlines()
    assert p.returncode == 2 and len(err) == 1 and "overlap" in err[0]
    assert not out.exists()
    h = _cli(["--help"])
    assert h.returncode == 0 and "--screen THR" in h.stdout


def test_c_abi_screen_refusals_without_gpu(tmp_path):
    """sd_run_files_screen: what is wrong with the request itself is SD_ERR_PARAM before a device is looked for."""
    m = tmp_path / "m.fa"
    m.write_text(">x\nACGTACGT\n")
    r = tmp_path / "r.fa"
    r.write_text(">r\nACGTACGT\n")
    o = [str(tmp_path / x) for x in ("raw.tsv", "fin.tsv", "alt.tsv")]
    with pytest.raises(lib.SdError) as e:
        lib.run_files(str(r), str(m), *o, screen=40, records_out=str(tmp_path / "x.sdr"))
    assert e.value.code == lib.SD_ERR_PARAM and "the record stream holds whole reads" in e.value.msg
    with pytest.raises(lib.SdError) as e:
        lib.run_files(str(r), str(m), *o, screen=-1)
    assert e.value.code == lib.SD_ERR_PARAM
    with pytest.raises(lib.SdError) as e:
        lib.run_files(str(r), str(m), *o, screen=40, part_size=500, overlap=500)
    assert e.value.code == lib.SD_ERR_PARAM and "overlap" in e.value.msg
