"""Parity of the HIP path (through the C-ABI of libsd_hip.so) against
  * the committed golden fixtures = stdout of the real reference binary, and
  * the CPU oracle on fresh seeded inputs,
bit-exact (integer / index work).  Runs only on a real MI355X: `pytest -m gpu`."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, case_names, load_case

from stringdecomposer_amd import lib, shard, synth

pytestmark = pytest.mark.gpu

FAMILIES = [("generic", lib.KERNEL_GENERIC), ("fast", lib.KERNEL_FAST)]


def _decompose_case(c, kernel, tmp_path):
    sc = tuple(c["scoring"]) if c["scoring"] else (-1, -1, -1, 1)
    out = str(tmp_path / "raw.tsv")
    ed = -1 if c["ed_thr"] is None else c["ed_thr"]
    if ed > -1:
        sc = (-1, -1, -1, 1)  # the reference ignores the scores in its 10-argument (--ed_thr) form
    lib.decompose_files(c["reads"], c["monomers"], out, scoring=sc, part_size=c["part"],
                        overlap=c["overlap"], kernel=kernel, ed_thr=ed)
    with open(out, "rb") as f:
        return f.read()


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize("name", case_names(include_edthr=True))
def test_golden_fixture_raw_tsv(name, fam, tmp_path):
    c = load_case(name)
    try:
        got = _decompose_case(c, fam[1], tmp_path)
    except lib.SdError as e:
        if fam[0] == "fast" and e.code == lib.SD_ERR_UNSUPPORTED and not name.startswith("weird_templates"):
            pytest.skip("fast family not applicable: " + e.msg)
        raise   # (the duplicate / 1-bp / palindromic templates of weird_templates* run on the fast family since round 4)
    assert hashlib.sha256(got).hexdigest() == c["sha256"], "raw TSV differs from the reference binary's"
    assert got == c["raw"]


def test_auto_family_picks_fast_for_default_config(tmp_path):
    c = load_case("td_default")
    mn, ms = synth.make_monomers(12, seed=1)
    e = lib.Engine(ms)
    assert e.info()["family"] == "fast"
    e.close()
    assert _decompose_case(c, lib.KERNEL_AUTO, tmp_path) == c["raw"]


@pytest.mark.parametrize("name", [n for n in case_names(include_errors=True) if n.startswith("err_")])
def test_error_cases(name, tmp_path):
    c = load_case(name)
    with pytest.raises(lib.SdError) as e:
        _decompose_case(c, lib.KERNEL_AUTO, tmp_path)
    assert e.value.code == lib.SD_ERR_SYMBOL
    assert e.value.msg.strip() == c["stderr_tail"][0].strip()


def test_empty_read_is_an_error_not_a_crash():
    mn, ms = synth.make_monomers(12, seed=1)
    with pytest.raises(lib.SdError) as e:
        lib.decompose(["a", "b"], [b"ACGT", b""], mn, ms)
    assert e.value.code == lib.SD_ERR_EMPTY


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize("sc", [(-1, -1, -1, 1), (-2, -3, -4, 2), (-1, -2, -1, 1), (0, 0, 0, 1), (-3, -1, -2, 3)])
def test_chunk_level_vs_oracle(oracle, fam, sc):
    """Engine-level: chunk-local records (template, start, end, score) vs AlignPartClassicDP."""
    mn, ms = synth.make_monomers(12, seed=21)
    tm = [m.decode() for m in ms] + [synth.revcomp_bytes(m).decode() for m in ms]
    rn, rs = synth.make_reads(ms, 6, read_len=2300, seed=31)
    lens = [2300, 1, 37, 640, 1999, 2048]
    rs = [s[:L] for s, L in zip(rs, lens)]
    e = lib.Engine(ms, scoring=sc, part_size=5000, overlap=500, kernel=fam[1])
    assert e.load_reads(rs) == len(rs)
    e.run()
    got = e.fetch()
    e.close()
    for s, g in zip(rs, got):
        exp = oracle.align_chunk(s.decode(), tm, sc)
        assert g == [(t, a, b, int(v)) for (t, a, b, v) in exp]


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_random_reads_vs_oracle_full_pipeline(oracle, fam):
    mn, ms = synth.make_monomers(12, seed=77)
    rn, rs = synth.make_reads(ms, 3, read_len=12345, seed=78)
    got = lib.decompose(rn, rs, mn, ms, kernel=fam[1])
    exp = oracle.decompose(rn, rs, mn, ms, threads=8)
    assert got == exp


def test_families_agree_at_bench_scale():
    """Size-independent property at BASELINE config-2 read length: both kernel families (independent
    implementations: stored back-pointers vs checkpoint + recomputation) give identical rows, the
    rows tile each read without gaps inside a chunk and every score is bounded by its span."""
    mn, ms = synth.make_monomers(12, seed=1)
    rn, rs = synth.make_reads(ms, 24, read_len=50000, seed=1)
    res = {}
    for name, k in FAMILIES:
        e = lib.Engine(ms, kernel=k)
        assert e.load_reads(rs) == 240
        e.run()
        res[name] = e.fetch()
        e.close()
    assert res["fast"] == res["generic"]
    for chunk in res["fast"]:
        assert chunk[0][1] == 0
        for a, b in zip(chunk, chunk[1:]):
            assert b[1] == a[2] + 1
        for (t, s, en, sc) in chunk:
            assert 0 <= t < 24 and s <= en and sc <= en - s + 1 + 174


def _digest(chunks):
    h = hashlib.sha256()
    for ch in chunks:
        h.update(repr(ch).encode())
    return h.hexdigest()


def test_full_c2_size_families_agree():
    """BASELINE config 2 at full size (1000 reads x 50 kb = 10 000 chunks, 54.5 M rows): the two
    independent device implementations agree on every record, and the records satisfy the
    structural invariants of a decomposition (tiling of each chunk, template range, score bound)."""
    mn, ms = synth.make_monomers(12, seed=1)
    rn, rs = synth.make_reads(ms, 1000, read_len=50000, seed=1)
    dig = {}
    for name, k in FAMILIES:
        e = lib.Engine(ms, kernel=k)
        assert e.load_reads(rs) == 10000
        e.run()
        got = e.fetch()
        e.close()
        dig[name] = _digest(got)
        if name == "fast":
            assert sum(len(c) for c in got) > 300000
            for ci, chunk in enumerate(got):
                n = 5500 if ci % 10 != 9 else 5000
                assert chunk[0][1] == 0 and chunk[-1][2] == n - 1
                assert all(b[1] == a[2] + 1 for a, b in zip(chunk, chunk[1:]))
        del got
    assert dig["fast"] == dig["generic"]


def test_full_c2_sample_of_200_reads_equals_the_reference_binary(tmp_path):
    """VERDICT r02 (weak 6): full-size C2 parity against the REAL reference, not only between two in-repo kernel
    families -- the whole C2 read set goes through the device as one batch of 10 000 chunks (the bench's launch shape)
    and the raw TSV rows of every 5th read (200 reads, 10 Mbp) must equal what oracle/_ref/dp prints for those reads
    (the C restatement stands in where the reference binary was not built).  Also: the fp16 range guard never trips."""
    from oracle import binding as ob
    mn, ms = synth.make_monomers(12, seed=1)
    rn, rs = synth.make_reads(ms, 1000, read_len=50000, seed=1)
    t0 = lib.guard_trips()
    got = lib.decompose(rn, rs, mn, ms, threads=8)
    assert lib.guard_trips() == t0
    # ALL 1000 reads: the sha256 of what the reference binary printed for this input in the build container
    # (tests/golden/make_fullsize_hashes.py; a hash of expected output, the GPU box needs no reference for it)
    with open(os.path.join(GOLDEN, "fullsize_sha256.json")) as f:
        gold = json.load(f)["c2"]
    assert got.count(b"\n") == gold["rows"] and len(got) == gold["bytes"]
    assert hashlib.sha256(got).hexdigest() == gold["sha256"]
    by_read = {}
    for line in got.split(b"\n")[:-1]:
        by_read.setdefault(line[:line.index(b"\t")], []).append(line)
    sel = list(range(0, 1000, 5))
    if ob.have_ref_dp():
        rfa, mfa = str(tmp_path / "r.fa"), str(tmp_path / "m.fa")
        synth.write_fasta(rfa, [rn[i] for i in sel], [rs[i] for i in sel])
        synth.write_fasta(mfa, mn, ms)
        rc, want, err = ob.run_ref_dp(rfa, mfa, threads=8)
        assert rc == 0, err.decode()[-500:]
    else:
        # Not silently: without the reference binary this is only a comparison with the C restatement (which
        # tests/test_oracle.py pins against the binary's fixtures) -- it is said so, and SD_REQUIRE_REF=1 turns it into a failure
        assert not os.environ.get("SD_REQUIRE_REF"), "oracle/_ref/dp is missing: this run cannot compare with the reference binary"
        import warnings
        warnings.warn("oracle/_ref/dp not built: full-size C2 compared with the C restatement of the reference only")
        ob.build()
        want = ob.decompose([rn[i] for i in sel], [rs[i] for i in sel], mn, ms, threads=8)
    mine = b"".join(b"\n".join(by_read[rn[i].encode()]) + b"\n" for i in sel)
    assert mine == want


@pytest.mark.parametrize("sc,cells,rebase", [((-2, -1, -3, 6), "f16", 128), ((-2, -2, -3, 8), "f16", 128),
                                             # beyond the range at 128 rows between rebases: 64 rows, then integer cells
                                             ((-2, -2, -3, 9), "f16", 64), ((-2, -2, -3, 18), "f16", 64), ((-2, -2, -3, 33), "int16", 128),
                                             ((-2, -2, -3, 40), "int16", 128),
                                             ((-1, -1, -1, 1), "f16", 128), ((0, 0, -1, 14), "f16", 128), ((0, 0, -1, 15), "f16", 64),
                                             ((0, 0, -1, 31), "int16", 128), ((0, 0, -1, 50), "int16", 128),
                                             # a large |del| with non-positive scores: the range is (Lmax-1)*|del| wide
                                             ((0, -6, -4, -1), "f16", 128), ((0, -7, -4, -1), "f16", 64), ((0, -9, -4, -1), "int16", 128),
                                             ((0, -10, -4, -1), "int16", 128), ((-1, -5, -2, 1), "f16", 128),
                                             # a common factor is divided out on the device and multiplied back
                                             ((-10, -10, -10, 10), "f16", 128), ((-4, -6, -8, 4), "f16", 128), ((0, 0, -3, 45), "f16", 64),
                                             ((0, 0, -3, 150), "int16", 128),
                                             # round 6: beyond saturating int16, inside the biased-u16 window
                                             ((0, 0, -1, 100), "u16", 128)])
@pytest.mark.parametrize("legacy", [False, True])
def test_fill_cell_format_switch_at_the_fp16_range_limit(oracle, sc, cells, rebase, legacy):
    """Round 6: the narrow fill keeps its cells as biased unsigned 16-bit integers (CellOps<CF_U16>: exact over +-15 k, one
    format for all of these scorings, 128 rows between rebases).  With FLAG_NO_U16 (`legacy`) the formats of rounds 1-5:
    packed fp16 cells while the score range keeps every value an exact integer
    (fast_plan_build: with 128 or 64 rows between two rebases of the stored cells), packed int16 beyond.
    Scorings on both sides of every switch, on reads that
    maximise score growth (exact repeats), insertions (unrelated sequence) and ordinary noise."""
    if legacy and cells == "u16":
        pytest.skip("no 16-bit format of rounds 1-5 holds this scoring")
    fl = lib.FLAG_NO_U16 if legacy else 0
    if not legacy:
        cells, rebase = "u16", 128
    mn, ms = synth.make_monomers(12, seed=3)
    st = synth.Stream(3, 5)
    rn, rs = synth.make_reads(ms, 2, read_len=12000, seed=4)
    rs = list(rs) + [(ms[0] * 40)[:6100], synth._ACGT[st.below(5600, 4)].tobytes(), ms[5] * 3 + b"A" * 700 + ms[2] * 20]
    rn = ["r%d" % i for i in range(len(rs))]
    e = lib.Engine(ms, scoring=sc, kernel=lib.KERNEL_FAST, flags=fl)
    assert e.info()["cells"] == cells and lib.plan_info(ms, scoring=sc, flags=fl)["rebase"] == rebase
    e.close()
    t0 = lib.guard_trips()
    got = lib.decompose(rn, rs, mn, ms, scoring=sc, kernel=lib.KERNEL_FAST, flags=fl)
    assert lib.guard_trips() == t0   # (the run-time check of the fp16 range agrees with the plan's period)
    assert got == oracle.decompose(rn, rs, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc)


FUZZ = os.path.join(GOLDEN, "fuzz")


@pytest.mark.parametrize("case", sorted(os.listdir(FUZZ)) if os.path.isdir(FUZZ) else [])
def test_fuzz_regressions(oracle, case):
    """Inputs on which tools/fuzz_gpu.py once found a mismatch (kept as data: reads, monomers, parameters).
    fuzz_fail_906_791: scoring 0,-4,-4,-1 on 300-480 bp monomers -- the fp16 cells left the exact-integer range
    because the range bound ignored that B can grow by (smax - del) per row (csrc/sd_fast.hip, fast_plan_build).
    fuzz_fail_1301_1135 (found while the plan learned to move lane boundaries, never in a committed build): a 5-bp
    template whose first lane was cut down to one cell -- cell 0 has no insertion move, so a pad behind it kept a
    stale value; the first lane now keeps at least two cells."""
    d = os.path.join(FUZZ, case)
    rn, rs, _ = lib.fasta_load(os.path.join(d, "r.fa"))
    mn, ms, _ = lib.fasta_load(os.path.join(d, "m.fa"))
    with open(os.path.join(d, "params.json")) as f:
        pj = json.load(f)
    sc, part, ov, ed = tuple(pj["scoring"]), pj["part_size"], pj["overlap"], pj["ed_thr"]
    exp = oracle.decompose(rn, rs, mn, ms, threads=8, sc=sc, part=part, overlap=ov, ed_thr=ed)
    for e2 in sorted({ed, -1}):
        for sub in (ms, ms[:1]):
            want = exp if (e2 == ed and sub is ms) else oracle.decompose(rn, rs, mn[:len(sub)], sub, threads=8, sc=sc,
                                                                        part=part, overlap=ov, ed_thr=e2)
            for fam in (lib.KERNEL_AUTO, lib.KERNEL_GENERIC):
                got = lib.decompose(rn, rs, mn[:len(sub)], sub, scoring=sc, part_size=part, overlap=ov, ed_thr=e2, kernel=fam)
                assert got == want, (case, e2, len(sub), fam)


def test_single_long_sequence_custom_scoring_vs_oracle(oracle):
    """BASELINE config 5 in miniature: one long sequence (1.2 Mb -> 240 chunks), custom -s scoring
    (honoured, as by the reference binary in its 9-argument form), against the oracle."""
    mn, ms = synth.make_monomers(12, seed=5)
    rn, rs = synth.make_reads(ms, 1, read_len=1200000, seed=5)
    sc = (-2, -3, -4, 2)
    got = lib.decompose(rn, rs, mn, ms, scoring=sc)
    exp = oracle.decompose(rn, rs, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc)
    assert got == exp


def test_64_monomer_set_wide_layout(oracle):
    """BASELINE config 4 shape: 64 monomers (128 templates, one per virtual lane, int8 table):
    chunk-level records vs the oracle, N in the reads, and agreement with the generic family on
    more chunks than the oracle can cover quickly."""
    mn, ms = synth.make_monomers(64, seed=11)
    tm = [m.decode() for m in ms] + [synth.revcomp_bytes(m).decode() for m in ms]
    rn, rs = synth.make_reads(ms, 3, read_len=900, seed=12)
    rs = [rs[0], rs[1][:333], rs[2][:40] + b"NNN" + rs[2][43:700]]
    for sc in [(-1, -1, -1, 1), (-2, -3, -4, 2)]:
        e = lib.Engine(ms, scoring=sc, kernel=lib.KERNEL_FAST)
        assert e.info()["cells_per_lane"] >= 176
        assert e.info()["cells"] == "f16/bf8-table"   # default scoring: table values 3 and 1 are exact in bf8
        e.load_reads(rs)
        e.run()
        got = e.fetch()
        e.close()
        for s, g in zip(rs, got):
            exp = oracle.align_chunk(s.decode(), tm, sc)
            assert g == [(t, a, b, int(v)) for (t, a, b, v) in exp]
    rn, rs = synth.make_reads(ms, 8, read_len=50000, seed=13)
    res = {}
    for name, k in FAMILIES:
        e = lib.Engine(ms, kernel=k)
        e.load_reads(rs)
        e.run()
        res[name] = e.fetch()
        e.close()
    assert res["fast"] == res["generic"]


@pytest.mark.parametrize("thr", [0, 8, 25, 60])
def test_ed_thr_prefilter_vs_oracle(oracle, thr):
    """--ed_thr (main.cpp:128-149): per-chunk infix edit distances, kept set and its order
    (which decides score ties) against the oracle, on reads with N and a custom scoring."""
    mn, ms = synth.make_monomers(12, seed=41)
    rn, rs = synth.make_reads(ms, 3, read_len=11000, seed=42)
    b = bytearray(rs[1])
    for pos in synth.Stream(42, 7).below(300, len(b)):
        b[int(pos)] = ord("N")
    rs[1] = bytes(b)
    rs[2] = rs[2][:777]
    for sc in [(-1, -1, -1, 1), (-2, -3, -4, 2)]:
        got = lib.decompose(rn, rs, mn, ms, scoring=sc, ed_thr=thr)
        exp = oracle.decompose(rn, rs, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc, ed_thr=thr)
        assert got == exp


def _random_monomers(st, n, lo, hi, with_n=False):
    """n related monomers (a common ancestor, 15 % substitutions) with lengths in [lo, hi]."""
    anc = st.below(hi + 16, 4)
    out = []
    for j in range(n):
        L = lo + int(st.below(1, hi - lo + 1)[0])
        codes = synth.mutate(anc, st, 0.15, 0.02, 0.02)
        while len(codes) < L:
            codes = np.concatenate([codes, st.below(L, 4)])
        m = bytearray(synth._to_ascii(codes[:L]))
        if with_n and j % 3 == 0 and L > 2:
            m[L // 2] = ord("N")
        out.append(bytes(m))
    return out


SHAPES = [  # (monomers, min len, max len, N in templates)
    (1, 8, 12, False), (2, 30, 60, False), (3, 100, 130, True), (5, 160, 186, False),
    (12, 165, 176, True), (20, 90, 110, False), (31, 60, 64, False), (40, 120, 176, False),
    (64, 167, 176, False), (64, 200, 224, False), (7, 230, 250, False), (9, 2, 40, False),
    (6, 300, 400, False), (3, 480, 512, True), (2, 513, 600, False),
]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d-%d%s" % (a, b, c, "N" if d else "") for a, b, c, d in SHAPES])
def test_random_template_set_shapes_vs_oracle(oracle, shape):
    """Layout corner cases of the kernel families (slots per lane, virtual lanes per template,
    narrow / wide / generic, N in templates) on random template sets, every record against the
    oracle.  Reads are random concatenations of mutated templates plus junk and N."""
    nm, lo, hi, with_n = shape
    st = synth.Stream(1234, nm * 1000 + lo)
    ms = _random_monomers(st, nm, lo, hi, with_n)
    mn = ["m%d" % j for j in range(nm)]
    reads = []
    for r in range(3):
        parts = []
        while sum(len(x) for x in parts) < 700 + 150 * r:
            j = int(st.below(1, nm)[0])
            codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8),
                                    np.frombuffer(ms[j].replace(b"N", b"A"), dtype=np.uint8))
            x = synth._to_ascii(synth.mutate(codes, st, 0.05, 0.03, 0.03))
            parts.append(synth.revcomp_bytes(x) if st.below(1, 2)[0] else x)
            if st.below(1, 4)[0] == 0:
                parts.append(synth._to_ascii(st.below(int(st.below(1, 40)[0]) + 1, 4)))
        b = bytearray(b"".join(parts))
        b[len(b) // 3] = ord("N")
        reads.append(bytes(b))
    rn = ["r%d" % i for i in range(len(reads))]
    for sc, part, ov, ed in [((-1, -1, -1, 1), 5000, 500, -1), ((-2, -3, -4, 2), 300, 50, -1),
                             ((-1, -2, -1, 3), 5000, 500, -1), ((-1, -1, -1, 1), 700, 100, 30)]:
        try:
            got = lib.decompose(rn, reads, mn, ms, scoring=sc, part_size=part, overlap=ov, ed_thr=ed)
        except lib.SdError as e:
            assert ed > -1 and hi > 512 and e.code == lib.SD_ERR_UNSUPPORTED  # --ed_thr: templates of up to 512 bp
            continue
        exp = oracle.decompose(rn, reads, mn, ms, threads=8, sc=sc, part=part, overlap=ov, ed_thr=ed)
        assert got == exp, (shape, sc, ed)


def test_device_batching_is_invisible():
    """Chunks are fed to the device in batches sized to the free HBM; forcing tiny batches (a
    single read then spans many batches) must not change a byte."""
    mn, ms = synth.make_monomers(12, seed=9)
    rn, rs = synth.make_reads(ms, 5, read_len=50000, seed=9)
    rs[1] = rs[1][:123]
    rs[3] = rs[3][:27111]
    ref = lib.decompose(rn, rs, mn, ms)
    for cap in (5500, 17000, 60001):
        assert lib.decompose(rn, rs, mn, ms, max_batch_rows=cap, threads=3) == ref


def test_cli_end_to_end_reference_golden(tmp_path):
    """The reference's own integration test (reference Makefile:16-19): CLI with --second-best on
    test_data, grep the log line, diff final_decomposition.tsv against the golden file."""
    td = os.path.join(GOLDEN, "test_data")
    out = str(tmp_path / "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"),
                        os.path.join(td, "read.fa"), os.path.join(td, "DXZ1_star_monomers.fa"),
                        "-o", out, "--second-best", "-t", "4"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    with open(os.path.join(out, "stringdecomposer.log")) as f:
        assert "Thank you for using StringDecomposer!" in f.read()
    with open(os.path.join(out, "final_decomposition.tsv"), "rb") as f, \
            open(os.path.join(td, "final_decomposition_fc89af8.tsv"), "rb") as g:
        assert f.read() == g.read()
    with open(os.path.join(out, "final_decomposition_raw.tsv"), "rb") as f:
        assert f.read() == load_case("td_default")["raw"]


def test_cli_scoring_ref_compat_and_ed_thr(tmp_path, oracle):
    """CLI flags: -s is honoured (documented difference), --ref-compat reproduces the reference
    CLI (scores ignored), --ed_thr is passed through; light mode writes an empty _alt.tsv."""
    mn, ms = synth.make_monomers(12, seed=51)
    rn, rs = synth.make_reads(ms, 2, read_len=6000, seed=52)
    rf, mf = str(tmp_path / "r.fa"), str(tmp_path / "m.fa")
    synth.write_fasta(rf, rn, rs, width=70)
    synth.write_fasta(mf, mn, ms)

    def run(extra, name):
        out = str(tmp_path / name)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), rf, mf, "-o", out,
                            "-t", "4"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()
        with open(os.path.join(out, "final_decomposition_raw.tsv"), "rb") as f:
            raw = f.read()
        assert os.path.getsize(os.path.join(out, "final_decomposition_alt.tsv")) == 0
        with open(os.path.join(out, "final_decomposition.tsv")) as f:
            final = f.read().splitlines()
        assert len(final) == raw.count(b"\n") and all(len(l.split("\t")) == 12 for l in final)
        return raw

    sc = (-2, -3, -4, 2)
    assert run(["--scoring=-2,-3,-4,2"], "a") == oracle.decompose(rn, rs, mn, ms, threads=8, sc=sc)
    default = oracle.decompose(rn, rs, mn, ms, threads=8)
    assert run(["--scoring=-2,-3,-4,2", "--ref-compat"], "b") == default
    assert run(["--ed_thr", "12"], "c") == oracle.decompose(rn, rs, mn, ms, threads=8, ed_thr=12)
    assert run(["-b", "700", "-v", "100"], "d") == oracle.decompose(rn, rs, mn, ms, threads=8, part=700, overlap=100)


def test_chunk_range_form_equals_one_shot(oracle):
    """the global chunk table cut into contiguous ranges (what each GPU of a multi-GPU job
    runs), records concatenated and assembled on the host == the one-shot call == the oracle.  One long
    sequence (so a single read spans several ranges) + ordinary reads; small device batches inside a range."""
    mn, ms = synth.make_monomers(12, seed=9)
    rn, rs = synth.make_reads(ms, 5, read_len=23000, seed=9)
    n1, s1 = synth.make_reads(ms, 1, read_len=260000, seed=10)
    rn, rs = ["chrX"] + list(rn), list(s1) + list(rs)
    sc = (-1, -2, -1, 1)
    one = lib.decompose(rn, rs, mn, ms, scoring=sc)
    n = lib.chunk_table_size([len(s) for s in rs])
    assert n == sum(len(lib.chunk_plan(len(s))) for s in rs)
    parts = []
    for g in range(3):
        lo, hi = shard.block_range(n, g, 3)
        parts.append(lib.decompose_chunk_range(rs, ms, lo, hi, scoring=sc, max_batch_rows=[0, 30000, 9000][g]))
    recs = np.concatenate([p[0] for p in parts])
    off = np.concatenate([[0]] + [p[1][1:] + sum(len(q[0]) for q in parts[:i]) for i, p in enumerate(parts)])
    got = lib.assemble_tsv(rn, [len(s) for s in rs], mn, recs, off, scoring=sc, threads=3)
    assert got == one
    assert got == oracle.decompose(rn, rs, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc)
    assert shard.decompose_sharded(rn, rs, mn, ms, scoring=sc) == one
    with pytest.raises(lib.SdError):
        lib.decompose_chunk_range(rs, ms, 0, n + 1)


@pytest.mark.parametrize("data", ["one_sequence", "read_set"])
def test_cli_two_processes_on_one_gpu(tmp_path, data):
    """The multi-GPU launch form of the CLI (one process per GPU under torch.distributed.run); here both
    ranks share GPU 0.  Output files equal the single-process run.  One sequence: sharded by chunk range, rank 0
    assembles; a read set: every rank runs its group of reads completely and the parts are spliced."""
    td = os.path.join(GOLDEN, "test_data")
    rfa, mfa = os.path.join(td, "read.fa"), os.path.join(td, "DXZ1_star_monomers.fa")
    if data == "read_set":
        mn, ms = synth.make_monomers(12, seed=71)
        rn, rs = synth.make_reads(ms, 7, read_len=21000, seed=72)
        rs[3] = rs[3][:4000]
        rfa, mfa = str(tmp_path / "r.fa"), str(tmp_path / "m.fa")
        synth.write_fasta(rfa, rn, rs, width=60)
        synth.write_fasta(mfa, mn, ms)
    outs = []
    # (three ranks on the one sequence: the middle rank's share lies INSIDE the read -- its entry position comes from rank 0's
    # edge, its last rows need rank 2's first records: shard._assemble_by_ranks / csrc/sd_seam.hpp)
    for nproc in ((1, 2, 3) if data == "one_sequence" else (1, 2)):
        out = str(tmp_path / ("o%d" % nproc))
        cmd = [sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), rfa,
               mfa, "-o", out, "-t", "4", "--second-best"]
        if nproc > 1:
            import socket
            with socket.socket() as sk:     # an ephemeral port: a fixed one collides with a run that is still closing
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                   "--master-addr", "127.0.0.1", "--master-port", str(port)] + cmd[1:]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        outs.append(out)
    for fn in ("final_decomposition_raw.tsv", "final_decomposition.tsv", "final_decomposition_alt.tsv"):
        with open(os.path.join(outs[0], fn), "rb") as a:
            one = a.read()
        for other in outs[1:]:
            with open(os.path.join(other, fn), "rb") as b:
                assert one == b.read(), (fn, other)
    if data == "one_sequence":   # the ranks wrote the raw TSV themselves (rank 0 logs its part), no gather on rank 0
        with open(os.path.join(outs[2], "stringdecomposer.log")) as f:
            assert "this rank wrote" in f.read()


def test_device_buffer_cache_reuse_and_release(oracle):
    """Engines hand their large device buffers to a process-wide cache; a later engine with other sizes
    and another template set must get correct results from recycled (stale) buffers, also after the
    cache was released."""
    mn1, ms1 = synth.make_monomers(12, seed=21)
    mn2, ms2 = synth.make_monomers(5, seed=22)
    rn1, rs1 = synth.make_reads(ms1, 40, read_len=30000, seed=21)
    rn2, rs2 = synth.make_reads(ms2, 3, read_len=9000, seed=22)
    a1 = lib.decompose(rn1, rs1, mn1, ms1)
    b1 = lib.decompose(rn2, rs2, mn2, ms2, scoring=(-1, -2, -1, 1))
    lib.release_cache()
    b2 = lib.decompose(rn2, rs2, mn2, ms2, scoring=(-1, -2, -1, 1))
    a2 = lib.decompose(rn1, rs1, mn1, ms1)
    assert a1 == a2 and b1 == b2
    assert b1 == oracle.decompose(rn2, rs2, mn2, ms2, threads=8, sc=(-1, -2, -1, 1))


@pytest.mark.parametrize("sub,cap", [(1, 0), (4, 0), (3, 21000), (7, 5600)])
def test_stream_rows_equal_oracle(oracle, sub, cap):
    """sd_stream_* (sequences in host memory -> rows in host memory, what bench.py times): jobs submitted
    back to back and cut into sub-batches -- a long read spans several of them -- give, formatted, the
    oracle's raw TSV; rows of a job do not depend on what else is in flight."""
    mn, ms = synth.make_monomers(12, seed=61)
    tn = list(mn) + [n + "'" for n in mn]
    rn, rs = synth.make_reads(ms, 9, read_len=17000, seed=62)
    n1, s1 = synth.make_reads(ms, 1, read_len=93000, seed=63)
    rs = rs[:4] + s1 + rs[4:]
    rs[2] = rs[2][:499]
    rs[7] = rs[7][:5500]
    rn = ["r%d" % i for i in range(len(rs))]
    jobs = [(rn, rs), (rn[5:], rs[5:]), (rn[:3], rs[:3]), (rn, rs)]
    st = lib.Stream(ms, sub_batches=sub, max_batch_rows=cap, threads=6)
    got = []
    for k, (_, seqs) in enumerate(jobs):
        st.submit(seqs)
        if k >= 1:
            got.append(st.collect(as_lists=True))
    got.append(st.collect(as_lists=True))
    stats = st.stats()
    st.close()
    assert stats["jobs"] == 4 and stats["batches"] >= 4 * min(sub, 3)
    for (names, seqs), rows in zip(jobs, got):
        txt = b"".join(lib.format_rows(n, tn, r) for n, r in zip(names, rows))
        assert txt == oracle.decompose(names, seqs, mn, ms, threads=8)
    with pytest.raises(lib.SdError):
        lib.Stream(ms).collect()
    # the same jobs through Stream.imap (two later jobs submitted before a job is collected: all three engines busy),
    # and with every depth from 0 to more jobs than there are
    for depth in (None, 0, 1, 3, 9):
        st = lib.Stream(ms, sub_batches=sub, max_batch_rows=cap, threads=6)
        again = list(st.imap([seqs for _, seqs in jobs] * 2, as_lists=True, depth=depth))
        st.close()
        assert again == got + got, depth


# (4, 520, 1000) / (3, 700, 2000): monomers beyond 512 bp -- a pair across 16 / 32 lanes (sd_nw_long.hip); the pairs edlib
# aligns by Hirschberg's split (~1.7 kb x 1.7 kb and beyond) go to host threads inside the same call
@pytest.mark.parametrize("shape", [(12, 160, 180), (64, 165, 178), (5, 20, 70), (3, 300, 500), (2, 1, 5), (7, 120, 260),
                                   (4, 520, 1000), (3, 700, 2000), (5, 600, 1500)])
def test_nw_identity_kernel_equals_host_and_edlib(shape):
    """K3 (main.py:29-60,107-150): the device identity kernel (one lane per (segment, template) pair) against
    the host implementation -- itself pinned against the reference's vendored edlib on CPU -- for every pair,
    all-vs-all and own-template, plain and homopolymer-compressed, and against edlib directly on a sample.  Every device
    call moves the route counters (lib.nw_route_counts) by what the dealing rule of tests/long_ident_cases.py gives for it."""
    import edlib_ref
    nm, lo, hi = shape
    st = synth.Stream(77, nm * 100 + lo)
    ms = _random_monomers(st, nm, lo, hi, with_n=(nm == 5))
    tm = [m.decode() for m in ms] + [synth.revcomp_bytes(m).decode() for m in ms]
    parts = []
    while sum(len(x) for x in parts) < 40000:
        j = int(st.below(1, nm)[0])
        codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(ms[j].replace(b"N", b"A"), dtype=np.uint8))
        x = synth._to_ascii(synth.mutate(codes, st, 0.08, 0.04, 0.04)) or b"A"
        parts.append(synth.revcomp_bytes(x) if st.below(1, 2)[0] else x)
        if st.below(1, 6)[0] == 0:
            parts.append(bytes([b"ACGT"[int(st.below(1, 4)[0])]]) * (1 + int(st.below(1, 30)[0])))
    seq = bytearray(b"".join(parts))
    for p in st.below(40, len(seq)):
        seq[int(p)] = ord("N")
    seq = bytes(seq)
    n = 300
    starts = np.sort(st.below(n, len(seq) - 2 * hi - 2))
    lens = st.below(n, 2 * hi) + 1
    lens[:5] = [1, 2, 64, 65, 2 * hi]
    lens[5:7] = [1100, 2600]          # longer than the short launch's checkpoint slots: the second launch
    starts[5:7] = np.minimum(starts[5:7], len(seq) - 2700)
    ends = starts + lens - 1
    pair = st.below(n, len(tm)).astype(np.int32)
    import long_ident_cases as lc
    tmb = [t.encode() for t in tm]

    def routed(before, pt):
        """The device call between `before` and now took the route the dealing rule gives it (lib.identity_segments runs the
        host form without a word when the device declines: equal results alone do not show which code ran)."""
        after = lib.nw_route_counts()
        moved = {k: after[k] - before[k] for k in lc.COUNT_KEYS}
        exp = lc.expected_counts([int(x) for x in lens], tmb, homo, pt)
        assert moved == exp, (shape, homo, moved, exp)
        if hi > 512 and not homo:
            assert moved["long_calls"] == 1
        if moved["long_calls"]:      # by the rule no pair of (4, 520, 1000) splits, about a tenth of the other two shapes' do
            assert moved["long_pairs"] > 0 and moved["short_pairs"] == 0
            assert (moved["long_host_pairs"] > 0) == (hi > 1000)
        else:
            assert moved["short_pairs"] > 0 and moved["declined_calls"] == 0
    for homo in (False, True):
        h = lib.identity_segments(seq, starts, ends, tm, homo, threads=8)
        before = lib.nw_route_counts()
        d = lib.identity_segments(seq, starts, ends, tm, homo, threads=8, device=0)
        routed(before, None)
        for a, b in zip(h, d):
            assert (a == b).all(), (shape, homo)
        hp = lib.identity_segments(seq, starts, ends, tm, homo, threads=8, pair_tmpl=pair)
        before = lib.nw_route_counts()
        dp = lib.identity_segments(seq, starts, ends, tm, homo, threads=8, pair_tmpl=pair, device=0)
        routed(before, pair)
        for a, b in zip(hp, dp):
            assert (a == b).all(), (shape, homo, "pair")
        for s_ in range(0, n, 37):
            for t_ in range(0, len(tm), 5):
                q, t = seq[starts[s_]:ends[s_] + 1].decode(), tm[t_]
                if homo:
                    q, t = edlib_ref.homo(q), edlib_ref.homo(t)
                assert edlib_ref.nw(q, t) == (int(d[0][s_, t_]), int(d[1][s_, t_]), int(d[2][s_, t_]))
    # input the kernel does not take falls back to the host implementation inside lib.identity_segments
    bad = seq[:100] + b"R" + seq[101:]
    a = lib.identity_segments(bad, starts[:20], ends[:20], tm, False, threads=2, device=0)
    b = lib.identity_segments(bad, starts[:20], ends[:20], tm, False, threads=2)
    assert all((x == y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("nm,lo,hi", [(100, 165, 178), (260, 150, 176), (70, 300, 480), (520, 90, 120), (48, 300, 340), (20, 700, 1100)])
def test_template_sets_beyond_the_fast_family_vs_oracle(oracle, nm, lo, hi):
    """Hundreds of monomers (the reference takes any monomer set, main.cpp:187-207): more than 128
    templates run on the generic family, more than 32 768 template cells on its tiled form (previous row
    in HBM); with and without --ed_thr (rank table instead of the fast family's lane constants)."""
    st = synth.Stream(4321, nm)
    ms = _random_monomers(st, nm, lo, hi)
    mn = ["m%d" % j for j in range(nm)]
    reads = []
    for r in range(3):
        parts = []
        while sum(len(x) for x in parts) < 500 + 300 * r:
            j = int(st.below(1, nm)[0])
            codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(ms[j], dtype=np.uint8))
            x = synth._to_ascii(synth.mutate(codes, st, 0.05, 0.03, 0.03))
            parts.append(synth.revcomp_bytes(x) if st.below(1, 2)[0] else x)
        b = bytearray(b"".join(parts))
        b[len(b) // 2] = ord("N")
        reads.append(bytes(b))
    rn = ["r%d" % i for i in range(len(reads))]
    e = lib.Engine(ms)
    info = e.info()
    e.close()
    # up to 1024 templates of <= 224 bp run on the multi-wave wide layout, longer ones on the tiled multi-wave layout
    # (sd_fast_wt.hip: a template over several virtual lanes) while eight waves hold them
    assert info["sum_template_len"] > (32768 if nm > 100 else 28000)
    # (more than 1024 virtual lanes: generic family, tiled over HBM)
    assert (info["family"], info["cells"]) == (("fast", "f16/bf8-codes x waves") if hi <= 224 and 2 * nm <= 1024
                                               else ("fast", "f16/bf8-codes tiled x waves") if 2 * nm <= 1024
                                               else ("generic", "int32"))
    for sc, part, ov, ed in [((-1, -1, -1, 1), 5000, 500, -1), ((-2, -3, -4, 2), 400, 60, -1),
                             ((-1, -1, -1, 1), 700, 100, 40), ((-1, -1, -1, 1), 5000, 500, 0)]:
        exp = oracle.decompose(rn, reads, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc, part=part, overlap=ov, ed_thr=ed)
        got = lib.decompose(rn, reads, mn, ms, scoring=sc, part_size=part, overlap=ov, ed_thr=ed)
        assert got == exp, (nm, sc, ed)
        gen = lib.decompose(rn, reads, mn, ms, scoring=sc, part_size=part, overlap=ov, ed_thr=ed, kernel=lib.KERNEL_GENERIC)
        assert gen == exp, (nm, sc, ed, "generic")


@pytest.mark.parametrize("layout", ["narrow12", "narrow3_short", "one_bp", "wide64", "waves140", "tiled30"])
@pytest.mark.parametrize("sc", [(1, -1, -1, 1), (2, -3, -4, 2), (1, -2, 0, 3), (3, 0, -2, 1)])
def test_positive_insertion_score_on_the_fast_family_vs_oracle(oracle, layout, sc):
    """VERDICT r05 (missing 2): the reference takes any scoring (main.cpp:187-207); the fast family refused every positive gap
    score.  A positive INSERTION score needs nothing from the kernels -- the stored domain S = E - base - tp*ins makes the
    insertion move 'keep' for any sign, B's growth per row is charged with max(0, smax - del, ins) in the range bound -- so it
    now runs there on every layout (a positive deletion score cannot: a whole template deleted gains (L - 1) * del in one row).
    Rows against the oracle and the generic family; reads that are mostly insertions (unrelated sequence), exact repeats,
    ordinary noise, N; small chunks (many seams), --ed_thr."""
    if layout == "narrow12":
        mn, ms = synth.make_monomers(12, seed=5)
    elif layout == "narrow3_short":
        mn, ms = synth.make_monomers(3, seed=6)
        ms = [m[:40 + 9 * j] for j, m in enumerate(ms)]
    elif layout == "one_bp":
        mn, ms = synth.make_monomers(4, seed=7)
        ms = [ms[0][:60], b"A", ms[1][:33], b"GC"]
    elif layout == "wide64":
        mn, ms = synth.make_monomers(64, seed=8)
    elif layout == "waves140":
        mn, ms = synth.make_monomers(140, seed=9)
    else:
        mn, ms = synth.make_monomers(60, seed=3)
        ms = [ms[2 * j] + ms[2 * j + 1] for j in range(30)]
    mn = ["m%d" % j for j in range(len(ms))]
    info = lib.plan_info(ms, scoring=sc)
    if info["family"] != "fast":
        assert layout in ("waves140", "tiled30") or max(sc) > 2, (info, "only the multi-wave layouts may leave the 16-bit range")
        pytest.skip("beyond the 16-bit range of this layout: " + info["why"])
    st = synth.Stream(61, len(ms))
    rn, rs = synth.make_reads(ms, 2, read_len=2600 if len(ms) > 20 else 7000, seed=12)
    big = max(ms, key=len)
    rs = list(rs) + [synth._ACGT[st.below(1500, 4)].tobytes(), (big * 30)[:1800], b"T" * 90 + big * 2 + b"N" * 5 + ms[0] * 3, b"C", b"GA"]
    rn = ["r%d" % i for i in range(len(rs))]
    for part, ov, ed in ((5000, 500, -1), (400, 60, -1), (700, 100, 25)):
        exp = oracle.decompose(rn, rs, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc, part=part, overlap=ov, ed_thr=ed)
        t0 = lib.guard_trips()
        got = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc, part_size=part, overlap=ov, ed_thr=ed)
        assert got == exp, (layout, sc, part, ed)
        assert lib.guard_trips() == t0, (layout, sc, "the plan's bound did not hold")
        if layout.startswith("narrow") or layout == "one_bp":   # the cell formats of rounds 1-5 and the one-block traceback too
            assert lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc, part_size=part, overlap=ov, ed_thr=ed,
                                 flags=lib.FLAG_NO_U16 | lib.FLAG_TRACE_V1) == exp, (layout, sc, part, ed, "legacy cells")
        assert lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_GENERIC, scoring=sc, part_size=part, overlap=ov, ed_thr=ed) == exp


@pytest.mark.parametrize("nm,lo,hi,waves", [(24, 400, 420, 2), (5, 950, 1000, 1), (40, 230, 700, None), (90, 120, 330, None)])
def test_tiled_multiwave_layout_vs_oracle(oracle, nm, lo, hi, waves):
    """csrc/sd_fast_wt.hip: template sets beyond the narrow layout (8192 cells in one wave) whose templates are longer
    than the widest lane (224 slots) -- a template lies over several virtual lanes of one of up to eight waves and the
    deletion chain crosses lanes and 32-row checkpoints.  Reads long enough for a dozen rebases of the fp16 state, N in
    reads and templates, small chunks (many seams), --ed_thr (compacted: a chunk's kept templates re-dealt over as many
    waves as they need; and the ranked form: per-chunk end offsets on every lane of a template), against the oracle."""
    st = synth.Stream(9090 + nm, hi)
    ms = _random_monomers(st, nm, lo, hi, with_n=True)
    mn = ["m%d" % j for j in range(nm)]
    pi = lib.plan_info(ms)
    assert (pi["family"], pi["cells"]) == ("fast", "f16/bf8-codes tiled x waves"), pi
    if waves:
        assert pi["waves"] == waves, pi
    reads = []
    for r in range(3):
        parts = []
        while sum(len(x) for x in parts) < 2600 + 900 * r:
            j = int(st.below(1, nm)[0])
            codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(ms[j].replace(b"N", b"A"), dtype=np.uint8))
            x = synth._to_ascii(synth.mutate(codes, st, 0.06, 0.03, 0.03))
            parts.append(synth.revcomp_bytes(x) if st.below(1, 2)[0] else x)
        b = bytearray(b"".join(parts))
        b[len(b) // 3] = ord("N")
        reads.append(bytes(b))
    reads.append(reads[0][:37])          # shorter than any template
    reads.append(reads[1][100:100 + hi])  # one template long
    rn = ["r%d" % i for i in range(len(reads))]
    for sc, part, ov, ed in [((-1, -1, -1, 1), 5000, 500, -1), ((-1, -1, -1, 1), 700, 100, -1),
                             ((-1, -1, -1, 1), 1500, 300, 60), ((-1, -1, -1, 1), 5000, 500, 0),
                             ((-1, -2, -1, 1), 1100, 150, -1)]:
        if lib.plan_info(ms, scoring=sc)["family"] != "fast":
            continue                    # (a scoring beyond the fp16 range of the set: the generic family, tested elsewhere)
        exp = oracle.decompose(rn, reads, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc, part=part, overlap=ov, ed_thr=ed)
        t0 = lib.guard_trips()          # (a process-wide count: tests that trip the guard on purpose may have run before)
        got = lib.decompose(rn, reads, mn, ms, scoring=sc, part_size=part, overlap=ov, ed_thr=ed)
        assert got == exp, (nm, sc, part, ed)
        assert lib.guard_trips() == t0
        if ed >= 0:   # the filter compacts a chunk's kept templates into fewer waves (sd_tiled_place); without: every template, ranked
            full = lib.decompose(rn, reads, mn, ms, scoring=sc, part_size=part, overlap=ov, ed_thr=ed, flags=lib.FLAG_NO_EDTHR_COMPACT)
            assert full == exp, (nm, sc, part, ed, "ranked form")


@pytest.mark.gpu
def test_ed_thr_on_a_set_beyond_eight_waves_filter_only_form(oracle):
    """1 200 templates (600 monomers of 100-250 bp) do not fit eight waves: without --ed_thr the generic family.  With it a
    chunk's KEPT templates mostly do (what the reference's prefilter is for, main.cpp:128-149): every chunk is filled in
    the compacted tiled form (FastPlan::filter_only, sd_tiled_place); a chunk whose kept templates do not fit either
    (--ed_thr 250 keeps everything) raises the guard flag and the batch is repeated on the generic family."""
    st = synth.Stream(606, 6)
    nm = 600
    ms = _random_monomers(st, nm, 100, 250)
    mn = ["m%d" % j for j in range(nm)]
    assert lib.plan_info(ms)["family"] == "generic"
    pi = lib.plan_info(ms, ed_thr=25)
    assert (pi["family"], pi["cells"], pi["waves"]) == ("fast", "f16/bf8-codes tiled x waves", 8), pi
    reads = []
    for r in range(4):
        parts = []
        while sum(len(x) for x in parts) < 1500 + 700 * r:
            j = int(st.below(1, nm)[0])
            codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(ms[j], dtype=np.uint8))
            x = synth._to_ascii(synth.mutate(codes, st, 0.05, 0.03, 0.03))
            parts.append(synth.revcomp_bytes(x) if st.below(1, 2)[0] else x)
        b = bytearray(b"".join(parts))
        b[len(b) // 2] = ord("N")
        reads.append(bytes(b))
    reads.append(reads[0][:50])
    rn = ["r%d" % i for i in range(len(reads))]
    thr = min(32, os.cpu_count() or 1)
    for part, ov, ed in ((5000, 500, 25), (600, 100, 40), (5000, 500, 0)):
        exp = oracle.decompose(rn, reads, mn, ms, threads=thr, part=part, overlap=ov, ed_thr=ed)
        t0 = lib.guard_trips()
        got = lib.decompose(rn, reads, mn, ms, part_size=part, overlap=ov, ed_thr=ed)
        assert got == exp, (part, ed)
        assert lib.guard_trips() == t0, (part, ed)        # every chunk's kept templates fit: no repeat
    e = lib.Engine(ms, ed_thr=25)
    assert e.info()["family"] == "fast"
    e.close()
    exp = oracle.decompose(rn, reads, mn, ms, threads=thr, ed_thr=250)
    t0 = lib.guard_trips()
    assert lib.decompose(rn, reads, mn, ms, ed_thr=250) == exp
    assert lib.guard_trips() > t0                          # kept sets beyond eight waves: repeated on the generic family


def _late_base_monomers():
    """Monomers whose lanes meet a base late or never: long homopolymer / two-letter prefixes, a base that is
    missing altogether, an N in the middle of a lane -- the cases that decide FastPlan::floor_slots."""
    st = synth.Stream(77, 3)
    rnd = lambda n, alpha=b"ACGT": bytes(alpha[int(x)] for x in st.below(n, len(alpha)))
    ms = [b"A" * 19 + rnd(150), rnd(30, b"AT") + rnd(140), rnd(171, b"ACT"), rnd(20) + b"N" + rnd(150),
          rnd(165), b"ACGT" + rnd(166), rnd(60) + b"C" * 25 + rnd(90), rnd(175), rnd(168), rnd(172),
          rnd(33, b"GC") + rnd(140), rnd(170)]   # 12 monomers -> 24 templates of 5 lanes: P = 35
    return ["m%d" % i for i in range(len(ms))], ms


@pytest.mark.parametrize("name", ["synthetic12", "synthetic12_i16", "dxz1_i16_ed", "dxz1", "late_bases", "late_bases_ed",
                                  "synthetic16", "synthetic20_ed",
                                  "wide64", "wide64_ed", "waves140",
                                  # the same narrow sets with the cell formats of rounds 1-5 (FLAG_NO_U16: fp16 / int16)
                                  "synthetic12+legacy", "synthetic12_i16+legacy", "dxz1_i16_ed+legacy", "dxz1+legacy",
                                  "late_bases_ed+legacy", "synthetic16+legacy", "synthetic20_ed+legacy"])
def test_fill_without_dominated_start_maxima(oracle, name):
    """csrc/sd_fast_fl.hip: behind the first FL slots of a lane the fill leaves out the maximum with the start
    term (the candidate is dominated there).  Same rows as the full kernel (SD_FILL_FULLFLOOR=1) and as the
    oracle, for template sets with small, typical and large floor_slots, with and without --ed_thr."""
    ed = -1
    sc = (-1, -1, -1, 1)
    legacy = name.endswith("+legacy")
    name = name.split("+")[0]
    fl = lib.FLAG_NO_U16 if legacy else 0
    if name.startswith("synthetic12"):
        mn, ms = synth.make_monomers(12, seed=1)
        if name.endswith("_i16"):
            sc = (-2, -2, -3, 40)                      # beyond the fp16 range: packed int16 cells (sd_fast_fl_i16.hip)
    elif name.startswith("dxz1"):
        mn, ms, _ = lib.fasta_load(os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa"))
        if name.endswith("_i16_ed"):
            sc, ed = (0, 0, -1, 30), 45          # (0,0,-1,15) takes fp16 cells with 64 rows between rebases since round 4
    elif name == "synthetic16":
        mn, ms = synth.make_monomers(16, seed=4)       # 32 templates of 4 lanes: P = 44 (sd_fast_fl_long.hip)
    elif name == "synthetic20_ed":
        mn, ms = synth.make_monomers(20, seed=6)       # 40 templates of 3 lanes: P = 60
        ed = 50
    elif name.startswith("wide64"):
        mn, ms = synth.make_monomers(64, seed=7)       # 128 templates: one per virtual lane, bf8 table
        ed = 60 if name.endswith("_ed") else -1
    elif name == "waves140":
        mn, ms = synth.make_monomers(140, seed=8)      # 280 templates: three waves per chunk
    else:
        mn, ms = _late_base_monomers()
        ed = 40 if name.endswith("_ed") else -1
    rn, rs = synth.make_reads(ms, 3, read_len=9000 if len(ms) <= 12 else 2500, seed=11)
    st = synth.Stream(5, 9)
    rs = list(rs) + [(ms[0].replace(b"N", b"A") * 30)[:3000], synth._ACGT[st.below(2500, 4)].tobytes(),
                     b"G" * 400 + ms[-1].replace(b"N", b"C") * 4 + b"N" * 3 + ms[1].replace(b"N", b"C") * 3]
    rn = ["r%d" % i for i in range(len(rs))]
    e = lib.Engine(ms, kernel=lib.KERNEL_FAST, ed_thr=ed, scoring=sc, flags=fl)
    info = e.info()
    e.close()
    if len(ms) <= 12:
        assert info["cells"] == (("int16" if "_i16" in name else "f16") if legacy else "u16") and 30 <= info["cells_per_lane"] <= 40
    elif len(ms) <= 20:
        assert info["cells"] == ("f16" if legacy else "u16") and 42 <= info["cells_per_lane"] <= 64
    else:
        assert info["cells"] in ("f16/bf8-table", "f16/bf8-codes x waves"), info
    lo, hi = {"synthetic12": (8, 16), "synthetic12_i16": (8, 16), "dxz1": (17, 24), "dxz1_i16_ed": (17, 24),
              "late_bases": (12, 40), "late_bases_ed": (12, 40),
              "synthetic16": (8, 24), "synthetic20_ed": (8, 32), "wide64": (8, 32), "wide64_ed": (8, 32), "waves140": (8, 48)}[name]
    assert lo <= info["floor_slots"] <= hi, info
    exp = oracle.decompose(rn, rs, mn, ms, threads=8, ed_thr=ed, sc=sc)
    got = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, ed_thr=ed, scoring=sc, flags=fl)
    os.environ["SD_FILL_FULLFLOOR"] = "1"
    try:
        full = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, ed_thr=ed, scoring=sc, flags=fl)
    finally:
        del os.environ["SD_FILL_FULLFLOOR"]
    assert full == exp
    assert got == exp
    if name.startswith("late_bases") or name == "dxz1":
        # the plan moves lane boundaries to where a lane meets all bases early; with uniform lanes the same sets
        # need the start term much deeper into the lanes (other FL variants, or the full kernel)
        os.environ["SD_PLAN_UNIFORM_LANES"] = "1"
        try:
            e = lib.Engine(ms, kernel=lib.KERNEL_FAST, ed_thr=ed, scoring=sc, flags=fl)
            uinfo = e.info()
            e.close()
            uni = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, ed_thr=ed, scoring=sc, flags=fl)
        finally:
            del os.environ["SD_PLAN_UNIFORM_LANES"]
        assert uinfo["floor_slots"] >= info["floor_slots"] and (name == "dxz1" or uinfo["floor_slots"] >= 25), (uinfo, info)
        assert uni == exp


@pytest.mark.parametrize("sc", [(-1, -1, -1, 1), (-2, -3, -4, 2), (-1, -1, -3, 1), (-1, -2, -5, 2), (1, -1, -1, 1)])
def test_floor_level_by_read_symbol_equals_one_level_and_oracle(oracle, sc):
    """Round 6: the narrow u16 fill takes the start-term floor in the first FL, FL - 4, FL - 8 or FL - 12 slots of a lane by the
    ROW's read symbol, applied in place in front of the slot loop (sd_fast_fill<..., FLS>) -- valid while every table value
    mm - del - ins is >= 0; scorings with a negative one ((-1,-1,-3,1): a mismatch costs more than a deletion plus an
    insertion) take the one-level kernels.  Same rows either way, and the oracle's: sets whose symbols need very different
    levels (a base that is missing from a monomer's first lanes, homopolymer prefixes), reads rich in one symbol, N."""
    mn, ms = _late_base_monomers()
    st = synth.Stream(91, 2)
    rn, rs = synth.make_reads([m.replace(b"N", b"A") for m in ms], 3, read_len=8000, seed=17)
    rs = list(rs) + [b"T" * 400 + ms[2] * 8 + b"G" * 300, synth._ACGT[st.below(3000, 2)].tobytes(),        # two-letter read
                     (ms[0] + b"N" + ms[5]) * 6, synth._ACGT[st.below(2500, 4)].tobytes()]
    rn = ["r%d" % i for i in range(len(rs))]
    info = lib.plan_info(ms, scoring=sc)
    assert (info["family"], info["cells"]) == ("fast", "u16"), info
    exp = oracle.decompose(rn, rs, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc)
    got = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc)
    assert got == exp, sc
    os.environ["SD_FILL_ONE_LEVEL"] = "1"
    try:
        one = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc)
    finally:
        del os.environ["SD_FILL_ONE_LEVEL"]
    assert one == exp, (sc, "one floor level")
    for ed, part in ((35, 5000), (-1, 333)):
        assert lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc, ed_thr=ed, part_size=part, overlap=77) == \
            oracle.decompose(rn, rs, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc, ed_thr=ed, part=part, overlap=77), (sc, ed, part)


def test_plan_choices_do_not_change_rows():
    """Lane boundaries moved by the plan, the slot count it picks among three, and the kernels that leave out
    dominated start-term maxima are pure optimisations: on random template sets (2-23 monomers of 100-200 bp, with
    N, homopolymer runs and late bases) the rows equal those of the plain layout with the full kernels."""
    st = synth.Stream(21, 8)
    for trial in range(14):
        n = 2 + int(st.below(1, 22)[0])
        ms = []
        for j in range(n):
            L = 100 + int(st.below(1, 101)[0])
            alpha = [b"ACGT", b"ACGT", b"AT", b"ACT"][int(st.below(1, 4)[0])]
            m = bytearray(bytes(alpha[int(x)] for x in st.below(L, len(alpha))))
            if int(st.below(1, 4)[0]) == 0:
                k = int(st.below(1, L - 30)[0])
                m[k:k + 20] = bytes([m[k]]) * 20
            if int(st.below(1, 6)[0]) == 0:
                m[int(st.below(1, L)[0])] = ord("N")
            ms.append(bytes(m))
        mn = ["m%d" % j for j in range(n)]
        rn, rs = synth.make_reads(ms, 2, read_len=4000, seed=100 + trial)
        ed = -1 if trial % 3 else 35
        got = lib.decompose(rn, rs, mn, ms, ed_thr=ed)
        os.environ["SD_FILL_FULLFLOOR"] = "1"
        os.environ["SD_PLAN_UNIFORM_LANES"] = "1"
        try:
            plain = lib.decompose(rn, rs, mn, ms, ed_thr=ed)
        finally:
            del os.environ["SD_FILL_FULLFLOOR"]
            del os.environ["SD_PLAN_UNIFORM_LANES"]
        assert got == plain, (trial, n, ed)


@pytest.mark.parametrize("thr,nm", [(0, 150), (25, 150), (48, 150), (60, 150), (200, 150), (30, 330), (52, 330), (75, 330)])
def test_ed_thr_compacts_large_template_sets(oracle, thr, nm):
    """--ed_thr with more than 128 templates (csrc/sd_fast_wn_ck.hip): a chunk is filled by ceil(kept / 128) waves
    holding exactly its kept templates, in their filtered order; chunks that need all W waves stay on the W-wave
    ranked kernel.  Thresholds from "only the nearest template" to "everything kept" (every class, and mixes of
    them; 330 monomers = 660 templates = six waves), against the oracle and against the same job with the
    compaction switched off."""
    mn, ms = synth.make_monomers(nm, seed=12)          # 150 monomers: 300 templates, three waves per chunk
    rn, rs = synth.make_reads(ms, 4, read_len=3200, seed=5)
    st = synth.Stream(8, 2)
    rs = list(rs) + [synth._ACGT[st.below(1500, 4)].tobytes(), (ms[3] * 9)[:1400] + b"N" * 2 + ms[77] * 3]
    rn = ["r%d" % i for i in range(len(rs))]
    kw = dict(part_size=700, overlap=100, ed_thr=thr)
    exp = oracle.decompose(rn, rs, mn, ms, threads=8, part=700, overlap=100, ed_thr=thr)
    got = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, **kw)
    full = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, flags=lib.FLAG_NO_EDTHR_COMPACT, **kw)
    assert full == exp
    assert got == exp


def test_multi_wave_wide_layout_long_reads_vs_generic_and_oracle(oracle):
    """More than 128 templates on the fast path (sd_fast_fill_wn: W waves per chunk, template codes in LDS,
    one workgroup barrier per row): 150 monomers = 300 templates = 3 waves, reads of 50 kb (checkpoints,
    rebases, several chunks) against the generic family, one read against the oracle, N in the reads."""
    mn, ms = synth.make_monomers(150, seed=31)
    rn, rs = synth.make_reads(ms, 6, read_len=50000, seed=32)
    rs[2] = rs[2][:20000] + b"N" * 7 + rs[2][20007:]
    e = lib.Engine(ms)
    assert e.info()["cells"] == "f16/bf8-codes x waves" and e.info()["n_templates"] == 300
    e.close()
    fast = lib.decompose(rn, rs, mn, ms)
    gen = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_GENERIC)
    assert fast == gen
    short = [rs[0][:6000], rs[2][19000:21000], rs[3][:1]]
    assert lib.decompose(rn[:3], short, mn, ms) == oracle.decompose(rn[:3], short, mn, ms, threads=min(32, os.cpu_count() or 1))


@pytest.mark.parametrize("thr", [0, 12, 40])
def test_ed_thr_on_the_generic_family_vs_oracle(oracle, thr):
    """--ed_thr with the generic kernels forced (kept set and tie order through the rank table)."""
    mn, ms = synth.make_monomers(12, seed=41)
    rn, rs = synth.make_reads(ms, 2, read_len=9000, seed=43)
    rs[1] = rs[1][:1500] + b"NNNN" + rs[1][1504:4000]
    for sc in [(-1, -1, -1, 1), (-1, -2, -1, 1)]:
        got = lib.decompose(rn, rs, mn, ms, scoring=sc, ed_thr=thr, kernel=lib.KERNEL_GENERIC)
        assert got == oracle.decompose(rn, rs, mn, ms, threads=min(32, os.cpu_count() or 1), sc=sc, ed_thr=thr)
        assert got == lib.decompose(rn, rs, mn, ms, scoring=sc, ed_thr=thr, kernel=lib.KERNEL_FAST)


def _final_cases():
    d = os.path.join(GOLDEN, "final")
    return sorted(os.listdir(d)) if os.path.isdir(d) else []


@pytest.mark.parametrize("name", _final_cases())
def test_cli_vs_unmodified_reference_cli(name, tmp_path):
    """The whole command line (native sd_run_files: DP, identities on the device, three TSVs) against the
    outputs of the UNMODIFIED reference command line committed under tests/golden/final/: raw and _alt by
    sha256, final byte for byte."""
    import json
    d = os.path.join(GOLDEN, "final", name)
    with open(os.path.join(d, "params.json")) as f:
        c = json.load(f)
    out = str(tmp_path / "o")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer")] +
                       [os.path.join(GOLDEN, x) for x in c["inputs"]] + ["-o", out, "-t", "8"] + c["args"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    rd = lambda fn: open(os.path.join(out, fn), "rb").read()  # noqa: E731
    assert hashlib.sha256(rd("final_decomposition_raw.tsv")).hexdigest() == c["raw_sha256"]
    with open(os.path.join(d, "final.tsv"), "rb") as f:
        assert rd("final_decomposition.tsv") == f.read()
    assert hashlib.sha256(rd("final_decomposition_alt.tsv")).hexdigest() == c["alt_sha256"]


def test_bench_line_contract():
    """bench.py --full prints ONE JSON line with the fields the driver parses (metric / value / unit / n_gpus / steps /
    warmup / ms_per_step / scaling / dtype / data / config.workload / roofline / cpu_baseline); small workload."""
    import json
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--reads", "120",
                        "--cpu-sample-reads", "2", "--sustain-seconds", "1.5"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["unit"] == "bp/s" and j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["scaling"] == "weak"
    assert j["higher_is_better"] is True and j["vs_baseline"] is None and j["data"] == "synthetic" and j["dtype"] == "u16"
    assert j["value"] > 1e8 and abs(j["value"] - 120 * 50000 / (j["ms_per_step"] / 1e3)) / j["value"] < 1e-6
    assert "workload" in j["config"] and "model" not in j["config"]
    r = j["roofline"]
    # the fill is VALU bound (measured issue ceiling); the notional HBM figure north_star asks for rides along
    assert r["bound"] == "valu" and r["unit"] == "G wave-inst/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0 < r["frac"] < 1 and 0 < r["isolated_frac"] < 1 and 0 < r["stream_span_frac"] < 1
    assert r["frac"] == r["step_frac"] and "profile_problems" not in j   # work over time; the committed counters match this build
    h = r["hbm_notional"]
    assert h["unit"] == "GB/s" and h["peak"] == 8000.0 and abs(h["frac"] - h["achieved"] / h["peak"]) < 1e-9
    assert h["isolated_frac"] > 0 and h["path_frac"] > 0
    c = j["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["parity_on_sample"] is True and c["cores"] >= 1 and c["value"] > 0
    assert j["other_pipe_mode"]["pipe_mode"] == 0 and j["device_resident"]["bp_per_s"] > 0
    su = j["sustained"]   # the headline's steps for seconds instead of K steps: same rows, a rate of the same order
    assert su["same_rows_as_headline"] is True and su["steps"] >= 3 and 1.0 < su["seconds"] < 60 and 0.3 < su["vs_timed_region"] < 3
    # three batches in flight, one engine each (the timed loop keeps two later steps outstanding)
    assert j["hbm_workspace_bytes"] == 3 * j["hbm_workspace_per_engine_bytes"] and "3 batches in flight" in j["timed_region"]
    assert j["full"] is True and j["config"]["rows_per_gpu"] > 0 and j["f16_guard_trips"] == 0 and "invalid" not in j


def test_bench_plain_run_is_the_headline_only():
    """bench.py without --full: the same headline fields, from the timed steps alone -- none of the figures that take runs
    of their own (CPU baseline, other stream mode, sustained leg, device-resident repeat, other cell formats, roofline)."""
    # (12 steps: the timed region of 3 is ~16 ms, and os.times() counts the CPU time asserted below in 10-ms ticks)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "12", "--warmup", "1", "--reads", "120"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["unit"] == "bp/s" and j["n_gpus"] == 1 and j["steps"] == 12 and j["warmup"] == 1 and j["scaling"] == "weak"
    assert j["higher_is_better"] is True and j["data"] == "synthetic" and j["dtype"] == "u16" and j["full"] is False
    assert j["value"] > 1e8 and abs(j["value"] - 120 * 50000 / (j["ms_per_step"] / 1e3)) / j["value"] < 1e-6
    assert "workload" in j["config"] and "3 batches in flight" in j["timed_region"] and j["f16_guard_trips"] == 0
    assert j["kernel_ms_per_step"]["fill"] > 0 and j["host_ms_per_step"]["process_cpu_ms"] > 0 and j["rows_out_per_gpu"] > 0
    for k in ("roofline", "cpu_baseline", "other_pipe_mode", "sustained", "device_resident"):
        assert j[k] is None, k
    assert "invalid" not in j and "dumped_outputs" not in j


def test_bench_dump_outputs_are_the_rows_of_the_timed_path(tmp_path):
    """bench.py --dump-outputs DIR: the rows the last timed step returned (rows.npy: template, start, end, score;
    read_row_offsets.npy) equal what the same stream path hands a caller for the same seeded reads, and a second run
    with the same arguments writes the same bytes."""
    args = ["--steps", "2", "--warmup", "1", "--reads", "120", "--no-cpu-baseline", "--timed-only"]
    files = []
    for k in range(2):
        d = str(tmp_path / ("dump%d" % k))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", d],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
        assert len(lines) == 1
        j = json.loads(lines[0])
        assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["dumped_outputs"]["sampled"] is False
        files.append({f: open(os.path.join(d, f), "rb").read() for f in ("rows.npy", "read_row_offsets.npy")})
    assert files[0] == files[1]
    rows, off = np.load(str(tmp_path / "dump0" / "rows.npy")), np.load(str(tmp_path / "dump0" / "read_row_offsets.npy"))
    assert rows.dtype == np.float64 and off.dtype == np.float64
    assert rows.shape == (j["rows_out_per_gpu"], 4) and off.shape == (121,) and off[0] == 0 and off[-1] == len(rows)
    mn, ms = synth.make_monomers(12, seed=1)
    rn, rs = synth.make_reads(ms, 120, read_len=50000, seed=1)
    st = lib.Stream(ms, threads=8)
    st.submit(rs)
    per_read = st.collect(as_lists=True)
    st.close()
    assert np.diff(off).astype(np.int64).tolist() == [len(x) for x in per_read]
    assert rows.astype(np.int64).tolist() == [list(r) for x in per_read for r in x]


@pytest.mark.gpu
@pytest.mark.parametrize("nm", [12, "12+legacy", 64, 140, "tiled"])
def test_f16_range_guard_trips_and_the_batch_is_repeated_with_integer_cells(oracle, nm):
    """VERDICT r02 (weak 6): the fp16 fills check at run time that their cells stay in the exact-integer range
    (F16Guard, csrc/sd_fast_dev.hpp).  With the real limit nothing trips; with a limit any input exceeds
    (sd_params.reserved[2], the test hook) the guard raises its flag, the engine repeats the batch with integer
    cells -- for more than 128 templates on the generic family -- and the rows still equal the oracle's."""
    fl = 0
    if nm == "12+legacy":   # the narrow layout's fp16 cells (F16Guard); 12: its biased-u16 cells (U16Guard), the default since round 6
        nm, fl = 12, lib.FLAG_NO_U16
    if nm == "tiled":   # thirty 342-bp monomers: the tiled multi-wave layout (fp16 only: the repeat runs on the generic family)
        mn, ms = synth.make_monomers(60, seed=3)
        mn, ms = mn[:30], [ms[2 * j] + ms[2 * j + 1] for j in range(30)]
        assert lib.plan_info(ms)["cells"] == "f16/bf8-codes tiled x waves"
        nm = 30
    else:
        mn, ms = synth.make_monomers(nm, seed=3)
    rn, rs = synth.make_reads(ms, 5, read_len=3000 if nm > 64 else 6000, seed=5)
    want = oracle.decompose(rn, rs, mn, ms, threads=8)
    t0 = lib.guard_trips()
    assert lib.decompose(rn, rs, mn, ms, flags=fl) == want
    assert lib.guard_trips() == t0
    assert lib.decompose(rn, rs, mn, ms, f16_guard=40, flags=fl) == want
    assert lib.guard_trips() > t0
    t1 = lib.guard_trips()
    # the streaming form: two batches, the first trips, the engine stays on integer cells
    st = lib.Stream(ms, sub_batches=2, f16_guard=40, flags=fl)
    st.submit(rs)
    rows = st.collect(as_lists=True)
    st.close()
    tn = mn + [m + "'" for m in mn]
    assert b"".join(lib.format_rows(n, tn, r) for n, r in zip(rn, rows)) == want
    assert lib.guard_trips() > t1


@pytest.mark.gpu
def test_traceback_word_range_guard_trips_and_the_batch_is_repeated_with_the_one_block_form(oracle):
    """The packed two-block traceback checks at run time that every checkpoint cell and start term it turns into a
    16-bit word lies inside the range the plan proved (sd_fast_trace2.hip).  With integer cells in the fill (no fp16
    guard there) and a limit any input exceeds (sd_params.reserved[2], the test hook) only the traceback's check can
    trip: the engine repeats the batch with sd_fast_trace and the rows still equal the oracle's."""
    mn, ms = synth.make_monomers(12, seed=4)
    rn, rs = synth.make_reads(ms, 4, read_len=7000, seed=6)
    want = oracle.decompose(rn, rs, mn, ms, threads=8)
    e = lib.Engine(ms, flags=lib.FLAG_NO_F16, f16_guard=30)
    assert e.info()["cells"] == "int16" and e.info()["trace"] == "two-block packed16"
    e.close()
    t0 = lib.guard_trips()
    assert lib.decompose(rn, rs, mn, ms, flags=lib.FLAG_NO_F16) == want
    assert lib.guard_trips() == t0
    assert lib.decompose(rn, rs, mn, ms, flags=lib.FLAG_NO_F16, f16_guard=30) == want
    assert lib.guard_trips() > t0


@pytest.mark.gpu
@pytest.mark.parametrize("second_best", [False, True])
def test_in_stream_identities_equal_the_text_based_path_across_batches(tmp_path, second_best):
    """The identities of the final TSV come in-stream with the records of every device batch (csrc/sd_ident.hip) and
    follow them through the seam merge; here the job is cut into many small batches, so that reads span batches (the
    carry path of RowJob) and chunk seams drop records, and the three files must equal those of the text-based path of
    round 2 (SD_FLAG_NO_STREAM_IDENT) byte for byte -- which the reference-CLI goldens pin."""
    mn, ms = synth.make_monomers(6, seed=21)
    rn, rs = synth.make_reads(ms, 14, read_len=9000, seed=22)
    rs[3] = rs[3][:700] + b"N" * 40 + rs[3][740:2500]            # N inside blocks, a short read
    rs[7] = rs[7][:200]                                            # shorter than a chunk
    rfa, mfa = str(tmp_path / "r.fa"), str(tmp_path / "m.fa")
    synth.write_fasta(rfa, rn, rs, width=70)
    synth.write_fasta(mfa, mn, ms)
    outs = {}
    for tag, flags in (("stream", 0), ("text", lib.FLAG_NO_STREAM_IDENT)):
        o = [str(tmp_path / ("%s_%s.tsv" % (tag, x))) for x in ("raw", "final", "alt")]
        lib.run_files(rfa, mfa, o[0], o[1], o[2], second_best=second_best, threads=4, part_size=1000, overlap=200,
                      max_batch_rows=7000, flags=flags)
        st = lib.last_run_stats()
        assert st["batches"] >= 10
        if tag == "stream":
            assert st["ident_pairs"] > 0 and st["text_identity_ms"] < 1e-3
        else:
            assert st["ident_pairs"] == 0 and st["text_identity_ms"] > 0
        outs[tag] = [open(x, "rb").read() for x in o]
    assert outs["stream"] == outs["text"]
    assert outs["stream"][1].count(b"\n") > 500


_FRESH_ORDER = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from stringdecomposer_amd import lib, synth
mn, ms = synth.make_monomers(6, seed=21)
tm = [m.decode() for m in ms]
seq = (ms[0] + ms[1]) * 20
st = np.arange(0, 3000, 150)
lib.identity_segments(seq, st, st + 160, tm, False, threads=4, device=0)     # a SMALL device identity call first ...
rn, rs = synth.make_reads(ms, 14, read_len=9000, seed=22)
synth.write_fasta(sys.argv[1] + "/r.fa", rn, rs, width=70)
synth.write_fasta(sys.argv[1] + "/m.fa", mn, ms)
o = [sys.argv[1] + "/" + x for x in ("raw", "final", "alt")]
# ... then a job of many device batches whose post-processing thread grows the identity buffers while batches are in flight
for flags in (0, lib.FLAG_NO_STREAM_IDENT):      # (the in-stream form first, as the suite's own test does: more queues in the process)
    lib.run_files(sys.argv[1] + "/r.fa", sys.argv[1] + "/m.fa", o[0], o[1], o[2], second_best=False, threads=4, part_size=1000,
                  overlap=200, max_batch_rows=7000, flags=flags)
print("done", lib.last_run_stats()["batches"])
"""


@pytest.mark.gpu
def test_no_device_wide_free_while_batches_are_in_flight(tmp_path):
    """Round 6: hipFree / hipHostFree wait for every queue of the process; issued from a worker thread while the batch
    pipeline had kernels in flight (a buffer of the text-based identities that had to grow after a smaller call) that wait
    never returned -- the job hung.  Latent since round 1 and invisible in the suite's own order; the two-call sequence
    that showed it, in a process of its own with a deadline."""
    p = subprocess.run([sys.executable, "-c", _FRESH_ORDER % ROOT, str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=180)
    assert p.returncode == 0 and b"done" in p.stdout, p.stdout.decode()[-2000:]


@pytest.mark.gpu
def test_second_best_job_is_cut_into_device_batches_with_the_same_files(tmp_path, monkeypatch):
    """A --second-best job that fits one device batch: ONE fill / traceback launch, the identities in slices of whole
    reads that the host fetches and formats while the next slice is on the device (run_files_impl; round 3 cut the job
    into four device batches instead, SD_IDENT_SLICES_OFF).  The three files depend neither on the number of slices nor
    on the number of device batches."""
    mn, ms = synth.make_monomers(12, seed=3)
    rn, rs = synth.make_reads(ms, 230, read_len=50000, seed=4)
    rs[5] = rs[5][:20000] + b"N" * 30 + rs[5][20030:]
    rs[7] = rs[7][:300]
    rfa, mfa = str(tmp_path / "r.fa"), str(tmp_path / "m.fa")
    synth.write_fasta(rfa, rn, rs, width=80)
    synth.write_fasta(mfa, mn, ms)
    outs = {}
    cases = (("default", {}, 1), ("one_slice", {"SD_IDENT_SLICES": "1"}, 1), ("three", {"SD_IDENT_SLICES": "3"}, 1),
             ("many", {"SD_IDENT_SLICES": "40"}, 1), ("batches", {"SD_IDENT_SLICES_OFF": "1"}, 4),
             ("seven_batches_sliced", {"SD_MIN_BATCHES": "7"}, 7), ("seven_batches", {"SD_MIN_BATCHES": "7", "SD_IDENT_SLICES_OFF": "1"}, 7))
    for tag, env, batches in cases:
        for k in ("SD_MIN_BATCHES", "SD_IDENT_SLICES", "SD_IDENT_SLICES_OFF"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        o = [str(tmp_path / ("%s_%s.tsv" % (tag, x))) for x in ("raw", "final", "alt")]
        lib.run_files(rfa, mfa, o[0], o[1], o[2], second_best=True, threads=8)
        st = lib.last_run_stats()
        assert st["batches"] == batches and st["text_identity_ms"] < 0.01   # every identity came from the device
        outs[tag] = [hashlib.sha256(open(x, "rb").read()).hexdigest() for x in o]
    assert len({tuple(v) for v in outs.values()}) == 1
    # ... and they are the text-based path's files
    o = [str(tmp_path / ("text_%s.tsv" % x)) for x in ("raw", "final", "alt")]
    lib.run_files(rfa, mfa, o[0], o[1], o[2], second_best=True, threads=8, flags=lib.FLAG_NO_STREAM_IDENT)
    assert [hashlib.sha256(open(x, "rb").read()).hexdigest() for x in o] == outs["default"]


@pytest.mark.gpu
@pytest.mark.parametrize("mlen", [20, 3])
def test_in_stream_identities_fall_back_when_a_batch_has_too_many_records(tmp_path, mlen):
    """A batch with more records than the identity outputs have room for (one per 48 rows: 20-bp monomers give one per
    ~20) is post-processed from the read text instead; same files.  With 3-bp monomers the records do not even fit the
    compaction's first buffer (one per 16 rows): the identity kernel must not touch the incomplete compact records
    (tools/fuzz_final.py found a GPU memory fault there)."""
    st0 = synth.Stream(5, 77)
    ms = [synth._to_ascii(st0.below(mlen + k, 4)) for k in range(4)]
    mn = ["s%d" % k for k in range(4)]
    rn, rs = synth.make_reads(ms, 3, read_len=120000, seed=9)
    rfa, mfa = str(tmp_path / "r.fa"), str(tmp_path / "m.fa")
    synth.write_fasta(rfa, rn, rs, width=0)
    synth.write_fasta(mfa, mn, ms)
    outs = []
    for flags in (0, lib.FLAG_NO_STREAM_IDENT):
        o = [str(tmp_path / ("%d_%s.tsv" % (flags, x))) for x in ("raw", "final", "alt")]
        lib.run_files(rfa, mfa, o[0], o[1], o[2], second_best=False, threads=4, flags=flags)
        if flags == 0:
            assert lib.last_run_stats()["text_identity_ms"] > 0     # the in-stream words were not used
        outs.append([open(x, "rb").read() for x in o])
    assert outs[0] == outs[1] and outs[0][1].count(b"\n") > 5000
    for sb in (True,):    # and every template per record
        o = [str(tmp_path / ("sb_%s.tsv" % x)) for x in ("raw", "final", "alt")]
        lib.run_files(rfa, mfa, o[0], o[1], o[2], second_best=sb, threads=4)
        assert open(o[0], "rb").read() == outs[0][0]


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", [(520, 900), (1100, 2000)])
def test_ed_thr_with_monomers_longer_than_512_bp(oracle, lo, hi):
    """main.cpp:128-149 runs edlib's prefilter for any monomer length; round 2 returned SD_ERR_UNSUPPORTED beyond 512 bp.
    The prefilter kernel now takes templates of up to 2048 bp (16 / 32 words per template); such sets run on the
    generic family."""
    st = synth.Stream(99, lo)
    nmono = 3 if hi <= 1000 else 2      # the narrow layout holds 128 virtual lanes x 64 slots = 8192 template cells
    ms = _random_monomers(st, nmono, lo, hi)
    mn = ["L%d" % j for j in range(nmono)]
    reads = []
    for r in range(2):
        parts = []
        while sum(len(x) for x in parts) < 4000 + 2500 * r:
            j = int(st.below(1, nmono)[0])
            codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(ms[j], dtype=np.uint8))
            x = synth._to_ascii(synth.mutate(codes, st, 0.06, 0.03, 0.03))
            parts.append(synth.revcomp_bytes(x) if st.below(1, 2)[0] else x)
        reads.append(b"".join(parts))
    rn = ["r0", "r1"]
    # round 3: such sets run on the FAST family too (up to 32 virtual lanes per template, traceback with 16 / 32 cells
    # per lane); the generic family stays the independent second implementation
    e = lib.Engine(ms)
    assert e.info()["family"] == "fast"
    e.close()
    for ed in (-1, 0, 150, 900):
        exp = oracle.decompose(rn, reads, mn, ms, threads=8, part=3000, overlap=400, ed_thr=ed)
        got = lib.decompose(rn, reads, mn, ms, part_size=3000, overlap=400, ed_thr=ed)
        assert got == exp, (lo, hi, ed)
        gen = lib.decompose(rn, reads, mn, ms, part_size=3000, overlap=400, ed_thr=ed, kernel=lib.KERNEL_GENERIC)
        assert gen == exp, (lo, hi, ed, "generic")
    exp = oracle.decompose(rn, reads, mn, ms, threads=8, sc=(-2, -3, -4, 2))
    assert lib.decompose(rn, reads, mn, ms, scoring=(-2, -3, -4, 2)) == exp


TR_SHAPES = [
    # (monomers, Lmin, Lmax, scoring, part, overlap, N in reads) -- the packed two-block traceback (sd_fast_trace2.hip)
    (12, 165, 178, (-1, -1, -1, 1), 5000, 500, False),    # C2's shape: three levels (QQ = 3, 2, 1)
    (12, 165, 178, (-2, -3, -4, 2), 1500, 200, True),     # BASELINE config 5's scoring
    (5, 20, 61, (-1, -1, -1, 1), 333, 77, True),          # one level, blocks shorter than a checkpoint interval apart
    (4, 62, 63, (-1, -2, -1, 1), 700, 100, False),        # the 62-cell level boundary
    (6, 187, 248, (-1, -1, -2, 2), 2000, 300, True),      # four registers per lane
    (3, 2, 9, (0, -1, -1, 1), 97, 13, True),              # tiny templates: an instance is a fraction of a block
    (8, 120, 130, (-3, -1, -2, 3), 640, 64, False),       # a chunk that ends exactly on a checkpoint row
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TR_SHAPES, ids=["%dx%d-%d_%s" % (s[0], s[1], s[2], "_".join(map(str, s[3]))) for s in TR_SHAPES])
def test_packed_two_block_traceback_vs_one_block_form_and_oracle(oracle, shape):
    """sd_fast_trace_pk (two 32-row blocks per wave, packed 16-bit tagged cells, main.cpp:217-269) against the oracle and
    against sd_fast_trace (SD_FLAG_TRACE_V1) on the same fills: every level of cells per lane, both block pairings
    (chunks shorter than 64 rows never pair), row-0 blocks, N, scorings whose words sit elsewhere in the 16-bit range."""
    nm, lo, hi, sc, part, ov, with_n = shape
    st = synth.Stream(1000 + nm * 7 + hi, 3)
    ms = []
    for j in range(nm):
        L = lo + int(st.below(1, hi - lo + 1)[0])
        ms.append(synth._ACGT[st.below(L, 4)].tobytes())
    mn = ["m%d" % j for j in range(nm)]
    rn, rs = synth.make_reads(ms, 6, read_len=max(4 * part, 900), seed=hi)
    rs = list(rs)
    # short reads around the pairing limits: 1, 31, 32, 33, 63, 64, 65, 96, 97 rows
    for L in (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 129):
        rs.append((b"".join(ms) * 3)[7:7 + L])
    if with_n:
        b = bytearray(rs[0]); b[50:53] = b"NNN"; b[700] = ord("N"); rs[0] = bytes(b)
        rs.append(b"N" * 70 + ms[0] * 2)
    rn = ["r%d" % i for i in range(len(rs))]
    kw = dict(part_size=part, overlap=ov, scoring=sc)
    e = lib.Engine(ms, kernel=lib.KERNEL_FAST, scoring=sc, part_size=part, overlap=ov)
    assert e.info()["trace"] == "two-block packed16"
    e.close()
    exp = oracle.decompose(rn, rs, mn, ms, threads=8, sc=sc, part=part, overlap=ov)
    got = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, **kw)
    v1 = lib.decompose(rn, rs, mn, ms, kernel=lib.KERNEL_FAST, flags=lib.FLAG_TRACE_V1, **kw)
    assert v1 == exp
    assert got == exp


ONE_BP_SETS = [
    [b"A", b"ACGTACGTTGCA"],                                  # the smallest: one 1-bp monomer beside a short one
    [b"G", b"C", b"ACGTTGCAAGGCTTAACCGG" * 4],                # two 1-bp monomers (each other's reverse complements twice over)
    [b"T", b"AC", b"ACGTACGTAGCTAGCTAGGATCCTAG" * 6, b"N"],   # with a 2-bp and an N monomer
    None,                                                     # 12 synthetic ~171-bp monomers + "A" in the middle of the order
    70,                                                       # 70 of them + "A": beyond one wave -> the tiled multi-wave layout
]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(ONE_BP_SETS)))
@pytest.mark.parametrize("sc", [(-1, -1, -1, 1), (-2, -3, -4, 2), (-1, -2, -1, 3), (0, -1, -1, 1)])
def test_one_bp_templates_on_the_fast_family_vs_oracle(oracle, k, sc):
    """VERDICT r03 (missing 1): a 1-bp template used to send the whole job to the generic family.  Its one cell is a
    k = 0 cell (start term only, no insertion move, main.cpp:188-193): the narrow fills now end such a lane at slot 0
    (the pads behind it would keep a value the cell has fallen below), and the packed traceback needs no cells for it.
    Every scoring of round 3's failed attempt (-2,-3,-4,2 differed on seven of nine sets), ties between the 1-bp
    template and its neighbours in the template order, reads made of long homopolymer runs, --ed_thr."""
    if ONE_BP_SETS[k] is None:
        mn, ms = synth.make_monomers(12, seed=9)
        ms = list(ms[:5]) + [b"A"] + list(ms[5:])
    elif ONE_BP_SETS[k] == 70:
        mn, ms = synth.make_monomers(70, seed=9)
        ms = list(ms[:33]) + [b"A"] + list(ms[33:])
        if lib.plan_info(ms, scoring=sc)["family"] != "fast":
            pytest.skip("scoring beyond the fp16 range of the tiled layout")
        assert lib.plan_info(ms, scoring=sc)["cells"] == "f16/bf8-codes tiled x waves"
    else:
        ms = list(ONE_BP_SETS[k])
    mn = ["m%d" % j for j in range(len(ms))]
    info = lib.plan_info(ms, scoring=sc)
    assert info["family"] == "fast", info
    st = synth.Stream(31 + k, 7)
    big = [m for m in ms if len(m) > 8]
    reads = [synth._to_ascii(st.below(900, 4)),
             b"A" * 300 + b"C" * 150 + b"ACGT" * 50 + b"T" * 90,
             (big[0] * 40)[:1200] if big else b"ACGT" * 100,
             b"".join((ms[int(j)] if len(ms[int(j)]) > 1 else ms[int(j)] * int(1 + st.below(1, 9)[0])) for j in st.below(60, len(ms)))[:1500],
             b"G", b"AC", b"N" * 40 + b"ACGTTGCA" * 30]
    reads = [r if r else b"A" for r in reads]
    rn = ["r%d" % i for i in range(len(reads))]
    for part, ov, ed in ((5000, 500, -1), (333, 77, -1), (700, 100, 12)):
        exp = oracle.decompose(rn, reads, mn, ms, threads=8, sc=sc, part=part, overlap=ov, ed_thr=ed)
        got = lib.decompose(rn, reads, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc, part_size=part, overlap=ov, ed_thr=ed)
        assert got == exp, (k, sc, part, ed)
        v1 = lib.decompose(rn, reads, mn, ms, kernel=lib.KERNEL_FAST, scoring=sc, part_size=part, overlap=ov, ed_thr=ed,
                           flags=lib.FLAG_TRACE_V1)
        assert v1 == exp, (k, sc, part, ed, "one-block traceback")


@pytest.mark.gpu
@pytest.mark.parametrize("nm,lo,hi,sc,cells", [
    (150, 150, 180, (-2, -2, -3, 40), "int16/int8-codes x waves"),          # 44 is not exact in bf8, G = 42 leaves fp16
    (100, 165, 178, (-3, -5, -4, 7), "int16/int8-codes x waves"),           # range bound 2 040 < . <= 12 000
    (40, 230, 700, (-2, -3, -4, 9), "int16/int8-codes tiled x waves"),      # tiled, 2+ waves
    (5, 950, 1000, (-1, -2, -1, 3), "int16/int8-codes tiled x waves"),      # tiled, one wave, a dozen lanes per template
    (200, 100, 224, (-1, -1, -1, 1), "forced")])                            # default scoring, SD_FLAG_NO_F16
def test_multi_wave_layouts_with_integer_cells_vs_oracle(oracle, nm, lo, hi, sc, cells):
    """Template sets beyond one wave whose scoring leaves the exact-integer range of fp16 (or is not exact in bf8): the
    multi-wave fills with int16 cells and int8 table bytes (sd_fast_wn_i16.hip) instead of the generic family -- with and
    without --ed_thr (ranked form: no compaction for integer cells), N in reads and templates, small chunks."""
    st = synth.Stream(977 + nm, nm)
    ms = _random_monomers(st, nm, lo, hi)
    ms[1] = ms[1][:7] + b"N" + ms[1][8:]
    mn = ["m%d" % j for j in range(nm)]
    reads = []
    for r in range(3):
        parts = []
        while sum(len(x) for x in parts) < 1500 + 900 * r:
            j = int(st.below(1, nm)[0])
            codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(ms[j].replace(b"N", b"A"), dtype=np.uint8))
            x = synth._to_ascii(synth.mutate(codes, st, 0.05, 0.03, 0.03))
            parts.append(synth.revcomp_bytes(x) if st.below(1, 2)[0] else x)
        b = bytearray(b"".join(parts))
        b[len(b) // 3] = ord("N")
        reads.append(bytes(b))
    rn = ["r%d" % i for i in range(len(reads))]
    flags = lib.FLAG_NO_F16 if cells == "forced" else 0
    e = lib.Engine(ms, scoring=sc, flags=flags)
    info = e.info()
    e.close()
    assert info["family"] == "fast" and info["cells"] == ("int16/int8-codes x waves" if cells == "forced" else cells), info
    for part, ov, ed in [(5000, 500, -1), (600, 90, -1), (5000, 500, 45), (700, 100, 0)]:
        scc = (-1, -1, -1, 1) if ed > -1 else sc   # (the reference's 10-argument form ignores the scores)
        if ed > -1 and cells != "forced":
            continue
        exp = oracle.decompose(rn, reads, mn, ms, threads=min(32, os.cpu_count() or 1), sc=scc, part=part, overlap=ov, ed_thr=ed)
        got = lib.decompose(rn, reads, mn, ms, scoring=scc, part_size=part, overlap=ov, ed_thr=ed, flags=flags)
        assert got == exp, (nm, sc, part, ed)


@pytest.mark.gpu
def test_fp16_guard_trip_on_a_multi_wave_set_repeats_on_the_fast_family(oracle):
    """A tripped fp16 range guard on more than 128 templates: the batch is repeated with the int16 multi-wave kernels
    (until round 5: on the generic family)."""
    mn, ms = synth.make_monomers(140, seed=3)
    rn, rs = synth.make_reads(ms, 4, read_len=3000, seed=5)
    want = oracle.decompose(rn, rs, mn, ms, threads=8)
    t0 = lib.guard_trips()
    e = lib.Engine(ms, f16_guard=40)
    e.load_reads(rs)
    e.run()
    rows = e.rows()
    info = e.info()
    e.close()
    assert lib.guard_trips() > t0
    assert info["family"] == "fast" and info["cells"] == "int16/int8-codes x waves", info
    tn = mn + [m + "'" for m in mn]
    assert b"".join(lib.format_rows(n, tn, r) for n, r in zip(rn, rows)) == want
