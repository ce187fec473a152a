"""Motif hits with insertions and deletions (--motif-edits) without a GPU: the host form (sd_motif_edit_host) against the
naive tables of tests/motif_edit_ref.py at the edges of the pattern, the words and a lane's stretch, every code, every
budget; the named cases; the figures of the test read; the refusals and their texts; the join with per-hit lengths; the
command line's request and files; the symbols and constants of the header."""
import argparse
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import motif_edit_ref as ref
from conftest import GOLDEN
from motif_ref import COMP, IUPAC
from stringdecomposer_amd import formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
CENPB = lib.MOTIF_BUILTIN["cenpb"]
CODES = "ACGTRYSWKMBDHVN"
BUDGETS = [0, 1, 3, 7]


def text_of(rng, n):
    """random ACGT with N and lower case among it"""
    return "".join(rng.choice("ACGT") if rng.random() >= 0.08 else rng.choice("Nacgtn") for _ in range(n))


def pattern_of(rng, L, K, codes="ACGTRYSWN"):
    """mixed IUPAC with inner Ns and more than K constrained positions"""
    while True:
        p = "".join(rng.choice(codes) for _ in range(L))
        if sum(c != "N" for c in p) > K and (L < 6 or "N" in p[1:-1]):
            return p


def edited(rng, pattern, kind):
    """an instance of the pattern with one deletion (0), one insertion (1) or no edit (2)"""
    inst = "".join(rng.choice(IUPAC[c]) for c in pattern)
    x = rng.randrange(1, max(2, len(inst) - 1))
    return [inst[:x] + inst[x + 1:], inst[:x] + rng.choice("ACGT") + inst[x:], inst][kind]


def host_equals_reference(reads, motifs, K, text=None, off=None, threads=1):
    lens = [len(s) for s in reads]
    got = lib.motif_edits(reads, motifs, K, threads=threads) if text is None else lib.motif_edits_text(text, off, lens, motifs, K, threads=threads)
    want, per = ref.scan(reads, [p for _, p in motifs], K)
    assert ref.as_tuples(got.hits) == want
    assert got.per.tolist() == per and got.per.dtype == np.int64 and got.per.sum() == len(got.hits)
    key = [(h[0], h[1], h[2], h[3] + h[4]) for h in want]
    assert key == sorted(key)   # the canonical order: read, motif, strand, end
    assert all(len(motifs[h[1]][1]) - h[5] <= h[4] <= len(motifs[h[1]][1]) + h[5] and h[5] <= K for h in want)
    return got


@pytest.mark.parametrize("L", [6, 17, 32, 33, 64])
def test_read_lengths_around_the_pattern_the_words_and_a_stretch(L):
    rng = random.Random(L)
    S = lib.motif_edits_info()["stretch"]
    for K in BUDGETS:
        if L <= K:
            continue
        p = pattern_of(rng, L, K)
        ns = (0, 1, max(L - K - 1, 0), L - K, L, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1, 3 * S - 1)
        reads = [text_of(rng, n) for n in ns]
        for r, s in enumerate(reads):   # an instance where the read can hold one: at the last base, or at the first
            if len(s) >= L + 1:
                inst = edited(rng, p, r % 3 if K else 2)
                at = len(s) - len(inst) if r % 2 else 0
                reads[r] = s[:at] + inst + s[at + len(inst):]
        got = host_equals_reference(reads, [("p", p), ("q", pattern_of(rng, L, K))], K, threads=2)
        assert len(got.hits) >= 4
        ends = {(int(h["read"]), int(h["start"]) + int(h["length"])) for h in got.hits}
        assert any(e == len(reads[r]) for r, e in ends) and any(h["start"] == 0 for h in got.hits)   # the last base; the first


def test_reads_in_one_buffer_with_gaps_and_offsets_not_ascending():
    rng = random.Random(3)
    reads = [text_of(rng, n) for n in (200, 0, 65, 130, 17)]
    order = [3, 0, 4, 2, 1]
    off, parts, at = [0] * len(reads), [], 0
    for r in order:
        gap = "TTCGAAAA" * rng.randrange(0, 3)   # bases that would match if they were read
        parts += [gap, reads[r]]
        off[r] = at + len(gap)
        at += len(gap) + len(reads[r])
    text = "".join(parts) + "TTCGAAAA"
    assert off != sorted(off)
    motifs = [("w", "WSNW"), ("pal", "GAATTC"), ("r", "RYRA"), ("c", "TTCGNNNNA")]
    got = host_equals_reference(reads, motifs, 1, text, off, threads=3)
    assert len(got.hits) > 20


def test_every_code_against_every_byte():
    text = "ACGTNacgtnRYKM-*U"
    for c in CODES[:-1]:
        for b in text:   # A c A against A b A: an exact hit exactly when the code matches the byte
            got = host_equals_reference(["GG" + "A" + b + "A" + "GG"], [("p", "A" + c + "A")], 1)
            assert ((0, 0, 0, 2, 3, 0) in ref.as_tuples(got.hits)) == (b in IUPAC[c]), (c, b)
    host_equals_reference([text * 3], [("c%d" % i, "T" + c + "C") for i, c in enumerate(CODES)], 1)
    host_equals_reference([text * 3], [("n", "ANNT"), ("m", "NACN")], 1)   # N matches every byte, and is not free to delete


def test_the_named_cases():
    hits = lambda reads, motifs, K: [(h[3], h[4], h[5]) for h in ref.as_tuples(lib.motif_edits(reads, motifs, K).hits) if h[2] == 0]
    assert hits(["AAAAAAAA"], [("a", "AAAA")], 0) == [(i, 4, 0) for i in range(5)]   # overlapping exact hits
    for K in (0, 1, 2):   # no satellites around an exact copy
        assert hits(["TTAGGG" * 6], [("tel", "TTAGGG")], K) == [(6 * i, 6, 0) for i in range(6)]
    assert hits(["C" + "A" * 12 + "C"], [("a", "AAAC")], 1) == [(1, 3, 1), (10, 4, 0)]   # the head of the plateau, then the exact one
    for reads, motifs, K in ((["AAAAAAAA"], [("a", "AAAA")], 0), (["TTAGGG" * 6], [("tel", "TTAGGG")], 2), (["C" + "A" * 12 + "C"], [("a", "AAAC")], 1)):
        host_equals_reference(reads, motifs, K)


@pytest.mark.parametrize("K", [0, 1, 2])
def test_no_edits_equals_the_hamming_scan_without_mismatches(K):
    rng = random.Random(K)
    reads = [text_of(rng, n) for n in (500, 64, 0, 129)] + ["ACGTTTCGAAAAACGCGGGA" * 8]
    motifs = ["cenpb", "tel=TTAGGG", ("w", "WSSW"), ("pal", "GAATTC"), ("a", "AAAA")]
    ham = lib.motif(reads, motifs, 0)
    got = lib.motif_edits(reads, motifs, K)
    exact = got.hits[got.edits == 0]   # at every K the exact occurrences are all there
    key = [(int(h["read"]), int(h["motif"]), int(h["strand_edits"]) >> 7, int(h["start"])) for h in exact]
    assert key == [(int(h["read"]), int(h["motif"]), int(h["strand"]), int(h["start"])) for h in ham.hits] and len(key) > 30
    assert (exact["length"] == np.array(ham.lengths)[exact["motif"]]).all()
    if K == 0:
        assert len(got.hits) == len(exact) and (got.per == ham.per).all()


def test_a_palindrome_is_counted_once():
    got = host_equals_reference(["GGAATTCCGAATCGG"], [("pal", "GAATTC"), ("not", "GAATTA")], 1)
    assert got.per[0, 0].tolist() == [2, 0] and got.per[0, 1, 1] > 0


def test_strand_minus_is_the_scan_of_the_reverse_complement():
    rng = random.Random(5)
    rc = lambda s: "".join(COMP[b] for b in reversed(s))
    s = "".join(rng.choice("ACGT") for _ in range(400))
    for at, kind in ((30, 0), (120, 1), (300, 2)):
        inst = edited(rng, CENPB, kind)
        s = s[:at] + inst + s[at + len(inst):]
    fw = lib.motif_edits([s], ["cenpb"], 2)
    bw = lib.motif_edits([rc(s)], ["cenpb"], 2)
    plus = sorted((int(h["start"]), int(h["length"]), int(h["strand_edits"]) & 127) for h in fw.hits[fw.strand == 0])
    assert len(plus) >= 3 and fw.per[0, 0, 0] == bw.per[0, 0, 1]
    # a - hit of the reverse complement is the same alignment read backwards: the same edits; its end mirrors a start
    minus = bw.hits[bw.strand == 1]
    assert sorted((bw.edits[bw.strand == 1]).tolist()) == sorted(e for _, _, e in plus)
    want, _ = ref.scan([rc(s)], [CENPB], 2)
    assert ref.as_tuples(bw.hits) == want and len(minus) == len(plus)


@pytest.mark.parametrize("motifs, K, text", [
    ([("a", "ACGTACGTAC")], 8, "edits = 8, must be an integer 0 .. 7"),
    ([("a", "ACGTACGTAC")], -1, "edits = -1, must be an integer 0 .. 7"),
    ([("a", "ACGTACGTAC")], True, "must be an integer 0 .. 7"),
    ([("a", "ACNNGT"), ("box", "NTTNNNN")], 2, "motif 'box': 2 constrained positions with 2 edits allowed"),
    ([("a", "ACGT"), ("b", "AC"), ("a", "GG")], 0, "motif name 'a' is given twice"),
    ([("m%d" % i, "ACGT") for i in range(1025)], 0, "1025 motifs, must be 1 .. 1024"),
    ([("x", "ACGU")], 0, "code 'U' at position 3"),
    ([("x", "A" * 65)], 0, "65 codes, must be 1 .. 64"),
])
def test_refusals(motifs, K, text):
    with pytest.raises(lib.SdError) as e:
        lib.motif_edits(["ACGT" * 10], motifs, K)
    assert text in e.value.msg and e.value.code == lib.SD_ERR_PARAM


def _host(lens, pats, K, text=b"N"):
    lens, off = np.array(lens, dtype=np.int64), np.zeros(len(lens), dtype=np.int64)
    out, n, per, err = C.c_void_p(0), C.c_int64(0), np.zeros(2 * len(pats) * len(lens), dtype=np.int64), C.create_string_buffer(512)
    rc = lib.load().sd_motif_edit_host(text, off.ctypes.data, lens.ctypes.data, len(lens), lib._strs(pats), len(pats), K, 1, C.byref(out), C.byref(n),
                                       per.ctypes.data, err, 512)
    return rc, err.value.decode()


def test_the_library_refuses_with_its_numbers():
    """the C-ABI's own checks: the budget, the constrained positions, and the item cap from the lengths alone"""
    assert _host([4], ["ACGTAC"], 8) == (lib.SD_ERR_PARAM, "sd_motif_edit_host: edits = 8, must be 0 .. 7")
    rc, msg = _host([4], ["ACGTAC", "NTTNN"], 2)
    assert rc == lib.SD_ERR_PARAM and "motif 'motif 1': 2 constrained positions with 2 edits allowed: it would hit everywhere" in msg
    tile = 64 * lib.MOTIF_EDIT_TILE_WORDS
    pats = ["".join(random.Random(i).choice("ACGT") for _ in range(8)) + "A" for i in range(1024)]
    rc, msg = _host([tile * 8200], pats, 0)
    assert rc == lib.SD_ERR_PARAM and "8200 read tiles x 2048 pattern-strands" in msg and str(lib.MOTIF_ITEMS_MAX) in msg


# ---- the test read ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def read():
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    return [n.split()[0] for n in rn], rs


@pytest.fixture(scope="module")
def box(read):
    """cenpb on the test read at K = 0, 1, 2 from the host form"""
    return {K: lib.motif_edits(read[1], ["cenpb"], K, threads=4) for K in (0, 1, 2)}


def test_the_figures_of_the_test_read(read, box):
    assert len(read[1]) == 1 and len(read[1][0]) == 94871
    assert box[0].per.tolist() == [[[69, 0]]] and box[1].per.tolist() == [[[161, 2]]] and box[2].per.tolist() == [[[384, 82]]]
    classes = lambda m: np.bincount(m.edits, minlength=3).tolist()
    assert classes(box[0]) == [69, 0, 0] and classes(box[1]) == [69, 94, 0] and classes(box[2]) == [69, 94, 303]
    lengths = lambda h: dict(zip(*(x.tolist() for x in np.unique(h["length"], return_counts=True))))
    assert lengths(box[1].hits) == {16: 18, 17: 127, 18: 18}
    assert lengths(box[2].hits) == {15: 83, 16: 172, 17: 173, 18: 37, 19: 1}
    one = box[1].hits[box[1].edits == 1]
    assert int((one["length"] != 17).sum()) == 36   # the boxes the Hamming scan cannot see
    want, per = ref.scan(read[1], [CENPB], 2)   # hit for hit against the naive tables
    assert ref.as_tuples(box[2].hits) == want and box[2].per.tolist() == per
    ham = lib.motif(read[1], ["cenpb"], 0)
    assert box[0].hits["start"].tolist() == ham.hits["start"].tolist()


def test_the_join_with_per_hit_lengths(read, box):
    names = read[0]
    final = formats.read_final(os.path.join(TD, "final_decomposition_fc89af8.tsv"))
    counts = formats.motif_edit_row_counts(box[1].hits, final, 1, names)
    naive = [sum(1 for h in box[1].hits if r.start <= h["start"] and h["start"] + h["length"] - 1 <= r.end) for r in final]
    assert counts.shape == (len(final), 1) and counts[:, 0].tolist() == naive and 150 <= counts.sum() <= len(box[1].hits)
    # the meaning of motif_row_counts stays: a length per motif
    ham = lib.motif(read[1], ["cenpb"], 1)
    as_edit = np.array([(h["start"], h["read"], h["motif"], 17, h["strand"] << 7 | h["mismatches"]) for h in ham.hits], dtype=lib.motif_edit_hit_dtype())
    assert (formats.motif_edit_row_counts(as_edit, final, 1, names) == formats.motif_row_counts(ham.hits, final, [17], names)).all()
    # L = 17: a hit of 18 bases that crosses a row's end by one base belongs to no row; of 17 and 16 bases it lies inside
    e = final[1].end
    hits = np.array([(e - 16, 0, 0, 18, 1), (e - 16, 0, 0, 17, 0), (e - 16, 0, 0, 16, 1), (final[1].start, 0, 0, 18, 129), (final[0].end - 3, 0, 0, 16, 1)],
                    dtype=lib.motif_edit_hit_dtype())
    assert formats.motif_edit_row_counts(hits, final[:3], 1, names).tolist() == [[0], [3], [0]]
    assert formats.motif_edit_row_counts(hits[:0], final[:3], 2, names).tolist() == [[0, 0]] * 3


def test_rows_and_files_round_trip(read, tmp_path):
    names, rs = read
    m = lib.motif_edits(rs, ["cenpb", "tel=TTAGGG"], 1, threads=4)
    rows = formats.motif_edit_rows(m, names, rs)
    key = [(r.start, r.end, m.names.index(r.motif), r.strand) for r in rows]
    assert len(rows) == len(m.hits) and key == sorted(key)
    assert {r.end - r.start + 1 for r in rows if r.motif == "cenpb"} == {16, 17, 18} and {r.mismatches for r in rows} == {0, 1}
    for r in rows[:300]:
        seg = rs[0][r.start:r.end + 1].decode()
        assert r.sequence == (seg if r.strand == "+" else "".join(COMP[b] for b in reversed(seg)))
    path = str(tmp_path / "m.tsv")
    formats.write_motif(path, rows)
    assert formats.read_motif(path) == rows and formats.format_motif(formats.read_motif(path)) == open(path).read()


# ---- the command line (host) --------------------------------------------------------------------------------------------
def test_the_command_line_request(tmp_path):
    from stringdecomposer_amd import motif as cli
    ns = lambda **kw: argparse.Namespace(**dict(dict(motif=["cenpb"], motif_file=None, motif_mismatches=0), **kw))
    assert cli.request(ns()) == (["cenpb"], [CENPB], 0) and cli.edits(ns()) is None and cli.wanted(ns())   # a namespace without the option
    assert cli.request(ns(motif_edits=2)) == (["cenpb"], [CENPB], 0) and cli.edits(ns(motif_edits=2)) == 2
    assert cli.request(ns(motif_edits=0, motif=["cenpb", "x=ACGT"])) == (["cenpb", "x"], [CENPB, "ACGT"], 0)
    for bad, text in ((ns(motif_edits=1, motif_mismatches=1), "--motif-edits cannot be combined with --motif-mismatches 1"),
                      (ns(motif_edits=8), "--motif-edits: K = 8, must be 0 .. 7"),
                      (ns(motif_edits=-1), "--motif-edits: K = -1, must be 0 .. 7"),
                      (ns(motif_edits=4, motif=["x=ACGT"]), "motif 'x': 4 constrained positions with 4 edits allowed"),
                      (ns(motif_edits=1, motif=["nosuch"]), "neither NAME=PATTERN nor one of the built-in motifs")):
        got = cli.request(bad)
        assert isinstance(got, str) and text in got and "\n" not in got, got
    parser = argparse.ArgumentParser()
    cli.add_arguments(parser)
    assert parser.parse_args([]).motif_edits is None and parser.parse_args(["--motif-edits", "2"]).motif_edits == 2


def test_the_command_line_refuses_before_any_work(tmp_path):
    out = str(tmp_path / "refused")
    for prog, extra in (("sd-motif", []), ("stringdecomposer", [os.path.join(TD, "DXZ1_star_monomers.fa")])):
        for opts, text in ((["--motif-edits", "1", "--motif-mismatches", "1"], "cannot be combined"), (["--motif-edits", "8"], "must be 0 .. 7")):
            p = subprocess.run([os.sys.executable, os.path.join(ROOT, "bin", prog), os.path.join(TD, "read.fa")] + extra +
                               ["-o", out, "--motif", "cenpb"] + opts, capture_output=True, text=True, timeout=120)
            assert p.returncode == 2 and len(p.stderr.strip().split("\n")) == 1 and text in p.stderr and not os.path.exists(out), p.stderr


def test_the_command_line_scan_and_files(read, tmp_path):
    """cli.scan in batches equals one call; cli.write on host threads writes the three files, which read back"""
    from stringdecomposer_amd import motif as cli
    reads = ["ACGTTTCGAAAAACGCGGGA" * 30, "", "TTAGGG" * 50, "TTTCGAAAAACCGGGA" * 5]
    motifs = ["cenpb", "tel=TTAGGG", ("w", "WSSWA")]
    whole = lib.motif_edits(reads, motifs, 1)
    got = cli.scan(reads, motifs, 0, None, 2, K=1)
    assert isinstance(got, formats.MotifEdits) and got.hits.tobytes() == whole.hits.tobytes() and (got.per == whole.per).all() and len(got.hits) > 50
    args = argparse.Namespace(motif=["cenpb"], motif_file=None, motif_mismatches=0, motif_edits=1, sequences=os.path.join(TD, "read.fa"),
                              monomers=os.path.join(TD, "DXZ1_star_monomers.fa"), lenient=False, threads=4)
    saved = cli.write(args, os.path.join(TD, "final_decomposition_fc89af8.tsv"), str(tmp_path), "o", None)
    assert [os.path.basename(f) for f in saved] == ["o_motif.tsv", "o_motif_rows.tsv", "o_motif_monomers.tsv"]
    rows = formats.read_motif(saved[0])
    m = lib.motif_edits(read[1], ["cenpb"], 1)
    assert formats.format_motif(rows) == open(saved[0]).read() == formats.format_motif(formats.motif_edit_rows(m, read[0], read[1]))
    assert sorted({r.end - r.start + 1 for r in rows}) == [16, 17, 18] and len(rows) == 163
    final = formats.read_final(os.path.join(TD, "final_decomposition_fc89af8.tsv"))
    counts = formats.motif_edit_row_counts(m.hits, final, 1, read[0])
    assert formats.format_motif_rows(formats.read_motif_rows(saved[1])) == open(saved[1]).read() == formats.format_motif_rows(formats.motif_row_lines(counts, final, m.names))
    mono = formats.read_motif_monomers(saved[2])
    assert sum(r.hits for r in mono) == counts.sum() and formats.format_motif_monomers(mono) == open(saved[2]).read()


# ---- the interface -------------------------------------------------------------------------------------------------------
SYMBOLS = ("sd_motif_edit_host", "sd_motif_edit_dev", "sd_motif_edit_reads_size_dev", "sd_motif_edit_reads_write_dev", "sd_motif_edit_info",
           "sd_motif_edit_kernel_bench")


def test_symbols_exported_and_declared():
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    L = lib.load()
    for s in SYMBOLS:
        assert hasattr(L, s) and re.search(r"\b(int|void) %s\(" % s, h) and s in doc, s
    assert "sd_motif_edit_hit;" in h and "SD_MOTIF_KMAX" in doc
    for name in ("motif_edits", "motif_edits_text", "motif_edits_device", "motif_edits_info", "motif_edits_kernel_bench", "motif_edit_hit_dtype"):
        assert callable(getattr(lib, name)), name


def test_constants_of_the_header():
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        h = f.read()
    val = lambda name: eval(re.search(r"#define %s (.+)" % name, h).group(1))
    info = lib.motif_edits_info()
    assert val("SD_MOTIF_KMAX") == lib.MOTIF_KMAX == 7
    assert val("SD_MOTIF_EDIT_TILE_WORDS") == lib.MOTIF_EDIT_TILE_WORDS == info["tile"] == 256 * info["stretch"] // 64
    assert info["stretch"] % 64 == 0 and info["pattern_block"] >= 1 and info["launch_wg"] >= 1
    assert info["launch_work"] == info["launch_wg"] * 64 * info["tile"] * info["pattern_block"]
    assert lib.MOTIF_EDIT_TILE_WORDS >= lib.MOTIF_TILE_WORDS   # the command line sizes its batches by the smaller tile
    d = lib.motif_edit_hit_dtype()
    assert d.itemsize == 16 and [d.fields[n][1] for n in ("start", "read", "motif", "length", "strand_edits")] == [0, 8, 12, 14, 15]
    assert lib.motif_hit_dtype().names == ("start", "read", "motif", "strand", "mismatches")   # the Hamming record does not change
