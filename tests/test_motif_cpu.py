"""IUPAC motif hits (--motif) without a GPU: the host form (sd_motif_host) against the naive scan of tests/motif_ref.py at
the edges of words, every code, every budget; the named cases; the refusals and their texts; the figures of the test read;
the joins with the final TSV; the files' readers and writers; the constants of the header."""
import os
import random
import re

import numpy as np
import pytest

import motif_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
CENPB = lib.MOTIF_BUILTIN["cenpb"]
CODES = "ACGTRYSWKMBDHVN"
LENGTHS = [1, 2, 17, 32, 33, 63, 64]


def text_of(rng, n):
    """random ACGT with N and lower case among it"""
    return "".join(rng.choice("ACGT") if rng.random() >= 0.08 else rng.choice("Nacgtn") for _ in range(n))


def pattern_of(rng, L, E, codes=CODES):
    while True:
        p = "".join(rng.choice(codes) for _ in range(L))
        if sum(c != "N" for c in p) > E:
            return p


def host_equals_reference(reads, motifs, E, text=None, off=None, threads=1):
    lens = [len(s) for s in reads]
    got = lib.motif(reads, motifs, E, threads=threads) if text is None else lib.motif_text(text, off, lens, motifs, E, threads=threads)
    want, per = ref.scan(reads, [p for _, p in motifs], E)
    assert ref.as_tuples(got.hits) == want
    assert got.per.tolist() == per and got.per.dtype == np.int64 and got.per.sum() == len(got.hits)
    key = [(h[0], h[1], h[2], h[3]) for h in want]
    assert key == sorted(key)   # the canonical order: read, motif, strand, start
    return got


@pytest.mark.parametrize("L", LENGTHS)
def test_read_lengths_around_the_pattern_and_the_words(L):
    rng = random.Random(L)
    for E in range(8):
        if L <= E:
            continue
        p = pattern_of(rng, L, E, "ACGTRYSWN" if L > 2 else "ACGTRY")
        reads = [text_of(rng, n) for n in (0, 1, max(L - 1, 0), L, L + 1, 63, 64, 65, 127, 128, 129)]
        for r, s in enumerate(reads):   # an instance where the read can hold one, half of them ending at the last base
            if len(s) >= L:
                at = len(s) - L if r % 2 else rng.randrange(len(s) - L + 1)
                inst = "".join(rng.choice(ref.IUPAC[c]) for c in p)
                reads[r] = s[:at] + inst + s[at + L:]
        got = host_equals_reference(reads, [("p", p), ("q", pattern_of(rng, L, E))], E)
        assert len(got.hits) >= 5


def test_reads_in_one_buffer_with_gaps_and_offsets_not_ascending():
    rng = random.Random(3)
    reads = [text_of(rng, n) for n in (200, 0, 65, 130, 17)]
    order = [3, 0, 4, 2, 1]
    off, parts, at = [0] * len(reads), [], 0
    for r in order:
        gap = "ACGT" * rng.randrange(0, 4)
        parts += [gap, reads[r]]
        off[r] = at + len(gap)
        at += len(gap) + len(reads[r])
    text = "".join(parts) + "TTCGAAAA"
    assert off != sorted(off)
    motifs = [("w", "WSN"), ("pal", "GAATTC"), ("r", "RYR"), ("c", "TTCGNNNNA")]
    host_equals_reference(reads, motifs, 1, text, off, threads=3)


def test_every_code_against_every_byte():
    text = "ACGTNacgtnRYKM-*U"
    for c in CODES[:-1]:
        got = host_equals_reference([text], [("x", c)], 0)
        plus = [int(h["start"]) for h in got.hits if h["strand"] == 0]
        assert plus == [i for i, b in enumerate(text) if b in ref.IUPAC[c]]   # upper-case ACGT of the set, nothing else
    got = host_equals_reference([text], [("n", "NNNA")], 0)   # N matches every byte
    assert [int(h["start"]) for h in got.hits if h["strand"] == 0] == [i for i in range(len(text) - 3) if text[i + 3] == "A"]
    lower = lib.motif([text], [("x", "acgtn")], 0)   # lower case in the pattern is folded
    assert ref.as_tuples(lower.hits) == ref.as_tuples(lib.motif([text], [("x", "ACGTN")], 0).hits) == [(0, 0, 0, 0, 0)]


@pytest.mark.parametrize("E", range(8))
def test_every_budget(E):
    rng = random.Random(20 + E)
    reads = [text_of(rng, 300), text_of(rng, 129)]
    motifs = [("a", pattern_of(rng, 9, E, "ACGT")), ("b", pattern_of(rng, 17, E)), ("c", pattern_of(rng, 64, E)), ("d", "N" * 10 + "ACGTACGTAC" + "N" * 5)]
    got = host_equals_reference(reads, motifs, E, threads=2)
    assert got.hits["mismatches"].max(initial=0) <= E
    if E >= 3:
        assert len(set(got.hits["mismatches"].tolist())) >= 2


def test_the_counter_saturates():
    assert len(lib.motif(["A" * 300], [("c", "C" * 64)], 7).hits) == 0   # 64 mismatches are not 0
    for E in range(8):
        assert len(lib.motif(["A" * 300], [("c", "C" * 64)], E).hits) == 0
        for k in (8, 9, 16, 17, 32, 33):   # k mismatches in a row, at either end of the pattern
            for s in ("A" * k + "C" * (64 - k), "C" * (64 - k) + "A" * k):
                assert len(lib.motif([s], [("c", "C" * 64)], E).hits) == 0
    got = lib.motif(["C" * 300], [("c", "C" * 64)], 7)
    assert len(got.hits) == 237 and got.per.tolist() == [[[237, 0]]] and got.hits["start"].tolist() == list(range(237))


def test_a_palindrome_is_counted_once():
    s = "TTGAATTCAAGAATTCGAATTC"
    got = host_equals_reference([s], [("eco", "GAATTC"), ("half", "GAATT")], 0)
    assert got.per.tolist() == [[[3, 0], [3, 3]]]
    names, patterns, strands = lib.motif_compile([("eco", "GAATTC"), ("half", "GAATT"), ("w", "WSNSW")], 0)
    assert [(x.motif, x.strand, x.length, x.constrained, x.palindrome) for x in strands] == [
        (0, 0, 6, 6, 1), (1, 0, 5, 5, 0), (1, 1, 5, 5, 0), (2, 0, 5, 4, 1)]


def test_the_last_base():
    for L in LENGTHS:
        inst = "".join(random.Random(L).choice("ACGT") for _ in range(L))
        p = inst if L > 2 else inst[0] * L
        body = ("G" if p[0] != "G" else "T") * 100
        got = lib.motif([body + p], [("p", p)], 0)
        assert (len(body), 0) in [(int(h["start"]), int(h["strand"])) for h in got.hits]      # a hit ending at the last base
        cut = lib.motif([body + p[:-1]], [("p", p)], 0) if L > 1 else lib.motif([body], [("p", p)], 0)
        assert len(body) not in cut.hits["start"][cut.hits["strand"] == 0].tolist()            # one further: none


def test_strand_minus_is_the_scan_of_the_reverse_complement():
    rng = random.Random(9)
    reads = [text_of(rng, 500)]
    rc = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}
    for p in ("TTCGNNNNA", "RYKMB", CENPB, "ACGNNT"):
        reads[0] += "".join(rng.choice(ref.IUPAC[c]) for c in p)   # an instance, so that every pattern has a hit
        q = "".join(rc[c] for c in reversed(p))
        a, b = lib.motif(reads, [("p", p)], 2), lib.motif(reads, [("q", q)], 2)
        minus = lambda m: sorted((int(h["start"]), int(h["mismatches"])) for h in m.hits if h["strand"] == 1)
        plus = lambda m: sorted((int(h["start"]), int(h["mismatches"])) for h in m.hits if h["strand"] == 0)
        assert minus(a) == plus(b) and plus(a) == minus(b) and len(plus(a)) + len(minus(a)) > 0


@pytest.mark.parametrize("motifs, E, text", [
    ([("a", "ACUG")], 0, "code 'U' at position 2 is not one of ACGTRYSWKMBDHVN"),
    ([("a", "AC-G")], 0, "code '-' at position 2"),
    ([("a", "A" * 65)], 0, "motif 'a': 65 codes, must be 1 .. 64"),
    ([("a", "")], 0, "motif 'a': 0 codes, must be 1 .. 64"),
    ([("a", "ACGT")], 8, "mismatches = 8, must be 0 .. 7"),
    ([("a", "ACGT")], -1, "mismatches = -1, must be 0 .. 7"),
    ([("a", "ACNNGT"), ("box", "NTTNNNN")], 2, "motif 'box': 2 constrained positions with 2 mismatches allowed"),
    ([("a", "ACGT"), ("b", "AC"), ("a", "GG")], 0, "motif name 'a' is given twice"),
    ([("a b", "ACGT")], 0, "a name must match [A-Za-z0-9_.-]+"),
    ([("m%d" % i, "ACGT") for i in range(1025)], 0, "1025 motifs, must be 1 .. 1024"),
    ([], 0, "0 motifs, must be 1 .. 1024"),
])
def test_refusals(motifs, E, text):
    for call in (lambda: lib.motif_compile(motifs, E), lambda: lib.motif(["ACGT" * 10], motifs, E)):
        with pytest.raises(lib.SdError) as e:
            call()
        assert text in e.value.msg and e.value.code == lib.SD_ERR_PARAM
    with pytest.raises(lib.SdError) as e:
        lib.motif_request(["nosuchmotif"])
    assert "cenpb" in e.value.msg
    assert lib.motif_request(["cenpb", "tel=TTAGGG", ("x", "AC")]) == (["cenpb", "tel", "x"], [CENPB, "TTAGGG", "AC"])


def test_the_item_cap_is_refused_with_its_numbers():
    """2^24 items: checked on the lengths alone, before any text is read"""
    import ctypes as C
    tile = 64 * lib.MOTIF_TILE_WORDS
    lens = np.array([tile * 8200], dtype=np.int64)   # 8 200 tiles x 2 048 pattern-strands
    off = np.zeros(1, dtype=np.int64)
    pats = [pattern_of(random.Random(i), 8, 0, "ACGT") + "A" for i in range(1024)]
    out, n, per, err = C.c_void_p(0), C.c_int64(0), np.zeros(2048, dtype=np.int64), C.create_string_buffer(512)
    rc = lib.load().sd_motif_host(b"N", off.ctypes.data, lens.ctypes.data, 1, lib._strs(pats), 1024, 0, 1, C.byref(out), C.byref(n), per.ctypes.data, err, 512)
    assert rc == lib.SD_ERR_PARAM and b"8200 read tiles x 2048 pattern-strands" in err.value and str(lib.MOTIF_ITEMS_MAX).encode() in err.value


# ---- the test read ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def read():
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    return [n.split()[0] for n in rn], rs


@pytest.fixture(scope="module")
def box(read):
    """cenpb on the test read at E = 0, 1, 2 from the host form"""
    return {E: lib.motif(read[1], ["cenpb"], E, threads=4) for E in (0, 1, 2)}


def test_the_figures_of_the_test_read(read, box):
    assert len(read[1]) == 1 and len(read[1][0]) == 94871
    assert box[0].per.tolist() == [[[69, 0]]] and box[1].per.tolist() == [[[128, 2]]] and box[2].per.tolist() == [[[263, 16]]]
    classes = lambda m: np.bincount(m.hits["mismatches"], minlength=3).tolist()
    assert classes(box[0]) == [69, 0, 0] and classes(box[1]) == [69, 61, 0] and classes(box[2]) == [69, 61, 149]
    want, per = ref.scan(read[1], [CENPB], 1)   # hit for hit
    assert ref.as_tuples(box[1].hits) == want and box[1].per.tolist() == per
    at0 = {h[3] for h in want if h[4] == 0}
    assert ref.as_tuples(box[0].hits) == [h for h in want if h[3] in at0 and h[4] == 0]


WITH_BOX = {"A_0": (46, 15, 26), "C_2": (46, 0, 22), "D_3": (46, 13, 18), "E_4": (46, 17, 23), "H_7": (47, 0, 12), "J_9": (47, 24, 29)}


def test_the_rows_and_monomers_of_the_test_read(read, box):
    names = read[0]
    final = formats.read_final(os.path.join(TD, "final_decomposition_fc89af8.tsv"))
    mono = [n.split()[0] for n in lib.fasta_load(os.path.join(TD, "DXZ1_star_monomers.fa"))[0]]
    got = {}
    for E in (0, 1):
        counts = formats.motif_row_counts(box[E].hits, final, box[E].lengths, names)
        assert counts.shape == (len(final), 1) and counts.sum() == len(box[E].hits)   # every hit lies wholly inside one row
        naive = [sum(1 for h in box[E].hits if r.start <= h["start"] and h["start"] + 16 <= r.end) for r in final]
        assert counts[:, 0].tolist() == naive
        rows = formats.motif_monomers(counts, final, box[E].names, mono)
        assert [r.monomer for r in rows] == [m + "'" for m in mono]   # monomer-file order; the read holds the reverse complements only
        got[E] = {r.monomer[:3]: (r.rows, r.rows_hit) for r in rows}
        lines = formats.motif_row_lines(counts, final, box[E].names)
        assert len(lines) == len(final) and sum(bool(l.counts) for l in lines) == sum(v[1] for v in got[E].values())
    for key in got[0]:
        want = WITH_BOX.get(key)
        if want:
            assert got[0][key] == (want[0], want[1]) and got[1][key] == (want[0], want[2]), key
        else:
            assert got[0][key][1] == 0 and got[1][key][1] == 0, key
    assert sum(1 for k in got[0] if k not in WITH_BOX) == 6
    # a hit across a row boundary belongs to no row
    hits = np.array([(final[0].end - 10, 0, 0, 0, 0), (final[1].start, 0, 0, 0, 0), (final[1].end - 16, 0, 0, 1, 1), (final[1].end - 15, 0, 0, 0, 0)],
                    dtype=lib.motif_hit_dtype())
    assert formats.motif_row_counts(hits, final[:3], [17], names).tolist() == [[0], [2], [0]]


def test_files_round_trip(read, box, tmp_path):
    names, rs = read
    m = lib.motif(rs, ["cenpb", "tel=TTAGGG", ("w", "WSSW")], 1, threads=4)
    rows = formats.motif_rows(m, names, rs)
    assert len(rows) == len(m.hits) and [(r.start, m.names.index(r.motif), r.strand) for r in rows] == sorted((r.start, m.names.index(r.motif), r.strand) for r in rows)
    for r in rows[:200]:
        seg = rs[0][r.start:r.end + 1].decode()
        assert r.end - r.start + 1 == len(m.patterns[m.names.index(r.motif)])
        assert r.sequence == (seg if r.strand == "+" else "".join(ref.COMP[b] for b in reversed(seg)))
    assert formats.motif_sequence(b"ACnGT", 1) == "ACNGT" and formats.motif_sequence(b"ACnGT", 0) == "ACnGT" and formats.motif_sequence(b"AAC", "-") == "GTT"
    final = formats.read_final(os.path.join(TD, "final_decomposition_fc89af8.tsv"))
    counts = formats.motif_row_counts(m.hits, final, m.lengths, names)
    texts = (formats.format_motif(rows), formats.format_motif_rows(formats.motif_row_lines(counts, final, m.names)),
             formats.format_motif_monomers(formats.motif_monomers(counts, final, m.names)))
    io = ((formats.write_motif, formats.read_motif, formats.format_motif), (formats.write_motif_rows, formats.read_motif_rows, formats.format_motif_rows),
          (formats.write_motif_monomers, formats.read_motif_monomers, formats.format_motif_monomers))
    for i, (text, (write, read_, fmt)) in enumerate(zip(texts, io)):
        path = str(tmp_path / ("f%d.tsv" % i))
        with open(path, "w", newline="") as f:
            f.write(text)
        back = read_(path)
        assert fmt(back) == text and len(back) > 0
        write(path + ".again", back)
        assert open(path + ".again", "rb").read() == text.encode()   # byte for byte
    assert re.search(r"\tcenpb:\d+,(tel:\d+,)?w:\d+\n", texts[1])
    none = formats.format_motif_rows([formats.MotifRowsRow("r", 1, 2, "m'", ())])   # a row without a hit
    assert none == "r\t1\t2\tm'\t*\n"
    with open(str(tmp_path / "none.tsv"), "w") as f:
        f.write(none)
    assert formats.read_motif_rows(str(tmp_path / "none.tsv")) == [formats.MotifRowsRow("r", 1, 2, "m'", ())]
    bad = str(tmp_path / "bad.tsv")
    with open(bad, "w") as f:
        f.write("r\t1\t2\t?\tm\t0\tAC\n")
    with pytest.raises(formats.FormatError):
        formats.read_motif(bad)


def test_constants_of_the_header():
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        h = f.read()
    val = lambda name: eval(re.search(r"#define %s (.+)" % name, h).group(1))
    assert val("SD_MOTIF_LMAX") == lib.MOTIF_LMAX and val("SD_MOTIF_EMAX") == lib.MOTIF_EMAX and val("SD_MOTIF_MAX") == lib.MOTIF_MAX
    assert val("SD_MOTIF_ITEMS_MAX") == lib.MOTIF_ITEMS_MAX and val("SD_MOTIF_HITS_MAX") == lib.MOTIF_HITS_MAX
    info = lib.motif_info()
    assert val("SD_MOTIF_TILE_WORDS") == lib.MOTIF_TILE_WORDS == info["tile"] and info["pattern_block"] >= 1
    assert info["launch_work"] % (64 * info["tile"] * info["pattern_block"]) == 0
    assert lib.motif_hit_dtype().itemsize == 16


def test_the_command_line_batches():
    from stringdecomposer_amd import motif as cli
    tile = 64 * lib.MOTIF_TILE_WORDS
    assert cli.batches([10, 20, 30], 2) == [(0, 3)]
    assert cli.batches([cli.BATCH_BASES, 5, cli.BATCH_BASES + 1, 7], 2) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    lens = [tile * 1000] * 5
    assert cli.batches(lens, lib.MOTIF_ITEMS_MAX // 2000) == [(0, 2), (2, 4), (4, 5)]
    assert cli.motif_blocks(1024, 8200) == [(0, 1023), (1023, 1024)] and cli.motif_blocks(3, 10) == [(0, 3)]
    reads = ["ACGTTTCGAAAAACGCGGGA" * 30, "", "TTAGGG" * 50]
    whole = lib.motif(reads, ["cenpb", "tel=TTAGGG", ("w", "WSSW")], 1)
    got = cli.scan(reads, ["cenpb", "tel=TTAGGG", ("w", "WSSW")], 1, None, 2)
    assert got.hits.tobytes() == whole.hits.tobytes() and (got.per == whole.per).all() and len(got.hits) > 50


def test_the_command_line_request(tmp_path):
    """--motif, --motif-file and --motif-mismatches as the command line reads them: the request, or one line of refusal"""
    import argparse
    from stringdecomposer_amd import motif as cli
    fa = str(tmp_path / "motifs.fa")
    with open(fa, "w") as f:
        f.write(">tel telomeric repeat\nTTAGGG\n>long\nACGTNN\nRYAC\n")
    ns = lambda **kw: argparse.Namespace(**dict(dict(motif=None, motif_file=None, motif_mismatches=0), **kw))
    assert not cli.wanted(ns()) and cli.wanted(ns(motif=["cenpb"])) and cli.wanted(ns(motif_file=fa))
    assert cli.request(ns(motif=["cenpb", "x=ACG"], motif_file=fa, motif_mismatches=1)) == (
        ["cenpb", "x", "tel", "long"], [CENPB, "ACG", "TTAGGG", "ACGTNNRYAC"], 1)
    for bad, text in ((ns(motif=["cenpb"], motif_mismatches=9), "mismatches = 9, must be 0 .. 7"),
                      (ns(motif=["nosuch"]), "neither NAME=PATTERN nor one of the built-in motifs"),
                      (ns(motif=["a/b=ACGT"]), "must match [A-Za-z0-9_.-]+"),
                      (ns(motif=["tel=TTAGGG"], motif_file=fa), "motif name 'tel' is given twice"),
                      (ns(motif=["x=ACGU"]), "code 'U' at position 3"),
                      (ns(motif_file=str(tmp_path / "none.fa")), "--motif-file"),
                      (ns(motif=["cenpb"], motif_mismatches=9, motif_file=None), "--motif")):
        got = cli.request(bad)
        assert isinstance(got, str) and text in got and "\n" not in got, got


def test_the_command_line_splits_a_batch_over_the_hit_cap(monkeypatch):
    """a call the library refuses for its hits is cut in two -- reads first, then motifs -- and the parts joined in canonical
    order; the cap stands in as 40 hits here"""
    from stringdecomposer_amd import motif as cli
    real, calls = lib.motif, []

    def capped(reads, motifs, E=0, device=None, threads=1):
        m = real(reads, motifs, E, device=device, threads=threads)
        calls.append((len(reads), len(motifs), len(m.hits)))
        if len(m.hits) > 40:
            raise lib.SdError(lib.SD_ERR_PARAM, "sd_motif_host: %d hits, the cap is 40 (MOTIF_HITS_MAX): use fewer reads or fewer motifs per call" % len(m.hits))
        return m
    reads = ["ACGTTTCGAAAAACGCGGGA" * 6, "", "TTAGGG" * 18, "GAATTC" * 9 + "ACGCGGGA"]   # the third read alone is over the cap, each of its motifs is not
    motifs = ["cenpb", "tel=TTAGGG", ("w", "WSSW"), ("pal", "GAATTC")]
    whole = real(reads, motifs, 1)
    assert len(whole.hits) > 80
    monkeypatch.setattr(lib, "motif", capped)
    got = cli.scan(reads, motifs, 1, None, 1)
    assert got.hits.tobytes() == whole.hits.tobytes() and (got.per == whole.per).all()
    assert any(c[0] == 1 and c[1] < 4 for c in calls) and all(c[2] <= 40 for c in calls if c[:2] == (1, 1))
    with pytest.raises(lib.SdError) as e:   # one read with one motif over the cap stays refused
        cli.scan(["TTAGGG" * 200], ["tel=TTAGGG"], 1, None, 1)
    assert "MOTIF_HITS_MAX" in e.value.msg
    monkeypatch.setattr(lib, "motif", lambda *a, **k: (_ for _ in ()).throw(lib.SdError(lib.SD_ERR_HIP, "another failure")))
    with pytest.raises(lib.SdError) as e:
        cli.scan(reads, motifs, 1, None, 1)
    assert e.value.msg == "another failure"
