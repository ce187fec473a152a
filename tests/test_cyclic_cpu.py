"""Cyclic pairs and the merge of seed monomers (--autocorr-merge, bin/sd-merge) without a GPU: the host form
(sd_cyclic_pairs_host, sd_cyclic_merge_host) against the naive table and the plain walk of tests/cyclic_ref.py; planted
rotations; the merge rule's properties; canonical records; the refusals and their texts; the files; the symbols and
constants of the header."""
import argparse
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import cyclic_ref as ref
import edlib_ref
from conftest import GOLDEN
from stringdecomposer_amd import autocorr, cyclic, formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
SYMBOLS = ("sd_cyclic_pairs_host", "sd_cyclic_pairs_dev", "sd_cyclic_merge_host", "sd_cyclic_merge_dev", "sd_cyclic_canon", "sd_cyclic_info",
           "sd_cyclic_kernel_bench")
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no device could be used: none is needed


def as_tuple(p, a, b):
    return int(p.dist[a, b]), int(p.end[a, b]), int(p.strand[a, b]), int(p.phase[a, b])


def merge_tuples(m):
    return [tuple(int(x[i]) for x in (m.cluster, m.centre, m.dist, m.end, m.strand)) for i in range(len(m.cluster))]


def same_merge(a, b):
    return a.n_clusters == b.n_clusters and all(np.array_equal(x, y) for x, y in zip(a[:6], b[:6]))


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert getattr(L, name) is not None and name in lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
    info = lib.cyclic_info()
    assert info["lmax_query"] == lib.CYCLIC_QMAX == 2048 and re.search(r"#define SD_CYCLIC_QMAX 2048\b", header)
    assert info["lmax_target"] == lib.CYCLIC_TMAX == 65535 and re.search(r"#define SD_CYCLIC_TMAX 65535\b", header)
    assert info["pairs_max"] == lib.CYCLIC_PAIRS_MAX == 1 << 24 and info["block"] == 128
    assert re.search(r"constexpr int CYCLIC_BLOCK = 128;", open(os.path.join(ROOT, "stringdecomposer_amd", "csrc", "sd_cyclic.hpp")).read())
    assert info["launch_work"] >= 2 * (2 * 65535 - 1) * 32   # one pair at the limits fits a launch
    assert lib.CYCLIC_LAUNCH_WG_MIN == 1024 and re.search(r"#define SD_CYCLIC_LAUNCH_WG_MIN 1024\b", header)


def test_host_form_equals_the_table_on_all_pairs():
    """40 random sequences at the edges of the words, every one against every one: 1 600 pairs"""
    rng = random.Random(11)
    lens = [1, 1, 2, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 171, 512, 513]
    lens += [rng.choice(lens) for _ in range(40 - len(lens))]
    seqs = [ref.rnd(rng, n) for n in lens]
    got = lib.cyclic_pairs(seqs, threads=4)
    assert got.dist.shape == (40, 40) and got.dist.dtype == np.int32 and got.strand.dtype == np.uint8
    for a, q in enumerate(seqs):
        for b, t in enumerate(seqs):
            assert as_tuple(got, a, b) == ref.pair(q, t), (len(q), len(t))
    one = lib.cyclic_pairs(seqs, threads=1)
    assert all(np.array_equal(x, y) for x, y in zip(got, one))
    if edlib_ref.have_edlib():
        for a in range(0, 40, 3):
            for b in range(0, 40, 7):
                s = int(got.strand[a, b])
                assert got.dist[a, b] == edlib_ref.hw(seqs[a], ref.doubled(seqs[b], s)) <= edlib_ref.hw(seqs[a], ref.doubled(seqs[b], 1 - s))


def test_pairs_with_a_side_at_and_past_the_last_word():
    """a dozen pairs with a side of 2 048 / 2 049 bases; two of them related, so that the distance is not near the length"""
    rng = random.Random(12)
    big = [ref.rnd(rng, 2048), ref.rnd(rng, 2049)]
    seqs = big + [ref.rnd(rng, 171), ref.rnd(rng, 700), ref.edited(rng, ref.rotated(big[0], 900, 1), 8) + "A",
                  ref.edited(rng, ref.rotated(big[1], 64, 0), 3)[:2048]]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 3), (3, 1), (4, 0), (0, 4), (5, 1), (1, 5), (4, 5), (2, 1)]
    for a, b in pairs:
        got = lib.cyclic_pairs(seqs, [a], [b])
        assert as_tuple(got, 0, 0) == ref.pair(seqs[a], seqs[b]), (a, b)
    assert lib.cyclic_pairs(seqs, [4], [0]).dist[0, 0] <= 9 and lib.cyclic_pairs(seqs, [5], [1]).dist[0, 0] <= 4


@pytest.mark.parametrize("n", [171, 2054])
def test_planted_rotations(n):
    c, cases = ref.planted(20 + n, n)
    got = lib.cyclic_pairs([c] + [q for q, _, _, _ in cases], list(range(1, len(cases) + 1)), [0], threads=4)
    for i, (q, r, strand, e) in enumerate(cases):
        g = as_tuple(got, i, 0)
        if e == 0:
            assert (g[0], g[3], g[2]) == (0, r, strand), (r, strand)
        else:
            assert g[0] <= e and g[2] == strand, (r, strand, e)
            assert g == ref.pair(q, c), (r, strand, e)   # the reference is the judge: distance, end, strand and phase


def test_merge_equals_the_walk_at_any_block():
    seqs, label, fam = ref.families(5, n=48)
    rng = random.Random(6)
    weights = [rng.randrange(4) for _ in seqs]
    for f in fam:   # unrelated: far beyond any radius of the rule at P = 85
        for g in fam:
            if f is not g and abs(len(f) - len(g)) <= ref.radius(85, len(f)):
                assert ref.pair(f, g)[0] > 2 * ref.radius(85, len(f))
    got = lib.cyclic_merge(seqs, weights, 85, threads=4)
    want, nc = ref.merge(seqs, weights, 85)
    assert got.n_clusters == nc == 3 and merge_tuples(got) == [tuple(w) for w in want]
    assert ref.same_partition(got.cluster.tolist(), label)
    assert got.phase.tolist() == [(e + 1) % len(seqs[c]) for (_, c, _, e, _) in want]
    for block in (1, 3, len(seqs)):
        assert same_merge(lib.cyclic_merge(seqs, weights, 85, block=block), got), block
    assert same_merge(lib.cyclic_merge(seqs, weights, 85, block=5, threads=3), got)


def test_merge_at_a_tight_percentage_equals_the_walk():
    """P = 97: sequences of one family fall into several clusters, and centres made inside a block attract later ones"""
    seqs, _, _ = ref.families(8, n=40, lens=(64, 100))
    weights = [len(seqs) - i if i % 3 == 0 else 0 for i in range(len(seqs))]
    want, nc = ref.merge(seqs, weights, 97)
    assert nc > 4
    for block in (None, 1, 3, 7, len(seqs)):
        got = lib.cyclic_merge(seqs, weights, 97, block=block)
        assert got.n_clusters == nc and merge_tuples(got) == [tuple(w) for w in want], block


def test_a_dimer_is_not_merged_into_its_monomer():
    """The monomer fits its dimer exactly, and the dimer fits the monomer written twice but for one base: only the length
    condition holds them apart.  It does at every P above 50.  At P <= 50 the dimer's own radius, floor((100 - P) 342 / 100),
    reaches the 171 bases between the lengths, and the rule as written merges a dimer that is visited after its monomer (a
    monomer never joins its dimer: its radius would have to be its whole length); there the library must equal the walk."""
    rng = random.Random(3)
    mono = ref.rnd(rng, 171)
    p = lib.cyclic_pairs([mono + mono, mono])
    assert p.dist.tolist() == [[0, 1], [0, 0]]
    for P in (51, 70, 85, 99, 100):
        for seqs in ([mono, mono + mono], [mono + mono, mono]):
            m = lib.cyclic_merge(seqs, None, P)
            assert m.n_clusters == 2 and m.cluster.tolist() == [0, 1], P
    for P in (1, 50):
        assert ref.radius(P, 342) >= 171 > ref.radius(P, 171)
        for seqs in ([mono, mono + mono], [mono + mono, mono]):
            m = lib.cyclic_merge(seqs, None, P)
            assert merge_tuples(m) == [tuple(w) for w in ref.merge(seqs, [0, 0], P)[0]]
            assert m.n_clusters == (1 if seqs[0] is mono else 2)


def test_ties_go_to_the_earliest_centre_and_the_weight_order_is_honoured():
    rng = random.Random(4)
    a = ref.rnd(rng, 100)
    b = a[:50] + ("A" if a[50] != "A" else "C") + a[51:]                                  # 1 edit from a
    q = a[:20] + ("G" if a[20] != "G" else "T") + a[21:50] + b[50] + a[51:]              # 1 from b; 2 from a
    q1 = a[:20] + ("G" if a[20] != "G" else "T") + a[21:]                                # 1 from a, 2 from b
    far = ref.rnd(rng, 100)
    # the weight order.  Radius 2 at P = 98.  All weights equal: a is M1, b and q1 join it at 1, q at 2 (b is no centre)
    seqs = [a, far, b, q1, q]
    m = lib.cyclic_merge(seqs, [0] * 5, 98)
    assert merge_tuples(m) == [tuple(w) for w in ref.merge(seqs, [0] * 5, 98)[0]]
    assert m.centre.tolist() == [0, 1, 0, 0, 0] and m.dist.tolist() == [0, 0, 1, 1, 2]
    # b heaviest, then a: b is M1, a joins it at 1; q1 is 2 from b, q 1
    m = lib.cyclic_merge(seqs, [5, 0, 9, 0, 0], 98)
    assert merge_tuples(m) == [tuple(w) for w in ref.merge(seqs, [5, 0, 9, 0, 0], 98)[0]]
    assert m.cluster.tolist() == [0, 1, 0, 0, 0] and m.centre.tolist() == [2, 1, 2, 2, 2] and m.dist.tolist() == [1, 0, 0, 2, 1]
    # a tie.  Radius 1 (P = 98 at 60 bases): c1 and c2, 2 edits apart, are both centres; mid is 1 edit from each, and
    # comes rotated on the other strand.  The earliest centre takes it, whichever of the two that is.
    assert ref.radius(98, 60) == 1
    c1 = ref.rnd(rng, 60)
    c2 = c1[:10] + ("A" if c1[10] != "A" else "C") + c1[11:40] + ("A" if c1[40] != "A" else "C") + c1[41:]
    mid = ref.rotated(c1[:10] + c2[10] + c1[11:], 13, 1)
    assert ref.pair(mid, c1)[0] == ref.pair(mid, c2)[0] == 1 and ref.pair(c2, c1)[0] == 2
    for first, second in ((c1, c2), (c2, c1)):
        m = lib.cyclic_merge([first, second, mid], [2, 2, 0], 98)
        assert m.n_clusters == 2 and m.centre.tolist() == [0, 1, 0] and m.dist.tolist() == [0, 0, 1] and m.strand.tolist() == [0, 0, 1]
        m = lib.cyclic_merge([first, second, mid], [2, 2, 0], 98, block=1)
        assert m.centre.tolist() == [0, 1, 0]


def test_canonical_records_do_not_depend_on_rotation_or_strand():
    rng = random.Random(9)
    for s in [ref.rnd(rng, n) for n in (1, 2, 7, 64, 171)] + ["ACAC", "AAAA", "ACGT", "TTGCAA", "ACACAT" * 5]:
        rec, rot, strand = lib.cyclic_canon(s)
        assert (rec, rot, strand) == ref.canon(s), s
        base = ref.revcomp(s) if strand else s
        assert base[rot:] + base[:rot] == rec
        for r in (0, 1, len(s) // 2, len(s) - 1):
            for st in (0, 1):
                assert lib.cyclic_canon(ref.rotated(s, r, st))[0] == rec


def _pairs_rc(seqs, q, t):
    text, ro, rl = lib._reads_text(seqs)
    qi, ti = np.asarray(q, dtype=np.int32), np.asarray(t, dtype=np.int32)
    out = [np.zeros(len(q) * len(t), dtype=d) for d in (np.int32, np.int32, np.uint8)]
    err = C.create_string_buffer(512)
    rc = lib.load().sd_cyclic_pairs_host(text or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), qi.ctypes.data, ti.ctypes.data, len(qi), len(ti), 1,
                                         out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, err, 512)
    return rc, err.value.decode()


def test_refusals_and_their_texts():
    assert _pairs_rc(["ACGT", "ACNT"], [0], [0]) == (lib.SD_ERR_PARAM, "sd_cyclic_pairs_host: sequence 1 holds a byte outside ACGT at position 2")
    assert _pairs_rc(["ACGT", "acgt"], [0], [0])[1].startswith("sd_cyclic_pairs_host: sequence 1 holds a byte outside ACGT")
    assert _pairs_rc(["ACGT", ""], [0], [0]) == (lib.SD_ERR_PARAM, "sd_cyclic_pairs_host: sequence 1 is empty")
    assert _pairs_rc(["ACGT"], [1], [0]) == (lib.SD_ERR_PARAM, "sd_cyclic_pairs_host: query 0 is not a sequence")
    assert _pairs_rc(["ACGT"], [0], [0])[0] == lib.SD_OK
    for call, word in ((lambda: lib.cyclic_pairs(["ACGT", "ACRT"]), "sequence 1 holds a byte outside ACGT"),
                       (lambda: lib.cyclic_pairs(["", "ACGT"]), "sequence 0 is empty"),
                       (lambda: lib.cyclic_merge(["ACGT", "ACG-"], names=["r1", "r2"]), "sequence 1 (r2) holds a byte outside ACGT"),
                       (lambda: lib.cyclic_merge(["ACGT"], P=0), "P = 0, must be an integer 1 .. 100"),
                       (lambda: lib.cyclic_merge(["ACGT"], P=101), "P = 101, must be an integer 1 .. 100"),
                       (lambda: lib.cyclic_merge(["ACGT"], block=0), "block = 0"),
                       (lambda: lib.cyclic_merge(["ACGT"], [1, 2]), "2 weights for 1 sequences"),
                       (lambda: lib.cyclic_pairs(["ACGT"], [3]), "queries holds an index outside the 1 sequences"),
                       (lambda: lib.cyclic_canon("ACGN"), "outside ACGT")):
        with pytest.raises(lib.SdError) as e:
            call()
        assert e.value.code == lib.SD_ERR_PARAM and word in e.value.msg, e.value.msg
    # the library's own check of P, behind the Python one
    text, ro, rl = lib._reads_text(["ACGT"])
    w, out, nc, err = np.zeros(1, dtype=np.int64), np.zeros(8, dtype=np.int32), C.c_int32(0), C.create_string_buffer(512)
    rc = lib.load().sd_cyclic_merge_host(text, ro.ctypes.data, rl.ctypes.data, 1, w.ctypes.data, 0, 0, 1, out.ctypes.data, out.ctypes.data,
                                         out.ctypes.data, out.ctypes.data, out.ctypes.data, C.byref(nc), err, 512)
    assert rc == lib.SD_ERR_PARAM and err.value.decode() == "sd_cyclic_merge_host: P = 0, the identity of a cluster is 1 .. 100 percent"


@pytest.mark.parametrize("prog,extra,word", [("sd-autocorr", ["--autocorr-merge", "85"], "--autocorr-merge 85: the merge clusters the seeds, it needs --autocorr-seeds"),
                                             ("sd-autocorr", ["--autocorr-seeds", "1", "--autocorr-merge", "0"], "--autocorr-merge 0: the identity of a cluster is 1 .. 100 percent"),
                                             ("sd-autocorr", ["--autocorr-seeds", "1", "--autocorr-merge", "101"], "1 .. 100 percent"),
                                             ("sd-autocorr", ["--autocorr-seeds", "1", "--autocorr-merge", "85", "--autocorr-merge-min-size", "0"], "--autocorr-merge-min-size 0"),
                                             ("stringdecomposer", ["--autocorr", "8", "--autocorr-merge", "85"], "it needs --autocorr-seeds"),
                                             ("stringdecomposer", ["--autocorr-merge", "85"], "it needs --autocorr and --autocorr-seeds"),
                                             ("stringdecomposer", ["--autocorr-seeds", "1", "--autocorr-merge", "85"], "it needs --autocorr and"),
                                             ("sd-merge", ["--merge", "0"], "--merge 0: the identity of a cluster is 1 .. 100 percent"),
                                             ("sd-merge", ["--merge-min-size", "0"], "--merge-min-size 0"),
                                             ("sd-merge", ["WORLD"], "WORLD_SIZE=2")])
def test_cli_refusals_before_device_work(tmp_path, prog, extra, word):
    env = dict(os.environ, **NO_DEVICE)
    if extra == ["WORLD"]:
        env.update(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
        extra = []
    args = [os.path.join(TD, "read.fa")] + ([os.path.join(TD, "DXZ1_star_monomers.fa")] if prog == "stringdecomposer" else [])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog)] + args + ["-o", str(tmp_path / "out")] + extra,
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 2, p.stderr
    assert p.stderr.count("\n") == 1 and p.stderr.startswith(prog + ": --") and word in p.stderr, p.stderr
    assert not os.path.exists(str(tmp_path / "out"))


def test_the_files_and_min_size(tmp_path):
    """the two files of the host form: the lines, the headers, the identity from integers, min-size on the .fa only"""
    seqs, label, fam = ref.families(14, n=12, lens=(40, 90))
    lone = ref.rnd(random.Random(1), 63)
    seqs.append(lone)
    names = ["read%d/0_%d period=%d count=%d" % (i, len(s), len(s), 10 + i) for i, s in enumerate(seqs[:-1])] + ["lone"]
    paths = [str(tmp_path / x) for x in ("a.fa", "a.tsv", "b.fa", "b.tsv")]
    m = cyclic.merge_files(names, [s.encode() for s in seqs], 85, paths[0], paths[1])
    m2 = cyclic.merge_files(names, seqs, 85, paths[2], paths[3], min_size=2, block=2)
    assert same_merge(m, m2) and open(paths[1]).read() == open(paths[3]).read()
    want, nc = ref.merge(seqs, [10 + i for i in range(12)] + [0], 85)
    assert m.n_clusters == nc == 3
    rows = formats.read_merge(paths[1])
    assert formats.format_merge(rows) == open(paths[1]).read() and len(rows) == 13
    for i, (row, w) in enumerate(zip(rows, want)):
        cl, ce, d, e, s = w
        assert row == formats.MergeRow(names[i].split()[0], len(seqs[i]), "M%d" % (cl + 1), names[ce].split()[0], d,
                                       "%.2f" % (100 * (len(seqs[i]) - d) / len(seqs[i])), "-+"[s == 0], (e + 1) % len(seqs[ce]))
        if ce == i:
            assert (row.distance, row.identity, row.strand, row.phase) == (0, "100.00", "+", 0)
    fa = open(paths[0]).read().split("\n")
    assert len(fa) == 2 * nc + 1 and len(open(paths[2]).read().split("\n")) == 2 * (nc - 1) + 1   # the lone cluster is left out
    assert "M3 " not in open(paths[2]).read() or "seeds=1" not in open(paths[2]).read()
    for c in range(nc):
        members = [i for i in range(13) if want[i][0] == c]
        centre = want[members[0]][1]
        rec, rot, strand = ref.canon(seqs[centre])
        assert fa[2 * c] == ">M%d period=%d seeds=%d count=%d centre=%s rotation=%d strand=%s" % (
            c + 1, len(rec), len(members), sum(cyclic.weight_of(names[i]) for i in members), names[centre].split()[0], rot, "+-"[strand])
        assert fa[2 * c + 1] == rec
    assert formats.merge_identity(3, 1) == "66.67" and formats.merge_identity(8, 1) == "87.50" and formats.merge_identity(2054, 0) == "100.00"
    assert formats.merge_identity(32, 3) == "90.62" == "%.2f" % 90.625   # printf's rounding, ties included
    assert formats.merge_identity(1000, 5) == "99.50" and formats.merge_identity(16, 1) == "93.75" and formats.merge_identity(32, 1) == "96.88"
    assert cyclic.weight_of("r/0_5 period=5 count=17") == 17 and cyclic.weight_of("count=3") == 0 and cyclic.weight_of("r count=x") == 0
    # the reader of bin/sd-merge keeps the whole header (the weight is in it), folds case and CRLF only when lenient
    src = str(tmp_path / "in.fa")
    with open(src, "wb") as f:
        f.write(b"".join(b">%s\r\n%s\r\n%s\r\n" % (n.encode(), s[:30].lower().encode(), s[30:].encode()) for n, s in zip(names, seqs)))
    assert cyclic.read_fasta(src, lenient=True) == (names, [s.encode() for s in seqs])
    assert cyclic.read_fasta(src)[1][0] == seqs[0][:30].lower().encode() + b"\r" + seqs[0][30:].encode() + b"\r"
    with pytest.raises(lib.SdError) as e:
        cyclic.merge_files(*cyclic.read_fasta(src), 85, paths[2], paths[3])
    assert "sequence 0 (read0/0_%d) holds a byte outside ACGT" % len(seqs[0]) in e.value.msg
    with open(paths[1], "a") as f:
        f.write("r\t5\tM1\tr\t0\t100.00\t*\t0\n")
    with pytest.raises(formats.FormatError):
        formats.read_merge(paths[1])


def test_the_reads_of_the_command_line_test_show_their_periods_on_the_host():
    """what tests/test_gpu_cyclic.py runs through bin/sd-autocorr, here through the host forms: every read's period is the
    planted one, and the seeds fall into the two arrays"""
    names, reads, label = ref.array_reads(4)
    ac = lib.autocorr(reads, 8, 4096, 0, threads=4)
    seeds = lib.autocorr_seeds(reads, names, ac, 1, 1, 8)
    assert [len(s) for _, s in seeds] == [(171, 340)[a] for a in label]
    m = lib.cyclic_merge([s for _, s in seeds], [cyclic.weight_of(n) for n, _ in seeds], 85, threads=4)
    assert m.n_clusters == 2 and ref.same_partition(m.cluster.tolist(), label) and set(m.strand.tolist()) == {0, 1}


def test_the_command_line_request():
    """autocorr.request: the merge needs the seeds; the defaults leave the request as it was"""
    def args(**kw):
        d = dict(autocorr="8", autocorr_window=0, autocorr_min_lag=1, autocorr_peaks="8,8", autocorr_spectrum=False, autocorr_seeds=None,
                 autocorr_merge=None, autocorr_merge_min_size=1)
        d.update(kw)
        return argparse.Namespace(**d)
    assert autocorr.request(args()) == (8, 4096, 0, 1, 8, 8) == autocorr.request(args(autocorr_seeds=1, autocorr_merge=85))
    assert "needs --autocorr-seeds" in autocorr.request(args(autocorr_merge=85))
    assert "1 .. 100 percent" in autocorr.request(args(autocorr_seeds=1, autocorr_merge=0))
    assert autocorr.merge_files("d", "o") == (os.path.join("d", "o_autocorr_merged.fa"), os.path.join("d", "o_autocorr_merge.tsv"))
