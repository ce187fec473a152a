"""The in-stream identity kernels (csrc/sd_ident.hip: sd_ident_pairs<K>, sd_ident_dist<K>, sd_ident_select) on every route
they choose at run time -- tests/ident_cases.py has one case per route and asserts that it lies on it.  Each case runs as
a file job (the three TSVs of the command line) and as a final-mode stream (typed rows), with --second-best (all templates,
plain and homopolymer-compressed, the compressed pass pruned) and without it (own template only), against

  b  the unmodified reference command line (tests/golden/final/ident_<case>/, made by tests/golden/make_final_golden.py),
  c  the other routes of the product: identities from the read text on the host, and the compressed pass without pruning,
  d  the pruning rule restated in numpy over the oracle's alignments: the number of pairs aligned in full, exactly,
  e  the identities and names of every row recomputed from the oracle's alignments, as doubles, exactly.

b prints two decimals and the two best compressed templates only; d and e are what a wrong bound or a wrong match count
on one of these routes cannot pass.

The cases and their routes (T; K plain / compressed; masks plain = compressed; selection):

  k1 8 1/1 lds two          k2 10 2/2 lds two          k4 8 4/3 lds two           k6_round 8 6/4 lds two
  k8_round 8 8/6 lds two    k8_edges 12 8/6 lds two    hpc_ties 14 4/2 lds two    t140 140 3/3 lds buffered
  t260_k8 260 8/6 global buffered     t520 520 3/3 global buffered     t1040 1040 2/2 global direct

These jobs have 12 to 50 records and the selection runs with thousands of waves, so each wave takes at most one record:
what they do NOT reach is a wave's buffer carrying candidates from one record to the next, and its flush inside the loop.
t600_waves (T = 600, ~7000 records of a set whose compressed templates are all the same) is the case for that."""
import functools
import gzip
import hashlib
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import ident_cases as ic
from stringdecomposer_amd import lib, main as sdmain, synth

pytestmark = pytest.mark.gpu

THREADS = 8
MODES = [False, True]
MODE_IDS = ["light", "second_best"]
_TMP = None


def _tmp():
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="sd_ident_routes_")
    return _TMP.name


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The case's FASTA files: the committed fixture's, or written here for a case without one."""
    c = ic.BY_NAME[name]
    if c.golden:
        return os.path.join(c.dir(), "reads.fa"), os.path.join(c.dir(), "monomers.fa")
    rfa, mfa = os.path.join(_tmp(), name + "_r.fa"), os.path.join(_tmp(), name + "_m.fa")
    synth.write_fasta(rfa, *c.reads(), width=80)
    synth.write_fasta(mfa, *c.monomers())
    return rfa, mfa


@functools.lru_cache(maxsize=None)
def _job(name, second_best, flags=0, max_batch_rows=0):
    """One file job, run once per process: ((raw, final, alt) bytes, last_run_stats())."""
    rfa, mfa = _inputs(name)
    o = [os.path.join(_tmp(), "%s_%d_%d_%d_%s.tsv" % (name, second_best, flags, max_batch_rows, x)) for x in ("raw", "final", "alt")]
    lib.run_files(rfa, mfa, o[0], o[1], o[2], min_identity=0, second_best=second_best, threads=THREADS, flags=flags,
                  max_batch_rows=max_batch_rows, lr_coef=sdmain._lr_coef())
    stats = lib.last_run_stats()
    files = []
    for x in o:
        with open(x, "rb") as f:
            files.append(f.read())
        os.unlink(x)
    return tuple(files), stats


def _golden(case, second_best):
    sfx = "" if second_best else "_light"
    with open(os.path.join(case.dir(), "params%s.json" % sfx)) as f:
        c = json.load(f)
    with open(os.path.join(case.dir(), "final%s.tsv" % sfx), "rb") as f:
        c["final"] = f.read()
    c["alt"] = None
    gz = os.path.join(case.dir(), "alt.tsv.gz")
    if second_best and os.path.exists(gz):
        with gzip.open(gz, "rb") as f:
            c["alt"] = f.read()
    return c


@pytest.mark.parametrize("second_best", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", ic.GOLDEN_CASES, ids=repr)
def test_in_stream_job_equals_the_reference(case, second_best):
    """a + b: the device served every identity of the job, and the three files are the reference's."""
    (raw, final, alt), st = _job(case.name, second_best)
    n, T = len(ic.raw_rows(case.name)), case.routes()["T"]
    print("%s %s: rows %d ident_pairs %d homo_pairs %d homo_full_pairs %d text_identity_ms %g batches %d" %
          (case.name, MODE_IDS[second_best], n, st["ident_pairs"], st["homo_pairs"], st["homo_full_pairs"],
           st["text_identity_ms"], st["batches"]))
    assert st["ident_pairs"] > 0 and st["text_identity_ms"] < 1e-3
    assert st["ident_pairs"] == (2 * n * T if second_best else n)
    if second_best:
        assert st["homo_pairs"] == n * T
    g = _golden(case, second_best)
    assert final == g["final"]
    assert (hashlib.sha256(raw).hexdigest(), raw.count(b"\n")) == (g["raw_sha256"], n)
    assert (hashlib.sha256(alt).hexdigest(), len(alt)) == (g["alt_sha256"], g["alt_bytes"])
    if g["alt"] is not None:
        assert alt == g["alt"]


@pytest.mark.parametrize("second_best", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", ic.GOLDEN_CASES, ids=repr)
def test_other_routes_write_the_same_files(case, second_best):
    """c: identities from the read text (the host NW the CPU suite pins to edlib), the compressed pass with every pair
    aligned in full, and -- t140 -- the job cut into at least three device batches."""
    files, st = _job(case.name, second_best)
    text, tst = _job(case.name, second_best, flags=lib.FLAG_NO_STREAM_IDENT)
    assert tst["ident_pairs"] == 0 and tst["text_identity_ms"] > 0
    assert text == files
    if second_best:
        full, fst = _job(case.name, True, flags=lib.FLAG_NO_IDENT_PRUNE)
        assert fst["ident_pairs"] == st["ident_pairs"] and fst["text_identity_ms"] < 1e-3 and fst["homo_full_pairs"] == 0
        assert full == files
    if case.name == "t140":
        cut, cst = _job(case.name, second_best, max_batch_rows=max(len(s) for s in case.reads()[1]))
        assert cst["batches"] >= 3 and cst["ident_pairs"] == st["ident_pairs"] and cst["text_identity_ms"] < 1e-3
        assert cut == files
        if second_best:
            assert (cst["homo_pairs"], cst["homo_full_pairs"]) == (st["homo_pairs"], st["homo_full_pairs"])


@pytest.mark.parametrize("case", ic.GOLDEN_CASES, ids=repr)
def test_pruned_pass_aligns_exactly_the_pairs_its_rule_keeps(case):
    """d: homo_full_pairs is the number of compressed pairs whose upper bound reaches the row's second largest lower
    bound, counted from the oracle's distances over the rows of at most 512 bp."""
    _, st = _job(case.name, True)
    want = ic.expected_full_pairs(case.name)
    print("%s: homo_pairs %d homo_full_pairs %d expected %d" % (case.name, st["homo_pairs"], st["homo_full_pairs"], want))
    assert st["homo_full_pairs"] == want
    if case.strict_prune:
        assert st["homo_full_pairs"] < st["homo_pairs"]


def _stream_rows(case, second_best, **kw):
    mn, ms = case.monomers()
    st = lib.Stream(ms, final=True, mono_names=mn, second_best=second_best, min_identity=0, threads=THREADS, **kw)
    try:
        st.submit(case.reads()[1])
        fr = st.collect()
        return fr, st.keys(), st.stats()
    finally:
        st.close()


def _check_rows(case, second_best, fr, keys):
    ref = ic.final_reference(case.name)
    rows = fr.rows
    assert keys == ic.interleaved(*case.monomers())[0]
    assert len(rows) == len(ref["read"]) and fr.row_off[-1] == len(rows)
    for f in ("read", "start", "end", "best"):
        assert np.array_equal(rows[f], ref[f]), f
    assert np.array_equal(rows["ident"], ref["ident"])   # exact: the same two integers divided the same way
    if not second_best:
        assert fr.alt is None
        return
    for f in ("second", "homo_best", "homo_second", "second_ident", "homo_ident", "homo_second_ident"):
        bad = np.nonzero(rows[f] != ref[f])[0]
        assert len(bad) == 0, (f, bad[:5], rows[f][bad[:5]], ref[f][bad[:5]])
    assert fr.alt.shape == ref["alt"].shape and np.array_equal(fr.alt, ref["alt"])


@pytest.mark.parametrize("second_best", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", ic.GOLDEN_CASES, ids=repr)
def test_rows_at_full_precision(case, second_best):
    """e: every row of the final-mode stream against the oracle's alignments and the reference's rule (own monomer; first
    maximum among the others; stable sort of the compressed scores): names and doubles exactly, every _alt column."""
    fr, keys, stats = _stream_rows(case, second_best)
    assert stats["ident_pairs"] > 0 and stats["fallback_blocks"] == 0
    _check_rows(case, second_best, fr, keys)


@pytest.mark.parametrize("second_best", MODES, ids=MODE_IDS)
def test_a_513_bp_monomer_takes_the_text_path(second_best):
    """k8_513 = k8_edges with one more base on its first monomer: the identity kernels decline the set, the job computes
    its identities from the read text -- the files of the host's post-processing of the oracle's rows, and the oracle's
    rows at full precision."""
    case = ic.BY_NAME["k8_513"]
    files, st = _job(case.name, second_best)
    assert st["ident_pairs"] == 0 and st["text_identity_ms"] > 0
    assert files[0] == ic.raw_tsv(case.name)
    rfa, mfa = _inputs(case.name)
    out = os.path.join(_tmp(), "k8_513_host_%d.tsv" % second_best)
    sdmain.convert_tsv(files[0].decode(), sdmain.load_fasta(rfa, "map"), sdmain.add_rc_monomers(sdmain.load_fasta(mfa)), out, 0,
                       not second_best, threads=4)
    with open(out, "rb") as f:
        assert f.read() == files[1]
    with open(out[:-4] + "_alt.tsv", "rb") as f:
        assert f.read() == files[2]
    fr, keys, stats = _stream_rows(case, second_best)
    assert stats["ident_pairs"] == 0
    _check_rows(case, second_best, fr, keys)
    # the 512-bp set on the same reads is taken: the two jobs differ in that one base, and both decompose the reads
    _, st512 = _job("k8_edges", second_best)
    assert st512["ident_pairs"] > 0


@functools.lru_cache(maxsize=None)
def _wave_job():
    """t600_waves as a file job that keeps no row (no identity reaches 101: the _alt text of 7000 rows x 600 keys would be
    150 MB) -> (rows [(read, template, start, end)], segments, last_run_stats())."""
    c = ic.WAVE_CASE
    rfa, mfa = _inputs(c.name)
    o = [os.path.join(_tmp(), "waves_%s.tsv" % x) for x in ("raw", "final", "alt")]
    lib.run_files(rfa, mfa, o[0], o[1], o[2], min_identity=101, second_best=True, threads=THREADS, lr_coef=sdmain._lr_coef())
    st = lib.last_run_stats()
    ridx = {n: i for i, n in enumerate(c.reads()[0])}
    tidx = {n: i for i, n in enumerate(ic.interleaved(*c.monomers())[0])}
    with open(o[0]) as f:
        rows = [(ridx[x[0]], tidx[x[1]], int(x[2]), int(x[3])) for x in (ln.split("\t") for ln in f)]
    assert os.path.getsize(o[1]) == 0 and os.path.getsize(o[2]) == 0
    for x in o:
        os.unlink(x)
    return rows, [c.reads()[1][r][s:e + 1] for r, _, s, e in rows], st


@functools.lru_cache(maxsize=None)
def _wave_reference():
    """Compressed pass of t600_waves over the job's own rows, from the oracle: (d, matches, columns) [rows, T], kept query
    symbols [rows], template lengths [T], short [rows]."""
    rows, segs, _ = _wave_job()
    tm = [ic.hpc(t) for t in ic.interleaved(*ic.WAVE_CASE.monomers())[1]]
    assert len(set(tm)) == 2   # (one template and its reverse complement: two alignments per row)
    hs = [ic.hpc(q) for q in segs]
    d, m, cols = ic._align(hs, tm)
    short = np.array([len(q) <= ic.SHORT_MAX for q in segs], dtype=bool)
    return d, m, cols, np.array([len(q) for q in hs], dtype=np.int64), np.array([len(t) for t in tm], dtype=np.int64), short


def test_waves_that_take_several_records_buffer_and_flush_inside_the_loop():
    """Several records per wave, d: with more records than twice the waves of the launch and about T / 2 candidates per
    record, a wave adds a second record's candidates to its buffer and flushes it before the third.  The number of pairs
    aligned in full is the restated rule's count, exactly -- a candidate lost or written twice on the way changes it."""
    c = ic.WAVE_CASE
    rows, segs, st = _wave_job()
    T, n = c.routes()["T"], len(rows)
    d, _, _, kept, tl, short = _wave_reference()
    keep = ic.keep_rule(d, kept, tl, short)
    cands = np.where(short, keep.sum(axis=1), -1)
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 3 * 4   # (grid of 3 workgroups of 4 waves per CU)
    mid, carried = ic.select_trace(cands, T, waves)
    print("t600_waves: rows %d waves %d homo_pairs %d homo_full_pairs %d expected %d; flushes inside the loop %d, records "
          "added to a filled buffer %d" % (n, waves, st["homo_pairs"], st["homo_full_pairs"], int(keep.sum()), mid, carried))
    assert n > 2 * waves and mid > 0 and carried > 0
    assert st["batches"] == 1 and st["text_identity_ms"] < 1e-3
    assert st["ident_pairs"] == 2 * n * T and st["homo_pairs"] == n * T
    assert st["homo_full_pairs"] == int(keep.sum()) < n * T


def test_rows_of_waves_that_take_several_records():
    """Several records per wave, c + e: the typed rows equal those of the unpruned pass (every compressed pair aligned in
    full, no selection), and their compressed columns -- names and doubles -- are the oracle's under the reference's stable
    sort (each strand's 300 templates tie: the first two of the better strand)."""
    c = ic.WAVE_CASE
    rows, _, _ = _wave_job()
    fr, keys, stats = _stream_rows(c, True)
    full, _, fstats = _stream_rows(c, True, flags=lib.FLAG_NO_IDENT_PRUNE)
    assert stats["ident_pairs"] == fstats["ident_pairs"] > 0 and stats["fallback_blocks"] == 0 and stats["batches"] == 1
    assert fr.rows.tobytes() == full.rows.tobytes() and np.array_equal(fr.row_off, full.row_off) and np.array_equal(fr.alt, full.alt)
    assert [(int(r), int(s), int(e)) for r, s, e in zip(fr.rows["read"], fr.rows["start"], fr.rows["end"])] == \
        [(r, s, e) for r, _, s, e in rows]
    assert np.array_equal(fr.rows["best"], [t for _, t, _, _ in rows])
    d, m, cols, _, _, _ = _wave_reference()
    hv = ic._percent(d, m, cols)
    order = np.argsort(-hv, axis=1, kind="stable")
    ar = np.arange(len(rows))
    for f, want in (("homo_best", order[:, 0]), ("homo_second", order[:, 1]), ("homo_ident", hv[ar, order[:, 0]]),
                    ("homo_second_ident", hv[ar, order[:, 1]])):
        bad = np.nonzero(fr.rows[f] != want)[0]
        assert len(bad) == 0, (f, len(bad), bad[:5], fr.rows[f][bad[:5]], want[bad[:5]])
