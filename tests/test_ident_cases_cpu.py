"""The cases of tests/ident_cases.py without a GPU: each lies on the routes of csrc/sd_ident.hip it exists for, stays below
the sizes at which a job leaves the in-stream path, its committed fixture is what the oracle's rows and the host's
post-processing give, and the numpy restatement of the pruned homopolymer pass keeps what the reference reports."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import ident_cases as ic
from stringdecomposer_amd import lib, main as sdmain

# the route every case exists for, as the kernels choose it: K plain / compressed, masks of the plain / compressed pass,
# form of the selection pass
TABLE = {
    "k1": (8, 1, 1, "lds", "lds", "two"),
    "k2": (10, 2, 2, "lds", "lds", "two"),
    "k4": (8, 4, 3, "lds", "lds", "two"),
    "k6_round": (8, 6, 4, "lds", "lds", "two"),
    "k8_round": (8, 8, 6, "lds", "lds", "two"),
    "k8_edges": (12, 8, 6, "lds", "lds", "two"),
    "t140": (140, 3, 3, "lds", "lds", "buffered"),
    "t260_k8": (260, 8, 6, "global", "global", "buffered"),
    "t520": (520, 3, 3, "global", "global", "buffered"),
    "t1040": (1040, 2, 2, "global", "global", "direct"),
    "hpc_ties": (14, 4, 2, "lds", "lds", "two"),
    "t600_waves": (600, 2, 1, "lds", "lds", "buffered"),
}


def test_words_rule():
    assert [ic.words(n) for n in (1, 64, 65, 128, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512)] == \
        [1, 1, 2, 2, 3, 4, 4, 6, 6, 6, 6, 8, 8, 8, 8]
    assert set(ic.words(n) for n in range(1, 513)) == {1, 2, 3, 4, 6, 8}   # the instantiated kernels


@pytest.mark.parametrize("case", ic.CASES + [ic.WAVE_CASE], ids=repr)
def test_case_lies_on_its_route(case):
    ic.check_routes(case)
    r = case.routes()
    if case.name == "k8_513":
        assert not r["taken"] and max(len(s) for s in case.monomers()[1]) == 513
        return
    assert (r["T"], r["K"], r["Kh"], r["masks"], r["masks_h"], r["select"]) == TABLE[case.name]
    assert r["taken"] and r["mask_bytes"] == r["T"] * 5 * r["K"] * 8 and r["mask_bytes_h"] == r["T"] * 5 * r["Kh"] * 8
    assert (r["masks"] == "global") == (r["mask_bytes"] > 60 * 1024)
    assert (r["masks_h"] == "global") == (r["mask_bytes_h"] > 60 * 1024)
    assert len(set(case.monomers()[0])) == len(case.monomers()[0])   # unique names: keys = the interleaved templates
    # together the cases reach every instantiated word count in both passes
    assert {c.routes()["K"] for c in ic.GOLDEN_CASES} == {1, 2, 3, 4, 6, 8}
    assert {c.routes()["Kh"] for c in ic.GOLDEN_CASES} >= {1, 2, 3, 4, 6}


@pytest.mark.parametrize("case", ic.CASES, ids=repr)
def test_rows_stay_on_the_in_stream_path(case, oracle):
    """Between 8 and 4096 rows (the identity outputs have room for at least 4096 records: no case leaves the in-stream path
    by size), every read one chunk (records = rows), and the N runs where the table puts them."""
    rows = ic.raw_rows(case.name)
    assert 8 <= len(rows) <= 4096
    rs = case.reads()[1]
    assert all(len(oracle.chunk_plan(len(s), ic.PART, ic.OVERLAP)) == 1 for s in rs)
    assert lib.chunk_table_size([len(s) for s in rs], ic.PART, ic.OVERLAP) == len(rs)
    lens = [e - s + 1 for _, _, s, e in rows]
    if case.name == "k2":     # the run of 8 N lies inside one block
        assert sum(rs[r][s:e + 1].count(b"N" * 8) for r, _, s, e in rows) == 1 and b"N" * 9 not in rs[1]
    if case.name == "t140":   # the run of 600 N lies inside one block, which is then a record of the long list
        assert [rs[r][s:e + 1].count(b"N") for (r, _, s, e), n in zip(rows, lens) if n > ic.SHORT_MAX] == [600]
        assert len(rs) >= 3
    if case.name in ("k1", "k2", "k4", "t520", "t1040", "hpc_ties"):
        assert max(lens) <= ic.SHORT_MAX


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("second_best", [False, True], ids=["light", "second_best"])
@pytest.mark.parametrize("case", ic.GOLDEN_CASES, ids=repr)
def test_fixture_is_the_oracles_rows_post_processed_by_the_host(case, second_best, tmp_path):
    """The committed inputs are the case's sequences, the reference's raw file hashes to the oracle's rows, and convert_tsv
    (host NW) over those rows writes the reference's final TSV byte for byte and its _alt TSV (by sha256 and length, byte
    for byte where it is stored)."""
    d = case.dir()
    with open(os.path.join(d, "params.json" if second_best else "params_light.json")) as f:
        c = json.load(f)
    assert c["args"] == (["--second-best"] if second_best else [])
    reads = sdmain.load_fasta(os.path.join(d, "reads.fa"), "map")
    mons = sdmain.load_fasta(os.path.join(d, "monomers.fa"))
    assert ([m.name for m in mons], [m.seq.encode() for m in mons]) == tuple(list(x) for x in case.monomers())
    assert ([reads[n].seq.encode() for n in case.reads()[0]], len(reads)) == (list(case.reads()[1]), len(case.reads()[0]))
    raw = ic.raw_tsv(case.name)
    assert hashlib.sha256(raw).hexdigest() == c["raw_sha256"]
    out = str(tmp_path / "final.tsv")
    sdmain.convert_tsv(raw.decode(), reads, sdmain.add_rc_monomers(mons), out, 0, not second_best, threads=4)
    final, alt = _read(out), _read(out[:-4] + "_alt.tsv")
    assert final == _read(os.path.join(d, "final.tsv" if second_best else "final_light.tsv"))
    assert final.count(b"\n") == c["final_rows"] == len(ic.raw_rows(case.name))
    assert (hashlib.sha256(alt).hexdigest(), len(alt)) == (c["alt_sha256"], c["alt_bytes"])
    assert (len(alt) > 0) == second_best
    gz = os.path.join(d, "alt.tsv.gz")
    with open(os.path.join(d, "params.json")) as f:
        assert os.path.exists(gz) == (json.load(f)["alt_bytes"] < 100 * 1000)   # (beyond it the sha256 alone)
    if second_best and os.path.exists(gz):
        with gzip.open(gz, "rb") as f:
            assert alt == f.read()


@pytest.mark.parametrize("case", ic.GOLDEN_CASES, ids=repr)
def test_pruning_rule_keeps_the_two_best(case):
    """The restated rule against the true compressed identities: the pairs it keeps include the two the reference reports
    for every row, every pair it drops is strictly below the row's second best -- and it drops some (except where every
    compressed template is the same)."""
    keep, short = ic.pruned(case.name)
    d, m, cols, _, _ = ic.alignments(case.name, True)
    true = ic._percent(d, m, cols)
    ref = ic.final_reference(case.name)
    n, T = true.shape
    assert keep.shape == (n, T) and not keep[~short].any()
    for i in np.nonzero(short)[0]:
        assert keep[i, ref["homo_best"][i]] and keep[i, ref["homo_second"][i]]
        second = np.sort(true[i])[-2]
        assert second == ref["homo_second_ident"][i]
        assert (true[i][~keep[i]] < second).all()
    # the bounds hold the truth
    lb, ub, m_lb = ic.bounds(d, ic.alignments(case.name, True)[3][:, None], ic.alignments(case.name, True)[4][None, :])
    frac = m.astype(np.float64) / cols
    assert (lb <= frac).all() and (frac <= ub).all() and (m_lb <= m).all()
    full, pairs = ic.expected_full_pairs(case.name), n * T
    assert 2 * int(short.sum()) <= full <= pairs
    if case.strict_prune:
        assert full < int(short.sum()) * T


def test_tie_case_ties():
    """hpc_ties: the compressed identities of a row take two values (forward / reverse templates), each seven times; the
    reference's stable sort reports the first two templates of the better strand.  The duplicate monomer ties the plain
    pass too."""
    ref = ic.final_reference("hpc_ties")
    d, m, cols, _, _ = ic.alignments("hpc_ties", True)
    true = ic._percent(d, m, cols)
    for i in range(len(true)):
        assert len(set(true[i, 0::2])) == 1 and len(set(true[i, 1::2])) == 1
        fwd = true[i, 0] >= true[i, 1]
        assert (ref["homo_best"][i], ref["homo_second"][i]) == ((0, 2) if fwd else (1, 3))
        assert ref["homo_ident"][i] == ref["homo_second_ident"][i]
    assert (ref["alt"][:, 0] == ref["alt"][:, 12]).all() and (ref["alt"][:, 1] == ref["alt"][:, 13]).all()


def test_selection_buffer_trace():
    """select_trace, the restated buffer of the selection pass: with one record per wave nothing is carried or flushed inside
    the loop (every small case); with three records of T / 2 candidates per wave at T = 600 the second is added to a filled
    buffer and the third forces a flush; long records are skipped; beyond 1024 templates there is no buffer."""
    assert ic.select_trace([7] * 50, 520, 3072) == (0, 0)
    assert ic.select_trace([300] * 9, 600, 3) == (3, 3)
    assert ic.select_trace([300, -1, 300, 300], 600, 1) == (1, 1)
    assert ic.select_trace([60] * 80, 140, 4) == (4, 4 * 18)   # (20 records a wave; 60 k + 140 > 1024 before the 16th)
    assert ic.select_trace([300] * 9, 1040, 3) == (0, 0)
