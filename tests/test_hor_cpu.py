"""Higher-order repeat units (--hor) without a device: the host form (sd_hor_rows, sd_hor_final_host) against the Python
restatement of tests/hor_ref.py -- the committed final goldens with the figures of the issue, planted label strings for
every clause of the rule, seeded random strings, the refusals, the three file formats and the command line's refusals."""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hor_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
DXZ1 = os.path.join(TD, "DXZ1_star_monomers.fa")
NEW = ["sd_hor_rows", "sd_hor_final_host", "sd_hor_name", "sd_hor_info"]
L_MONO = 10   # bases of a planted row


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    info = lib.hor_info()
    assert (info["mmax"], info["pmax"]) == (lib.HOR_MMAX, lib.HOR_PMAX) == (2048, 64)
    assert "#define SD_HOR_MMAX 2048" in header and "#define SD_HOR_PMAX 64" in header


# ---- helpers --------------------------------------------------------------------------------------------------------
def same(got, exp, what=""):
    """a formats.Hor against the dict of hor_ref.analyse, every array"""
    assert got.T.tolist() == exp["T"], "%s: T differs" % what
    for name in ("rows", "hor", "pos", "kinds", "lens", "row_unit"):
        assert np.asarray(getattr(got, name)).tolist() == exp[name], "%s: %s differs" % (what, name)
    assert got.long == exp["long"], "%s: long orders differ" % what
    assert got.units.tolist() == exp["units"], "%s: units differ" % what


def host_equals_ref(cols, M, G=0, C=2, threads=3, what=""):
    got = lib.hor_rows(*cols, M, G, C, threads=threads)
    same(got, ref.analyse(*cols, M, G, C), what)
    return got


def planted(reads):
    """reads: per read a list of (key, usable, gap before the row) -> the five columns; rows of L_MONO bases"""
    read, start, end, key, usable = [], [], [], [], []
    for r, rows in enumerate(reads):
        at = 0
        for k, u, gap in rows:
            at += gap
            read.append(r)
            start.append(at)
            end.append(at + L_MONO - 1)
            key.append(k)
            usable.append(u)
            at += L_MONO
    return read, start, end, key, usable


def walk(monos, copies, strand=0, skip=lambda copy: ()):
    """`copies` copies of the order `monos` as rows of one read: forward, or on the reverse strand from its end; skip(copy):
    the positions (1-based) a copy lacks"""
    out = []
    for c in range(copies):
        seq = [(p, m) for p, m in enumerate(monos, 1) if p not in skip(c)]
        for p, m in (seq if strand == 0 else seq[::-1]):
            out.append((2 * m + strand, 1, 0))
    return out


def names_of(h):
    return [formats.hor_mask_name(u[3]) for u in h.units.tolist()]


def golden_columns(final, monomers):
    """the columns of a final TSV: key by the monomer's position in its file, ' = the reverse complement"""
    mono = [n.split()[0] for n in lib.fasta_load(monomers)[0]]
    index = {n: m for m, n in enumerate(mono)}
    reads, cols = [], ([], [], [], [], [])
    for r in formats.read_final(final):
        if not reads or reads[-1] != r.read:
            reads.append(r.read)
        rev = r.monomer.endswith("'")
        for c, v in zip(cols, (len(reads) - 1, r.start, r.end, 2 * index[r.monomer.rstrip("'")] + rev, r.reliability == "+")):
            c.append(int(v))
    return cols, mono, reads


# ---- the committed goldens, with the figures of the issue ---------------------------------------------------------------
def test_golden_dxz1_one_cycle_of_twelve_in_file_order():
    """557 rows: one cycle of the 12 monomers in file order, 47 units, 45 of them 1-12.  The read lies on the reverse
    strand, so in file order it begins inside a copy and walks down to position 1 (the unit 1-10) and ends with the top of
    one (6-12): the two partial units of the issue, which lists them by their place in the array."""
    cols, mono, _ = golden_columns(os.path.join(GOLDEN, "final", "td_light", "final.tsv"), DXZ1)
    assert len(cols[0]) == 557 and len(mono) == 12
    h = host_equals_ref(cols, 12, what="td_light")
    assert h.kinds.tolist() == [0] and h.lens.tolist() == [12] and h.long == []
    assert h.hor.tolist() == [0] * 12 and h.pos.tolist() == list(range(1, 13))
    names = names_of(h)
    assert len(names) == 47 and collections.Counter(names) == {"1-12": 45, "6-12": 1, "1-10": 1}
    assert names[0] == "1-10" and names[-1] == "6-12" and set(names[1:-1]) == {"1-12"}
    assert all(u[7] == 1 for u in h.units.tolist())


def test_golden_all_rows_reverse_four_monomers():
    d = os.path.join(GOLDEN, "final", "ident_k1")
    cols, mono, _ = golden_columns(os.path.join(d, "final.tsv"), os.path.join(d, "monomers.fa"))
    assert mono == ["M0", "M1", "M2", "M3"] and all(k & 1 for k in cols[3])
    h = host_equals_ref(cols, 4, what="ident_k1")
    assert h.kinds.tolist() == [0] and h.lens.tolist() == [4] and h.pos.tolist() == [1, 2, 3, 4]


def test_golden_filtered_rows_cycle_without_gap_path_with_gap():
    cols, mono, _ = golden_columns(os.path.join(GOLDEN, "final", "td_second_best_i95", "final.tsv"), DXZ1)
    h = host_equals_ref(cols, 12, what="i95 G 0")
    assert h.kinds.tolist() == [0] and h.lens.tolist() == [12] and h.pos.tolist() == list(range(1, 13)) and len(h.units) == 119
    h = host_equals_ref(cols, 12, G=400, what="i95 G 400")
    assert h.kinds.tolist() == [1] and h.lens.tolist() == [9]
    order = sorted((p, mono[m][0]) for m, p in enumerate(h.pos.tolist()) if p)
    assert "".join(x for _, x in order) == "FGHJKACDE"


# ---- planted strings, a clause of the rule each ---------------------------------------------------------------------------
def test_planted_cycle_with_units_that_lack_positions_5_and_6():
    lacking = {c for c in range(100) if c % 10 == 3}
    cols = planted([walk(range(12), 100, skip=lambda c: (5, 6) if c in lacking else ())])
    h = host_equals_ref(cols, 12)
    assert h.kinds.tolist() == [0] and h.lens.tolist() == [12]
    assert collections.Counter(names_of(h)) == {"1-12": 90, "1-4_7-12": 10}
    v = formats.hor_variants(h)
    assert [(x.name, x.units, x.rows, x.bases) for x in v] == [("1-12", 90, 1080, 10800), ("1-4_7-12", 10, 100, 1000)]
    assert int(h.T[3][6]) == 10 and int(h.T[3][4]) == 90


def test_planted_reverse_read_and_a_strand_switch():
    fwd = host_equals_ref(planted([walk(range(5), 6)]), 5)
    rev = host_equals_ref(planted([walk(range(5), 6, strand=1)]), 5)
    assert fwd.T.tolist() == rev.T.tolist() and fwd.pos.tolist() == rev.pos.tolist() == [1, 2, 3, 4, 5]
    assert set(names_of(rev)) == {"1-5"} and all(u[7] == 1 for u in rev.units.tolist()) and all(u[7] == 0 for u in fwd.units.tolist())
    # one read, forward copies then reverse copies: the pair across the switch is not adjacent
    both = host_equals_ref(planted([walk(range(5), 3) + walk(range(5), 3, strand=1)]), 5)
    assert names_of(both) == ["1-5"] * 6 and [u[7] for u in both.units.tolist()] == [0, 0, 0, 1, 1, 1]
    assert int(both.T[4][4]) == 0 and int(both.T.sum()) == 2 * 14


def test_planted_two_cycles_and_a_cycle_of_one():
    h = host_equals_ref(planted([walk([4, 5, 6, 7], 5), walk([2, 0, 1], 5), walk([3], 4)]), 8)
    assert h.kinds.tolist() == [0, 0, 0] and h.lens.tolist() == [3, 1, 4]
    assert h.hor.tolist() == [0, 0, 0, 1, 2, 2, 2, 2] and h.pos.tolist() == [1, 2, 3, 1, 1, 2, 3, 4]   # rotated to the smallest
    assert int(h.T[3][3]) == 3
    by_order = collections.Counter((u[6], formats.hor_mask_name(u[3])) for u in h.units.tolist())
    assert by_order == {(2, "1-4"): 5, (0, "3"): 1, (0, "1-3"): 4, (0, "1-2"): 1, (1, "1"): 4}


def test_planted_unreliable_rows_and_rows_without_a_monomer_split_units():
    rows = walk(range(6), 8)
    rows[8] = (rows[8][0], 0, 0)       # a '?' row at position 3 of the second copy
    rows[22] = (-1, 1, 0)              # best = -1 at position 5 of the fourth copy
    h = host_equals_ref(planted([rows]), 6)
    names = names_of(h)
    assert names[1:3] == ["1-2", "4-6"] and names[4:6] == ["1-4", "6"] and len(names) == 10
    assert h.row_unit[8] == -1 and h.row_unit[22] == -1 and int(h.rows.sum()) == 46


def test_planted_gap_of_one():
    rows = walk(range(4), 6)
    rows[9] = (rows[9][0], 1, 1)       # one base before position 2 of the third copy
    tight = host_equals_ref(planted([rows]), 4, G=0)
    loose = host_equals_ref(planted([rows]), 4, G=1)
    assert names_of(tight) == ["1-4", "1-4", "1", "2-4", "1-4", "1-4", "1-4"] and names_of(loose) == ["1-4"] * 6
    assert int(loose.T[0][1]) == int(tight.T[0][1]) + 1


def test_planted_counts_of_exactly_c_minus_one_and_c():
    cols = planted([walk(range(3), 2)])   # 0 -> 1 and 1 -> 2 twice, 2 -> 0 once
    h = host_equals_ref(cols, 3, C=2)
    assert h.kinds.tolist() == [1] and h.lens.tolist() == [3] and int(h.T[2][0]) == 1
    h = host_equals_ref(cols, 3, C=3)
    assert h.kinds.tolist() == [] and len(h.units) == 0 and h.row_unit.tolist() == [-1] * 6
    h = host_equals_ref(cols, 3, C=1)
    assert h.kinds.tolist() == [0]


def test_planted_ties_in_succ_and_pred():
    pair = lambda a, b: [(2 * a, 1, 0), (2 * b, 1, 0)]   # noqa: E731
    # succ(0): 1 and 2 three times each -> 1; pred(3): 1 and 2 twice each -> 1; so 0 -> 1 -> 3 is kept and 2 hangs off
    reads = [pair(0, 1)] * 3 + [pair(0, 2)] * 3 + [pair(1, 3)] * 2 + [pair(2, 3)] * 2
    h = host_equals_ref(planted(reads), 4)
    assert h.kinds.tolist() == [1] and h.hor.tolist() == [0, 0, -1, 0] and h.pos.tolist() == [1, 2, 0, 3]


def test_planted_orders_of_64_and_65():
    h = host_equals_ref(planted([walk(range(64), 3)]), 64)
    assert h.kinds.tolist() == [0] and h.lens.tolist() == [64] and names_of(h) == ["1-64"] * 3 and h.long == []
    assert int(h.units[0]["mask"]) == (1 << 64) - 1
    h = host_equals_ref(planted([walk(range(65), 3), walk([65, 66], 3)]), 67)
    assert h.long == [(0, 65)] and h.kinds.tolist() == [0] and h.lens.tolist() == [2]
    assert h.hor.tolist() == [-1] * 65 + [0, 0] and set(h.row_unit[:195].tolist()) == {-1} and names_of(h) == ["1-2"] * 3
    path = host_equals_ref(planted([walk(range(70), 2)]), 70)   # never wraps twice: a path of 70 from its head
    assert path.long == [(0, 70)] and path.kinds.tolist() == []


def test_reads_of_no_and_one_row_and_an_empty_job():
    cols = planted([walk(range(3), 4), [], [(2, 1, 0)], [(-1, 1, 0)], [(4, 0, 0)]])
    h = host_equals_ref(cols, 3)
    assert names_of(h) == ["1-3"] * 4 + ["2"] and h.units[-1]["read"] == 2 and h.row_unit.tolist()[-3:] == [4, -1, -1]
    for M in (1, 12):
        h = host_equals_ref(([], [], [], [], []), M)
        assert h.T.shape == (M, M) and not h.T.any() and len(h.units) == 0 and len(h.row_unit) == 0 and h.kinds.tolist() == []


def random_columns(rng, M, n, wander=0.1):
    """label strings that mostly walk 0 .. M - 1 round, with wrong labels, '?', rows without a monomer, gaps and strand
    switches thrown in"""
    reads, left = [], n
    while left > 0:
        k = min(left, int(rng.integers(1, 60)))
        strand, m, rows = int(rng.integers(0, 2)), int(rng.integers(0, M)), []
        for _ in range(k):
            x = rng.random()
            key = 2 * (int(rng.integers(0, M)) if x < wander else m) + strand
            rows.append((-1 if x > 0.98 else key, 0 if 0.9 < x < 0.95 else 1, int(rng.integers(1, 4)) if rng.random() < 0.05 else 0))
            m = (m + (1 if strand == 0 else -1)) % M
            if rng.random() < 0.02:
                strand ^= 1
        reads.append(rows)
        left -= k
    return planted(reads)


@pytest.mark.parametrize("M", [1, 2, 12, 65])
def test_seeded_random_label_strings(M):
    rng = np.random.default_rng(100 + M)
    for t in range(25):
        cols = random_columns(rng, M, int(rng.integers(1, 700)), wander=float(rng.choice([0.0, 0.1, 0.6])))
        h = host_equals_ref(cols, M, G=int(rng.integers(0, 3)), C=int(rng.integers(1, 4)), threads=1 + t % 4, what="M %d case %d" % (M, t))
        assert int(h.T.sum()) <= len(cols[0])


def test_more_rows_than_a_host_block_and_final_rows():
    rng = np.random.default_rng(7)
    cols = random_columns(rng, 12, 70001)
    h = host_equals_ref(cols, 12, threads=4, what="70 001 rows")
    assert len(h.units) > 3000 and h.kinds.tolist() == [0]
    one = lib.hor_rows(*cols, 12, threads=1)
    assert one.units.tobytes() == h.units.tobytes() and one.row_unit.tobytes() == h.row_unit.tobytes()
    rows = np.zeros(len(cols[0]), dtype=lib.final_dtype())
    rows["read"], rows["start"], rows["end"], rows["best"], rows["reliable"] = cols
    f = lib.final_hor_host((rows, None, None), 12, threads=4)
    assert f.units.tobytes() == h.units.tobytes() and f.T.tobytes() == h.T.tobytes() and f.row_unit.tobytes() == h.row_unit.tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,code,text", [
    ({"n_mono": 0}, lib.SD_ERR_PARAM, "n_mono = 0, must be 1 .. 2048"),
    ({"n_mono": -3}, lib.SD_ERR_PARAM, "n_mono = -3"),
    ({"n_mono": 2049}, lib.SD_ERR_UNSUPPORTED, "n_mono = 2049, at most 2048"),
    ({"G": -1}, lib.SD_ERR_PARAM, "G = -1, must be 0 or more"),
    ({"C_": 0}, lib.SD_ERR_PARAM, "C = 0, must be 1 or more"),
    ({"key": [0, 6, 2]}, lib.SD_ERR_PARAM, "key 6 of row 1 lies outside -1 .. 5"),
    ({"key": [0, 1, -2]}, lib.SD_ERR_PARAM, "key -2 of row 2 lies outside -1 .. 5"),
    ({"cap_units": 1}, lib.SD_ERR_PARAM, "2 units, cap_units is 1"),
    ({"G": 1.5}, lib.SD_ERR_PARAM, "G = 1.5, must be an integer"),
    ({"usable": [1, 1]}, lib.SD_ERR_PARAM, "differ in length"),
])
def test_refusals(kw, code, text):
    args = dict(read=[0, 0, 1], start=[0, 10, 0], end=[9, 19, 9], key=[0, 2, 0], usable=[1, 1, 1], n_mono=3, G=0, C_=1)
    args.update(kw)
    for call in (lib.hor_rows,):
        with pytest.raises(lib.SdError) as e:
            call(**args)
        assert e.value.code == code and text in e.value.msg, e.value.msg
    if "key" in kw:
        rows = np.zeros(3, dtype=lib.final_dtype())
        rows["best"], rows["reliable"] = kw["key"], 1
        with pytest.raises(lib.SdError) as e:
            lib.final_hor_host((rows, None, None), 3)
        assert e.value.code == code and text in e.value.msg and "sd_hor_final_host" in e.value.msg


def test_a_refused_capacity_leaves_everything_but_the_units():
    cols = planted([walk(range(3), 4)])
    full = lib.hor_rows(*cols, 3)
    assert len(full.units) == 4 and len(lib.hor_rows(*cols, 3, cap_units=4).units) == 4
    with pytest.raises(lib.SdError) as e:
        lib.hor_rows(*cols, 3, cap_units=3)
    assert e.value.code == lib.SD_ERR_PARAM and "4 units" in e.value.msg


# ---- names, files -------------------------------------------------------------------------------------------------------
def test_names_of_masks():
    rng = np.random.default_rng(3)
    masks = [1, 1 << 63, (1 << 64) - 1, 0xFFF, 0xFCF, 0xFE0, 4, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA]
    masks += [int(x) for x in rng.integers(1, 1 << 63, 200, dtype=np.uint64)] + [int(x) for x in rng.integers(1, 1 << 12, 100)]
    for m in masks:
        assert lib.hor_name(m) == ref.name(m) == formats.hor_mask_name(m), hex(m)
        assert formats.hor_mask_of(ref.name(m)) == m
    assert (lib.hor_name(0xFFF), lib.hor_name(0xFCF), lib.hor_name(0xFE0), lib.hor_name(4)) == ("1-12", "1-4_7-12", "6-12", "3")
    assert len(lib.hor_name(0x5555555555555555)) < lib.HOR_NAME_MAX - 1


def test_formats_round_trip_and_variants_sum_to_the_units(tmp_path):
    rng = np.random.default_rng(21)
    cols = random_columns(rng, 12, 4000)
    h = host_equals_ref(cols, 12)
    reads = ["read_%d" % r for r in range(max(cols[0]) + 1)]
    monos = ["m%d" % m for m in range(12)]
    units, orders, variants = formats.hor_units(h, reads), formats.hor_orders(h, monos), formats.hor_variants(h)
    assert len(units) == len(h.units) > 100 and len(orders) == 12 and len(variants) > 5
    for name, rows, fmt, write, read in (("u", units, formats.format_hor, formats.write_hor, formats.read_hor),
                                         ("o", orders, formats.format_hor_orders, formats.write_hor_orders, formats.read_hor_orders),
                                         ("v", variants, formats.format_hor_variants, formats.write_hor_variants, formats.read_hor_variants)):
        fn = str(tmp_path / name)
        write(fn, rows)
        back = read(fn)
        assert back == rows and fmt(back) == open(fn, newline="").read()
    # the lines against the restatement: units in file order, variants in its order
    exp = ref.analyse(*cols, 12)
    assert [(u.read, u.start, u.end, u.strand, u.order, u.name, u.rows) for u in units] == [
        (reads[r], s, e, "+-"[st], "H%d" % (o + 1), ref.name(m), k) for _, s, e, m, r, k, o, st in exp["units"]]
    assert [u.complete for u in units] == [int(m == 0xFFF) for _, _, _, m, *_ in exp["units"]]
    assert [(v.order, v.name, v.units, v.rows, v.bases) for v in variants] == [
        ("H%d" % (o + 1), ref.name(m), a, b, c) for o, m, a, b, c in ref.variants(exp["units"])]
    assert sum(v.units for v in variants) == len(units) and sum(v.rows for v in variants) == sum(u.rows for u in units)
    assert sum(v.bases for v in variants) == sum(u.end - u.start + 1 for u in units)
    # the orders file: the monomers by position, their usable rows, the edge to the next position (the wrap of a cycle)
    assert [o.monomer for o in orders] == monos and [o.rows for o in orders] == exp["rows"]
    assert [o.count for o in orders] == [exp["T"][m][(m + 1) % 12] for m in range(12)] and {o.kind for o in orders} == {"cycle"}
    with open(str(tmp_path / "bad"), "w") as f:
        f.write("r\t0\t9\t+\tH1\t2-1\t1\t0\n")
    with pytest.raises(formats.FormatError):
        formats.read_hor(str(tmp_path / "bad"))


def test_orders_file_of_a_path_ends_with_a_count_of_zero():
    h = host_equals_ref(planted([walk([2, 0, 1], 2)]), 3)   # 2 -> 0 -> 1 twice, 1 -> 2 once
    rows = formats.hor_orders(h, ["a", "b", "c"])
    assert [(r.kind, r.position, r.monomer, r.count) for r in rows] == [("path", 1, "c", 2), ("path", 2, "a", 2), ("path", 3, "b", 0)]


# ---- the command line's refusals need no device -----------------------------------------------------------------------------
def cli(*extra, monomers=DXZ1, env=None):
    cmd = [sys.executable, "-m", "stringdecomposer_amd.main", os.path.join(TD, "read.fa"), monomers] + list(extra)
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("extra,word", [(["--hor", "--hor-gap", "-1"], "--hor-gap -1"), (["--hor", "--hor-min-count", "0"], "--hor-min-count 0"),
                                        (["--hor", "--records"], "--records")])
def test_command_line_refusals_need_no_device(tmp_path, extra, word):
    r = cli("-o", str(tmp_path), *extra)
    assert r.returncode == 2 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert not os.listdir(str(tmp_path))


def test_command_line_refuses_a_distributed_launch_and_a_repeated_name(tmp_path):
    r = cli("-o", str(tmp_path / "o"), "--hor", env=dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 2 and "torch.distributed" in r.stderr
    twice = str(tmp_path / "twice.fa")
    with open(twice, "w") as f:
        f.write(">a\nACGTACGTAC\n>b\nACGTTTGTAC\n>a\nACGAACGTAC\n")
    r = cli("-o", str(tmp_path / "o"), "--hor", monomers=twice)
    assert r.returncode == lib.SD_ERR_PARAM and "not unique" in r.stderr
