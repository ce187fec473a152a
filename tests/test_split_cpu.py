"""The subfamilies of a monomer's instances (--split) without a device: the host form (sd_split_host) against the numpy
restatement of tests/split_ref.py, every tie rule, the caps and limits of the procedure, members and non-members of a
job's rows, the file formats, the consensus of a subfamily against --profile's, and the planted classes of the issue."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import split_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
NEW = ["sd_split_host", "sd_split_dev", "sd_split_final_host", "sd_split_info", "sd_split_kernel_bench"]


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    info = lib.split_info()
    assert (info["kmax"], info["lmax"], info["nmax"]) == (lib.SPLIT_KMAX, lib.SPLIT_LMAX, lib.SPLIT_NMAX) == (64, 512, 1 << 26)
    assert "#define SD_SPLIT_KMAX 64" in header and "#define SD_SPLIT_LMAX 512" in header


def as_split(d):
    return formats.Split(d["centres"], d["assign"], d["d1"], d["d2"], d["sizes"], d["rounds"], d["iters"])


def same_split(a, b, what=""):
    assert a.centres.shape == b.centres.shape, "%s: %d centres against %d" % (what, len(a.centres), len(b.centres))
    for name in ("centres", "assign", "d1", "d2", "sizes"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), "%s: %s differs" % (what, name)
    assert (a.rounds, a.iters) == (b.rounds, b.iters), what


def host_equals_ref(sym, R, K=64, S=8, I=16, threads=3, trace=None):
    got = lib.split_rows(sym, R, K, S, I, threads=threads)
    same_split(got, as_split(ref.split(sym, R, K, S, I, trace=trace)), "n %d L %d R %d K %d S %d I %d" % (sym.shape + (R, K, S, I)))
    return got


def test_host_equals_reference_on_random_rows():
    rng = np.random.default_rng(5)
    for t in range(120):
        n = int(rng.integers(1, 40))
        L = int(rng.choice([1, 2, 5, 63, 64, 65, 130, 513]))
        sym = rng.integers(0, 6 if t % 2 else 2, (n, L)).astype(np.uint8)
        host_equals_ref(sym, int(rng.integers(1, max(2, L // 2 + 1))), int(rng.integers(1, 8)), int(rng.integers(1, 5)),
                        int(rng.integers(1, 4)), threads=1 + t % 4)


@pytest.mark.parametrize("L,n", [(64, 90), (171, 150), (513, 60)])
def test_host_equals_reference_on_planted_rows(L, n):
    rng = np.random.default_rng(L)
    sym, _ = ref.planted(rng, 3, n // 3 - 2, L, 0.25, 0.04, junk=6)
    got = host_equals_ref(sym, lib.split_radius(12, L), 64, 4, 6)
    assert len(got.centres) >= 3 and got.rounds > len(got.centres) - 1, "junk rows were tried and rejected"


def test_radius_of_a_percentage():
    assert [lib.split_radius(p, L) for p, L in ((1, 1), (12, 171), (15, 171), (100, 171), (1, 50), (1, 101))] == [1, 21, 26, 171, 1, 2]


def test_column_mode_ties_go_to_the_smallest_code():
    # column 0: T and C twice each -> C; column 1: DEL and N once each, A never -> N; column 2: all six once -> A
    sym = np.array([[3, 5, 0, 1, 2, 3], [1, 4, 1, 1, 2, 3], [3, 2, 2, 1, 2, 3], [1, 2, 3, 1, 2, 3], [0, 3, 4, 1, 2, 3], [2, 3, 5, 1, 2, 3]], dtype=np.uint8)
    sym[:, 1] = [5, 4, 5, 4, 0, 0]
    got = host_equals_ref(sym, 6, S=1)
    assert len(got.centres) == 1 and got.centres[0].tolist() == [1, 0, 0, 1, 2, 3]
    sym[:, 1] = [5, 4, 5, 4, 3, 2]
    assert lib.split_rows(sym, 6).centres[0].tolist() == [1, 4, 0, 1, 2, 3]


def test_assignment_ties_go_to_the_smallest_centre():
    a, b, t = [0] * 8, [1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0]   # t is 2 columns from a and 2 from b
    sym = np.array([a] * 10 + [b] * 10 + [t] * 3, dtype=np.uint8)
    got = host_equals_ref(sym, 2, K=3, S=8)
    assert len(got.centres) == 2 and got.centres[0].tolist() == b and got.centres[1].tolist() == a
    assert got.assign[20:].tolist() == [0, 0, 0] and got.d1[20:].tolist() == [2, 2, 2] and got.d2[20:].tolist() == [2, 2, 2]
    # the same rows with a first: a is seeded from the first row either way, the tie still goes to index 0
    sym2 = np.array([b] * 10 + [a] * 10 + [t] * 3, dtype=np.uint8)
    got2 = host_equals_ref(sym2, 2, K=3, S=8)
    assert got2.centres[0].tolist() == a and got2.centres[1].tolist() == b and got2.assign[20:].tolist() == [0, 0, 0]


def test_seed_tie_goes_to_the_smallest_row():
    x, y = [1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 1, 1]   # both 4 columns from the mode of all
    for first, second in ((x, y), (y, x)):
        sym = np.array([[0] * 8] * 5 + [first] + [[0] * 8] * 5 + [second], dtype=np.uint8)
        trace = []
        got = host_equals_ref(sym, 4, K=2, S=1, trace=trace)
        assert trace[0][:3] == (5, 4, "kept") and got.centres[1].tolist() == first and got.assign[5] == 1 and got.assign[11] == 0


def test_radius_above_every_distance_gives_one_subfamily():
    rng = np.random.default_rng(3)
    sym, _ = ref.planted(rng, 3, 20, 65, 0.3, 0.05)
    far = int(lib.split_rows(sym, 65).d1.max())
    got = host_equals_ref(sym, far + 1)
    assert len(got.centres) == 1 and got.rounds == 0 and (got.d2 == -1).all() and got.sizes.tolist() == [60]
    assert len(lib.split_rows(sym, far, min_size=1).centres) > 1


def test_cap_on_subfamilies_is_honoured():
    rng = np.random.default_rng(4)
    sym, label = ref.planted(rng, 5, 20, 100, 0.3, 0.02)
    assert len(host_equals_ref(sym, 12, K=64).centres) == 5
    for K in (1, 2, 3):
        got = host_equals_ref(sym, 12, K=K)
        assert len(got.centres) == K and int(got.assign.max()) == K - 1


def test_rejected_round_restores_the_state_and_retires_only_its_seed():
    rng = np.random.default_rng(8)
    sym, _ = ref.planted(rng, 2, 30, 80, 0.3, 0.03)
    junk = np.full((1, 80), 5, dtype=np.uint8)   # a row of deletions: farther from everything than any planted row
    sym = np.concatenate([sym[:17], junk, sym[17:]])
    trace = []
    got = host_equals_ref(sym, 10, S=8, trace=trace)
    assert [t[2] for t in trace[:2]] == ["rejected", "kept"] and trace[0][0] == 17 and trace[0][3] < 8
    assert len(got.centres) == 2 and got.rounds == len(trace)
    # what the junk row left behind: nothing -- without it the other rows get the same centres and distances
    rest = lib.split_rows(np.delete(sym, 17, axis=0), 10, min_size=8)
    assert np.array_equal(rest.centres, got.centres) and np.array_equal(rest.assign, np.delete(got.assign, 17))
    assert np.array_equal(rest.d1, np.delete(got.d1, 17))


def test_a_cluster_emptied_by_lloyd_keeps_its_centre(monkeypatch):
    rng = np.random.default_rng(1082)
    n, L = int(rng.integers(6, 14)), int(rng.integers(3, 7))
    sym = rng.integers(0, 2, (n, L)).astype(np.uint8)
    I = int(rng.integers(1, 3))
    emptied, plain = [], ref.lloyd_modes

    def spy(rows, a, centres):
        emptied.extend(c for c in range(len(centres)) if not (a == c).any())
        return plain(rows, a, centres)
    monkeypatch.setattr(ref, "lloyd_modes", spy)
    host_equals_ref(sym, 1, K=6, S=1, I=I)
    assert emptied, "this input empties a cluster during a Lloyd iteration"


def test_round_limit():
    sym = np.full((32, 40), 4, dtype=np.uint8)
    for i in range(12):   # twelve rows 3 columns from the rest and 6 from each other: every one is tried alone and rejected
        sym[20 + i, 3 * i:3 * i + 3] = 0
    got = host_equals_ref(sym, 3, K=2, S=2)
    assert got.rounds == 8 and len(got.centres) == 1, "4 K rounds, every one rejected"
    got = host_equals_ref(sym, 3, K=4, S=2)
    assert got.rounds == 12 and len(got.centres) == 1, "the candidates ran out before 4 K = 16 rounds"


def test_empty_and_single():
    got = lib.split_rows(np.zeros((0, 7), dtype=np.uint8), 1)
    assert got.centres.shape == (0, 7) and len(got.assign) == 0 and got.rounds == 0
    got = host_equals_ref(np.array([[5, 4, 3, 2, 1, 0]], dtype=np.uint8), 1)
    assert got.centres.tolist() == [[5, 4, 3, 2, 1, 0]] and got.assign.tolist() == [0] and got.d1.tolist() == [0] and got.d2.tolist() == [-1]


def test_refusals():
    sym = np.zeros((4, 5), dtype=np.uint8)
    for kw in ({"R": 0}, {"K": 0}, {"K": 65}, {"min_size": 0}, {"max_iter": 0}, {"R": True}):
        args = dict(R=1, K=4, min_size=1, max_iter=1)
        args.update(kw)
        with pytest.raises(lib.SdError) as e:
            lib.split_rows(sym, args["R"], args["K"], args["min_size"], args["max_iter"])
        assert e.value.code == lib.SD_ERR_PARAM
    with pytest.raises(lib.SdError):
        lib.split_rows(np.full((2, 3), 6, dtype=np.uint8), 1)
    with pytest.raises(lib.SdError):
        lib.split_msa(formats.Msa(np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.uint8), [5]), [], [5], 0)


def handmade_msa(rng, lens, n):
    """rows of two monomers on both strands with N and deleted columns, a third of them status 0 or 2"""
    pt = rng.integers(0, 2 * len(lens), n).astype(np.int32)
    at = np.zeros(n + 1, dtype=np.int64)
    for i, il in enumerate(pt):
        at[i + 1] = at[i] + formats.msa_pitch(lens[il >> 1])
    rows = np.zeros(int(at[-1]), dtype=np.uint8)
    status = np.where(rng.random(n) < 0.33, rng.choice([0, 2], n), 1).astype(np.uint8)
    variants = [[rng.integers(0, 4, L) for _ in range(2)] for L in lens]
    for i, il in enumerate(pt):
        L = lens[il >> 1]
        x = variants[il >> 1][int(rng.integers(0, 2))].copy()
        e = rng.random(L) < 0.05
        x[e] = rng.integers(0, 6, int(e.sum()))
        rows[at[i]:at[i] + L] = x if status[i] == 1 else formats.MSA_NONE
        rows[at[i] + L:at[i] + 2 * L + 1] = rng.integers(0, 3, L + 1) * (rng.random(L + 1) < 0.1)   # insertions: no part of the distance
    return formats.Msa(rows, at, status, list(lens)), pt


def test_members_of_a_job_and_the_rows_that_are_none():
    rng = np.random.default_rng(12)
    lens = [70, 33]
    msa, pt = handmade_msa(rng, lens, 200)
    splits = lib.split_msa(msa, pt, lens, 15, K=8, min_size=4, max_iter=6, threads=2)
    job = lib.final_split_host(msa, pt, lens, 15, K=8, min_size=4, max_iter=6, threads=2)
    member = msa.status == 1
    assert (job.sub[~member] == -1).all() and (job.d1[~member] == -1).all() and (job.d2[~member] == -1).all()
    assert {0, 2} <= set(msa.status[~member].tolist()) and {int(x) & 1 for x in pt[member]} == {0, 1}
    for m, sp in enumerate(splits):
        pick = formats.split_members(msa, pt, m)
        sym = formats.msa_matrix(msa, pt, m)
        assert len(pick) == len(sym) > 20 and (sym >= 4).any()
        same_split(sp, as_split(ref.split(sym, lib.split_radius(15, lens[m]), 8, 4, 6)), "monomer %d" % m)
        assert len(sp.centres) >= 2
        assert np.array_equal(job.sub[pick], sp.assign) and np.array_equal(job.d1[pick], sp.d1) and np.array_equal(job.d2[pick], sp.d2)
        assert np.array_equal(job.centres[job.cen_off[m]:job.cen_off[m + 1]].reshape(-1, lens[m]), sp.centres)
        assert job.info[m].tolist() == [len(pick), len(sp.centres), sp.rounds, sp.iters]
        assert job.sizes[m, :len(sp.centres)].tolist() == sp.sizes.tolist()


def test_formats_round_trip(tmp_path):
    rng = np.random.default_rng(13)
    lens = [40, 25]
    msa, pt = handmade_msa(rng, lens, 120)
    names = ["mA", "mB"]
    splits = lib.split_msa(msa, pt, lens, 15, K=8, min_size=4, max_iter=6)
    meta = [("read%d" % (i // 50), 10 * i, 10 * i + 8, names[il >> 1] + ("'" if il & 1 else "")) for i, il in enumerate(pt)]
    rows = formats.split_rows(msa, pt, names, splits, meta)
    assert len(rows) == 120 and sum(r.subfamily == "*" for r in rows) == int((msa.status != 1).sum())
    for r, i in ((r, i) for i, r in enumerate(rows) if r.subfamily != "*"):
        assert r.subfamily.startswith(names[pt[i] >> 1] + ".") and r.d1 >= 0 and set(r.columns) <= set("ACGTN-")
    p = str(tmp_path / "x_split.tsv")
    formats.write_split(p, rows)
    assert formats.read_split(p) == rows and formats.format_split(formats.read_split(p)) == open(p).read()
    summary = formats.split_summary(names, splits)
    assert len(summary) == sum(len(s.centres) for s in splits)
    for x in summary:
        mine = [r for r in rows if r.subfamily == x.subfamily]
        assert (x.size, x.sum_d1, x.max_d1) == (len(mine), sum(r.d1 for r in mine), max(r.d1 for r in mine))
        m, j = names.index(x.monomer), int(x.subfamily.rsplit(".", 1)[1])
        others = [(ref.hamming(splits[m].centres[j], c), o) for o, c in enumerate(splits[m].centres) if o != j]
        assert (x.nearest, x.distance) == ("%s.%d" % (x.monomer, min(others)[1]), min(others)[0])
    p = str(tmp_path / "x_split_summary.tsv")
    formats.write_split_summary(p, summary)
    assert formats.read_split_summary(p) == summary
    with open(p, "a") as f:
        f.write("only\tthree\tcolumns\n")
    with pytest.raises(formats.FormatError):
        formats.read_split_summary(p)


RC = {"A": "T", "C": "G", "G": "C", "T": "A"}


def mutate(rng, s, sub, indel):
    out = []
    for ch in s:
        x = rng.random()
        if x < indel / 2:
            continue
        if x < indel:
            out.append(str(rng.choice(list("ACGT"))))
        out.append(str(rng.choice(list("ACGT"))) if rng.random() < sub else ch)
    return "".join(out)


def test_split_consensus_equals_the_consensus_of_the_profile_of_the_same_rows():
    rng = np.random.default_rng(14)
    monos = ["".join(rng.choice(list("ACGT"), L)) for L in (90, 60)]
    variants = []
    for m in monos:   # the second variant of a monomer carries an insertion that most of its instances keep
        v = [RC[c] if rng.random() < 0.25 else c for c in m]
        v.insert(len(v) // 2, "G")
        v.insert(len(v) // 2, "T")
        variants.append("".join(v))
    text, st, en, pt = [], [], [], []
    at = 0
    for i in range(160):
        m, rc = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        s = mutate(rng, (monos, variants)[int(rng.integers(0, 2))][m], 0.02, 0.02)
        s = "".join(RC[c] for c in reversed(s)) if rc else s
        text.append(s)
        st.append(at)
        en.append(at + len(s) - 1)
        pt.append(2 * m + rc)
        at += len(s)
    text = "".join(text)
    msa = lib.msa_segments(text, st, en, monos, pt, threads=2)
    assert (msa.status == 1).all()
    splits = lib.split_msa(msa, pt, [len(m) for m in monos], 12, K=8, min_size=4, max_iter=6)
    inserted = {i: formats.msa_inserted(msa, i, pt[i], text[st[i]:en[i] + 1]) for i in range(len(pt))}
    assert all(v is not None for v in inserted.values()) and sum(bool(v) for v in inserted.values()) > 40
    grew = 0
    for m, sp in enumerate(splits):
        assert len(sp.centres) >= 2
        got = formats.split_consensus(msa, pt, m, "m%d" % m, monos[m], sp, inserted)
        pick = formats.split_members(msa, pt, m)
        for j in range(len(sp.centres)):
            rows = [i for x, i in enumerate(pick) if sp.assign[x] == j]
            counts = lib.profile_segments(text, [st[i] for i in rows], [en[i] for i in rows], monos, [pt[i] for i in rows], threads=2)
            prof = formats.Profile(["m%d.%d" % (m, j)], [monos[m]], [counts[m]])
            assert np.array_equal(formats.split_profile(msa, pt, m, "m%d" % m, monos[m], sp, inserted).counts[j], counts[m])
            assert got[j] == formats.consensus(prof)[0]
            grew += len(got[j][2]) > len(monos[m])
    assert grew >= 2, "the variants' insertions reach their consensus"
    assert formats.split_consensus(msa, pt, 0, "x", "ACGT", formats.Split(np.zeros((0, 4), np.uint8), [], [], [], [], 0, 0)) == [("x.0", 0, "ACGT")]


def test_planted_classes_are_recovered():
    """the condition of the issue: 4 classes x 60 rows, L = 171, 20 % divergence, 5 % noise, P = 15, S = 8"""
    rng = np.random.default_rng(171)
    sym, label = ref.planted(rng, 4, 60, 171, 0.20, 0.05)
    got = host_equals_ref(sym, lib.split_radius(15, 171), 64, 8, 16)
    assert lib.split_radius(15, 171) == 26
    for c in range(len(got.centres)):
        assert len(set(label[got.assign == c].tolist())) <= 1, "cluster %d mixes classes" % c
    assert len(got.centres) >= 4


def cli(*extra):
    cmd = [sys.executable, "-m", "stringdecomposer_amd.main", os.path.join(TD, "read.fa"), os.path.join(TD, "DXZ1_star_monomers.fa")]
    return subprocess.run(cmd + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("extra,word", [(["--split", "0"], "1 <= P <= 100"), (["--split", "12,65"], "1 <= K <= 64"),
                                        (["--split", "x"], "expected P or P,K"), (["--split", "12", "--split-min-size", "0"], "--split-min-size"),
                                        (["--split", "12", "--split-iters", "0"], "--split-iters"),
                                        (["--split", "12", "--records"], "--records")])
def test_command_line_refusals_need_no_device(tmp_path, extra, word):
    r = cli("-o", str(tmp_path), *extra)
    assert r.returncode == 2 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert not os.listdir(str(tmp_path))


def test_command_line_refuses_a_distributed_launch_and_a_repeated_name(tmp_path):
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    cmd = [sys.executable, "-m", "stringdecomposer_amd.main", os.path.join(TD, "read.fa"), os.path.join(TD, "DXZ1_star_monomers.fa"),
           "-o", str(tmp_path / "o"), "--split", "12"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "torch.distributed" in r.stderr
    twice = str(tmp_path / "twice.fa")
    with open(twice, "w") as f:
        f.write(">a\nACGTACGTAC\n>a\nACGTTCGTAC\n")
    cmd[4] = twice
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == lib.SD_ERR_PARAM and "not unique" in r.stderr
