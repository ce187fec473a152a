"""One row per instance (--msa) without a device: the host form (sd_msa_segments) against a Python fold of edlib's
paths written from the layout in include/sd_hip.h (tests/msa_ref.py), the rows summed per monomer against the profile
of the same pairs, the file format, and the rows of final-mode jobs (lib.final_msa_host) over the reference's goldens."""
import os
import re

import numpy as np
import pytest

import msa_cases
import msa_ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINAL = os.path.join(GOLDEN, "final")
NEW = ["sd_msa_row_offsets", "sd_msa_segments", "sd_msa_segments_dev", "sd_msa_final_size_dev", "sd_msa_final_write_dev"]


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert re.search(r"#define\s+SD_MSA_DEL\s+5\b", header) and formats.MSA_DEL == 5
    assert re.search(r"#define\s+SD_MSA_NONE\s+7\b", header) and formats.MSA_NONE == 7
    assert re.search(r"#define\s+SD_MSA_PITCH\(L\)\s+\(\(2 \* \(L\) \+ 1 \+ 15\) & ~15\)", header)


def test_row_offsets_against_pitch():
    tlen = [1, 63, 64, 65, 171, 512, 7, 8]
    for L in tlen:
        assert formats.msa_pitch(L) == msa_ref.pitch(L) == (2 * L + 1 + 15) // 16 * 16
        assert formats.msa_pitch(L) >= 2 * L + 1 and formats.msa_pitch(L) % 16 == 0
    pt = [0, 1, 15, 4, 9, 8, 10, 2, 3, 12, 14, 11]
    at = lib.msa_row_offsets(tlen, pt)
    assert at[0] == 0 and len(at) == len(pt) + 1
    assert [int(x) for x in np.diff(at)] == [msa_ref.pitch(tlen[p >> 1]) for p in pt]
    assert lib.msa_row_offsets(tlen, []).tolist() == [0]
    with pytest.raises(lib.SdError) as e:
        lib.msa_row_offsets(tlen, [0, 16])
    assert e.value.code == lib.SD_ERR_PARAM


def _check_counts(msa, pt, monos, prof):
    """formats.msa_counts against the profile of the same pairs: columns 0..6, and ins_bases where no count saturated"""
    cnt = formats.msa_counts(msa, pt, len(monos))
    sat = [np.zeros(len(m) + 1, dtype=bool) for m in monos]
    for i, il in enumerate(pt):
        sat[il >> 1] |= formats.msa_row(msa, i, il)[1] == 255
    for c, p, s in zip(cnt, prof, sat):
        assert c.shape == (p.shape[0], 8)
        assert (c[:, :7] == p[:, :7]).all()
        assert (c[~s, 7] == p[~s, 7:12].sum(axis=1)).all()
        assert (c[s, 7] <= p[s, 7:12].sum(axis=1)).all()
    return sat


def test_host_rows_equal_python_fold_on_the_edges():
    seq, st, en, pt, monos, named = msa_cases.edges(extra_byte="R")
    msa = lib.msa_segments(seq, st, en, monos, pt, threads=3)
    msa_ref.same(msa, msa_ref.segments(seq, st, en, monos, pt))
    L = len(monos[1])
    row = lambda what: formats.msa_row(msa, named[what], pt[named[what]])   # noqa: E731
    # the edges are where they were meant to be (forward coordinates)
    assert row("ins_slot_0")[1][0] == 5 and row("ins_slot_0_rc")[1][L] == 5
    assert row("ins_slot_L")[1][L] == 5 and row("ins_slot_L_rc")[1][0] == 5
    assert row("del_first")[0][0] == formats.MSA_DEL and row("del_first_rc")[0][L - 1] == formats.MSA_DEL
    assert row("del_last")[0][L - 1] == formats.MSA_DEL and row("del_last_rc")[0][0] == formats.MSA_DEL
    for w in ("ins_300", "ins_300_rc"):
        assert row(w)[1][80] == 255 and int(row(w)[1].sum()) == 255
    assert (row("with_N")[0] == 4).sum() == 3 and (row("with_N_rc")[0] == 4).sum() == 3
    assert row("other_byte")[0][50] == 4
    assert en[named["one_base"]] == st[named["one_base"]] and msa.status[named["one_base"]] == 1
    e = named["empty"]
    assert msa.status[e] == 0 and (row("empty")[0] == formats.MSA_NONE).all() and not row("empty")[1].any()
    assert all(int(s) == 1 for i, s in enumerate(msa.status) if i != e)
    for i, il in enumerate(pt):   # padding
        assert not msa.rows[int(msa.row_at[i]) + 2 * len(monos[il >> 1]) + 1:int(msa.row_at[i + 1])].any()
    a, b = (formats.msa_row(msa, named["exact"], 2)[0], formats.msa_row(msa, named["exact_rc"], 3)[0])
    assert (a == b).all() and "".join("ACGT"[v] for v in a) == monos[1]   # either orientation lands on the forward monomer
    sat = _check_counts(msa, pt, monos, lib.profile_segments(seq, st, en, monos, pt, threads=3))
    assert sat[1][80] and sum(int(s.sum()) for s in sat) == 1
    mat = formats.msa_matrix(msa, pt, 1)
    assert mat.shape == (sum(1 for i, p in enumerate(pt) if p >> 1 == 1 and msa.status[i] == 1), L)
    assert (mat[0] == a).all()


@pytest.mark.parametrize("lengths,n_seg,alphabet", [((171,) * 12, 120, "ACGTN"), ((1, 63, 64, 65), 120, "ACGTN"),
                                                    ((130, 200), 60, "ACGTNRy")],
                         ids=["12x171", "1_63_64_65", "other_bytes"])
def test_host_rows_equal_python_fold_on_mutated_instances(lengths, n_seg, alphabet):
    monos = [msa_cases.random_monomer(n, 100 + i) for i, n in enumerate(lengths)]
    seq, st, en, pt = msa_cases.segments(monos, n_seg, seed=len(lengths), max_extra=12, alphabet=alphabet)
    one = lib.msa_segments(seq, st, en, monos, pt, threads=1)
    msa_ref.same(one, msa_ref.segments(seq, st, en, monos, pt))
    many = lib.msa_segments(seq, st, en, monos, pt, threads=5)
    assert (many.rows == one.rows).all() and (many.status == one.status).all()
    assert {0, 1} == {p & 1 for p in pt}
    _check_counts(one, pt, monos, lib.profile_segments(seq, st, en, monos, pt, threads=2))


def test_write_read_round_trip(tmp_path):
    seq, st, en, pt, monos, named = msa_cases.edges()
    msa = lib.msa_segments(seq, st, en, monos, pt)
    names = ["m%d" % i for i in range(len(monos))]
    meta = [("read/%d" % (i % 3), s, e, names[p >> 1] + ("'" if p & 1 else "")) for i, (s, e, p) in enumerate(zip(st, en, pt))]
    rows = formats.msa_rows(msa, pt, meta)
    assert rows[named["empty"]].columns == "." * len(monos[1]) and rows[named["empty"]].insertions == ()
    assert rows[named["ins_300"]].insertions == ((80, 255),)
    assert rows[named["del_first"]].columns == "-" + monos[1][1:]
    path = str(tmp_path / "x_msa.tsv")
    formats.write_msa(path, rows)
    text = open(path).read()
    assert text.startswith("read\tstart\tend\tmonomer\tcolumns\tinsertions\n") and text.count("\n") == len(rows) + 1
    back = formats.read_msa(path)
    assert back == rows
    again, pt2 = formats.msa_from_rows(back, names, [len(m) for m in monos])
    assert pt2 == list(pt)
    assert (again.rows == msa.rows).all() and (again.row_at == msa.row_at).all() and (again.status == msa.status).all()
    with open(path, "a") as f:
        f.write("r\t1\t2\tm0\tAC?\t.\n")
    with pytest.raises(formats.FormatError):
        formats.read_msa(path)


def _fasta(path):
    names, seqs, _ = lib.fasta_load(path)
    return [n.split()[0] for n in names], [s.decode().upper() for s in seqs]


@pytest.mark.parametrize("case,reads_fa,mono_fa", [
    ("td_light", os.path.join(GOLDEN, "test_data", "read.fa"), os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa")),
    ("syn64_second_best", os.path.join(FINAL, "syn64_second_best", "reads.fa"),
     os.path.join(FINAL, "syn64_second_best", "monomers.fa"))], ids=["td_light", "syn64_second_best"])
def test_final_msa_host_over_golden_rows(case, reads_fa, mono_fa):
    rn, rs = _fasta(reads_fa)
    mn, ms = _fasta(mono_fa)
    tsv = os.path.join(FINAL, case, "final.tsv")
    final, keys = msa_ref.final_rows_of_tsv(tsv, rn, mn, lib.final_dtype())
    msa, pt = lib.final_msa_host(final, rs, keys, mn, ms, threads=4)
    assert len(pt) == len(final[0]) > 100
    msa_ref.same(msa, msa_ref.of_final(tsv, dict(zip(rn, rs)), mn, ms))
    assert set(msa.status.tolist()) <= {0, 1}


def test_repeated_monomer_name_is_refused():
    mn, ms = synth.make_monomers(3, seed=2)
    mn = [mn[0], mn[1], mn[0]]
    rows = np.zeros(0, dtype=lib.final_dtype())
    with pytest.raises(lib.SdError) as e:
        lib.final_msa_host((rows, np.zeros(2, dtype=np.int64), None), [b"ACGT"], [mn[0], mn[0] + "'"], mn, ms)
    assert e.value.code == lib.SD_ERR_PARAM and "a row's key must name one template" in e.value.msg


def _cli(args, env_extra=None):
    import subprocess
    import sys
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer")] + args, env=env,
                          capture_output=True, text=True, timeout=120)


def test_cli_msa_refusals_come_before_any_work(tmp_path):
    m = tmp_path / "m.fa"
    m.write_text(">x\nACGTACGT\n>y\nTTGACCA\n>x\nGGGACT\n")
    r = tmp_path / "r.fa"
    r.write_text(">r\nACGTACGTTTGACCA\n")
    p = _cli([str(r), str(m), "-o", str(tmp_path / "out"), "--msa"])
    assert p.returncode == lib.SD_ERR_PARAM
    err = p.stderr.strip().splitlines()
    assert len(err) == 1 and "--msa" in err[0] and "not unique" in err[0] and "a row's key must name one template" in err[0]
    assert not (tmp_path / "out" / "final_decomposition.tsv").exists()
    m.write_text(">x\nACGTACGT\n")
    p = _cli([str(r), str(m), "-o", str(tmp_path / "out"), "--msa"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2
    err = p.stderr.strip().splitlines()
    assert len(err) == 1 and "torch.distributed" in err[0] and "--msa" in err[0]
    h = _cli(["--help"])
    assert h.returncode == 0 and "--msa" in h.stdout and "255" in " ".join(h.stdout.split())
