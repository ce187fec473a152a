"""CPU checks of the column profiles (--profile): the host form of sd_profile_segments against a Python fold of edlib's
paths, the invariants of the counters, the consensus rules, and the command line's refusals (which come before any
work on a GPU).  No device compute happens here."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import profile_ref
from stringdecomposer_amd import formats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _random_set(seed, n_seg=300, seq_len=4000, alphabet="ACGT", lens=(1, 60), seg=(0, 90)):
    r = random.Random(seed)
    seq = "".join(r.choice(alphabet) for _ in range(seq_len))
    monos = ["".join(r.choice("ACGT") for _ in range(r.randint(*lens))) for _ in range(5)]
    st = [r.randint(0, seq_len - seg[1] - 1) for _ in range(n_seg)]
    en = [s + r.randint(*seg) for s in st]
    pt = [r.randrange(2 * len(monos)) for _ in st]
    return seq, st, en, monos, pt


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape
        assert (x == y).all()


@pytest.mark.parametrize("seed,alphabet", [(1, "ACGT"), (2, "ACGTN"), (3, "ACGTNNNN")])
def test_host_profile_equals_edlib_fold(seed, alphabet):
    """Random pairs against both orientations, with and without N bases."""
    seq, st, en, monos, pt = _random_set(seed, alphabet=alphabet)
    got = lib.profile_segments(seq, st, en, monos, pt, threads=4)
    _same(got, profile_ref.profile_segments(seq, st, en, monos, pt))


def test_host_profile_one_base_templates_and_empty_segments():
    """1-bp monomers; a segment that is empty (end < start) is no instance."""
    seq, st, en, _, pt = _random_set(4, n_seg=120, seg=(0, 12))
    monos = ["A", "C", "G"]
    pt = [p % 6 for p in pt]
    st2, en2 = list(st) + [10], list(en) + [8]
    got = lib.profile_segments(seq, st2, en2, monos, pt + [1], threads=2)
    _same(got, profile_ref.profile_segments(seq, st, en, monos, pt))


def test_host_profile_threads_do_not_matter():
    seq, st, en, monos, pt = _random_set(5)
    _same(lib.profile_segments(seq, st, en, monos, pt, threads=1), lib.profile_segments(seq, st, en, monos, pt, threads=7))


def _long_block():
    d = os.path.join(GOLDEN, "final", "long_block")
    rn, rs, _ = lib.fasta_load(os.path.join(d, "reads.fa"))
    mn, ms, _ = lib.fasta_load(os.path.join(d, "monomers.fa"))
    return d, dict(zip(rn, [s.decode().upper() for s in rs])), mn, [s.decode().upper() for s in ms]


def test_host_profile_hirschberg_pair():
    """The long_block golden: a 21-kb block against its 171-bp monomer is aligned by Hirschberg's split in edlib."""
    d, reads, mn, ms = _long_block()
    rows = formats.read_final(os.path.join(d, "final.tsv"))
    assert any(r.end - r.start + 1 > 19000 for r in rows)
    text = "".join(reads[r.read] for r in rows[:1])
    seq, st, en, pt = "", [], [], []
    for r in rows:
        st.append(len(seq) + r.start)
        en.append(len(seq) + r.end)
        seq += reads[r.read]
        pt.append(2 * mn.index(r.monomer.rstrip("'")) + (1 if r.monomer.endswith("'") else 0))
    assert text
    got = lib.profile_segments(seq, st, en, ms, pt, threads=4)
    if profile_ref.edlib_ref.have_edlib():
        _same(got, profile_ref.profile_segments(seq, st, en, ms, pt))
    # whichever edlib is at hand: the '=' columns of the folded paths are the identity path's matches
    _, m, _ = lib.identity_segments(seq, st, en, [profile_ref.rc(ms[p >> 1]) if p & 1 else ms[p >> 1] for p in range(2 * len(ms))],
                                    pair_tmpl=pt, threads=4)
    eq = sum(int(sum(c[g, "ACGT".index(s[g])] for g in range(len(s)))) for c, s in zip(got, ms))
    assert eq == int(m.sum())


def test_profile_invariants():
    """A..del sum to n at every position; aligned plus inserted bases are the summed block lengths; nothing aligned at
    g = L."""
    seq, st, en, monos, pt = _random_set(6, alphabet="ACGTN")
    got = lib.profile_segments(seq, st, en, monos, pt, threads=3)
    for m, c in enumerate(got):
        n = sum(1 for p in pt if p >> 1 == m)
        L = len(monos[m])
        assert (c[:L, :6].sum(axis=1) == n).all()
        assert (c[L, :6] == 0).all()
        assert int(c[:, :5].sum() + c[:, 7:].sum()) == sum(e - s + 1 for s, e, p in zip(st, en, pt) if p >> 1 == m)
        assert (c[:, 6] <= n).all() and (c[:, 6] <= c[:, 7:].sum(axis=1)).all()


def _prof(seq, rows):
    return formats.Profile(["m"], [seq], [np.asarray(rows, dtype=np.int64)])


def test_consensus_tie_rules():
    z = [0] * 12
    # g0: A wins; g1: tie C / G with ref G -> G; g2: tie A / C, ref T not tied -> A; g3: del wins -> nothing;
    # slot 1: 2 of 4 instances insert (not more than half) -> nothing; slot 4 (end): 3 of 4 insert, tie T / A -> A
    rows = [[4, 0, 0, 0, 0, 0] + z[6:],
            [0, 2, 2, 0, 0, 0, 2, 0, 0, 1, 1, 0],
            [2, 2, 0, 0, 0, 0] + z[6:],
            [1, 0, 0, 0, 0, 3] + z[6:],
            [0] * 6 + [3, 2, 0, 0, 2, 0]]
    assert formats.consensus(_prof("AGTC", rows)) == [("m", 4, "AGAA")]
    # ref among the tied wins over the order; del tied with ref keeps ref; an N column
    rows = [[0, 0, 1, 1, 0, 0] + z[6:], [0, 0, 0, 1, 0, 1] + z[6:], [0, 0, 0, 0, 2, 0] + z[6:], z]
    assert formats.consensus(_prof("TTA", rows)) == [("m", 2, "TTN")]
    # an insertion before the first position, ties among inserted bases go to the first of ACGTN
    rows = [[0, 0, 0, 3, 0, 0, 2, 0, 1, 1, 0, 0], [0] * 6 + [0] * 6]
    assert formats.consensus(_prof("T", rows)) == [("m", 3, "CT")]
    # no instances: the monomer's own sequence
    assert formats.consensus(_prof("ACG", [z] * 4)) == [("m", 0, "ACG")]


def test_profile_file_round_trip(tmp_path):
    seq, st, en, monos, pt = _random_set(7)
    prof = formats.Profile(["a%d" % i for i in range(len(monos))], monos, lib.profile_segments(seq, st, en, monos, pt))
    p = str(tmp_path / "x_profile.tsv")
    formats.write_profile(p, prof)
    back = formats.read_profile(p)
    assert back.names == prof.names and back.seqs == prof.seqs
    _same(back.counts, prof.counts)
    lines = open(p).read().splitlines()
    assert lines[0].split("\t") == ["name", "g", "ref", "n"] + list(formats.PROFILE_COLUMNS)
    assert len(lines) == 1 + sum(len(m) + 1 for m in monos)
    assert all(len(x.split("\t")) == 16 for x in lines)
    flat = np.concatenate([x.reshape(-1) for x in prof.counts])
    as_lists = formats.profile_from_counts(prof.names, prof.seqs, list(flat), numpy=False)
    assert isinstance(as_lists.counts[0], list)
    assert formats.format_profile(as_lists) == formats.format_profile(prof)
    assert formats.consensus(as_lists) == formats.consensus(prof)
    c = str(tmp_path / "x_consensus.fa")
    formats.write_consensus(c, prof)
    got = open(c).read().splitlines()
    assert got[0].startswith(">a0 instances=")


def test_profile_segments_argument_checks():
    with pytest.raises(lib.SdError) as e:
        lib.profile_segments("ACGT", [0], [3], ["ACG"], [2])   # template index beyond the interleaved set
    assert e.value.code == lib.SD_ERR_PARAM
    with pytest.raises(lib.SdError) as e:
        lib.profile_segments("ACGT", [0], [4], ["ACG"], [0])   # segment past the sequence
    assert e.value.code == lib.SD_ERR_PARAM


def _cli(args, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer")] + args, env=env,
                          capture_output=True, text=True, timeout=120)


def test_cli_profile_refuses_repeated_names(tmp_path):
    m = tmp_path / "m.fa"
    m.write_text(">x\nACGTACGT\n>y\nTTGACCA\n>x\nGGGACT\n")
    r = tmp_path / "r.fa"
    r.write_text(">r\nACGTACGTTTGACCA\n")
    p = _cli([str(r), str(m), "-o", str(tmp_path / "out"), "--profile"])
    assert p.returncode == lib.SD_ERR_PARAM
    err = p.stderr.strip().splitlines()
    assert len(err) == 1 and "not unique" in err[0]
    assert not (tmp_path / "out" / "final_decomposition.tsv").exists()
    # a name that collides with another's reverse-complement key
    m.write_text(">x\nACGTACGT\n>x'\nTTGACCA\n")
    p = _cli([str(r), str(m), "-o", str(tmp_path / "out"), "--profile"])
    assert p.returncode == lib.SD_ERR_PARAM and "x'" in p.stderr


def test_cli_profile_refuses_distributed_launch(tmp_path):
    m = tmp_path / "m.fa"
    m.write_text(">x\nACGTACGT\n")
    r = tmp_path / "r.fa"
    r.write_text(">r\nACGTACGT\n")
    p = _cli([str(r), str(m), "-o", str(tmp_path / "out"), "--profile"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2
    err = p.stderr.strip().splitlines()
    assert len(err) == 1 and "torch.distributed" in err[0]


def test_c_abi_refusals_without_gpu():
    """Repeated names are refused by sd_run_files itself; a raw-mode stream refuses the flag; no profile before a
    profiled run."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        m = os.path.join(d, "m.fa")
        with open(m, "w") as f:
            f.write(">x\nACGTACGT\n>x\nTTGACCA\n")
        r = os.path.join(d, "r.fa")
        with open(r, "w") as f:
            f.write(">r\nACGTACGTTTGACCA\n")
        o = [os.path.join(d, x) for x in ("raw.tsv", "final.tsv", "alt.tsv")]
        with pytest.raises(lib.SdError) as e:
            lib.run_files(r, m, o[0], o[1], o[2], profile=True)
        assert e.value.code == lib.SD_ERR_PARAM and "not unique" in e.value.msg
    with pytest.raises(lib.SdError) as e:
        lib.Stream(["ACGTACGT"], flags=lib.FLAG_PROFILE)
    assert e.value.code == lib.SD_ERR_PARAM
    with pytest.raises(lib.SdError) as e:
        lib.last_run_profile()
    assert e.value.code == lib.SD_ERR_PARAM
