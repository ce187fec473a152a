"""The final mode of the stream (lib.Stream(final=True) / sd_stream_create_final) on the device: its typed rows, formatted
by formats.final_rows + format_final / format_alt, are the text the command line writes -- against the unmodified
reference command line's goldens and against lib.run_files on multi-batch jobs -- with the identities computed in-stream
(and by the fallback where the in-stream kernels do not take a pair)."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

from stringdecomposer_amd import formats, lib, main as sdmain, synth

pytestmark = pytest.mark.gpu

FINAL = os.path.join(GOLDEN, "final")
THREADS = 8


def _fasta(path):
    names, seqs, _ = lib.fasta_load(path)
    return [n.split()[0] for n in names], [s.upper() for s in seqs]


def _case(name):
    with open(os.path.join(FINAL, name, "params.json")) as f:
        c = json.load(f)
    a = c["args"]
    kw = {"second_best": "--second-best" in a,
          "min_identity": int(a[a.index("-i") + 1]) if "-i" in a else 0,
          "part_size": int(a[a.index("-b") + 1]) if "-b" in a else 5000}
    return c, _fasta(os.path.join(GOLDEN, c["inputs"][0])), _fasta(os.path.join(GOLDEN, c["inputs"][1])), kw


def _stream(mono, sub_batches=1, **kw):
    return lib.Stream(mono[1], sub_batches=sub_batches, final=True, mono_names=mono[0], threads=THREADS, **kw)


def _text(st, fr, read_names):
    fin, alt = formats.final_rows(fr, read_names, st.keys())
    return formats.format_final(fin).encode(), formats.format_alt(alt).encode()


def _one_job(mono, reads, sub_batches=1, **kw):
    st = _stream(mono, sub_batches=sub_batches, **kw)
    try:
        st.submit(reads[1])
        fr = st.collect()
        return _text(st, fr, reads[0]), st.stats(), fr
    finally:
        st.close()


@pytest.mark.parametrize("sub_batches", [1, 3])
@pytest.mark.parametrize("name", sorted(os.listdir(FINAL)))
def test_stream_final_equals_reference_goldens(name, sub_batches):
    """Every golden case of the unmodified reference command line, through Stream(final=True) with the case's -b / -i /
    --second-best: final.tsv byte for byte, _alt.tsv byte for byte (alt.tsv.gz) or by its sha256.  With sub_batches=3 the
    long reads span device batches (identity words carried by value).  long_block holds a 21-kb block that edlib aligns
    by Hirschberg's split: its identities come from the fallback."""
    c, reads, mono, kw = _case(name)
    (fin, alt), stats, fr = _one_job(mono, reads, sub_batches=sub_batches, **kw)
    with open(os.path.join(FINAL, name, "final.tsv"), "rb") as f:
        assert fin == f.read()
    gz = os.path.join(FINAL, name, "alt.tsv.gz")
    if os.path.exists(gz):
        with gzip.open(gz, "rb") as f:
            assert alt == f.read()
    assert hashlib.sha256(alt).hexdigest() == c["alt_sha256"]
    assert len(fr.rows) == c["final_rows"] == stats["final_rows"]
    assert fr.row_off[0] == 0 and fr.row_off[-1] == len(fr.rows) and len(fr.row_off) == len(reads[0]) + 1
    if name in ("long_k17", "long_k32_mixed"):   # monomers beyond 512 bp: the in-stream kernels decline the set, every
        assert stats["ident_pairs"] == 0 and stats["fallback_blocks"] > 0   # identity comes from the fallback
    else:
        assert stats["ident_pairs"] > 0 and stats["ident_ms"] > 0   # the in-stream kernels ran
    if name in ("long_block", "long_k17", "long_k32_mixed"):
        assert stats["fallback_blocks"] > 0
    else:
        assert stats["fallback_blocks"] == 0
    assert stats["batches"] == min(sub_batches, lib.chunk_table_size([len(r) for r in reads[1]], kw["part_size"], 500))


def _multi_batch_job(n_mono=12, seed=7):
    """Reads of mixed length (two of them long enough to span batches of max_batch_rows 20 000) with runs of N, and a
    monomer set in which two monomers share a name (one key)."""
    mn, ms = synth.make_monomers(n_mono, seed=seed)
    mn = list(mn)
    mn[5] = mn[2]
    rn, rs = [], []
    for i, ln in enumerate([3000, 47000, 800, 12000, 61000, 5200, 9000]):
        n, s = synth.make_reads(ms, 1, read_len=ln, seed=seed, first_index=i)
        s = bytearray(s[0])
        if i in (1, 3, 4):
            s[ln // 3:ln // 3 + 40] = b"N" * 40
        rn.append(n[0])
        rs.append(bytes(s))
    return (mn, ms), (rn, rs)


@pytest.mark.parametrize("second_best", [False, True])
def test_stream_final_equals_run_files_on_a_multi_batch_job(second_best, tmp_path):
    """A job cut into many device batches (sub_batches 4 and a 20 000-row cap), reads that span batches, N in reads and a
    repeated monomer name: the formatted rows equal what lib.run_files writes for the same reads as FASTA."""
    mono, reads = _multi_batch_job()
    kw = dict(second_best=second_best, min_identity=0, max_batch_rows=20000)
    (fin, alt), stats, _ = _one_job(mono, reads, sub_batches=4, **kw)
    assert stats["batches"] >= 4 and stats["ident_pairs"] > 0
    rfa, mfa = str(tmp_path / "r.fa"), str(tmp_path / "m.fa")
    synth.write_fasta(rfa, *reads)
    synth.write_fasta(mfa, *mono)
    out = [str(tmp_path / x) for x in ("raw.tsv", "final.tsv", "alt.tsv")]
    lib.run_files(rfa, mfa, *out, threads=THREADS, lr_coef=sdmain._lr_coef(), **kw)
    with open(out[1], "rb") as f:
        assert fin == f.read()
    with open(out[2], "rb") as f:
        assert alt == f.read()
    assert len(fin) > 0 and (len(alt) > 0) == second_best


def test_stream_final_fallback_equals_in_stream():
    """FLAG_NO_STREAM_IDENT sends every block to the fallback of the file path: the same typed rows, no in-stream pairs."""
    mono, reads = _multi_batch_job(seed=11)
    a = _one_job(mono, reads, sub_batches=3, second_best=True, max_batch_rows=30000)
    b = _one_job(mono, reads, sub_batches=3, second_best=True, max_batch_rows=30000, flags=lib.FLAG_NO_STREAM_IDENT)
    assert a[1]["ident_pairs"] > 0 and a[1]["fallback_blocks"] == 0
    assert b[1]["ident_pairs"] == 0 and b[1]["fallback_blocks"] > 0
    assert a[2].rows.tobytes() == b[2].rows.tobytes() and np.array_equal(a[2].row_off, b[2].row_off)
    assert np.array_equal(a[2].alt, b[2].alt)
    assert a[0] == b[0]


@pytest.mark.parametrize("second_best", [False, True])
def test_stream_final_pipelined_jobs_equal_jobs_one_at_a_time(second_best):
    """Five jobs through imap(depth=2) -- batches of several jobs in flight at once -- give the rows of the same jobs
    submitted and collected one at a time."""
    mn, ms = synth.make_monomers(10, seed=5)
    jobs = [synth.make_reads(ms, 3 + j, read_len=9000 + 4000 * j, seed=20 + j) for j in range(5)]
    kw = dict(sub_batches=2, second_best=second_best, min_identity=60 if not second_best else 0, max_batch_rows=25000)
    st = _stream((mn, ms), **kw)
    piped = list(st.imap([j[1] for j in jobs], depth=2))
    assert st.stats()["jobs"] == 5
    st.close()
    for (rn, rs), got in zip(jobs, piped):
        st = _stream((mn, ms), **kw)
        st.submit(rs)
        want = st.collect()
        st.close()
        assert got.rows.tobytes() == want.rows.tobytes() and np.array_equal(got.row_off, want.row_off)
        assert (got.alt is None) == (not second_best)
        if second_best:
            assert got.alt.shape == (len(got.rows), 20) and np.array_equal(got.alt, want.alt)


def test_stream_modes_do_not_mix():
    """A final-mode stream is collected with the final call only, and a raw stream has no keys."""
    mn, ms = synth.make_monomers(4, seed=9)
    rn, rs = synth.make_reads(ms, 2, read_len=4000, seed=9)
    st = _stream((mn, ms))
    st.submit(rs)
    L = lib.load()
    import ctypes as C
    rows, off, n = C.POINTER(lib.Rec)(), C.POINTER(C.c_int64)(), C.c_int64()
    assert L.sd_stream_collect(st.h, C.byref(rows), C.byref(off), C.byref(n), None, 0) == lib.SD_ERR_PARAM
    fr = st.collect()   # the job is still there
    assert len(fr.rows) > 0 and st.keys() == ["M0", "M0'", "M1", "M1'", "M2", "M2'", "M3", "M3'"]
    st.close()
    raw = lib.Stream(ms)
    with pytest.raises(lib.SdError) as e:
        raw.keys()
    assert e.value.code == lib.SD_ERR_PARAM
    raw.close()
