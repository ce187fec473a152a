"""Final rows selected on the device (Stream(final=True, device_final=True) -> collect_final_device / imap(device=True),
lib.final_select_device): the selection kernels against the host's selection on the CPU test's word sets, and the rows
of device-final streams against the reference command line's goldens and against the bytes the host final stream returns
for the same jobs.  Every comparison is exact.  The host streams' rows are computed once per parameter set."""
import ctypes as C
import gzip
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import final_select_cases as fsc
import regrow_case
from conftest import GOLDEN

from stringdecomposer_amd import formats, lib, synth

pytestmark = pytest.mark.gpu

FINAL = os.path.join(GOLDEN, "final")
THREADS = 8
GUARD = 0x5A


# ---- 1. the selection kernels alone -------------------------------------------------------------------------------

def _select_both(case, min_identity):
    a = (case["names"], case["seqs"], case["rows"], case["row_off"], case["widx"], case["words"], case["hwords"], case["read_len"])
    kw = dict(min_identity=min_identity, second_best=case["second_best"], lr_coef=fsc.COEF)
    want, want_und = lib.final_select_host(*a, **kw)
    got, und, intact = lib.final_select_device(*a, **kw)
    assert intact, "a guard byte behind rows / row_off / alt was overwritten"
    assert und == want_und
    assert got.row_off.tolist() == want.row_off.tolist()
    assert got.rows.tobytes() == want.rows.tobytes()          # (padding included)
    if case["second_best"]:
        assert got.alt.tobytes() == want.alt.tobytes() and got.alt.shape == want.alt.shape
    else:
        assert got.alt is None
    return want, und


@pytest.mark.parametrize("min_identity", [0, 95])
@pytest.mark.parametrize("second_best", [False, True])
@pytest.mark.parametrize("n_mono", [1, 3, 12, 130])
def test_selection_kernels_equal_the_host_selection(n_mono, second_best, min_identity):
    """T = 2, 6, 24 and 260 interleaved templates: groups of 8, 8, 32 lanes per row, and a wave that strides 260 words
    (across 64 and across 256).  The sets hold reads without rows, tied maxima in most rows, rows at the threshold and
    five rows no word decides."""
    case = fsc.make(n_mono, second_best, n_rows=2000 if n_mono <= 12 else 600)
    want, und = _select_both(case, min_identity)
    n = len(case["rows"])
    assert und == 5 and 0 in np.diff(case["row_off"])
    assert (0 < len(want.rows) < n - und) if min_identity else len(want.rows) == n - und


@pytest.mark.parametrize("second_best", [False, True])
def test_selection_kernels_without_reads_and_without_rows(second_best):
    none = fsc.make(3, second_best, no_reads=True)
    want, und = _select_both(none, 0)
    assert len(want.rows) == 0 and want.row_off.tolist() == [0] and und == 0
    case = fsc.make(3, second_best, n_rows=50)
    case["row_off"] = np.zeros(4, dtype=np.int64)      # three reads, no rows
    case["rows"], case["widx"], case["read_len"] = case["rows"][:0], case["widx"][:0], np.array([10, 20, 30], dtype=np.int64)
    want, und = _select_both(case, 0)
    assert len(want.rows) == 0 and want.row_off.tolist() == [0, 0, 0, 0]


# ---- 2. streams ---------------------------------------------------------------------------------------------------

def _fasta(path):
    names, seqs, _ = lib.fasta_load(path)
    return [n.split()[0] for n in names], [s.upper() for s in seqs]


def _golden_case(name):
    with open(os.path.join(FINAL, name, "params.json")) as f:
        c = json.load(f)
    a = c["args"]
    kw = {"second_best": "--second-best" in a,
          "min_identity": int(a[a.index("-i") + 1]) if "-i" in a else 0,
          "part_size": int(a[a.index("-b") + 1]) if "-b" in a else 5000}
    return c, _fasta(os.path.join(GOLDEN, c["inputs"][0])), _fasta(os.path.join(GOLDEN, c["inputs"][1])), kw


def _stream(mono, device_final=True, **kw):
    return lib.Stream(mono[1], final=True, mono_names=mono[0], threads=THREADS, device_final=device_final, **kw)


def _to_dev(buf):
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).to("cuda:0")


def _device_reads(seqs):
    return lib.DeviceReads(_to_dev(b"".join(seqs) + b"#"), [len(s) for s in seqs])


def _checked(dfr, n_reads, second_best, n_keys):
    """DeviceFinalRows -> FinalRows on the host, its shapes and places checked"""
    assert dfr.rows.dtype == torch.uint8 and dfr.rows.shape == (dfr.n_rows, 80) and dfr.rows.is_cuda
    assert dfr.row_off.dtype == torch.int64 and dfr.row_off.shape == (n_reads + 1,) and dfr.row_off.device == dfr.rows.device
    if second_best:
        assert dfr.alt.dtype == torch.float64 and dfr.alt.shape == (dfr.n_rows, n_keys) and dfr.alt.device == dfr.rows.device
    else:
        assert dfr.alt is None
    fr = dfr.to_host()
    assert fr.rows.dtype == lib.final_dtype() and int(fr.row_off[0]) == 0 and int(fr.row_off[-1]) == dfr.n_rows == len(fr.rows)
    return fr


def _same(got, want):
    assert got.rows.tobytes() == want.rows.tobytes()
    assert np.array_equal(got.row_off, want.row_off)
    assert (got.alt is None) == (want.alt is None)
    if want.alt is not None:
        assert got.alt.shape == want.alt.shape and got.alt.tobytes() == want.alt.tobytes()


@pytest.mark.parametrize("sub_batches", [1, 3])
@pytest.mark.parametrize("name", sorted(os.listdir(FINAL)))
def test_device_final_equals_reference_goldens(name, sub_batches):
    """Every golden case of the unmodified reference command line through collect_final_device, copied to the host and
    formatted by the existing formatters.  long_block holds a 21-kb block that edlib aligns by Hirschberg's split: the
    kernels count it and the job takes the text-based path."""
    c, reads, mono, kw = _golden_case(name)
    st = _stream(mono, sub_batches=sub_batches, **kw)
    try:
        st.submit(reads[1])
        dfr = st.collect_final_device()
        fr = _checked(dfr, len(reads[1]), kw["second_best"], len(st.keys()))
        fin, alt = formats.final_rows(dfr, reads[0], st.keys())     # (a DeviceFinalRows goes in as it is)
        fin, alt = formats.format_final(fin).encode(), formats.format_alt(alt).encode()
        stats = st.stats()
    finally:
        st.close()
    with open(os.path.join(FINAL, name, "final.tsv"), "rb") as f:
        assert fin == f.read()
    gz = os.path.join(FINAL, name, "alt.tsv.gz")
    if os.path.exists(gz):
        with gzip.open(gz, "rb") as f:
            assert alt == f.read()
    assert hashlib.sha256(alt).hexdigest() == c["alt_sha256"]
    assert len(fr.rows) == c["final_rows"] == stats["final_rows"]
    if name in ("long_k17", "long_k32_mixed"):   # monomers beyond 512 bp: the in-stream kernels decline the set, every
        assert stats["ident_pairs"] == 0 and stats["fallback_blocks"] > 0   # identity comes from the text-based path
        return
    assert stats["ident_pairs"] > 0
    if name == "long_block":
        assert stats["fallback_blocks"] > 0
    else:
        assert stats["fallback_blocks"] == 0 and stats["host_assemble_ms"] == 0


def _multi_batch_job(n_mono=12, seed=7):
    """(test_gpu_stream_final.py's job) seven reads of 800 - 61 000 bp, two of them spanning batches of 20 000 rows, runs
    of N, and a monomer set in which two monomers share a name."""
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


MB = dict(sub_batches=4, max_batch_rows=20000)


@pytest.fixture(scope="module")
def job():
    return _multi_batch_job()


@pytest.fixture(scope="module")
def host_rows(job):
    """FinalRows of the host final stream for the multi-batch job, by (second_best, min_identity); computed on demand, once"""
    mono, reads = job
    have = {}

    def get(second_best, min_identity=0):
        key = (second_best, min_identity)
        if key not in have:
            st = _stream(mono, device_final=False, second_best=second_best, min_identity=min_identity, **MB)
            try:
                st.submit(reads[1])
                have[key] = st.collect()
                assert st.stats()["batches"] >= 4
            finally:
                st.close()
        return have[key]
    return get


def _one(mono, reads_in, n_reads, **kw):
    st = _stream(mono, **kw)
    try:
        st.submit(reads_in)
        dfr = st.collect_final_device()
        return _checked(dfr, n_reads, bool(kw.get("second_best")), len(st.keys())), st.stats()
    finally:
        st.close()


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("second_best", [False, True])
def test_same_rows_as_the_host_final_stream(job, host_rows, second_best, source):
    mono, reads = job
    src = reads[1] if source == "host" else _device_reads(reads[1])
    got, stats = _one(mono, src, len(reads[1]), second_best=second_best, **MB)
    _same(got, host_rows(second_best))
    assert len(got.rows) > 0 and stats["batches"] >= 4 and stats["ident_pairs"] > 0
    assert stats["fallback_blocks"] == 0 and stats["host_assemble_ms"] == 0 and stats["final_rows"] == len(got.rows)


@pytest.mark.parametrize("second_best", [False, True])
def test_min_identity_drops_rows_on_the_device(job, host_rows, second_best):
    mono, reads = job
    ident = np.sort(host_rows(second_best).rows["ident"])
    thr = 95 if ident[0] < 95 <= ident[-1] else int(np.ceil(ident[len(ident) // 2]))   # 95, or the set's median
    want = host_rows(second_best, thr)
    assert 0 < len(want.rows) < len(ident), "the threshold %d must split the rows" % thr
    got, stats = _one(mono, _device_reads(reads[1]), len(reads[1]), second_best=second_best, min_identity=thr, **MB)
    _same(got, want)
    assert stats["fallback_blocks"] == 0


@pytest.mark.parametrize("second_best", [False, True])
def test_text_based_path_on_demand(job, host_rows, second_best):
    """FLAG_NO_STREAM_IDENT: no identity words, every job finished by the host from the text -- the same bytes."""
    mono, reads = job
    for src in (reads[1], _device_reads(reads[1])):
        got, stats = _one(mono, src, len(reads[1]), second_best=second_best, flags=lib.FLAG_NO_STREAM_IDENT, **MB)
        _same(got, host_rows(second_best))
        assert stats["ident_pairs"] == 0 and stats["fallback_blocks"] > 0


@pytest.mark.parametrize("second_best", [False, True])
def test_pipelined_jobs_equal_jobs_one_at_a_time(second_best):
    """Five jobs through imap(depth=2, device=True), one of them a read too short to yield a row at this threshold."""
    mn, ms = synth.make_monomers(10, seed=5)
    jobs = [synth.make_reads(ms, 3 + j, read_len=9000 + 4000 * j, seed=20 + j)[1] for j in range(5)]
    jobs[2] = [jobs[2][0][:60]]
    kw = dict(sub_batches=2, second_best=second_best, min_identity=70, max_batch_rows=25000)
    st = _stream((mn, ms), **kw)
    try:
        piped = [_checked(d, len(j), second_best, 20) for d, j in zip(st.imap([_device_reads(j) for j in jobs], depth=2, device=True), jobs)]
        assert st.stats()["jobs"] == 5 and st.stats()["fallback_blocks"] == 0
    finally:
        st.close()
    assert len(piped[2].rows) == 0 and piped[2].row_off.tolist() == [0, 0]
    for j, got in zip(jobs, piped):
        want, _ = _one((mn, ms), j, len(j), **kw)
        _same(got, want)
    assert sum(len(p.rows) for p in piped) > 0


def test_buffer_one_row_short(job, host_rows):
    """cap_rows = n_rows - 1: an error that names both counts, nothing written into or behind any of the three buffers,
    and the job is still there for the call with enough room."""
    mono, reads = job
    want = host_rows(True)
    n_rows, nr, nk = len(want.rows), len(reads[1]), want.alt.shape[1]
    L = lib.load()
    st = _stream(mono, second_best=True, **MB)
    try:
        st.submit(reads[1])
        c_nr, c_n, c_nk = C.c_int32(), C.c_int64(), C.c_int32()
        st._check(L.sd_stream_peek_final_dev(st.h, C.byref(c_nr), C.byref(c_n), C.byref(c_nk), st._err, 4096))
        assert (c_nr.value, c_n.value, c_nk.value) == (nr, n_rows, nk)
        rows = torch.full(((n_rows + 2) * 80,), GUARD, dtype=torch.uint8, device="cuda:0")
        off = torch.full(((nr + 1 + 2) * 8,), GUARD, dtype=torch.uint8, device="cuda:0")
        alt = torch.full(((n_rows + 2) * nk * 8,), GUARD, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        n = C.c_int64()
        args = lambda cap: (st.h, C.c_void_p(rows.data_ptr()), cap, C.c_void_p(off.data_ptr()), C.c_void_p(alt.data_ptr()),   # noqa: E731
                            None, C.byref(n), st._err, 4096)
        rc = L.sd_stream_collect_final_dev(*args(n_rows - 1))
        assert rc == lib.SD_ERR_PARAM and n.value == n_rows
        msg = st._err.value.decode()
        assert str(n_rows) in msg and str(n_rows - 1) in msg
        torch.cuda.synchronize()
        assert bool((rows == GUARD).all()) and bool((off == GUARD).all()) and bool((alt == GUARD).all())
        st._check(L.sd_stream_collect_final_dev(*args(n_rows)))
        st._n_reads.pop(0)
        torch.cuda.synchronize()
        assert n.value == n_rows
        assert bool((rows[n_rows * 80:] == GUARD).all()) and bool((off[(nr + 1) * 8:] == GUARD).all())
        assert bool((alt[n_rows * nk * 8:] == GUARD).all())
        got = lib.DeviceFinalRows(rows[:n_rows * 80].reshape(n_rows, 80), off[:(nr + 1) * 8].view(torch.int64),
                                  alt[:n_rows * nk * 8].view(torch.float64).reshape(n_rows, nk), n_rows)
        _same(got.to_host(), want)
    finally:
        st.close()


# ---- 3. ordering, lifetime, modes -----------------------------------------------------------------------------------

def test_rows_are_ordered_on_the_callers_stream(job, host_rows):
    """collect_final_device(stream=s) on a side stream, the rows consumed on s with no host synchronisation in between;
    the tensors of job k are still what they were after jobs k + 1 and k + 2 (which reuse workspaces) were collected."""
    mono, reads = job
    want = host_rows(True)
    s = torch.cuda.Stream(device=0)
    st = _stream(mono, second_best=True, **MB)
    try:
        st.submit(reads[1])
        st.submit(_device_reads(reads[1]))
        first = st.collect_final_device(stream=s)
        with torch.cuda.stream(s):
            copy_rows, copy_alt = first.rows.clone(), first.alt.clone()      # consumed on s, no synchronisation before it
            sum_rows, max_alt = first.rows.to(torch.int64).sum(dim=0), first.alt.max(dim=0).values   # (exact in any order)
        second = st.collect_final_device(stream=s)
        st.submit(reads[1])
        third = st.collect_final_device(stream=s)
        s.synchronize()
    finally:
        st.close()
    assert copy_rows.cpu().numpy().tobytes() == want.rows.tobytes()
    assert copy_alt.cpu().numpy().tobytes() == want.alt.tobytes()
    want_bytes = torch.from_numpy(np.frombuffer(want.rows.tobytes(), dtype=np.uint8).reshape(-1, 80).copy())
    assert torch.equal(sum_rows.cpu(), want_bytes.to(torch.int64).sum(dim=0))
    assert torch.equal(max_alt.cpu(), torch.from_numpy(want.alt).max(dim=0).values)
    for d in (first, second, third):
        _same(d.to_host(), want)


def test_close_right_after_collect_with_the_copy_still_queued(job, host_rows):
    """Stream.close() with the copy still queued on the caller's stream: the library waits for it before its buffers go
    back, and the rows are what they should be."""
    mono, reads = job
    s = torch.cuda.Stream(device=0)
    busy = torch.randn(4096, 4096, device="cuda:0")
    torch.cuda.synchronize()
    st = _stream(mono, second_best=True, **MB)
    try:
        st.submit(reads[1])
        st.collect_final_device()                      # (warm: the next collect allocates nothing that synchronises)
        st.submit(reads[1])
        nr, n, nk = C.c_int32(), C.c_int64(), C.c_int32()
        st._check(st.L.sd_stream_peek_final_dev(st.h, C.byref(nr), C.byref(n), C.byref(nk), st._err, 4096))
        done = torch.cuda.Event()
        with torch.cuda.stream(s):
            for _ in range(60):
                busy @ busy
            done.record(s)
        got = st.collect_final_device(stream=s)
        assert not done.query(), "the consumer stream was meant to be backlogged at close"
    finally:
        st.close()
    other, _ = _one(mono, reads[1][::-1], len(reads[1]), second_best=True, **MB)      # whoever takes the buffers next
    s.synchronize()
    _same(got.to_host(), host_rows(True))
    assert len(other.rows) == len(got.rows)


def test_modes_do_not_mix(job):
    """The wrong collect for a stream's mode is refused in both directions and leaves the job collectable."""
    mono, reads = job
    L = lib.load()
    small = reads[1][:1]
    st = _stream(mono)
    try:
        st.submit(small)
        rows, off, n = C.POINTER(lib.Rec)(), C.POINTER(C.c_int64)(), C.c_int64()
        frows, alt = C.POINTER(lib.FinalRec)(), C.POINTER(C.c_double)()
        assert L.sd_stream_collect(st.h, C.byref(rows), C.byref(off), C.byref(n), st._err, 4096) == lib.SD_ERR_PARAM
        assert "sd_stream_collect_final_dev" in st._err.value.decode()
        assert L.sd_stream_collect_final(st.h, C.byref(frows), C.byref(off), C.byref(n), C.byref(alt), st._err, 4096) == lib.SD_ERR_PARAM
        assert "sd_stream_collect_final_dev" in st._err.value.decode()
        buf = torch.zeros(64, dtype=torch.int64, device="cuda:0")
        assert L.sd_stream_collect_dev(st.h, C.c_void_p(buf.data_ptr()), 0, C.c_void_p(buf.data_ptr()), None, C.byref(n),
                                       st._err, 4096) == lib.SD_ERR_PARAM
        nr = C.c_int32()
        assert L.sd_stream_peek_dev(st.h, C.byref(nr), C.byref(n), st._err, 4096) == lib.SD_ERR_PARAM
        with pytest.raises(lib.SdError) as e:
            st.collect()
        assert e.value.code == lib.SD_ERR_PARAM
        st._n_reads.insert(0, 1)                       # (collect() took the count off before the refusal)
        assert st.collect_final_device().n_rows > 0    # the job is still there
    finally:
        st.close()
    for kw in (dict(final=True, mono_names=mono[0]), dict(device_rows=True), dict()):
        st = lib.Stream(mono[1], threads=THREADS, **kw)
        try:
            st.submit(small)
            with pytest.raises(lib.SdError) as e:
                st.collect_final_device()
            assert e.value.code == lib.SD_ERR_PARAM and "SD_FLAG_DEVICE_FINAL" in e.value.msg
            nn = C.c_int64()
            buf = torch.zeros(64, dtype=torch.int64, device="cuda:0")
            assert L.sd_stream_collect_final_dev(st.h, None, 0, C.c_void_p(buf.data_ptr()), None, None, C.byref(nn),
                                                 st._err, 4096) == lib.SD_ERR_PARAM
            got = st.collect_device() if kw.get("device_rows") else st.collect()
            assert (got.n_rows if kw.get("device_rows") else (len(got.rows) if kw.get("final") else got)) > 0
        finally:
            st.close()


# ---- 4. the store and the identity words regrown behind a later batch -------------------------------------------------

@pytest.fixture(scope="module")
def regrow_host_rows():
    """FinalRows of the host final stream for regrow_case's job, by second_best; computed on demand, once"""
    have = {}

    def get(second_best):
        if second_best not in have:
            mono, job = regrow_case.job()
            st = _stream(mono, device_final=False, second_best=second_best, max_batch_rows=regrow_case.MAX_BATCH_ROWS)
            try:
                st.submit(job)
                have[second_best] = st.collect()
            finally:
                st.close()
        return have[second_best]
    return get


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("second_best", [False, True])
def test_store_and_words_regrown_with_records_in_them(regrow_host_rows, second_best, source):
    """regrow_case's job on a fresh stream: six chunks in six batches, and the first sizing of the store is provably too
    small for them, so a later batch moves the records and the identity words kept so far (with second_best the
    homopolymer words too) into larger blocks."""
    mono, job = regrow_case.job()
    got, stats = _one(mono, job if source == "host" else _device_reads(job), len(job), second_best=second_best,
                      max_batch_rows=regrow_case.MAX_BATCH_ROWS)
    assert stats["batches"] == regrow_case.n_chunks(job)
    _same(got, regrow_host_rows(second_best))
    assert len(got.rows) > 0 and stats["fallback_blocks"] == 0 and stats["ident_pairs"] > 0
