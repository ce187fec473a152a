"""Rows assembled on the device (Stream(device_rows=True) -> collect_device / imap(device=True), Engine.rows_device,
lib.seam_merge_device): the assembly kernels against the literal host merge, and the device rows of streams and engines
against the rows the same stream returns in host memory and against a committed golden.  Every comparison is exact.
The reads are short (the longest 23 kb) and every stream is created once per parameter set; one test takes two jobs of
the benchmark's shape, cut from one small device buffer, because only record stores of that size go through the buffer pool."""
import ctypes as C

import numpy as np
import pytest
import torch

import regrow_case
import seam_cases
from conftest import load_case

from stringdecomposer_amd import lib, synth

pytestmark = pytest.mark.gpu

THREADS = 8
READ_LENGTHS = [1, 499, 500, 5000, 5499, 5500, 5501, 23000]
SENTINEL = -559038737      # 0xDEADBEEF as int32


# ---- 1. the assembly kernels alone --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def merge_cases():
    """The lists of the CPU test plus one of 20 000 records (1 250 pieces of 16, 2 500 of 8: the chain's shuffle scan
    runs many rounds of 64 with a carry), and what the literal merge makes of each."""
    lists = seam_cases.all_lists()
    lists.append(seam_cases.random_list(seam_cases.random.Random(77), 20000))
    lists.append([])
    return lists, seam_cases.pack(lists), seam_cases.expected(lists)


@pytest.mark.parametrize("piece", [8, 0])
def test_merge_kernels_equal_the_literal_merge(merge_cases, piece):
    lists, (recs, off), exp = merge_cases
    assert len(exp[-2]) < len(lists[-2]) == 20000
    rows, row_off, intact = lib.seam_merge_device(recs, off, piece=piece, pad=4)
    assert intact, "a sentinel word beside rows / row_off was overwritten"
    assert int(row_off[0]) == 0 and int(row_off[-1]) == len(rows) == sum(len(e) for e in exp)
    for r in range(len(lists)):
        assert seam_cases.rows_of(rows, row_off, r) == exp[r], "list %d (%d records), piece %d" % (r, len(lists[r]), piece)


def test_merge_kernels_without_reads():
    rows, row_off, intact = lib.seam_merge_device(np.zeros((0, 4), np.int32), [0], pad=2)
    assert intact and len(rows) == 0 and list(row_off) == [0]
    rows, row_off, intact = lib.seam_merge_device(np.zeros((0, 4), np.int32), [0, 0, 0], pad=2)
    assert intact and len(rows) == 0 and list(row_off) == [0, 0, 0]


# ---- 2. streams ---------------------------------------------------------------------------------------------------

def _to_dev(buf):
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).to("cuda:0")


def _device_reads(seqs):
    return lib.DeviceReads(_to_dev(b"".join(seqs) + b"#"), [len(s) for s in seqs])


def _lists(dr):
    """DeviceRows -> list over reads of [(tmpl, start, end, score), ...]"""
    assert dr.rows.dtype == torch.int32 and dr.rows.shape == (dr.n_rows, 4) and dr.rows.is_cuda
    assert dr.row_off.dtype == torch.int64 and dr.row_off.is_cuda and dr.row_off.device == dr.rows.device
    rows, off = dr.rows.cpu().numpy(), dr.row_off.cpu().numpy()
    assert int(off[0]) == 0 and int(off[-1]) == dr.n_rows
    return [seam_cases.rows_of(rows, off, r) for r in range(len(off) - 1)]


@pytest.fixture(scope="module")
def mono():
    return synth.make_monomers(12, seed=3)


@pytest.fixture(scope="module")
def reads(mono):
    return [synth.make_reads(mono[1], 1, read_len=n, seed=11 + i)[1][0] for i, n in enumerate(READ_LENGTHS)]


def _host_rows(ms, jobs, **kw):
    st = lib.Stream(ms, threads=THREADS, **kw)
    try:
        return list(st.imap(jobs, as_lists=True)), st.stats()
    finally:
        st.close()


def _device_rows(ms, jobs, **kw):
    st = lib.Stream(ms, threads=THREADS, device_rows=True, **kw)
    try:
        return [_lists(dr) for dr in st.imap(jobs, device=True)], st.stats()
    finally:
        st.close()


@pytest.fixture(scope="module")
def default_rows(mono, reads):
    return _host_rows(mono[1], [reads])[0][0]


def test_reads_do_merge(mono, reads, default_rows):
    """A pass cannot come from inputs that never merge: the 23-kb read has more records before the merge than rows."""
    e = lib.Engine(mono[1], threads=THREADS)
    try:
        e.load_reads(reads)
        e.run()
        per_chunk = e.fetch()
    finally:
        e.close()
    n_chunks = [len(lib.chunk_plan(len(s))) for s in reads]
    assert sum(n_chunks) == len(per_chunk)
    before, at = [], 0
    for n in n_chunks:
        before.append(sum(len(c) for c in per_chunk[at:at + n]))
        at += n
    assert any(b > len(r) for b, r in zip(before, default_rows)), (before, [len(r) for r in default_rows])


@pytest.mark.parametrize("source", ["host", "device"])
def test_stream_rows_default_chunks(mono, reads, default_rows, source):
    job = reads if source == "host" else _device_reads(reads)
    got, stats = _device_rows(mono[1], [job])
    assert got == [default_rows]
    assert stats["host_assemble_ms"] == 0 and stats["jobs"] == 1


@pytest.mark.parametrize("source", ["host", "device"])
def test_stream_rows_thirty_chunks(mono, source):
    read = synth.make_reads(mono[1], 1, read_len=6000, seed=5)[1]
    assert len(lib.chunk_plan(6000, 200, 50)) == 30
    exp, _ = _host_rows(mono[1], [read], part_size=200, overlap=50)
    got, _ = _device_rows(mono[1], [read if source == "host" else _device_reads(read)], part_size=200, overlap=50)
    assert got == exp
    assert len(exp[0][0]) > 0


@pytest.mark.parametrize("source", ["host", "device"])
def test_read_that_spans_batches(mono, reads, default_rows, source):
    """max_batch_rows = 6000: every 5.5-kb chunk is a batch of its own, so the 23-kb read's five chunks arrive in five
    appends, and the store outgrows what its first batch sized it for."""
    long_read = [reads[-1]]
    st = lib.Stream(mono[1], threads=THREADS, device_rows=True, max_batch_rows=6000)
    try:
        st.submit(long_read if source == "host" else _device_reads(long_read))
        alone = _lists(st.collect_device())
        assert st.stats()["batches"] >= 3
        st.submit(reads if source == "host" else _device_reads(reads))
        every = _lists(st.collect_device())
    finally:
        st.close()
    assert alone == [default_rows[-1]]
    assert every == default_rows


def test_two_jobs_outstanding_then_an_empty_job(mono, reads, default_rows):
    a, b = reads[:5], reads[5:]
    st = lib.Stream(mono[1], threads=THREADS, device_rows=True)
    try:
        got = list(st.imap([a, _device_reads(b), []], device=True, depth=2))
        assert st.stats()["jobs"] == 3
    finally:
        st.close()
    assert [_lists(g) for g in got[:2]] == [default_rows[:5], default_rows[5:]]
    assert got[2].n_rows == 0 and got[2].rows.shape == (0, 4) and got[2].row_off.cpu().tolist() == [0]


def test_device_list_of_one_entry(mono, reads, default_rows):
    got, _ = _device_rows(mono[1], [reads], devices=[0])
    assert got == [default_rows]


# ---- 3. a committed golden ----------------------------------------------------------------------------------------

def test_golden_raw_tsv_from_device_tensors():
    c = load_case("syn12_part700_ov100")
    rn, rs, _ = lib.fasta_load(c["reads"])
    mn, ms, _ = lib.fasta_load(c["monomers"])
    got, _ = _device_rows(ms, [_device_reads(rs)], part_size=c["part"], overlap=c["overlap"])
    tn = list(mn) + [n + "'" for n in mn]
    assert b"".join(lib.format_rows(n, tn, r) for n, r in zip(rn, got[0])) == c["raw"]


# ---- 4. scaled scores, the generic family -------------------------------------------------------------------------

def test_scaled_scores(mono, reads):
    scoring = (-2, -4, -2, 2)
    info = lib.plan_info(mono[1], scoring=scoring)
    if info["family"] != "fast" or info["score_factor"] == 1:
        pytest.skip("no fast-family plan divides a common factor out of %r: %r" % (scoring, info))
    job = reads[3:7]
    exp, _ = _host_rows(mono[1], [job], scoring=scoring)
    got, _ = _device_rows(mono[1], [job], scoring=scoring)
    assert got == exp
    assert any(r[3] % info["score_factor"] == 0 and r[3] != 0 for r in exp[0][0])


def test_generic_family(mono, reads):
    job = reads[1:6]
    exp, _ = _host_rows(mono[1], [job], kernel=lib.KERNEL_GENERIC)
    got, _ = _device_rows(mono[1], [job], kernel=lib.KERNEL_GENERIC)
    assert got == exp


# ---- 5. the engine ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["host", "device"])
def test_engine_rows_device(mono, reads, default_rows, source):
    e = lib.Engine(mono[1], threads=THREADS)
    try:
        e.load_reads(reads if source == "host" else _device_reads(reads))
        e.run()
        exp = e.rows()
        got = e.rows_device()
        again = e.rows_device()
        assert _lists(got) == exp == default_rows
        assert _lists(again) == exp
    finally:
        e.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------

def test_refusals(mono, reads):
    mn, ms = mono
    with pytest.raises(lib.SdError) as e:
        lib.Stream(ms, final=True, mono_names=mn, device_rows=True)
    assert e.value.code == lib.SD_ERR_PARAM and "final" in e.value.msg
    with pytest.raises(lib.SdError) as e:
        lib.Stream(ms, devices=[0, 0], device_rows=True)
    assert e.value.code == lib.SD_ERR_PARAM and "one entry" in e.value.msg
    st = lib.Stream(ms, threads=THREADS, device_rows=True)
    try:
        st.submit(reads[:4])
        with pytest.raises(lib.SdError) as e:
            st.collect()
        assert e.value.code == lib.SD_ERR_PARAM and "sd_stream_collect_dev" in e.value.msg
        assert len(_lists(st.collect_device())) == 4      # (the refusal left the job where it was)
    finally:
        st.close()
    st = lib.Stream(ms, threads=THREADS)
    try:
        st.submit(reads[:2])
        with pytest.raises(lib.SdError) as e:
            st.collect_device()
        assert e.value.code == lib.SD_ERR_PARAM and "SD_FLAG_DEVICE_ROWS" in e.value.msg
        assert st.collect() > 0
    finally:
        st.close()


def test_buffer_one_row_short(mono, reads, default_rows):
    """cap_rows = n_rows - 1: an error that names both counts, nothing written (neither into the buffer nor behind it), and
    the job is still there for the call with enough room."""
    L = lib.load()
    st = lib.Stream(mono[1], threads=THREADS, device_rows=True)
    try:
        st.submit(reads)
        nr, cap = C.c_int32(), C.c_int64()
        st._check(L.sd_stream_peek_dev(st.h, C.byref(nr), C.byref(cap), st._err, 4096))
        n_rows = sum(len(r) for r in default_rows)
        assert nr.value == len(reads) and cap.value >= n_rows
        rows = torch.full((n_rows + 8, 4), SENTINEL, dtype=torch.int32, device="cuda:0")
        off = torch.full((nr.value + 1 + 8,), SENTINEL, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        n = C.c_int64()
        rc = L.sd_stream_collect_dev(st.h, C.c_void_p(rows.data_ptr()), n_rows - 1, C.c_void_p(off.data_ptr()), None,
                                     C.byref(n), st._err, 4096)
        assert rc == lib.SD_ERR_PARAM and n.value == n_rows
        msg = st._err.value.decode()
        assert str(n_rows) in msg and str(n_rows - 1) in msg
        torch.cuda.synchronize()
        assert bool((rows == SENTINEL).all()) and bool((off == SENTINEL).all())
        st._check(L.sd_stream_collect_dev(st.h, C.c_void_p(rows.data_ptr()), n_rows, C.c_void_p(off.data_ptr()), None,
                                          C.byref(n), st._err, 4096))
        st._n_reads.pop(0)
        torch.cuda.synchronize()
        assert n.value == n_rows
        assert bool((rows[n_rows:] == SENTINEL).all()) and bool((off[nr.value + 1:] == SENTINEL).all())
        got = lib.DeviceRows(rows[:n_rows], off[:nr.value + 1], n_rows)
        assert _lists(got) == default_rows
    finally:
        st.close()


# ---- 7. ordering --------------------------------------------------------------------------------------------------

def test_rows_are_ordered_on_the_callers_stream(mono, reads, default_rows):
    """collect_device(stream=s) on a side stream, the rows consumed on s with no host synchronisation in between; and the
    tensors of job k are still what they were after job k + 1 has been collected."""
    a, b = reads[:5], reads[5:]
    flat = lambda rows: torch.tensor([x for r in rows for x in r], dtype=torch.int32).reshape(-1, 4)
    s = torch.cuda.Stream(device=0)
    st = lib.Stream(mono[1], threads=THREADS, device_rows=True)
    try:
        st.submit(a)
        st.submit(_device_reads(b))
        first = st.collect_device(stream=s)
        with torch.cuda.stream(s):
            copy_first = first.rows.clone()                 # consumed on s, no synchronisation before it
            sum_first = first.rows.to(torch.int64).sum(dim=0)
        second = st.collect_device(stream=s)
        with torch.cuda.stream(s):
            copy_second = second.rows.clone()
        st.submit(a)                                        # a third job reuses a record store
        third = st.collect_device(stream=s)
        s.synchronize()
    finally:
        st.close()
    exp_first, exp_second = flat(default_rows[:5]), flat(default_rows[5:])
    assert torch.equal(copy_first.cpu(), exp_first) and torch.equal(copy_second.cpu(), exp_second)
    assert torch.equal(sum_first.cpu(), exp_first.to(torch.int64).sum(dim=0))
    assert torch.equal(first.rows.cpu(), exp_first)         # job k after jobs k + 1 and k + 2
    assert torch.equal(second.rows.cpu(), exp_second)
    assert torch.equal(third.rows.cpu(), exp_first)
    assert first.row_off.cpu().tolist() == np.cumsum([0] + [len(r) for r in default_rows[:5]]).tolist()


def test_backlogged_consumer_stream_and_a_larger_next_job(mono):
    """The copy into the caller's tensors runs on the CALLER's stream, whenever that stream gets to it, and reads the
    job's record store until then.  Here that stream is busy for about two seconds when job A is collected, and the next
    job, B, is larger: it must get a store of its own (a store of this size that is regrown goes to the buffer pool,
    where B's own buffers would take it).  Jobs of the benchmark's shape, so that the stores are above the pool's 4 MB:
    1 000 and 1 250 reads of 50 kb, cut from one periodic buffer on the device.  Reference: the same jobs collected with
    nothing queued ahead."""
    unit = np.frombuffer(b"".join(mono[1]), dtype=np.uint8)
    step, length, n_a, n_b = 17, 50000, 1000, 1250
    buf = torch.from_numpy(np.tile(unit, (length + step * n_b) // len(unit) + 2)).to("cuda:0")

    def job(n):
        return lib.DeviceReads(buf, [length] * n, offsets=[step * r for r in range(n)])

    s = torch.cuda.Stream(device=0)
    busy = torch.randn(8192, 8192, device="cuda:0")
    # a plain stream runs B once and leaves its engine's buffers in the library's pool, so that no multi-GB allocation
    # falls between the two collects below (the matmuls queued on `s` must outlast them)
    warm = lib.Stream(mono[1], threads=THREADS)
    try:
        warm.submit(job(n_b))
        assert warm.collect() > 0
    finally:
        warm.close()
    torch.cuda.synchronize()
    st = lib.Stream(mono[1], threads=THREADS, device_rows=True)
    try:
        st.submit(job(n_a))
        ref_a = st.collect_device()
        ref_a = (ref_a.rows.cpu(), ref_a.row_off.cpu())
        assert ref_a[0].shape[0] * 16 > (4 << 20), "the store must be one the pool takes"
        st.submit(job(n_a))
        done = torch.cuda.Event()
        with torch.cuda.stream(s):
            for _ in range(300):
                busy @ busy
            done.record(s)
        got_a = st.collect_device(stream=s)          # returns with the copy still queued behind the matmuls
        assert not done.query(), "the consumer stream was meant to be backlogged when A was collected"
        st.submit(job(n_b))
        got_b = st.collect_device()
        pending = not done.query()
        st.submit(job(n_b))
        ref_b = st.collect_device()
        s.synchronize()
        torch.cuda.synchronize()
    finally:
        st.close()
    # (`pending`: whether A's copy was still queued when B had been assembled.  It is when this test runs alone; late in
    # a long process something between the two collects -- an allocation that synchronises the device -- can let the
    # matmuls finish first, which makes the run a plain ordering check, so it is reported, not asserted.)
    assert torch.equal(got_a.rows.cpu(), ref_a[0]) and torch.equal(got_a.row_off.cpu(), ref_a[1]), "pending=%r" % pending
    assert torch.equal(got_b.rows.cpu(), ref_b.rows.cpu()) and torch.equal(got_b.row_off.cpu(), ref_b.row_off.cpu())
    assert got_b.n_rows > got_a.n_rows > 0


def test_close_right_after_collect_with_the_copy_still_queued(mono, reads, default_rows):
    """Stream.close() (and Engine.close()) with a copy still queued on the caller's stream: the library waits for it before
    its buffers go back, and the rows are what they should be."""
    s = torch.cuda.Stream(device=0)
    busy = torch.randn(4096, 4096, device="cuda:0")
    torch.cuda.synchronize()
    st = lib.Stream(mono[1], threads=THREADS, device_rows=True)
    e = lib.Engine(mono[1], threads=THREADS)
    try:
        st.submit(reads)
        e.load_reads(reads)
        e.run()
        first = _lists(e.rows_device())                  # (the run's assembly is made here, once)
        done = torch.cuda.Event()
        with torch.cuda.stream(s):
            for _ in range(60):
                busy @ busy
            done.record(s)
        got = st.collect_device(stream=s)
        got_e = e.rows_device(stream=s)                  # only the copy, queued behind the matmuls
        assert not done.query(), "the consumer stream was meant to be backlogged at close"
    finally:
        st.close()
        e.close()
    assert first == default_rows
    other, _ = _device_rows(mono[1], [reads[::-1]])      # whoever takes the buffers next
    s.synchronize()
    assert _lists(got) == default_rows and _lists(got_e) == default_rows
    assert other[0] == default_rows[::-1]


# ---- 8. the store regrown behind a later batch ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def regrow_rows():
    (_, ms), job = regrow_case.job()
    return _host_rows(ms, [job])[0]


@pytest.mark.parametrize("source", ["host", "device"])
def test_store_regrown_with_records_in_it(regrow_rows, source):
    """regrow_case's job on a fresh stream: six chunks in six batches, and the first sizing of the store is provably too
    small for them, so a later batch moves the records appended so far into a larger block."""
    (_, ms), job = regrow_case.job()
    got, stats = _device_rows(ms, [job if source == "host" else _device_reads(job)], max_batch_rows=regrow_case.MAX_BATCH_ROWS)
    assert stats["batches"] == regrow_case.n_chunks(job)
    assert got == regrow_rows
    assert len(regrow_rows[0][0]) > 0 and len(regrow_rows[0][1]) > 0
