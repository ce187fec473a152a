"""Profiles folded on the device (Stream(final=True, device_final=True, device_profile=True), lib.final_profile_device):
the plan / group / fold kernels against the existing host fold (lib.profile_segments(device=None)), and the profiles of
such streams against those of the host profile stream (Stream(final=True, profile=True)) for the same jobs.  The counts
are integers: every comparison is exact.  The host streams' profiles are computed once per parameter set."""
import json
import os
import random

import numpy as np
import pytest
import torch

import device_profile_cases as dpc
from conftest import GOLDEN

from stringdecomposer_amd import formats, lib, synth

pytestmark = pytest.mark.gpu

FINAL = os.path.join(GOLDEN, "final")
THREADS = 8


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------

def _both(case, ms):
    want, short, long_ = dpc.expected(case, ms, threads=THREADS)
    got, pairs, intact = lib.final_profile_device(case["text"], case["read_off"], case["rows"], case["row_off"], case["keep"], ms,
                                                  threads=THREADS)
    assert intact, "a guard word behind the count buffer was overwritten"
    dpc.same(got, want)
    assert sum(formats.profile_instances(c) for c in got) == short + long_
    return pairs, short, long_


def _monos(n, length, seed=7):
    return [m.decode() for m in synth.make_monomers(n, seed=seed, length=length)[1]]


def test_kernels_12x171_groups_of_every_size():
    """4 000 rows, every fourth dropped, five reads of which one has no rows.  Of the 3 000 kept pairs monomer 0 has
    none (dropped rows of it only), monomer 1 exactly 128 -- a whole number of 64-pair items -- and monomer 2 1 100."""
    ms = _monos(12, 171)
    r = random.Random(1)
    kept_of = [1] * 128 + [2] * 1100 + [3 + r.randrange(9) for _ in range(3000 - 1228)]
    r.shuffle(kept_of)
    which, keep, k = [], [], 0
    for i in range(4000):
        if i % 4 == 3:
            which.append(r.randrange(3))
            keep.append(0)
        else:
            which.append(kept_of[k])
            keep.append(1)
            k += 1
    seq, st, en, pt = dpc.segments(ms, 4000, seed=12, which=which)
    case = dpc.as_rows(seq, st, en, pt, 12, [0, 900, 1700, 3100, 4000], keep, empty_read=2)
    assert len(case["read_off"]) == 6 and 0 in np.diff(case["row_off"])
    pairs, short, long_ = _both(case, ms)
    assert pairs == (3000, 0) == (short, long_)
    want, _, _ = dpc.expected(case, ms, threads=THREADS)
    inst = [formats.profile_instances(c) for c in want]
    assert inst[0] == 0 and inst[1] == 128 and inst[2] == 1100


@pytest.mark.parametrize("n_mono,length,n_seg", [(130, 60, 600), (5, 480, 300)], ids=["130x60", "5x480"])
def test_kernels_many_monomers_and_long_templates(n_mono, length, n_seg):
    """130 monomers: more than the lanes of a wave in the histogram; 480 bp: eight words per template."""
    ms = _monos(n_mono, length)
    seq, st, en, pt = dpc.segments(ms, n_seg, seed=n_mono)
    keep = [0 if i % 5 == 2 else 1 for i in range(n_seg)]
    case = dpc.as_rows(seq, st, en, pt, n_mono, [0, n_seg // 3, n_seg // 3, n_seg], keep)
    pairs, short, long_ = _both(case, ms)
    assert pairs == (short, 0) and long_ == 0 and short == sum(keep)


def test_kernels_one_base_templates():
    """Templates of 1, 2 and 171 bases (K = 1 .. 3)."""
    ms = ["A", "CG", _monos(1, 171, seed=9)[0]]
    seq, st, en, pt = dpc.segments(ms, 500, seed=3, max_extra=8)
    case = dpc.as_rows(seq, st, en, pt, 3, [0, 200, 500], [1] * 500)
    pairs, short, long_ = _both(case, ms)
    assert pairs == (500, 0)


def test_kernels_boundary_lengths():
    """Segments of 1, 1023, 1024 and 1025 bases and one of 1 500: the last two are left to the host, and the counts are
    the host fold's all the same.  A row that runs past its read's end and one that begins behind it."""
    ms = _monos(3, 171, seed=4)
    seq, st, en, pt = dpc.segments(ms, 60, seed=8)
    r = random.Random(3)
    pos = len(seq)
    for ln in (1, 1023, 1024, 1025, 1500):
        seq += "".join(r.choice("ACGT") for _ in range(ln))
        st.append(pos)
        en.append(pos + ln - 1)
        pt.append(r.randrange(6))
        pos += ln
    case = dpc.as_rows(seq, st, en, pt, 3, [0, 20, 65], [1] * 65)
    rl = int(case["read_off"][-1] - case["read_off"][-2])
    case["rows"] = np.concatenate([case["rows"], np.array([[1, rl - 100, rl + 500, 0], [4, rl + 10, rl + 200, 0]], dtype=np.int32)])
    case["row_off"][-1] += 2
    case["keep"] = np.concatenate([case["keep"], np.array([1, 1], dtype=np.uint8)])
    pairs, short, long_ = _both(case, ms)
    assert pairs == (64, 2) == (short, long_)


def test_kernels_kilobase_monomers_go_to_the_host():
    ms = _monos(3, 1100)
    seq, st, en, pt = dpc.segments(ms, 30, seed=5)
    case = dpc.as_rows(seq, st, en, pt, 3, [0, 10, 30], [1] * 30)
    pairs, short, long_ = _both(case, ms)
    assert pairs == (0, 30)


def test_kernels_without_reads_and_without_rows():
    ms = _monos(3, 171)
    none = dict(text="", read_off=np.zeros(1, dtype=np.int64), rows=np.zeros((0, 4), dtype=np.int32),
                row_off=np.zeros(1, dtype=np.int64), keep=np.zeros(0, dtype=np.uint8))
    assert _both(none, ms)[0] == (0, 0)
    bare = dict(none, text="ACGT" * 15, read_off=np.array([0, 10, 30, 60], dtype=np.int64), row_off=np.zeros(4, dtype=np.int64))
    assert _both(bare, ms)[0] == (0, 0)


# ---- 2. streams against the host profile stream ---------------------------------------------------------------------

def _job(seed=7):
    """(the multi-batch job of test_gpu_device_final.py with unique names) twelve monomers, five reads of 800 - 61 000
    bp, two of them spanning batches of 20 000 rows, runs of N in three."""
    mn, ms = synth.make_monomers(12, seed=seed)
    rs = []
    for i, ln in enumerate([3000, 47000, 800, 12000, 61000]):
        s = bytearray(synth.make_reads(ms, 1, read_len=ln, seed=seed, first_index=i)[1][0])
        if i in (1, 3, 4):
            s[ln // 3:ln // 3 + 40] = b"N" * 40
        rs.append(bytes(s))
    return (list(mn), ms), rs


MB = dict(sub_batches=4, max_batch_rows=20000)
PLAIN = {}


def _stream(mono, **kw):
    return lib.Stream(mono[1], final=True, mono_names=mono[0], threads=THREADS, **kw)


def _device_reads(seqs):
    return lib.DeviceReads(torch.frombuffer(bytearray(b"".join(seqs) + b"#"), dtype=torch.uint8).to("cuda:0"), [len(s) for s in seqs])


@pytest.fixture(scope="module")
def job():
    return _job()


@pytest.fixture(scope="module")
def host(job):
    """(FinalRows, Profile) of the host profile stream for a read list, by (second_best, min_identity, flags); once each"""
    mono, reads = job
    have = {}

    def get(second_best=False, min_identity=0, flags=0):
        key = (second_best, min_identity, flags)
        if key not in have:
            st = _stream(mono, profile=True, second_best=second_best, min_identity=min_identity, flags=flags, **MB)
            try:
                st.submit(reads)
                rows = st.collect()
                assert st.stats()["batches"] >= 4
                have[key] = (rows, st.profile())
            finally:
                st.close()
        return have[key]
    return get


def _one(mono, reads_in, device_profile=True, **kw):
    st = _stream(mono, device_final=True, device_profile=device_profile, **kw)
    try:
        st.submit(reads_in)
        rows = st.collect_final_device().to_host()
        return rows, (st.profile() if device_profile else None), st.stats()
    finally:
        st.close()


def _same_rows(got, want):
    assert got.rows.tobytes() == want.rows.tobytes() and np.array_equal(got.row_off, want.row_off)
    assert (got.alt is None) == (want.alt is None)
    if want.alt is not None:
        assert got.alt.tobytes() == want.alt.tobytes()


@pytest.fixture(scope="module")
def threshold(host):
    """(test_min_identity_drops_rows_on_the_device's choice) 95, or the set's median"""
    def get(second_best):
        ident = np.sort(host(second_best)[0].rows["ident"])
        thr = 95 if ident[0] < 95 <= ident[-1] else int(np.ceil(ident[len(ident) // 2]))
        assert 0 < len(host(second_best, thr)[0].rows) < len(ident), "the threshold %d must split the rows" % thr
        return thr
    return get


@pytest.mark.parametrize("split", [False, True], ids=["all_rows", "min_identity"])
@pytest.mark.parametrize("second_best", [False, True])
@pytest.mark.parametrize("source", ["host", "device"])
def test_stream_profile_equals_the_host_profile_stream(job, host, threshold, source, second_best, split):
    mono, reads = job
    thr = threshold(second_best) if split else 0
    want_rows, want = host(second_best, thr)
    src = reads if source == "host" else _device_reads(reads)
    kw = dict(second_best=second_best, min_identity=thr, **MB)
    rows, got, stats = _one(mono, src, **kw)
    assert got.names == want.names and got.seqs == want.seqs
    dpc.same(got.counts, want.counts)
    assert sum(formats.profile_instances(c) for c in got.counts) == len(rows.rows) > 0
    _same_rows(rows, want_rows)
    if (second_best, thr) not in PLAIN:             # the device-final stream without the flag, once per parameter set
        PLAIN[(second_best, thr)] = _one(mono, src, device_profile=False, **kw)[0]
    _same_rows(rows, PLAIN[(second_best, thr)])
    assert stats["profile_pairs_device"] == len(rows.rows) and stats["profile_pairs_host"] == 0
    assert stats["profile_text_to_host"] == 0 and stats["fallback_blocks"] == 0 and stats["batches"] >= 4
    assert stats["profile_ms"] > 0


# ---- 3. pipelined jobs, reset, the profile on the device ----------------------------------------------------------------

def test_pipelined_jobs_reset_and_profile_device():
    mn, ms = synth.make_monomers(10, seed=5)
    jobs = [synth.make_reads(ms, 3 + j, read_len=9000 + 4000 * j, seed=20 + j)[1] for j in range(5)]
    jobs[2] = [jobs[2][0][:60]]
    kw = dict(sub_batches=2, min_identity=70, max_batch_rows=25000)
    total = None
    for j in jobs:                                   # one at a time, on the host profile stream
        st = _stream((mn, ms), profile=True, **kw)
        try:
            st.submit(j)
            st.collect()
            p = st.profile()
        finally:
            st.close()
        total = p.counts if total is None else [a + b for a, b in zip(total, p.counts)]
    side = torch.cuda.Stream(device=0)
    st = _stream((mn, ms), device_final=True, device_profile=True, **kw)
    try:
        n_rows = sum(d.n_rows for d in st.imap([_device_reads(j) for j in jobs], depth=2, device=True))
        got = st.profile()
        dpc.same(got.counts, total)
        assert sum(formats.profile_instances(c) for c in got.counts) == n_rows > 0
        # on a side stream: a fill of the buffer's memory before the call, a read behind it, no host synchronisation
        dp = st.profile_device(stream=side)
        with torch.cuda.stream(side):
            copy = dp.counts.clone()
        assert dp.counts.dtype == torch.int64 and dp.counts.is_cuda and dp.counts.shape == (dp.offsets[-1],)
        L = lib.load()
        import ctypes as C
        n = C.c_int64()
        buf = torch.empty(dp.offsets[-1] + 16, dtype=torch.int64, device="cuda:0")
        with torch.cuda.stream(side):
            buf.fill_(-7)
        st._check(L.sd_stream_profile_dev(st.h, 0, C.c_void_p(buf.data_ptr()), dp.offsets[-1] + 16, C.c_void_p(side.cuda_stream),
                                          C.byref(n), st._err, 4096))
        with torch.cuda.stream(side):
            seen = buf.clone()
        side.synchronize()
        assert n.value == dp.offsets[-1]
        assert bool((seen[n.value:] == -7).all()), "guard words behind the caller's count buffer"
        flat = np.concatenate([c.reshape(-1) for c in got.counts])
        assert np.array_equal(seen[:n.value].cpu().numpy(), flat) and np.array_equal(copy.cpu().numpy(), flat)
        dpc.same(dp.to_host().counts, got.counts)
        assert dp.to_host().names == got.names
        # a short buffer is refused with the exact size
        rc = L.sd_stream_profile_dev(st.h, 0, C.c_void_p(buf.data_ptr()), n.value - 1, None, C.byref(n), st._err, 4096)
        assert rc == lib.SD_ERR_PARAM and str(dp.offsets[-1]) in st._err.value.decode() and n.value == dp.offsets[-1]
        dpc.same(st.profile(reset=True).counts, total)
        assert all((c == 0).all() for c in st.profile().counts)
        assert bool((st.profile_device().counts == 0).all())
        assert st.stats()["jobs"] == 5 and st.stats()["profile_pairs_device"] == n_rows
    finally:
        st.close()


# ---- 4. the text-based path and the host's pairs --------------------------------------------------------------------------

def test_text_based_jobs_fold_on_the_host(job, host):
    mono, reads = job
    want_rows, want = host(False)
    for src in (reads, _device_reads(reads)):
        rows, got, stats = _one(mono, src, flags=lib.FLAG_NO_STREAM_IDENT, **MB)
        _same_rows(rows, want_rows)
        dpc.same(got.counts, want.counts)
        assert stats["profile_pairs_device"] == 0 and stats["profile_pairs_host"] == len(rows.rows)
        assert stats["fallback_blocks"] > 0


def _fasta(path):
    names, seqs, _ = lib.fasta_load(path)
    return [n.split()[0] for n in names], [s.upper() for s in seqs]


def test_long_block_golden():
    """A ~19.6-kb block that edlib aligns by Hirschberg's split: the job takes the text-based path."""
    with open(os.path.join(FINAL, "long_block", "params.json")) as f:
        c = json.load(f)
    reads, mono = _fasta(os.path.join(GOLDEN, c["inputs"][0])), _fasta(os.path.join(GOLDEN, c["inputs"][1]))
    kw = dict(second_best=True, part_size=30000)
    st = _stream(mono, profile=True, **kw)
    try:
        st.submit(reads[1])
        want_rows = st.collect()
        want = st.profile()
    finally:
        st.close()
    rows, got, stats = _one(mono, reads[1], **kw)
    _same_rows(rows, want_rows)
    dpc.same(got.counts, want.counts)
    assert len(rows.rows) == c["final_rows"] == sum(formats.profile_instances(x) for x in got.counts)
    assert stats["fallback_blocks"] > 0


def test_kilobase_monomers_fold_on_the_host():
    mn, ms = synth.make_monomers(3, seed=13, length=1100)
    reads = synth.make_reads(ms, 1, read_len=20000, seed=13)[1]
    st = _stream((mn, ms), profile=True)
    try:
        st.submit(reads)
        want_rows = st.collect()
        want = st.profile()
    finally:
        st.close()
    rows, got, stats = _one((mn, ms), _device_reads(reads))
    _same_rows(rows, want_rows)
    dpc.same(got.counts, want.counts)
    assert len(rows.rows) > 0 and stats["profile_pairs_device"] == 0 and stats["profile_pairs_host"] == len(rows.rows)


# ---- 5. lifetime ------------------------------------------------------------------------------------------------------

def test_close_right_after_collect_with_the_fold_still_queued(job, host):
    """Stream.close() right behind collect_final_device(): the fold was enqueued a moment ago on the stream's own
    stream; the library waits for it before its buffers go back.  Nothing is waited for here, and whoever takes the
    buffers next computes what it should."""
    mono, reads = job
    st = _stream(mono, device_final=True, device_profile=True, **MB)
    try:
        st.submit(_device_reads(reads))
        st.collect_final_device()                      # (warm)
        st.submit(_device_reads(reads))
        st.submit(reads)
        st.collect_final_device()
        got = st.collect_final_device()
    finally:
        st.close()
    rows, prof, _ = _one(mono, reads[::-1], **MB)
    assert got.n_rows == len(host(False)[0].rows) == len(rows.rows)
    assert sum(formats.profile_instances(c) for c in prof.counts) == len(rows.rows)
