"""The stream on several devices of one process (lib.Stream(devices=...) / sd_stream_create_devices,
sd_stream_create_final_devices) on the device: one pipeline per entry, each on a thread of its own, batches dealt across
entries and job boundaries.  Repeated ordinals put several pipelines on one MI355X, so every test but the last runs on a
machine with one GPU.  Every result is compared with the plain stream or with the reference command line's goldens."""
import ctypes as C
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

from stringdecomposer_amd import formats, lib, synth

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


def _final_stream(mono, **kw):
    return lib.Stream(mono[1], final=True, mono_names=mono[0], threads=THREADS, **kw)


def _raw_rows(ms, jobs, as_lists=True, **kw):
    """Every job through a fresh raw stream, one at a time; plus the stream's stats and per-entry stats."""
    st = lib.Stream(ms, threads=THREADS, **kw)
    try:
        out = []
        for rs in jobs:
            st.submit(rs)
            out.append(st.collect(as_lists=as_lists))
        return out, st.stats(), st.device_stats()
    finally:
        st.close()


def _long_read_job(seed=7):
    """Reads of mixed length with runs of N, among them one of 420 kb: cut into batches of 20 000 rows its chunks land
    in batches dealt to different entries."""
    mn, ms = synth.make_monomers(12, seed=seed)
    rs = []
    for i, ln in enumerate([3000, 420000, 800, 12000, 61000, 5200, 9000]):
        _, s = synth.make_reads(ms, 1, read_len=ln, seed=seed, first_index=i)
        s = bytearray(s[0])
        if i in (1, 3, 4):
            s[ln // 3:ln // 3 + 40] = b"N" * 40
        rs.append(bytes(s))
    return ms, rs


@pytest.mark.parametrize("sub_batches", [1, 3])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
@pytest.mark.parametrize("name", sorted(os.listdir(FINAL)))
def test_stream_devices_final_equals_reference_goldens(name, devices, sub_batches):
    """Every golden case of the reference command line through Stream(final=True, devices=...): final.tsv and _alt.tsv
    byte for byte (or by the committed sha256), with the job cut into at least two batches per entry."""
    c, reads, mono, kw = _case(name)
    st = _final_stream(mono, sub_batches=sub_batches, devices=devices, **kw)
    try:
        st.submit(reads[1])
        fr = st.collect()
        fin, alt = formats.final_rows(fr, reads[0], st.keys())
        fin, alt = formats.format_final(fin).encode(), formats.format_alt(alt).encode()
        stats, dev = st.stats(), st.device_stats()
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
    n_chunks = lib.chunk_table_size([len(r) for r in reads[1]], kw["part_size"], 500)
    assert stats["batches"] == min(n_chunks, max(sub_batches, 2 * len(devices)))
    assert len(dev) == len(devices) and sum(d["batches"] for d in dev) == stats["batches"]


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_stream_devices_raw_rows_equal_plain_stream(devices):
    """A job cut into many batches -- a 20 000-row cap, and sub_batches 12 at the default budget -- whose 420-kb read
    spans batches dealt to different entries: the rows (as lists and as the row count of the array form) are the
    plain stream's."""
    ms, rs = _long_read_job()
    (want,), _, _ = _raw_rows(ms, [rs])
    (want_n,), _, _ = _raw_rows(ms, [rs], as_lists=False)
    assert want_n == sum(len(r) for r in want) > 0
    for kw in ({"max_batch_rows": 20000}, {"sub_batches": 12}):
        (got,), stats, dev = _raw_rows(ms, [rs], devices=devices, **kw)
        assert got == want
        (got_n,), _, _ = _raw_rows(ms, [rs], as_lists=False, devices=devices, **kw)
        assert got_n == want_n
        assert stats["batches"] >= max(12 if "sub_batches" in kw else 20, 2 * len(devices))
        assert len(dev) == len(devices) and all(d["batches"] > 0 for d in dev)
        assert sum(d["batches"] for d in dev) == stats["batches"]
        assert all(d["device"] == 0 and d["busy_ms"] > 0 for d in dev)


@pytest.mark.parametrize("final", [False, True])
def test_stream_devices_imap_equals_jobs_one_at_a_time(final):
    """Five jobs through imap (default depth) on devices=[0, 0] -- batches of several jobs in flight on both entries --
    give the rows of the same jobs through a plain stream, one at a time."""
    mn, ms = synth.make_monomers(10, seed=5)
    jobs = [synth.make_reads(ms, 3 + j, read_len=9000 + 4000 * j, seed=20 + j)[1] for j in range(5)]
    kw = dict(sub_batches=2, max_batch_rows=25000)
    if final:
        kw.update(second_best=True)
        st = _final_stream((mn, ms), devices=[0, 0], **kw)
        piped = list(st.imap(jobs))
        st.close()
        for rs, got in zip(jobs, piped):
            st = _final_stream((mn, ms), **kw)
            st.submit(rs)
            want = st.collect()
            st.close()
            assert got.rows.tobytes() == want.rows.tobytes() and np.array_equal(got.row_off, want.row_off)
            assert np.array_equal(got.alt, want.alt)
    else:
        st = lib.Stream(ms, threads=THREADS, devices=[0, 0], **kw)
        piped = list(st.imap(jobs, as_lists=True))
        assert st.stats()["jobs"] == 5
        st.close()
        want, _, _ = _raw_rows(ms, jobs)
        assert piped == want


def test_stream_devices_read_buffers_are_free_after_submit():
    """Raw mode packs from the caller's buffers: they are overwritten as soon as submit returns (two jobs outstanding),
    and the rows are still those of the original reads."""
    ms, rs = _long_read_job(seed=9)
    jobs = [rs, rs[2:5]]
    want, _, _ = _raw_rows(ms, jobs)
    st = lib.Stream(ms, threads=THREADS, devices=[0, 0], max_batch_rows=20000)
    L = st.L
    err = C.create_string_buffer(4096)
    try:
        bufs = []
        for reads in jobs:
            b = [C.create_string_buffer(s, len(s)) for s in reads]
            ptrs = C.cast((C.c_void_p * len(b))(*[C.addressof(x) for x in b]), C.POINTER(C.c_char_p))
            lens = (C.c_int64 * len(b))(*[len(s) for s in reads])
            assert L.sd_stream_submit(st.h, ptrs, lens, len(b), err, 4096) == lib.SD_OK, err.value
            st._n_reads.append(len(b))
            for x in b:
                C.memset(x, ord("T"), C.sizeof(x))
            bufs.append(b)
        got = [st.collect(as_lists=True) for _ in jobs]
    finally:
        st.close()
    assert got == want


def _error_sequence(ms, jobs, **kw):
    """Submits every job (an error does not stop the sequence), then collects the jobs that were taken."""
    st = lib.Stream(ms, threads=THREADS, **kw)
    out = []
    try:
        taken = 0
        for rs in jobs:
            try:
                st.submit(rs)
                taken += 1
                out.append("ok")
            except lib.SdError as e:
                out.append((e.code, e.msg))
        out += [st.collect(as_lists=True) for _ in range(taken)]
    finally:
        st.close()   # returns: no driver thread is left behind
    return out


def test_stream_devices_host_input_errors_as_plain_stream():
    """A job with an empty read between two valid jobs is refused by submit with the plain stream's code and message
    (SD_ERR_EMPTY, a host validation) and the valid jobs' rows are unchanged; the final mode does the same.  The stream
    does not check the alphabet (sd_hip.h): a job with a symbol outside ACGTN gives what the plain stream gives."""
    ms, rs = _long_read_job(seed=3)
    a, b = rs[:3], rs[3:]
    empty = [a[0], b"", a[1]]
    bad = [b[0][:7000] + b"X" + b[0][7001:], b[1]]
    for devices in ([0, 0], [0, 0, 0]):
        want = _error_sequence(ms, [a, empty, b], max_batch_rows=20000)
        assert want[1][0] == lib.SD_ERR_EMPTY and want[1][1] == "ERROR: Sequence #1 is empty"
        assert _error_sequence(ms, [a, empty, b], max_batch_rows=20000, devices=devices) == want
        assert _error_sequence(ms, [a, bad, b], devices=devices) == _error_sequence(ms, [a, bad, b])
    mn = ["m%d" % i for i in range(len(ms))]
    for devices in (None, [0, 0]):
        st = _final_stream((mn, ms), devices=devices)
        try:
            with pytest.raises(lib.SdError) as e:
                st.submit(empty)
            assert e.value.code == lib.SD_ERR_EMPTY and e.value.msg == "ERROR: Sequence #1 is empty"
            st.submit(a)
            assert len(st.collect().rows) > 0
        finally:
            st.close()


def test_stream_one_entry_is_the_plain_stream():
    """devices=[0] is the plain stream on device 0: the same rows and the same batch count, one entry."""
    ms, rs = _long_read_job(seed=4)
    for kw in ({}, {"max_batch_rows": 20000}, {"sub_batches": 3}):
        want, ws, wd = _raw_rows(ms, [rs, rs[:2]], **kw)
        got, gs, gd = _raw_rows(ms, [rs, rs[:2]], devices=[0], **kw)
        assert got == want
        assert gs["batches"] == ws["batches"]
        assert len(gd) == len(wd) == 1 and gd[0]["batches"] == wd[0]["batches"] == ws["batches"]


def test_stream_on_every_visible_device():
    """With two or more GPUs: devices=list(range(n)) gives the plain stream's rows, raw and final."""
    n = lib.device_count()
    if n < 2:
        pytest.skip("needs two or more visible devices")
    ms, rs = _long_read_job(seed=6)
    want, _, _ = _raw_rows(ms, [rs, rs[1:4]])
    got, _, dev = _raw_rows(ms, [rs, rs[1:4]], devices=list(range(n)), max_batch_rows=50000)
    assert got == want and [d["device"] for d in dev] == list(range(n))
    mn = ["m%d" % i for i in range(len(ms))]
    outs = []
    for devices in (None, list(range(n))):
        st = _final_stream((mn, ms), devices=devices, second_best=True)
        st.submit(rs)
        outs.append(st.collect())
        st.close()
    assert outs[0].rows.tobytes() == outs[1].rows.tobytes() and np.array_equal(outs[0].alt, outs[1].alt)
