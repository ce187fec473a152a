"""The TSV text of device rows, formatted on the device (lib.format_final_device / format_raw_device,
Stream.collect_final_text_device / collect_text_device; csrc/sd_text_dev.hip) against its host twin on synthetic rows --
text, row_pos and read_pos, byte for byte -- and against the reference command line's goldens through device streams."""
import ctypes as C
import gzip
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import text_format_cases as tc
from conftest import GOLDEN, load_case

from stringdecomposer_amd import lib, synth

pytestmark = pytest.mark.gpu

FINAL = os.path.join(GOLDEN, "final")
THREADS = 8
FILL = 0xA5
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_final(fr):
    rows = _dev(np.frombuffer(fr.rows.tobytes(), dtype=np.uint8).reshape(-1, 80).copy())
    return lib.DeviceFinalRows(rows, _dev(fr.row_off), None if fr.alt is None else _dev(fr.alt), len(fr.rows))


def _device_raw(rows, off):
    return lib.DeviceRows(_dev(rows), _dev(off), len(rows))


def _same_text(dt, want, n_rows, n_reads):
    """a DeviceText against (bytes, row_pos, read_pos) of the host twin"""
    text, row_pos, read_pos = want
    assert dt.text.dtype == torch.uint8 and dt.text.shape == (len(text),) and dt.text.is_cuda
    assert dt.row_pos.dtype == torch.int64 and dt.row_pos.shape == (n_rows + 1,) and dt.row_pos.device == dt.text.device
    assert dt.read_pos.dtype == torch.int64 and dt.read_pos.shape == (n_reads + 1,) and dt.read_pos.device == dt.text.device
    assert dt.row_pos.cpu().numpy().tolist() == row_pos.tolist()
    assert dt.read_pos.cpu().numpy().tolist() == read_pos.tolist()
    assert dt.to_bytes() == text


# ---- 1. device equals host ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_keys", [1, 24, 260])
@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 1025])
def test_final_and_alt_text_equal_the_host_twin(n_rows, n_keys):
    """Rows across a wave (63 / 64 / 65) and across several workgroups (1025); 1, 10 and less than one final row per _alt
    workgroup (n_keys 260: two rounds of lines); names of 1 .. 300 bytes and one of 70 000, longer than the staging tile;
    reads without rows; identities of the CPU test's value set; int64 extremes."""
    job = tc.final_job(n_rows, n_keys)
    want, want_alt = lib.format_final_host(*job, threads=THREADS, positions=True)
    final, alt = lib.format_final_device(_device_final(job[0]), job[1], job[2])
    _same_text(final, want, n_rows, 8)
    _same_text(alt, want_alt, n_rows, 8)


@pytest.mark.parametrize("n_rows", [0, 1, 65, 1025])
def test_light_mode_has_no_alt_text(n_rows):
    job = tc.final_job(n_rows, 24, second_best=False)
    want, want_alt = lib.format_final_host(*job, threads=THREADS, positions=True)
    final, alt = lib.format_final_device(_device_final(job[0]), job[1], job[2])
    assert alt is None and want_alt is None
    _same_text(final, want, n_rows, 8)


@pytest.mark.parametrize("n_tmpl", [1, 24])
@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 1025])
def test_raw_text_equals_the_host_twin(n_rows, n_tmpl):
    rows, off, names, tn = tc.raw_job(n_rows, n_tmpl)
    want = lib.format_raw_host(rows, off, names, tn, threads=THREADS, positions=True)
    _same_text(lib.format_raw_device(_device_raw(rows, off), names, tn), want, n_rows, 8)


def test_no_reads():
    none = lib.FinalRows(tc.final_array(0), np.zeros(1, dtype=np.int64), np.zeros((0, 3)))
    final, alt = lib.format_final_device(_device_final(none), [], ["a", "b", "c"])
    assert final.to_bytes() == b"" == alt.to_bytes()
    assert final.row_pos.tolist() == [0] == final.read_pos.tolist() == alt.row_pos.tolist() == alt.read_pos.tolist()
    raw = lib.format_raw_device(_device_raw(np.zeros((0, 4), dtype=np.int32), np.zeros(1, dtype=np.int64)), [], ["t"])
    assert raw.to_bytes() == b"" and raw.row_pos.tolist() == [0] == raw.read_pos.tolist()


# ---- 2. the calls themselves: guard bytes, refusals ---------------------------------------------------------------------

def _final_calls(job, shift=0, text_fill=None):
    """sd_text_final_size_dev, then sd_text_final_write_dev into tensors with 64 + shift guard bytes before and 64 behind
    the text -> (rc of the size call, final tensor, alt tensor, final bytes, alt bytes); the write call is skipped
    when the size call refuses."""
    L = lib.load()
    fr, names, keys = job
    d = _device_final(fr)
    n, nr, nk = len(fr.rows), len(names), len(keys)
    pos = [torch.empty(n + 1, dtype=torch.int64, device=DEV), torch.empty(n + 1, dtype=torch.int64, device=DEV),
           torch.empty(nr + 1, dtype=torch.int64, device=DEV), torch.empty(nr + 1, dtype=torch.int64, device=DEV)]
    want = lib.format_final_host(*job, threads=THREADS) if text_fill is None else text_fill
    lead = 64 + shift
    ft = torch.full((lead + len(want[0]) + 64,), FILL, dtype=torch.uint8, device=DEV)
    at = torch.full((lead + len(want[1]) + 64,), FILL, dtype=torch.uint8, device=DEV)
    t = lib.TextTables(names, keys)
    err = C.create_string_buffer(1024)
    fb, ab = C.c_int64(), C.c_int64()
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    try:
        rc = L.sd_text_final_size_dev(t.h, p(d.rows), n, p(d.row_off), p(d.alt), nk, 0, None, p(pos[0]), p(pos[1]), p(pos[2]),
                                      p(pos[3]), C.byref(fb), C.byref(ab), err, 1024)
        if rc == lib.SD_OK:
            assert (fb.value, ab.value) == (len(want[0]), len(want[1]))
            rc2 = L.sd_text_final_write_dev(t.h, p(d.rows), n, p(d.alt), nk, 0, None, p(pos[0]), p(pos[1]),
                                            C.c_void_p(ft.data_ptr() + lead), fb.value, C.c_void_p(at.data_ptr() + lead), ab.value,
                                            err, 1024)
            assert rc2 == lib.SD_OK, err.value
        torch.cuda.synchronize()
    finally:
        t.close()
    return rc, ft.cpu().numpy(), at.cpu().numpy(), want, lead, err.value


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("n_rows,n_keys", [(1, 1), (65, 24), (1025, 24), (65, 260)])
def test_guard_bytes_around_the_text_stay(n_rows, n_keys, shift):
    """64 bytes of 0xA5 on each side of both texts (shift 5: a text buffer that does not begin on a 16-byte line): the
    narrow stores at the ends of a workgroup's range touch the range's own bytes only"""
    rc, ft, at, want, lead, msg = _final_calls(tc.final_job(n_rows, n_keys, long_name=False), shift)
    assert rc == lib.SD_OK, msg
    for got, text in ((ft, want[0]), (at, want[1])):
        assert got[lead:lead + len(text)].tobytes() == text
        assert (got[:lead] == FILL).all() and (got[lead + len(text):] == FILL).all()


@pytest.mark.parametrize("where", ["ident", "homo_second_ident", "alt"])
def test_unprintable_identity_is_refused_and_nothing_written(where):
    fr, names, keys = tc.final_job(300, 24, long_name=False)
    sizes = lib.format_final_host(fr, names, keys, threads=THREADS)
    if where == "alt":
        fr.alt[170, 23] = float("nan")
    else:
        fr.rows[where][170] = float("inf") if where == "ident" else float("nan")
    rc, ft, at, _, _, msg = _final_calls((fr, names, keys), text_fill=sizes)
    assert rc == lib.SD_ERR_UNSUPPORTED and b"1 identities" in msg
    assert (ft == FILL).all() and (at == FILL).all()
    with pytest.raises(lib.SdError) as e:
        lib.format_final_device(_device_final(fr), names, keys)
    assert e.value.code == lib.SD_ERR_UNSUPPORTED


def test_bad_indices_and_offsets_are_refused_by_the_length_pass():
    fr, names, keys = tc.final_job(300, 4, long_name=False)
    for field, value in (("read", 8), ("read", -1), ("best", 4), ("second", -2), ("homo_second", 1 << 30)):
        rows = fr.rows.copy()
        rows[field][170] = value
        with pytest.raises(lib.SdError) as e:
            lib.format_final_device(_device_final(lib.FinalRows(rows, fr.row_off, fr.alt)), names, keys)
        assert e.value.code == lib.SD_ERR_PARAM
    off = fr.row_off.copy()
    off[2] = off[3] + 1
    with pytest.raises(lib.SdError) as e:
        lib.format_final_device(_device_final(lib.FinalRows(fr.rows, off, fr.alt)), names, keys)
    assert e.value.code == lib.SD_ERR_PARAM
    with pytest.raises(lib.SdError) as e:
        lib.format_final_device(_device_final(fr), names, keys[:3])
    assert e.value.code == lib.SD_ERR_PARAM
    rows, off, rn, tn = tc.raw_job(300, 4, long_name=False)
    bad = rows.copy()
    bad[170, 0] = 4
    with pytest.raises(lib.SdError) as e:
        lib.format_raw_device(_device_raw(bad, off), rn, tn)
    assert e.value.code == lib.SD_ERR_PARAM
    bad = off.copy()
    bad[4] = bad[5] + 3
    with pytest.raises(lib.SdError) as e:
        lib.format_raw_device(_device_raw(rows, bad), rn, tn)
    assert e.value.code == lib.SD_ERR_PARAM
    final, _ = lib.format_final_device(_device_final(fr), names, keys)          # (and the calls still work)
    assert final.to_bytes() == lib.format_final_host(fr, names, keys)[0]


# ---- 3. the reference's own bytes through device streams -------------------------------------------------------------

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


@pytest.mark.parametrize("name", sorted(os.listdir(FINAL)))
def test_final_goldens_from_device_streams(name):
    """Stream(final=True, device_final=True) -> collect_final_text_device: final.tsv and alt.tsv of the unmodified reference
    command line.  long_block's rows come from the stream's text-based path; formatting is the same call."""
    c, reads, mono, kw = _golden_case(name)
    st = lib.Stream(mono[1], final=True, mono_names=mono[0], threads=THREADS, device_final=True, **kw)
    try:
        st.submit(reads[1])
        dfr, (final, alt) = st.collect_final_text_device(reads[0])
        stats = st.stats()
    finally:
        st.close()
    assert dfr.n_rows == c["final_rows"] == final.row_pos.shape[0] - 1
    with open(os.path.join(FINAL, name, "final.tsv"), "rb") as f:
        assert final.to_bytes() == f.read()
    if not kw["second_best"]:
        assert alt is None
    else:
        text = alt.to_bytes()
        assert hashlib.sha256(text).hexdigest() == c["alt_sha256"]
        gz = os.path.join(FINAL, name, "alt.tsv.gz")
        if os.path.exists(gz):
            with gzip.open(gz, "rb") as f:
                assert text == f.read()
    # (long_k17 / long_k32_mixed: monomers beyond 512 bp, which the in-stream identity kernels decline)
    assert (stats["fallback_blocks"] > 0) == (name in ("long_block", "long_k17", "long_k32_mixed"))


@pytest.mark.parametrize("name", ["td_default", "syn12_ties", "syn64_10kb"])
def test_raw_goldens_from_device_streams(name):
    c = load_case(name)
    rn, rs, _ = lib.fasta_load(c["reads"])
    mn, ms, _ = lib.fasta_load(c["monomers"])
    st = lib.Stream(ms, mono_names=list(mn), threads=THREADS, device_rows=True, part_size=c["part"], overlap=c["overlap"])
    try:
        st.submit(rs)
        drows, text = st.collect_text_device(list(rn))
    finally:
        st.close()
    assert text.to_bytes() == c["raw"]
    assert text.row_pos.shape[0] == drows.n_rows + 1 and int(text.read_pos[-1]) == len(c["raw"])


# ---- 4. ordering, tables -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def job():
    mn, ms = synth.make_monomers(12, seed=5)
    rn, rs = synth.make_reads(ms, 6, read_len=9000, seed=5)
    return (mn, ms), (rn, rs)


def test_text_is_ordered_on_the_callers_stream(job):
    """collect_final_device(stream=s), then format_final_device(stream=s) with no host synchronisation between them; a
    copy enqueued on s sees the whole text"""
    mono, reads = job
    s = torch.cuda.Stream(device=0)
    st = lib.Stream(mono[1], final=True, mono_names=mono[0], threads=THREADS, device_final=True, second_best=True)
    try:
        st.submit(reads[1])
        dfr = st.collect_final_device(stream=s)
        final, alt = lib.format_final_device(dfr, reads[0], st.keys(), stream=s)
        with torch.cuda.stream(s):
            copy_final, copy_alt = final.text.clone(), alt.text.clone()
        keys = st.keys()
        s.synchronize()
    finally:
        st.close()
    want = lib.format_final_host(dfr.to_host(), reads[0], keys, threads=THREADS)
    assert dfr.n_rows > 100 and len(want[1]) > 100000
    assert copy_final.cpu().numpy().tobytes() == want[0]
    assert copy_alt.cpu().numpy().tobytes() == want[1]


def test_one_table_object_over_three_jobs(job):
    mono, reads = job
    names, seqs = reads
    st = lib.Stream(mono[1], final=True, mono_names=mono[0], threads=THREADS, device_final=True, second_best=True)
    try:
        tables = lib.TextTables(names, st.keys())
        for k in range(3):
            st.submit(seqs[k:] + seqs[:k])
        shared, fresh = [], []
        for k in range(3):
            dfr, (final, alt) = st.collect_final_text_device(names, tables=tables)
            shared.append((final.to_bytes(), alt.to_bytes()))
            final, alt = lib.format_final_device(dfr, names, st.keys())
            fresh.append((final.to_bytes(), alt.to_bytes()))
        torch.cuda.synchronize()
        tables.close()
    finally:
        st.close()
    assert shared == fresh and len(set(shared)) == 3 and all(a and b for a, b in shared)
