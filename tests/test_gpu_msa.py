"""One row per instance (--msa) on the device: the row kernel (sd_msa_segments_dev) against the host form at every K and
at the limits where a pair changes hands, the device-resident chain (Stream(device_final=True) on DeviceReads ->
lib.final_msa_device) against lib.final_msa_host on the rows of the same job, and the command line's _msa.tsv."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import msa_cases
import msa_ref
import profile_ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8


def _same(a, b):
    assert (a.row_at == b.row_at).all()
    assert (a.status == b.status).all()
    assert a.rows.shape == b.rows.shape
    bad = np.nonzero(a.rows != b.rows)[0]
    assert bad.size == 0, "first differing byte at %d (pair %d)" % (bad[0], np.searchsorted(b.row_at, bad[0], side="right") - 1)


def _dev_equals_host(seq, st, en, monos, pt):
    dev = lib.msa_segments(seq, st, en, monos, pt, threads=THREADS, device=0)
    host = lib.msa_segments(seq, st, en, monos, pt, threads=THREADS)
    _same(dev, host)
    return host


@pytest.mark.parametrize("length", [1, 64, 65, 130, 200, 260, 390, 512])
def test_device_rows_equal_host_at_every_k(length):
    """K = 1, 1, 2, 3, 4, 6 (5 words), 8 (7 words), 8; 512 bp is past what 64 staged rows of LDS hold: written through."""
    monos = [msa_cases.random_monomer(length, 7 * length + i) for i in range(3)]
    seq, st, en, pt = msa_cases.segments(monos, 300, seed=length, max_extra=min(40, 4 * length))
    host = _dev_equals_host(seq, st, en, monos, pt)
    assert {0, 1} == {p & 1 for p in pt} and "N" in seq
    assert (host.status == 1).all()


def test_device_rows_at_the_segment_limits():
    """Segments of 1, 1024 and 1025 bp (the last is the host's), either orientation, among ordinary pairs."""
    monos = [msa_cases.random_monomer(171, 50 + i) for i in range(4)]
    seq, st, en, pt = msa_cases.segments(monos, 200, seed=9)
    r = random.Random(2)
    for n in (1, 1024, 1025):
        for o in (0, 1):
            t = profile_ref.rc(monos[1]) if o else monos[1]
            q = t[:1] if n == 1 else "".join(r.choice("ACGTN") for _ in range((n - 171) // 2)) + t
            q += "".join(r.choice("ACGT") for _ in range(n - len(q)))
            assert len(q) == n
            st.append(len(seq))
            en.append(len(seq) + n - 1)
            pt.append(2 + o)
            seq += q
    st.append(7)   # an empty segment: no instance
    en.append(6)
    pt.append(5)
    host = _dev_equals_host(seq, st, en, monos, pt)
    assert host.status[-1] == 0 and (host.status[:-1] == 1).all()


def test_set_with_a_513_bp_monomer_is_the_hosts():
    monos = [msa_cases.random_monomer(171, 1), msa_cases.random_monomer(513, 2)]
    seq, st, en, pt = msa_cases.segments(monos, 120, seed=4)
    _dev_equals_host(seq, st, en, monos, pt)


def test_groups_of_one_and_of_sixty_five_pairs():
    monos = [msa_cases.random_monomer(171, 60 + i) for i in range(3)]
    a = msa_cases.segments(monos[:1], 1, seed=1)
    b = msa_cases.segments(monos[1:2], 65, seed=2)
    seq = a[0] + b[0]
    st = a[1] + [x + len(a[0]) for x in b[1]]
    en = a[2] + [x + len(a[0]) for x in b[2]]
    pt = a[3] + [p + 2 for p in b[3]]
    _dev_equals_host(seq, st, en, monos, pt)


def test_edges_on_the_device():
    """The hand-made edges of test_msa_cpu (insertions in slot 0 and L, first and last position deleted, the insertion
    run of 300 bases that saturates, templates of 1, 63, 64 and 65 bp in one set) through the kernel."""
    seq, st, en, pt, monos, named = msa_cases.edges()
    host = _dev_equals_host(seq, st, en, monos, pt)
    msa_ref.same(host, msa_ref.segments(seq, st, en, monos, pt))
    assert formats.msa_row(host, named["ins_300"], 2)[1][80] == 255


def test_device_rows_realistic_shape():
    mn, ms = synth.make_monomers(12, seed=7, length=171)
    ms = [m.decode() for m in ms]
    seq, st, en, pt = msa_cases.segments(ms, 3000, seed=12)
    host = _dev_equals_host(seq, st, en, ms, pt)
    prof = lib.profile_segments(seq, st, en, ms, pt, threads=THREADS, device=0)
    for c, p in zip(formats.msa_counts(host, pt, len(ms)), prof):
        assert (c[:, :7] == p[:, :7]).all()


# ---- the device-resident chain -----------------------------------------------------------------------------------------

def _device_reads(rs):
    import torch
    data = torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).to("cuda:0")
    return lib.DeviceReads(data, [len(s) for s in rs])


def _final_job(mn, ms, rs, **kw):
    """(DeviceFinalRows from Stream(device_final=True) on DeviceReads, the DeviceReads, keys, FinalRows of the plain stream)"""
    dr = _device_reads(rs)
    st = lib.Stream(ms, final=True, mono_names=mn, threads=THREADS, device_final=True, **kw)
    try:
        st.submit(dr)
        dfr = st.collect_final_device()
        keys = st.keys()
    finally:
        st.close()
    st = lib.Stream(ms, final=True, mono_names=mn, threads=THREADS, **kw)
    try:
        st.submit(rs)
        fr = st.collect()
        assert st.keys() == keys
    finally:
        st.close()
    return dfr, dr, keys, fr


@pytest.fixture(scope="module")
def synth_job():
    mn, ms = synth.make_monomers(12, seed=21)
    rn, rs = synth.make_reads(ms, 3, read_len=20000, seed=21)
    return mn, ms, rs


@pytest.mark.parametrize("kw", [{}, {"second_best": True, "min_identity": 95}], ids=["light", "second_best_i95"])
def test_final_msa_device_equals_host_on_the_rows_of_the_job(synth_job, kw):
    import torch
    mn, ms, rs = synth_job
    dfr, dr, keys, fr = _final_job(mn, ms, rs, **kw)
    assert dfr.n_rows == len(fr.rows) > (0 if kw else 100)   # (-i 95 keeps a handful of the synthetic instances)
    host, pt = lib.final_msa_host(fr, rs, keys, mn, ms, threads=THREADS)
    side = torch.cuda.Stream(device=dfr.rows.device)
    dm = lib.final_msa_device(dfr, dr, keys, mn, ms, stream=side)
    assert dm.rows.is_cuda and dm.rows.dtype == torch.uint8 and dm.row_at.dtype == torch.int64 and dm.status.dtype == torch.uint8
    with torch.cuda.stream(side):   # ordered on the side stream: a copy enqueued there, and that stream alone waited for
        got = [x.to("cpu", non_blocking=False) for x in (dm.rows, dm.row_at, dm.status)]
    side.synchronize()
    got = formats.Msa(got[0].numpy(), got[1].numpy(), got[2].numpy(), dm.tlen)
    _same(got, host)
    plan, _ = lib.final_msa_classes(fr, [len(s) for s in rs], keys, mn, ms)
    assert dm.classes == plan and plan[2] == 0 and not (got.status == 2).any()
    _same(dm.to_host(), host)
    # the rows of the job, summed per monomer, are its profile
    text = b"".join(rs)
    off = np.cumsum([0] + [len(s) for s in rs])
    st_ = [int(off[r] + max(s, 0)) for r, s in zip(fr.rows["read"], fr.rows["start"])]
    en_ = [int(off[r] + min(e, len(rs[r]) - 1)) for r, e in zip(fr.rows["read"], fr.rows["end"])]
    prof = lib.profile_segments(text, st_, en_, ms, pt, threads=THREADS)
    for c, p in zip(formats.msa_counts(got, pt, len(ms)), prof):
        assert (c[:, :7] == p[:, :7]).all()


def test_row_offsets_of_more_than_a_tile_of_rows():
    """300 final rows of one read, made by hand from the segments of msa_cases, against monomers of three pitches: the
    scan of the pitches runs over two tiles of 256 rows; row_at is sd_msa_row_offsets' on the host"""
    import torch
    monos = [msa_cases.random_monomer(n, 90 + n) for n in (64, 130, 171)]
    names = ["m%d" % i for i in range(len(monos))]
    keys = [n + s for n in names for s in ("", "'")]   # key k = interleaved template k
    seq, st, en, pt = msa_cases.segments(monos, 300, seed=17)
    rows = np.zeros(len(st), dtype=lib.final_dtype())
    rows["start"], rows["end"], rows["best"] = st, en, pt
    dfr = lib.DeviceFinalRows(torch.from_numpy(rows.view(np.uint8).reshape(len(st), -1)).to("cuda:0"),
                              torch.tensor([0, len(st)], dtype=torch.int64, device="cuda:0"), None, len(st))
    dm = lib.final_msa_device(dfr, _device_reads([seq.encode()]), keys, names, monos)
    want = lib.msa_row_offsets([len(m) for m in monos], pt)
    assert len({int(b - a) for a, b in zip(want[:-1], want[1:])}) == 3
    assert (dm.row_at.cpu().numpy() == want).all() and dm.rows.numel() == int(want[-1])
    assert dm.classes == (0, len(st), 0)
    _same(dm.to_host(), lib.msa_segments(seq, st, en, monos, pt, threads=THREADS))


def test_a_long_block_is_left_out_and_counted():
    """A run of 929 N inside one monomer instance (the construction of the long_block golden): the decomposition covers
    it with one block of 1 100 bases, which the row kernel does not take (segments up to 1024 bp).  Exactly that row has
    status 2 and an empty row; every other row equals the host's."""
    mn, ms = synth.make_monomers(12, seed=22)
    rn, rs = synth.make_reads(ms, 2, read_len=6000, seed=22)
    unit = ms[0] if isinstance(ms[0], bytes) else ms[0].encode()
    a = bytes(rs[0][:171 * 12])
    rs = [rs[1], a + unit[:100] + b"N" * 929 + unit[100:] + a]
    dfr, dr, keys, fr = _final_job(mn, ms, rs)
    plan, cls = lib.final_msa_classes(fr, [len(s) for s in rs], keys, mn, ms)
    lens = (fr.rows["end"] - fr.rows["start"] + 1).tolist()
    long_rows = [i for i, n in enumerate(lens) if n > 1024]
    assert len(long_rows) == 1 and plan[2] == 1 and cls[long_rows[0]] == 2
    host, pt = lib.final_msa_host(fr, rs, keys, mn, ms, threads=THREADS)
    dm = lib.final_msa_device(dfr, dr, keys, mn, ms)
    got = dm.to_host()
    assert dm.classes == plan
    assert got.status.tolist() == [2 if i == long_rows[0] else 1 for i in range(len(lens))]
    assert (got.row_at == host.row_at).all()
    for i in range(len(lens)):
        a, b = int(host.row_at[i]), int(host.row_at[i + 1])
        if i == long_rows[0]:
            col, ins = formats.msa_row(got, i, pt[i])
            assert (col == formats.MSA_NONE).all() and not ins.any() and not got.rows[a + 2 * len(col) + 1:b].any()
            assert host.status[i] == 1
        else:
            assert (got.rows[a:b] == host.rows[a:b]).all(), i


def test_small_cap_and_foreign_pointers_are_refused(synth_job):
    import ctypes as C
    import torch
    mn, ms, rs = synth_job
    dfr, dr, keys, fr = _final_job(mn, ms, rs[:1])
    want = int(lib.final_msa_host(fr, rs[:1], keys, mn, ms)[0].row_at[-1])
    with pytest.raises(lib.SdError) as e:
        lib.final_msa_device(dfr, dr, keys, mn, ms, cap=want - 16)
    assert e.value.code == lib.SD_ERR_PARAM and str(want) in e.value.msg
    # nothing written: the calls themselves, into a filled buffer
    L = lib.load()
    t = lib.MsaTables(keys, mn, ms)
    n = dfr.n_rows
    row_at = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    status = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out = torch.full((want,), 0xA5, dtype=torch.uint8, device="cuda:0")
    err = C.create_string_buffer(1024)
    total, cls = C.c_int64(), (C.c_int64 * 3)()
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    try:
        assert L.sd_msa_final_size_dev(t.h, p(dfr.rows), n, C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, 0, None, p(row_at),
                                       C.byref(total), cls, err, 1024) == lib.SD_OK
        assert total.value == want and sum(cls) == n
        assert L.sd_msa_final_write_dev(t.h, p(dfr.rows), n, 0, None, p(row_at), p(out), want - 1, p(status), err,
                                        1024) == lib.SD_ERR_PARAM
        assert str(want).encode() in err.value
        torch.cuda.synchronize()
        assert (out == 0xA5).all() and (status == 0xA5).all()
        # host memory where device memory belongs
        host = np.zeros(want, dtype=np.uint8)
        assert L.sd_msa_final_write_dev(t.h, p(dfr.rows), n, 0, None, p(row_at), C.c_void_p(host.ctypes.data), want, p(status), err,
                                        1024) == lib.SD_ERR_PARAM
        text = np.frombuffer(b"".join(rs[:1]), dtype=np.uint8).copy()
        assert L.sd_msa_final_size_dev(t.h, p(dfr.rows), n, C.c_void_p(text.ctypes.data), dr.c_off, dr.c_lens, dr.n, 0, None,
                                       p(row_at), C.byref(total), cls, err, 1024) == lib.SD_ERR_PARAM
        if torch.cuda.device_count() > 1:   # another device's memory
            far = torch.empty(want, dtype=torch.uint8, device="cuda:1")
            assert L.sd_msa_final_size_dev(t.h, p(dfr.rows), n, C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, 0, None, p(row_at),
                                           C.byref(total), cls, err, 1024) == lib.SD_OK
            assert L.sd_msa_final_write_dev(t.h, p(dfr.rows), n, 0, None, p(row_at), p(far), want, p(status), err,
                                            1024) == lib.SD_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert (out == 0xA5).all() and (status == 0xA5).all()
    finally:
        t.close()


# ---- the command line --------------------------------------------------------------------------------------------------

def _cli(out, extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), os.path.join(TD, "read.fa"),
                        os.path.join(TD, "DXZ1_star_monomers.fa"), "-o", out, "-t", str(THREADS)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return p


@pytest.mark.parametrize("extra", [[], ["--second-best", "-i", "95"]], ids=["light", "second_best_i95"])
def test_cli_msa(tmp_path, extra):
    a, b = str(tmp_path / "plain"), str(tmp_path / "msa")
    _cli(a, extra)
    _cli(b, extra + ["--profile", "--msa"])
    for f in ("final_decomposition.tsv", "final_decomposition_alt.tsv", "final_decomposition_raw.tsv"):
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert not os.path.exists(os.path.join(a, "final_decomposition_msa.tsv"))
    final = os.path.join(b, "final_decomposition.tsv")
    fin = formats.read_final(final)
    rows = formats.read_msa(os.path.join(b, "final_decomposition_msa.tsv"))
    assert [(r.read, r.start, r.end, r.monomer) for r in rows] == [(r.read, r.start, r.end, r.monomer) for r in fin]
    assert len(rows) > 100
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    mn, ms, _ = lib.fasta_load(os.path.join(TD, "DXZ1_star_monomers.fa"))
    mn, ms = [n.split()[0] for n in mn], [s.decode().upper() for s in ms]
    msa, pt = formats.msa_from_rows(rows, mn, [len(s) for s in ms])
    # the file against the Python fold over the written rows
    reads = {n.split()[0]: s.decode().upper() for n, s in zip(rn, rs)}
    msa_ref.same(msa, msa_ref.of_final(final, reads, mn, ms))
    # and folded, against the profile the same run wrote
    prof = formats.read_profile(os.path.join(b, "final_decomposition_profile.tsv"))
    assert prof.names == mn
    for c, p in zip(formats.msa_counts(msa, pt, len(ms)), prof.counts):
        assert (c[:, :7] == p[:, :7]).all()
    assert "final_decomposition_msa.tsv" in open(os.path.join(b, "stringdecomposer.log")).read()
