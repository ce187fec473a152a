"""Reads that already lie in device memory (lib.DeviceReads -> sd_stream_submit_dev / sd_engine_load_reads_dev): the
device packer against the host's word for word, and the rows of the raw stream, --ed_thr, the final mode, several
entries and the engine against the same reads given from the host and against the committed goldens.  Every comparison
is exact.  The tensors stay referenced until their test ends, and nothing here releases the caching allocator."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case

from stringdecomposer_amd import formats, lib, synth

pytestmark = pytest.mark.gpu

THREADS = 8
FINAL = os.path.join(GOLDEN, "final")
PAD = ord("#")          # outside the alphabet: a packer that read a padding byte would report it
SENTINEL = 0xDEADBEEF


def _to_dev(buf, device=0):
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).to("cuda:%d" % device)


def _concat(seqs, device=0, **kw):
    """The reads back to back in a 1-D tensor, one padding byte behind the last."""
    t = _to_dev(b"".join(seqs) + bytes([PAD]), device)
    return lib.DeviceReads(t, [len(s) for s in seqs], **kw)


def _padded_shuffled(seqs, seed=5, **kw):
    """The reads as rows of a padded 2-D tensor, in shuffled row order (explicit offsets), padding outside the alphabet."""
    width = max(len(s) for s in seqs) + 7
    rows = np.random.RandomState(seed).permutation(len(seqs) + 2)[:len(seqs)]
    host = np.full((len(seqs) + 2, width), PAD, dtype=np.uint8)
    for s, r in zip(seqs, rows):
        host[r, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    t = torch.from_numpy(host).to("cuda:0")
    return lib.DeviceReads(t, [len(s) for s in seqs], offsets=[int(r) * width for r in rows], **kw)


LAYOUTS = {"concat": _concat, "padded": _padded_shuffled}


# ---- 1. the packer alone ------------------------------------------------------------------------------------------

LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 5499, 5500, 5501]
SHIFTS = [0, 1, 2, 3, 5, 15]
N_AT = {"none": [], "first": [0], "last": [-1], "15_16": [15, 16], "31_32": [31, 32]}


@pytest.fixture(scope="module")
def packer_run():
    """Every (N variant, length, source shift) chunk in ONE buffer whose other bytes are outside the alphabet, packed in
    one call; the host's words per chunk."""
    rng = np.random.RandomState(20240607)
    chunks, off, buf = [], [], bytearray()
    for var, at in N_AT.items():
        for ln in LENGTHS:
            for sh in SHIFTS:
                s = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), ln).tobytes())
                for p in at:
                    if -ln <= p < ln:
                        s[p] = ord("N")
                buf += bytes([PAD]) * ((-len(buf)) % 64 + sh)
                off.append(len(buf))
                buf += s
                chunks.append((var, ln, sh, bytes(s)))
    buf += bytes([PAD])    # the byte behind the last chunk
    t = _to_dev(bytes(buf))
    got = lib.pack_bases_device(t, off, [c[1] for c in chunks], fill=SENTINEL)
    torch.cuda.synchronize()
    return t, off, chunks, got, [lib.pack_bases(c[3]) for c in chunks]


def test_packer_words_equal_the_hosts(packer_run):
    _, off, chunks, (w, m, hn, bad), host = packer_run
    assert bad == -1, "the packer read a byte outside its chunks"
    assert len(chunks) == len(N_AT) * len(LENGTHS) * len(SHIFTS)
    wo = mo = 0
    for (var, ln, sh, _), (hw, hm, hhn), got_n in zip(chunks, host, hn):
        nw, nm = (ln + 15) // 16, (ln + 31) // 32
        assert np.array_equal(w[wo:wo + nw], hw), (var, ln, sh)
        assert bool(got_n) == hhn, (var, ln, sh)
        if hhn:
            assert np.array_equal(m[mo:mo + nm], hm), (var, ln, sh)
        else:   # a chunk without N writes no mask word: its own and its neighbours' stay as they were
            assert (m[mo:mo + nm] == SENTINEL).all(), (var, ln, sh)
        wo += nw
        mo += nm
    assert wo == len(w) and mo == len(m)
    assert sum(int(x) for x in hn) == sum(1 for h in host if h[2]) > 0


def test_packer_reports_the_smallest_offending_position():
    rng = np.random.RandomState(3)
    s = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 12000).tobytes())
    s[7003] = ord("a")
    s[9000] = ord("*")
    s[11999] = 0
    t = _to_dev(bytes(s))
    off, ln = [0, 5000, 10000, 6900], [5500, 5500, 2000, 200]       # 7003 lies in chunks 1 and 3
    w, m, hn, bad = lib.pack_bases_device(t, off, ln)
    assert bad == 7003
    # the bytes are packed under the same masked formula as on the host
    for o, n, hw in zip(off, ln, np.split(w, np.cumsum([(x + 15) // 16 for x in ln])[:-1])):
        assert np.array_equal(hw, lib.pack_bases(bytes(s[o:o + n]))[0])
    assert lib.pack_bases_device(t, [0, 7004], [7003, 1997])[3] == 9000
    assert lib.pack_bases_device(t, [0], [7003])[3] == -1
    torch.cuda.synchronize()


# ---- 2. / 3. raw rows from the fixtures ------------------------------------------------------------------------------

RAW_CASES = ["syn12_N_multiline", "syn12_boundary_lengths", "syn12_part333_ov77", "syn12_part700_ov100", "syn64_10kb",
             "weird_templates", "td_edthr_10"]


def _raw_case(name):
    c = load_case(name)
    rn, rs, _ = lib.fasta_load(c["reads"])
    mn, ms, _ = lib.fasta_load(c["monomers"])
    kw = dict(part_size=c["part"], overlap=c["overlap"], threads=THREADS)
    if c["ed_thr"] is not None:
        kw["ed_thr"] = c["ed_thr"]
    return c, (rn, rs), (mn, ms), kw


@pytest.fixture(scope="module")
def host_rows():
    """Rows of every raw case from host input, computed once."""
    out = {}
    for name in RAW_CASES:
        c, (rn, rs), (mn, ms), kw = _raw_case(name)
        st = lib.Stream(ms, **kw)
        try:
            st.submit(rs)
            out[name] = st.collect(as_lists=True)
        finally:
            st.close()
    return out


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", RAW_CASES)
def test_raw_rows_from_device_input(name, layout, host_rows):
    """The fixture's reads from device memory -- back to back, or padded rows in shuffled order -- give the rows of the
    host-input stream with the same parameters, and, formatted, the committed raw TSV.  part333 / part700: chunk starts
    at no multiple of 16, many seams; syn64_10kb: the wide layout; td_edthr_10: the prefilter reads the packed words."""
    c, (rn, rs), (mn, ms), kw = _raw_case(name)
    d = LAYOUTS[layout](rs)
    st = lib.Stream(ms, sub_batches=2 if layout == "padded" else 1, **kw)
    try:
        st.submit(d)
        got = st.collect(as_lists=True)
        stats = st.stats()
    finally:
        st.close()
    assert got == host_rows[name]
    tn = list(mn) + [n + "'" for n in mn]
    assert b"".join(lib.format_rows(n, tn, r) for n, r in zip(rn, got)) == c["raw"]
    assert stats["jobs"] == 1 and stats["batches"] >= 1


# ---- 4. final mode ------------------------------------------------------------------------------------------------

def _fasta(path):
    names, seqs, _ = lib.fasta_load(path)
    return [n.split()[0] for n in names], [s.upper() for s in seqs]


def _final_job(mono, reads, kw, profile):
    st = lib.Stream(mono[1], final=True, mono_names=mono[0], threads=THREADS, profile=profile, **kw)
    try:
        st.submit(reads)
        fr = st.collect()
        return fr, st.stats(), st.keys(), st.profile() if profile else None
    finally:
        st.close()


@pytest.mark.parametrize("profile", [False, True])
@pytest.mark.parametrize("name", ["td_second_best", "long_block"])
def test_final_rows_from_device_input(name, profile):
    """FinalRows from device input equal those from host input field by field (alt included) and, formatted, the
    reference command line's final.tsv; long_block's 21-kb block takes the fallback, which fetches the text of its read
    from the job's device copy.  With profile=True the profiles are equal too."""
    with open(os.path.join(FINAL, name, "params.json")) as f:
        c = json.load(f)
    a = c["args"]
    kw = {"second_best": "--second-best" in a, "min_identity": int(a[a.index("-i") + 1]) if "-i" in a else 0,
          "part_size": int(a[a.index("-b") + 1]) if "-b" in a else 5000}
    rn, rs = _fasta(os.path.join(GOLDEN, c["inputs"][0]))
    mono = _fasta(os.path.join(GOLDEN, c["inputs"][1]))
    want, _, _, wprof = _final_job(mono, rs, kw, profile)
    d = _concat(rs)
    got, stats, keys, gprof = _final_job(mono, d, kw, profile)
    assert got.rows.dtype == want.rows.dtype and got.rows.tobytes() == want.rows.tobytes()
    for field in got.rows.dtype.names:
        assert np.array_equal(got.rows[field], want.rows[field]), field
    assert np.array_equal(got.row_off, want.row_off)
    assert (got.alt is None) == (want.alt is None) and (got.alt is None or np.array_equal(got.alt, want.alt))
    fin, _ = formats.final_rows(got, rn, keys)
    with open(os.path.join(FINAL, name, "final.tsv"), "rb") as f:
        assert formats.format_final(fin).encode() == f.read()
    if name == "long_block":
        assert stats["fallback_blocks"] > 0
    if profile:
        assert gprof.names == wprof.names and gprof.seqs == wprof.seqs
        assert len(gprof.counts) == len(wprof.counts)
        for x, y in zip(gprof.counts, wprof.counts):
            assert np.array_equal(x, y)
        assert sum(int(x.sum()) for x in gprof.counts) > 0


# ---- 5. ordering ---------------------------------------------------------------------------------------------------

def test_buffer_may_be_overwritten_on_its_stream_after_submit():
    """On a non-default torch stream: fill the tensor, submit with that stream, overwrite the tensor with 'A' on the
    same stream right after submit returns -- three jobs outstanding before the first collect.  The rows are those of
    the untouched input: the library's reads of the buffer are ordered before the overwrite without a host wait."""
    mn, ms = synth.make_monomers(12, seed=31)
    jobs = [synth.make_reads(ms, 6, read_len=21000 + 3000 * j, seed=40 + j)[1] for j in range(3)]
    st = lib.Stream(ms, threads=THREADS)
    try:
        want = list(st.imap(jobs, as_lists=True))
    finally:
        st.close()
    side = torch.cuda.Stream(device=0)
    host = [torch.frombuffer(bytearray(b"".join(rs)), dtype=torch.uint8).pin_memory() for rs in jobs]
    bufs = [torch.empty(len(h), dtype=torch.uint8, device="cuda:0") for h in host]
    st = lib.Stream(ms, threads=THREADS)
    try:
        for rs, h, t in zip(jobs, host, bufs):
            with torch.cuda.stream(side):
                t.copy_(h, non_blocking=True)                                  # the bytes are produced on `side`
                d = lib.DeviceReads(t, [len(s) for s in rs])                   # stream=None: the current stream
                assert d.stream == side.cuda_stream
                st.submit(d)
                t.fill_(ord("A"))                                              # ... and destroyed on it at once
        got = [st.collect(as_lists=True) for _ in jobs]
    finally:
        st.close()
    torch.cuda.synchronize()
    assert got == want
    assert all(bool((t == ord("A")).all()) for t in bufs)


# ---- 6. several entries ----------------------------------------------------------------------------------------------

def test_two_entries_on_one_device_give_the_plain_rows(host_rows):
    c, (rn, rs), (mn, ms), kw = _raw_case("syn12_part700_ov100")
    d = _concat(rs)
    st = lib.Stream(ms, devices=[0, 0], **kw)
    try:
        st.submit(d)
        st.submit(d)
        got = [st.collect(as_lists=True), st.collect(as_lists=True)]
        dealt = st.device_stats()
    finally:
        st.close()
    assert got[0] == got[1] == host_rows["syn12_part700_ov100"]
    assert len(dealt) == 2 and sum(x["batches"] for x in dealt) >= 4


def test_memory_of_another_device_is_unsupported():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    mn, ms = synth.make_monomers(4, seed=9)
    rn, rs = synth.make_reads(ms, 2, read_len=4000, seed=9)
    d = _concat(rs, device=1)
    st = lib.Stream(ms, device=0)
    try:
        with pytest.raises(lib.SdError) as e:
            st.submit(d)
        assert e.value.code == lib.SD_ERR_UNSUPPORTED
        assert "device 1" in e.value.msg and "device 0" in e.value.msg
        assert st.stats()["batches"] == 0 and st.stats()["jobs"] == 0     # no work was started
        st.submit(rs)                                                       # and the stream is as it was
        assert st.collect() > 0
    finally:
        st.close()


def test_host_memory_is_a_param_error():
    mn, ms = synth.make_monomers(4, seed=9)
    host = np.frombuffer(b"ACGT" * 1000, dtype=np.uint8).copy()
    st = lib.Stream(ms)
    try:
        with pytest.raises(lib.SdError) as e:
            st.submit(lib.DeviceReads((host.ctypes.data, host.nbytes, 0), [4000]))
        assert e.value.code == lib.SD_ERR_PARAM
        with pytest.raises(lib.SdError) as e:
            t = _to_dev(b"ACGT" * 10)
            st.submit(lib.DeviceReads(t, [20, 0, 20], offsets=[0, 20, 20]))
        assert e.value.code == lib.SD_ERR_EMPTY and "#1" in e.value.msg
    finally:
        st.close()


# ---- 7. alphabet -----------------------------------------------------------------------------------------------------

def test_an_invalid_byte_is_reported_with_read_position_and_byte(host_rows):
    """One 'a' in read 2 at position 4711 of a five-read job: SD_ERR_SYMBOL naming the read, the position and the byte,
    by the stream's failure rule; the byte was packed under the masked formula, so nothing faulted, and a fresh stream
    (and this one) still computes a fixture correctly."""
    mn, ms = synth.make_monomers(12, seed=3)
    rn, rs = synth.make_reads(ms, 5, read_len=9000, seed=8)
    rs = [bytes(s) for s in rs]
    rs[2] = rs[2][:4711] + b"a" + rs[2][4712:]
    st = lib.Stream(ms, threads=THREADS)
    try:
        bad = _concat(rs)
        with pytest.raises(lib.SdError) as e:
            st.submit(bad)
            st.collect()
        assert e.value.code == lib.SD_ERR_SYMBOL
        assert "#2 " in e.value.msg and "position 4711" in e.value.msg and "97" in e.value.msg and "0x61" in e.value.msg
        good = list(rs)
        good[2] = good[2].replace(b"a", b"A")
        mended = _concat(good)
        st.submit(mended)                            # the failure dropped the job; the stream goes on
        assert st.collect() > 0
    finally:
        st.close()
    c, (rn, rs), (mn, ms), kw = _raw_case("syn12_N_multiline")
    st = lib.Stream(ms, **kw)
    try:
        fixture = _concat(rs)
        st.submit(fixture)
        assert st.collect(as_lists=True) == host_rows["syn12_N_multiline"]
    finally:
        st.close()


# ---- 8. engine ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["single_monomer", "syn12_ties"])
def test_engine_load_reads_from_device(name):
    c, (rn, rs), (mn, ms), kw = _raw_case(name)
    rows = []
    d = _padded_shuffled(rs)
    for reads in (rs, d):
        e = lib.Engine(ms, **kw)
        try:
            n = e.load_reads(reads)
            e.run()
            rows.append((n, e.rows()))
        finally:
            e.close()
    assert rows[0] == rows[1] and rows[0][0] > 0
    tn = list(mn) + [n + "'" for n in mn]
    assert b"".join(lib.format_rows(n, tn, [tuple(x) for x in r]) for n, r in zip(rn, rows[1][1])) == c["raw"]


# ---- the guard-trip re-run of a device-packed batch ---------------------------------------------------------------------

def test_guard_trip_repeats_a_device_packed_batch_with_its_own_mask_table():
    """Which chunks run maskless is decided by the packer, in the device's descriptor table; a batch repeated with
    integer cells (the fp16 range guard, forced by the f16_guard hook) re-uploads the table and must keep that: reads
    with and without N, two batches, the rows of the host-input stream."""
    mn, ms = synth.make_monomers(12, seed=3)
    rn, rs = synth.make_reads(ms, 5, read_len=6000, seed=5)
    rs = [bytearray(s) for s in rs]
    rs[1][100:140] = b"N" * 40
    rs[3][5990:6000] = b"N" * 10
    rs = [bytes(s) for s in rs]
    rows = []
    d = _concat(rs)
    for reads in (rs, d):
        t0 = lib.guard_trips()
        st = lib.Stream(ms, sub_batches=2, f16_guard=40, threads=THREADS)
        try:
            st.submit(reads)
            rows.append(st.collect(as_lists=True))
        finally:
            st.close()
        assert lib.guard_trips() > t0
    assert rows[0] == rows[1] and sum(len(r) for r in rows[1]) > 0
