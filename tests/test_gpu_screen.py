"""The screen on the device (--screen; csrc/sd_filter.hip's KeyMin sink, csrc/sd_screen.hip).

Kernel: the keys of sd_screen_chunks at every instantiation the launch selection can take -- sd_hw_dist_u<3, lo|hi>,
sd_hw_dist<3> through the handle's switch, sd_hw_dist<8>, sd_hw_dist<32> -- with template counts at which a chunk's
templates lie inside a wave (T = 2), straddle waves (24, 66) and workgroups (300), and chunk counts 1, 3 and 70 (one LDS
slot, a few, more than one workgroup's worth), against the host twin and, where the pair count allows it, against the
oracle's exact infix distances reduced by the key rule.  The same inputs through DeviceReads (padded rows, explicit
offsets) and with the keys left on the device.

File job: `--screen 40` on a FASTA with a read that has one array, one with two, one that is all array, an all-random
read and a 150-bp read (tests/screen_cases.py), against the oracle on the regions' substrings (raw rows), against this
project's plain job on a FASTA of the substrings (final and _alt rows, profile), against the regions computed from the
oracle's distance matrix (region file); a threshold that passes everything against the job without the flag; two
pipelines on one device; and the in-memory route Screener -> screen_regions -> region_reads -> Stream -> rows_from_regions.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prefilter_cases as pc
import screen_cases as sc
from oracle import binding as oracle
from stringdecomposer_amd import formats, lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = 8
_host = {}


def _host_keys(case):
    """The host twin's keys of a kernel case, once per template set and read list."""
    if case.name not in _host:
        ms, tm, reads = case.data()
        same = [c for c in sc.KERNEL_CASES if c.name in _host and c.data()[1] == tm and c.data()[2] == reads]
        _host[case.name] = _host[same[0].name] if same else lib.screen_chunks_host(ms, reads, sc.PART, sc.OVERLAP)
    return _host[case.name]


def _to_dev(buf):
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).to("cuda:0")


# ---- kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.KERNEL_CASES, ids=lambda c: c.name)
def test_keys_equal_the_host_twin(case):
    ms, tm, reads = case.data()
    s = lib.Screener(ms, general=case.general)
    try:
        assert s.kernel() == case.kernel(), (s.kernel(), case.kernel())
        got = s.chunks(reads, sc.PART, sc.OVERLAP)
    finally:
        s.close()
    host = _host_keys(case)
    assert len(got.key) == case.n_chunks and got.chunk_read.tolist() == host.chunk_read.tolist()
    assert got.chunk_off.tolist() == host.chunk_off.tolist() and got.chunk_len.tolist() == host.chunk_len.tolist()
    bad = np.flatnonzero(got.key != host.key)
    assert not len(bad), "%s: %d of %d keys differ from the host twin; first: chunk %d (%d bp), device %#x, host %#x" % (
        s.kernel(), len(bad), len(host.key), bad[0], got.chunk_len[bad[0]], got.key[bad[0]], host.key[bad[0]])
    if case.exact:
        assert got.key.tolist() == case.oracle_keys().tolist()
    d = got.key >> 16
    assert d.min() < d.max() or case.n_chunks == 1      # the case is no constant


def test_keys_of_device_reads():
    """Padded rows and explicit offsets, once each; the keys as a device tensor against the host copy."""
    case = next(c for c in sc.KERNEL_CASES if c.name == "u3_hi_T24_c3")
    ms, tm, reads = case.data()
    exp = case.oracle_keys()
    s = lib.Screener(ms)
    try:
        width = max(len(r) for r in reads) + 5
        rows = torch.full((len(reads), width), ord("#"), dtype=torch.uint8)
        for i, r in enumerate(reads):
            rows[i, :len(r)] = torch.frombuffer(bytearray(r), dtype=torch.uint8)
        padded = lib.DeviceReads(rows.to("cuda:0"), [len(r) for r in reads])
        got = s.chunks(padded, sc.PART, sc.OVERLAP)
        assert got.key.tolist() == exp.tolist()
        # explicit offsets: the reads in reverse order in the buffer, odd gaps between them
        order = list(range(len(reads)))[::-1]
        buf, off, at = bytearray(), [0] * len(reads), 3
        buf += b"###"
        for r in order:
            off[r] = at
            buf += reads[r] + b"#" * 7
            at += len(reads[r]) + 7
        placed = lib.DeviceReads(_to_dev(bytes(buf)), [len(r) for r in reads], offsets=off)
        dk = s.chunks(placed, sc.PART, sc.OVERLAP, device_out=True)
        assert dk.key.is_cuda and dk.key.dtype == torch.int32 and len(dk.key) == len(exp)
        assert dk.key.cpu().numpy().view(np.uint32).tolist() == exp.tolist()
        lens = [len(r) for r in reads]
        thr = int(np.median(exp >> 16))
        assert sc.region_tuples(lib.screen_regions(dk, lens, thr, sc.PART, sc.OVERLAP)) == \
            sc.regions_of(exp, dk.chunk_read.tolist(), lens, thr, sc.PART, sc.OVERLAP)
        with pytest.raises(lib.SdError):
            s.chunks(reads, sc.PART, sc.OVERLAP, device_out=True)
    finally:
        s.close()


# ---- the file job ----------------------------------------------------------------------------------------------------
def _read(fn):
    with open(fn, "rb") as f:
        return f.read()


def _outs(d, tag):
    return [os.path.join(d, "%s_%s.tsv" % (tag, x)) for x in ("raw", "final", "alt", "screen")]


def _run(fx, tag, screen, second_best=True, **kw):
    o = _outs(fx["dir"], tag)
    prof = lib.run_files(fx["reads_fa"], fx["mono_fa"], o[0], o[1], o[2], second_best=second_best, threads=THREADS,
                         part_size=sc.F_PART, overlap=sc.F_OVERLAP, screen=screen,
                         screen_tsv_out=o[3] if screen is not None else None, **kw)
    return [_read(x) for x in o[:3]] + [_read(o[3]) if screen is not None else None, prof]


def _shift(text, names, bases, cols=(2, 3)):
    """TSV text of a job on the substrings (reads named g<i>) -> the parents' rows."""
    out = []
    for ln in text.decode().split("\n")[:-1]:
        f = ln.split("\t")
        g = int(f[0][1:])
        f[0] = names[g]
        for c in cols:
            f[c] = str(int(f[c]) + bases[g])
        out.append("\t".join(f) + "\n")
    return "".join(out).encode()


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("screen"))
    mn, ms, rn, reads = sc.file_fixture()
    keys, cr, regions = sc.file_reference()
    f = {"dir": d, "reads_fa": os.path.join(d, "reads.fa"), "mono_fa": os.path.join(d, "mono.fa"), "sub_fa": os.path.join(d, "sub.fa"),
         "mn": mn, "ms": ms, "rn": rn, "reads": reads, "keys": keys, "cr": cr, "regions": regions}
    synth.write_fasta(f["reads_fa"], rn, reads, width=70)
    synth.write_fasta(f["mono_fa"], mn, ms)
    f["subs"] = [reads[r][s:e + 1] for r, s, e, _, _ in regions]
    f["g_names"] = [rn[r] for r, _, _, _, _ in regions]
    f["g_bases"] = [s for _, s, _, _, _ in regions]
    synth.write_fasta(f["sub_fa"], ["g%d" % i for i in range(len(regions))], f["subs"], width=70)
    f["screened"] = _run(f, "scr", sc.F_THR, profile=True)
    # the plain job on the substrings (the plain path is pinned by the goldens)
    o = _outs(d, "sub")
    f["sub_prof"] = lib.run_files(f["sub_fa"], f["mono_fa"], o[0], o[1], o[2], second_best=True, threads=THREADS,
                                  part_size=sc.F_PART, overlap=sc.F_OVERLAP, profile=True)
    f["sub"] = [_read(x) for x in o[:3]]
    return f


def test_fixture_is_not_trivial(fx):
    """From exact distances, before anything else: a read without a region, one with two, one that passes entirely."""
    per_read = [[g for g in fx["regions"] if g[0] == r] for r in range(len(fx["reads"]))]
    assert [len(x) for x in per_read] == [1, 2, 1, 0, 0]
    r, s, e, n, _ = per_read[2][0]
    assert (s, e) == (0, len(fx["reads"][2]) - 1) and n == fx["cr"].count(2)
    assert 12000 <= per_read[0][0][1] and per_read[0][0][2] < 30000           # the flanks of the long read are left out
    d = fx["keys"] >> 16
    assert ((d > sc.F_THR) & (d < 60)).any() and (d <= 20).any() and (d > 70).any()   # the threshold cuts between real values


def test_region_file(fx):
    assert fx["screened"][3].decode() == sc.screen_text(fx["regions"], fx["rn"], fx["mn"])
    rows = formats.parse_screen(fx["screened"][3].decode())
    assert formats.format_screen(rows).encode() == fx["screened"][3]


def test_raw_rows_equal_the_oracle_on_the_substrings(fx):
    exp = "".join(sc.shifted_raw(oracle.decompose([name], [sub], fx["mn"], fx["ms"], threads=THREADS, part=sc.F_PART,
                                                  overlap=sc.F_OVERLAP), name, base)
                  for name, sub, base in zip(fx["g_names"], fx["subs"], fx["g_bases"]))
    assert exp.count("\n") > 150
    assert fx["screened"][0] == exp.encode()


def test_final_and_alt_rows_equal_the_plain_job_on_the_substrings(fx):
    assert fx["sub"][1].count(b"\n") > 150 and fx["sub"][2].count(b"\n") > 150 * 12
    assert fx["screened"][1] == _shift(fx["sub"][1], fx["g_names"], fx["g_bases"])
    assert fx["screened"][2] == _shift(fx["sub"][2], fx["g_names"], fx["g_bases"])
    # ... and the raw rows of the two agree too (this project against itself; the oracle is the test above)
    assert fx["screened"][0] == _shift(fx["sub"][0], fx["g_names"], fx["g_bases"])
    # no row lies outside a region, and reads without a region have none
    for r in formats.parse_final(fx["screened"][1].decode()):
        assert any(fx["rn"][g[0]] == r.read and g[1] <= r.start and r.end <= g[2] for g in fx["regions"])


def test_profile_behind_the_screen(fx):
    assert formats.format_profile(fx["screened"][4]) == formats.format_profile(fx["sub_prof"])
    assert sum(formats.profile_instances(c) for c in fx["screened"][4].counts) > 100


def test_threshold_that_passes_everything_is_the_plain_job(fx):
    plain = _run(fx, "plain", None)
    every = _run(fx, "all", 2048)
    assert every[:3] == plain[:3] and len(plain[0]) > len(fx["screened"][0])
    lens = [len(r) for r in fx["reads"]]
    assert [(x.read, x.start, x.end) for x in formats.parse_screen(every[3].decode())] == \
        [(n, 0, ln - 1) for n, ln in zip(fx["rn"], lens)]
    light = _run(fx, "light", sc.F_THR, second_best=False)
    assert light[0] == fx["screened"][0] and light[3] == fx["screened"][3]


def test_two_pipelines_on_one_device(fx):
    two = _run(fx, "two", sc.F_THR, devices=[0, 0])
    assert two[:4] == fx["screened"][:4]
    c = lib.last_run_screen()
    assert c == {"reads": 5, "reads_with_region": 3, "bases_read": sum(len(r) for r in fx["reads"]),
                 "bases_decomposed": sum(len(s) for s in fx["subs"])}
    ed = _run(fx, "ed", sc.F_THR, ed_thr=60)       # --ed_thr keeps its meaning inside the regions
    o = _outs(fx["dir"], "sub_ed")
    lib.run_files(fx["sub_fa"], fx["mono_fa"], o[0], o[1], o[2], second_best=True, threads=THREADS, part_size=sc.F_PART,
                  overlap=sc.F_OVERLAP, ed_thr=60)
    assert ed[0] == _shift(_read(o[0]), fx["g_names"], fx["g_bases"]) and ed[3] == fx["screened"][3]


def test_command_line_with_profile_and_msa(fx):
    out = os.path.join(fx["dir"], "cli")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), fx["reads_fa"], fx["mono_fa"], "-o", out,
                        "-t", str(THREADS), "-b", str(sc.F_PART), "-v", str(sc.F_OVERLAP), "--screen", str(sc.F_THR),
                        "--second-best", "--profile", "--msa"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    fn = lambda x: os.path.join(out, "final_decomposition" + x)
    assert [_read(fn(x)) for x in ("_raw.tsv", ".tsv", "_alt.tsv", "_screen.tsv")] == fx["screened"][:4]
    assert _read(fn("_profile.tsv")).decode() == formats.format_profile(fx["sub_prof"])
    final = formats.read_final(fn(".tsv"))
    msa = formats.read_msa(fn("_msa.tsv"))
    assert [(m.read, m.start, m.end, m.monomer) for m in msa] == [(r.read, r.start, r.end, r.monomer) for r in final]
    # a forward instance's columns are bases of the parent read at the row's absolute position: a subsequence of them
    reads = dict(zip(fx["rn"], fx["reads"]))
    fwd = [m for m in msa if not m.monomer.endswith("'") and set(m.columns) != {"."}][:20]
    assert len(fwd) == 20
    for m in fwd:
        it = iter(reads[m.read][m.start:m.end + 1].decode())
        assert all(ch in it for ch in m.columns.replace("-", "")), m
    log = open(os.path.join(out, "stringdecomposer.log")).read()
    assert "Screen (threshold 40): 5 reads, 3 with a region, %d bases read, %d bases decomposed" % (
        sum(len(r) for r in fx["reads"]), sum(len(s) for s in fx["subs"])) in log


# ---- the in-memory route ---------------------------------------------------------------------------------------------
def test_in_memory_route_equals_the_file_job(fx):
    reads, lens = fx["reads"], [len(r) for r in fx["reads"]]
    dreads = lib.DeviceReads(_to_dev(b"".join(reads) + b"#"), lens)
    s = lib.Screener(fx["ms"])
    st = lib.Stream(fx["ms"], threads=THREADS, device_rows=True, mono_names=fx["mn"], part_size=sc.F_PART, overlap=sc.F_OVERLAP)
    try:
        keys = s.chunks(dreads, sc.F_PART, sc.F_OVERLAP, device_out=True)
        regions = lib.screen_regions(keys, lens, sc.F_THR, sc.F_PART, sc.F_OVERLAP)
        assert sc.region_tuples(regions) == fx["regions"]
        sub = lib.region_reads(dreads, regions)
        assert sub.ptr == dreads.ptr and sub.read_lens == [len(x) for x in fx["subs"]]      # no base moved
        st.submit(sub)
        local = st.collect_device()
        rows = lib.rows_from_regions(local, None, regions, len(reads))
        tn = st.tmpl_names()
    finally:
        st.close()
        s.close()
    off = rows.row_off.cpu().tolist()
    r = rows.rows.cpu().numpy()
    got = [(fx["rn"][i], tn[int(x[0])], int(x[1]), int(x[2]), float(x[3])) for i in range(len(reads)) for x in r[off[i]:off[i + 1]]]
    exp = [(x.read, x.monomer, x.start, x.end, x.score) for x in formats.parse_raw(fx["screened"][0].decode())]
    assert len(off) == len(reads) + 1 and off[-1] == len(r) == local.n_rows and got == exp
    # the host route: memoryview slices through a plain stream
    hs = lib.Stream(fx["ms"], threads=THREADS, part_size=sc.F_PART, overlap=sc.F_OVERLAP)
    try:
        hs.submit(lib.region_reads(reads, regions))
        lists = hs.collect(as_lists=True)
    finally:
        hs.close()
    flat = np.array([x for l in lists for x in l], dtype=np.int32).reshape(-1, 4)
    hoff = np.cumsum([0] + [len(l) for l in lists])
    hrows, hro = lib.rows_from_regions(flat, hoff, regions, len(reads))
    assert hrows.tolist() == r.tolist() and hro.tolist() == off
