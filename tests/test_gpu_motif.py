"""IUPAC motif hits (--motif) on the device: the size and write kernels (sd_motif_dev) against the host form, array for
array, at the edges of words, tiles, pattern blocks and launches, a thinned subset against the naive scan of
tests/motif_ref.py, the device-resident form on DeviceReads, and the command line's files."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import motif_ref as ref
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8
INFO = lib.motif_info()
T, PB = INFO["tile"], INFO["pattern_block"]
CENPB = lib.MOTIF_BUILTIN["cenpb"]


def text_of(rng, n):
    """random ACGT with about 1 % N and 1 % lower case"""
    return "".join(rng.choice("ACGT") if rng.random() >= 0.02 else rng.choice("Nacgt") for _ in range(n))


def instance(rng, pattern, mismatches=0, strand=0):
    """bases that the pattern hits with exactly `mismatches` mismatches (on - its reverse complement)"""
    con = [j for j, c in enumerate(pattern) if c != "N"]
    bad = set(rng.sample(con, mismatches))
    s = []
    for j, c in enumerate(pattern):
        allowed = ref.IUPAC[c]
        s.append(rng.choice([b for b in "ACGT" if b not in allowed]) if j in bad else rng.choice(allowed))
    s = "".join(s)
    return s if strand == 0 else "".join(ref.COMP[b] for b in reversed(s))


def plant(s, at, piece):
    return s[:at] + piece + s[at + len(piece):]


def layout(reads, rng):
    """the reads in one buffer in a shuffled order with gaps of bases that would match if they were read"""
    order = list(range(len(reads)))
    rng.shuffle(order)
    off, parts, at = [0] * len(reads), [], 0
    for r in order:
        gap = "".join(rng.choice("ACGT") for _ in range(rng.randrange(0, 9)))
        parts += [gap, reads[r]]
        off[r] = at + len(gap)
        at += len(gap) + len(reads[r])
    return "".join(parts) + "ACGT", off, [len(s) for s in reads]


def dev_equals_host(text, off, lens, motifs, E, min_launches=1):
    """the device form equals the host form array for array, and the kernels were launched for it"""
    before = lib.motif_info()["launches"]
    dev = lib.motif_text(text, off, lens, motifs, E, device=0)
    launched = lib.motif_info()["launches"] - before
    host = lib.motif_text(text, off, lens, motifs, E, threads=THREADS)
    assert dev.hits.dtype == host.hits.dtype and len(dev.hits) == len(host.hits), "%d hits on the device, %d on the host" % (len(dev.hits), len(host.hits))
    assert dev.hits.tobytes() == host.hits.tobytes()
    assert dev.per.shape == host.per.shape and (dev.per == host.per).all()
    assert launched >= min_launches, "the kernels were launched %d times" % launched
    return dev


def equals_reference_in(dev, reads, patterns, E, r, a, b):
    """the hits of read r that lie wholly in [a, b) equal the naive scan of that stretch; -> their number"""
    want, _ = ref.scan([reads[r][a:b]], patterns, E)
    want = [(r, m, s, i + a, mm) for _, m, s, i, mm in want]
    h = dev.hits
    inside = (h["read"] == r) & (h["start"] >= a) & (h["start"] + np.array([len(p) for p in patterns])[h["motif"]] <= b)
    assert ref.as_tuples(h[inside]) == want
    return len(want)


@pytest.mark.parametrize("E", [0, 1, 3, 7])
def test_read_lengths_around_words_and_tiles(E):
    rng = random.Random(E)
    L = 17
    patterns = [CENPB, "GAATTC" if E < 6 else "GAATTCNNGAATTC", "".join(rng.choice("ACGT") for _ in range(33)),
                "".join(rng.choice("ACGTRYSWKMBDHVN") for _ in range(64)), "ACGTACGTAC"]
    motifs = [("m%d" % i, p) for i, p in enumerate(patterns)]
    ns = [0, 1, L, 63, 64, 65, 64 * T - 1, 64 * T, 64 * T + 1, 128 * T + L - 1]
    reads = [text_of(rng, n) for n in ns]
    for r, n in enumerate(ns):   # instances anywhere, then one across the tile's end, then one that ends at the last base
        spots = [(p, rng.randrange(n - len(p) + 1)) for p in patterns if n >= len(p)]
        across, last = patterns[(r + 1) % len(patterns)], patterns[r % len(patterns)]
        spots += [(across, 64 * T - len(across) // 2)] if n >= 64 * T + 64 else []
        spots += [(last, n - len(last))] if n >= len(last) else []
        for p, at in spots:
            reads[r] = plant(reads[r], at, instance(rng, p, min(E, 2), rng.randrange(2)))
    text, off, lens = layout(reads, rng)
    dev = dev_equals_host(text, off, lens, motifs, E)
    assert dev.per.sum() == len(dev.hits) >= 20
    key = [(int(h["read"]), int(h["motif"]), int(h["strand"]), int(h["start"])) for h in dev.hits]
    assert key == sorted(key)   # the canonical order
    for r, n in enumerate(ns):   # a thinned subset against the naive scan: the short reads whole, the long ones around their edges
        if n <= 65:
            equals_reference_in(dev, reads, patterns, E, r, 0, n)
        else:
            edge = min(n, 64 * T + 40)
            assert equals_reference_in(dev, reads, patterns, E, r, n - 150, n) >= 1
            equals_reference_in(dev, reads, patterns, E, r, edge - 180, edge)


@pytest.mark.parametrize("L", [17, 33, 64])
def test_hits_across_word_and_tile_boundaries(L):
    """a planted hit starting at every bit 0 .. 63 of the last word of the first tile, a read per bit: every hit of 33 and 64
    codes spans the word's end -- which is the tile's end -- and so do those of 17 codes from bit 48 on; each is found
    exactly once, in the read and at the start where it was planted, and nothing else is"""
    rng = random.Random(L)
    pattern = "".join(rng.choice("ACGT") for _ in range(L))
    n = 64 * T + 300
    reads = [plant("".join(rng.choice("ACGT") for _ in range(n)), 64 * (T - 1) + bit, pattern) for bit in range(64)]
    text, off, lens = layout(reads, rng)
    dev = dev_equals_host(text, off, lens, [("p", pattern)], 0)
    assert ref.as_tuples(dev.hits) == [(bit, 0, 0, 64 * (T - 1) + bit, 0) for bit in range(64)]
    assert dev.per[:, 0].tolist() == [[1, 0]] * 64
    both = dev_equals_host(text, off, lens, [("p", pattern), ("q", instance(rng, pattern, 0, 1))], 0)   # and on strand -
    assert ref.as_tuples(both.hits) == [(bit, m, m, 64 * (T - 1) + bit, 0) for bit in range(64) for m in (0, 1)]


@pytest.mark.parametrize("E", [0, 1, 3, 7])
def test_the_mismatch_budget(E):
    """sites of exactly E mismatches are hits with that count, sites of E + 1 are none; a site of 64 mismatches at E = 7 is none"""
    rng = random.Random(10 + E)
    pattern = "ACGTTGCAWSNNACGGTCAGTCCA" + "T" * 40   # 64 codes, 62 constrained
    n = 64 * T + 500
    s = "".join(rng.choice("ACGT") for _ in range(n))
    ok = [70, 64 * T - 40, 64 * T + 200]
    no = [300, 64 * T - 200, n - 64]
    for at in ok:
        s = plant(s, at, instance(rng, pattern, E))
    for at in no:
        s = plant(s, at, instance(rng, pattern, E + 1))
    s = plant(s, 1000, instance(rng, "A" * 64, 0))   # against C x 64 below: 64 mismatches
    dev = dev_equals_host(s, [0], [n], [("p", pattern), ("c", "C" * 64)], E)
    assert [h for h in ref.as_tuples(dev.hits) if h[1] == 0] == [(0, 0, 0, at, E) for at in ok]
    assert dev.per[0, 1].tolist() == [0, 0]
    equals_reference_in(dev, [s], [pattern, "C" * 64], E, 0, 0, 600)


def motifs_of(rng, n_strands):
    """motifs with n_strands pattern-strands: short degenerate patterns, one or two palindromes among them"""
    pal = ["GAATTC", "ACGT"][:2 - n_strands % 2]
    out = [("pal%d" % i, p) for i, p in enumerate(pal)]
    while 2 * (len(out) - len(pal)) + len(pal) < n_strands:
        p = "".join(rng.choice("ACGTRYSWKMBDHVN") for _ in range(rng.randrange(4, 8)))
        if sum(c != "N" for c in p) >= 3 and ref.revcomp_sets(ref.sets(p)) != ref.sets(p) and p not in [q for _, q in out]:
            out.append(("m%d" % len(out), p))
    return out


@pytest.mark.parametrize("n_strands", [PB - 1, PB, PB + 1, 2 * PB + 1])
def test_pattern_blocks(n_strands):
    rng = random.Random(n_strands)
    motifs = motifs_of(rng, n_strands)
    strands = lib.motif_compile(motifs, 1)[2]
    assert len(strands) == n_strands and sum(s.palindrome for s in strands) in (1, 2)
    reads = [text_of(rng, 64 * T + 100), text_of(rng, 300), ""]
    text, off, lens = layout(reads, rng)
    dev = dev_equals_host(text, off, lens, motifs, 1)
    assert len(dev.hits) > 1000 and all(dev.per[:, m, 1].sum() == 0 for m, (name, _) in enumerate(motifs) if name.startswith("pal"))
    equals_reference_in(dev, reads, [p for _, p in motifs], 1, 1, 0, 300)


def test_a_call_of_several_launches():
    """more (tile, pattern block) units than one launch takes: the same arrays from several launches of each pass"""
    rng = np.random.default_rng(4)
    launch_units = INFO["launch_work"] // (64 * T * PB)
    n_motifs = 8 * PB   # 16 PB pattern-strands: 16 blocks
    tiles = launch_units // 16 + 2
    n = 64 * T * tiles - 77
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    seen, motifs = set(), []
    while len(motifs) < n_motifs:
        p = "".join("ACGT"[x] for x in rng.integers(0, 4, 7))
        if p not in seen and ref.revcomp_sets(ref.sets(p)) != ref.sets(p):
            seen.add(p)
            motifs.append(("k%d" % len(motifs), p))
    units = tiles * 16
    assert units > launch_units
    before = lib.motif_info()["launches"]
    dev = dev_equals_host(s, [0], [n], motifs, 0)
    assert lib.motif_info()["launches"] - before == 2 * -(-units // launch_units) >= 4
    assert len(dev.hits) > 10000
    first = dev.hits[dev.hits["motif"] < 3]   # a thinned subset: three motifs at the sequence's end
    want, _ = ref.scan([s[n - 3000:]], [p for _, p in motifs[:3]], 0)
    assert ref.as_tuples(first[first["start"] >= n - 3000]) == [(0, m, st, i + n - 3000, mm) for _, m, st, i, mm in want]


def test_the_device_resident_form():
    """motif_device on a DeviceReads of padded rows, on a caller's stream, into stale buffers, twice without a wait"""
    rng = random.Random(12)
    reads = [text_of(rng, n) for n in (300, 0, 64 * T + 65, 64, 1000)]
    for r in (0, 2, 4):
        reads[r] = plant(reads[r], len(reads[r]) - 17, instance(rng, CENPB, 1, r % 2))
    width = max(len(s) for s in reads) + 13
    rows = np.frombuffer(("".join(s + "A" * (width - len(s)) for s in reads)).encode(), dtype=np.uint8).reshape(len(reads), width)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        data = torch.from_numpy(rows.copy()).to("cuda:0", non_blocking=False)
        dr = lib.DeviceReads(data, [len(s) for s in reads])
    requests = ((["cenpb", "tel=TTAGGG"], 1), ([("w", "WSWSNNA"), ("pal", "GAATTC")], 0))
    hosts = [lib.motif(reads, m, E, threads=THREADS) for m, E in requests]
    with torch.cuda.stream(side):
        stale_hits = [torch.full((len(h.hits) + 5, 16), 0x77, dtype=torch.uint8, device="cuda:0") for h in hosts]
        stale_per = [torch.full(h.per.shape, 77, dtype=torch.int64, device="cuda:0") for h in hosts]
    before = lib.motif_info()["launches"]
    got = [lib.motif_device(dr, m, E, stream=side, hits=stale_hits[i], per=stale_per[i]) for i, (m, E) in enumerate(requests)]   # no wait in between
    assert lib.motif_info()["launches"] >= before + 4
    side.synchronize()
    for i, (m, E) in enumerate(requests):
        assert got[i].hits.is_cuda and got[i].hits.data_ptr() == stale_hits[i].data_ptr() and got[i].per.data_ptr() == stale_per[i].data_ptr()
        back = got[i].to_host()
        assert got[i].n_hits == len(hosts[i].hits) > 0 and back.hits.tobytes() == hosts[i].hits.tobytes() and (back.per == hosts[i].per).all()
        assert (stale_hits[i][got[i].n_hits:] == 0x77).all()   # nothing behind the last record
        fresh = lib.motif(dr, m, E)   # torch's own buffers, the current stream
        assert fresh.hits.tobytes() == hosts[i].hits.tobytes() and (fresh.per == hosts[i].per).all()
    # a capacity one record short is refused with the exact size; host memory in the place of device memory is refused
    L = lib.load()
    names, patterns = lib.motif_request(requests[0][0])
    pats = lib._strs(patterns)
    err = C.create_string_buffer(512)
    n = C.c_int64(0)
    per = torch.empty(hosts[0].per.shape, dtype=torch.int64, device="cuda:0")
    hits = torch.full((len(hosts[0].hits), 16), 0x55, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    args = (C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, pats, len(names), 1, 0, None)
    assert L.sd_motif_reads_size_dev(*args, C.c_void_p(per.data_ptr()), C.byref(n), err, 512) == lib.SD_OK and n.value == len(hosts[0].hits)
    rc = L.sd_motif_reads_write_dev(*args, C.c_void_p(hits.data_ptr()), n.value - 1, err, 512)
    assert rc == lib.SD_ERR_PARAM and str(n.value).encode() in err.value and str(n.value - 1).encode() in err.value
    torch.cuda.synchronize()
    assert (hits == 0x55).all()   # nothing written
    hostbuf = np.zeros(16 * n.value, dtype=np.uint8)
    rc = L.sd_motif_reads_write_dev(*args, C.c_void_p(hostbuf.ctypes.data), n.value, err, 512)
    assert rc == lib.SD_ERR_PARAM and b"not in device memory" in err.value
    hostper = np.zeros(hosts[0].per.size, dtype=np.int64)
    rc = L.sd_motif_reads_size_dev(*args, C.c_void_p(hostper.ctypes.data), C.byref(n), err, 512)
    assert rc == lib.SD_ERR_PARAM and b"not in device memory" in err.value
    # a write call for another budget than the size call's is refused, and writes nothing
    assert L.sd_motif_reads_size_dev(*args, C.c_void_p(per.data_ptr()), C.byref(n), err, 512) == lib.SD_OK and n.value == len(hosts[0].hits)
    other = (C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, pats, len(names), 2, 0, None)
    rc = L.sd_motif_reads_write_dev(*other, C.c_void_p(hits.data_ptr()), n.value, err, 512)
    assert rc == lib.SD_ERR_PARAM and b"was not for these reads and motifs" in err.value
    torch.cuda.synchronize()
    assert (hits == 0x55).all()


# ---- the command line --------------------------------------------------------------------------------------------------

OPTS = ["--motif", "cenpb", "--motif-mismatches", "1", "--motif", "tel=TTAGGG"]
TSVS = ("final_decomposition.tsv", "final_decomposition_alt.tsv", "final_decomposition_raw.tsv")
OURS = ("final_decomposition_motif.tsv", "final_decomposition_motif_rows.tsv", "final_decomposition_motif_monomers.tsv")
WITH_BOX = {"A_0": (46, 26), "C_2": (46, 22), "D_3": (46, 18), "E_4": (46, 23), "H_7": (47, 12), "J_9": (47, 29)}   # rows, with a box at E = 1


def _run(prog, out, extra, rc=0):
    args = [os.path.join(TD, "read.fa")] + ([os.path.join(TD, "DXZ1_star_monomers.fa")] if prog == "stringdecomposer" else [])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog)] + args + ["-o", out, "-t", str(THREADS)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == rc, p.stderr
    return p


def test_cli_files(tmp_path):
    plain, with_flag, alone = (str(tmp_path / d) for d in ("plain", "flag", "alone"))
    _run("stringdecomposer", plain, [])
    _run("stringdecomposer", with_flag, OPTS)
    _run("sd-motif", alone, OPTS)
    for f in TSVS:   # the decomposition does not change
        assert open(os.path.join(with_flag, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
        assert not os.path.exists(os.path.join(alone, f))
    assert open(os.path.join(alone, OURS[0]), "rb").read() == open(os.path.join(with_flag, OURS[0]), "rb").read()
    assert not os.path.exists(os.path.join(alone, OURS[1])) and not os.path.exists(os.path.join(alone, OURS[2]))
    rn, rs, _ = lib.fasta_load(os.path.join(TD, "read.fa"))
    names = [n.split()[0] for n in rn]
    mono = [n.split()[0] for n in lib.fasta_load(os.path.join(TD, "DXZ1_star_monomers.fa"))[0]]
    patterns = [CENPB, "TTAGGG"]
    want, per = ref.scan(rs, patterns, 1)   # the reference, once for the three files
    m = formats.Motifs(np.array([(i, r, mo, s, mm) for r, mo, s, i, mm in want], dtype=lib.motif_hit_dtype()), np.array(per), ["cenpb", "tel"], patterns, 1)
    rows = formats.read_motif(os.path.join(with_flag, OURS[0]))
    assert formats.format_motif(rows) == open(os.path.join(with_flag, OURS[0])).read() == formats.format_motif(formats.motif_rows(m, names, rs))
    assert sum(r.motif == "cenpb" for r in rows) == 130
    order = [(r.start, ["cenpb", "tel"].index(r.motif), r.strand) for r in rows]
    assert order == sorted(order)   # read, start, motif, strand
    final = formats.read_final(os.path.join(with_flag, TSVS[0]))
    counts = formats.motif_row_counts(m.hits, final, m.lengths, names)
    rrows = formats.read_motif_rows(os.path.join(with_flag, OURS[1]))
    assert formats.format_motif_rows(rrows) == open(os.path.join(with_flag, OURS[1])).read() == formats.format_motif_rows(formats.motif_row_lines(counts, final, m.names))
    assert len(rrows) == len(final)
    mrows = formats.read_motif_monomers(os.path.join(with_flag, OURS[2]))
    assert formats.format_motif_monomers(mrows) == open(os.path.join(with_flag, OURS[2])).read() == formats.format_motif_monomers(formats.motif_monomers(counts, final, m.names, mono))
    box = {r.monomer: (r.rows, r.rows_hit) for r in mrows if r.motif == "cenpb"}
    for name, (n_rows, hit) in box.items():   # the final TSV of this run is the reference's: the figures of the golden rows
        assert name.endswith("'") and (n_rows, hit) == WITH_BOX.get(name[:3], (n_rows, 0)), name
    assert sorted(k[:3] for k, v in box.items() if v[1]) == sorted(WITH_BOX)
    log = open(os.path.join(with_flag, "stringdecomposer.log")).read()
    assert all(f in log for f in OURS)


def test_cli_refusal(tmp_path):
    out = str(tmp_path / "refused")
    p = _run("stringdecomposer", out, ["--motif", "cenpb", "--motif-mismatches", "9"], rc=2)
    assert len(p.stderr.strip().split("\n")) == 1 and "mismatches = 9" in p.stderr and not os.path.exists(out)
    p = _run("sd-motif", out, ["--motif", "cenpb", "--motif-mismatches", "9"], rc=2)
    assert len(p.stderr.strip().split("\n")) == 1 and not os.path.exists(out)
