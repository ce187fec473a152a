"""Motif hits with insertions and deletions (--motif-edits) on the device: the size and write kernels (sd_motif_edit_dev)
against the host form, array for array, at the edges of words, stretches, tiles, pattern blocks and launches; planted
instances with one insertion, deletion or substitution across every stretch end and the tile end; a thinned subset against
the naive tables of tests/motif_edit_ref.py; the device-resident form on DeviceReads; the command line's files."""
import argparse
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch   # before the library is loaded: one HIP runtime in the process, whichever test of the module runs first

import motif_edit_ref as ref
from conftest import GOLDEN
from motif_ref import COMP, IUPAC, revcomp_sets, sets
from stringdecomposer_amd import formats, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8
INFO = lib.motif_edits_info()
T, S, PB = INFO["tile"], INFO["stretch"], INFO["pattern_block"]
TILE = 64 * T
CENPB = lib.MOTIF_BUILTIN["cenpb"]


def text_of(rng, n):
    """random ACGT with about 1 % N and 1 % lower case"""
    return "".join(rng.choice("ACGT") if rng.random() >= 0.02 else rng.choice("Nacgt") for _ in range(n))


def acgt(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def plant(s, at, piece):
    return s[:at] + piece + s[at + len(piece):]


def one_edit(rng, pattern, kind):
    """(bases, edits): the pattern (ACGT only) with one deletion (0), one insertion (1) or one substitution (2) in its
    middle third, where no reading of the end as another kind of edit is as cheap"""
    L = len(pattern)
    x = rng.randrange(L // 3, 2 * L // 3)
    other = lambda b: rng.choice([c for c in "ACGT" if c != b])
    if kind == 0:
        return pattern[:x] + pattern[x + 1:], 1
    if kind == 1:
        return pattern[:x] + other(pattern[x]) + pattern[x:], 1   # (differs from the base behind it: the insertion has one place)
    return pattern[:x] + other(pattern[x]) + pattern[x + 1:], 1


def layout(reads, rng):
    """the reads in one buffer in a shuffled order with gaps of bases that would match if they were read"""
    order = list(range(len(reads)))
    rng.shuffle(order)
    off, parts, at = [0] * len(reads), [], 0
    for r in order:
        gap = acgt(rng, rng.randrange(0, 9))
        parts += [gap, reads[r]]
        off[r] = at + len(gap)
        at += len(gap) + len(reads[r])
    return "".join(parts) + "ACGT", off, [len(s) for s in reads]


def dev_equals_host(text, off, lens, motifs, K, min_launches=1):
    """the device form equals the host form byte for byte, and the kernels were launched for it"""
    before = lib.motif_edits_info()["launches"]
    dev = lib.motif_edits_text(text, off, lens, motifs, K, device=0)
    launched = lib.motif_edits_info()["launches"] - before
    host = lib.motif_edits_text(text, off, lens, motifs, K, threads=THREADS)
    assert dev.hits.dtype == host.hits.dtype and len(dev.hits) == len(host.hits), "%d hits on the device, %d on the host" % (len(dev.hits), len(host.hits))
    assert dev.hits.tobytes() == host.hits.tobytes()
    assert dev.per.shape == host.per.shape and (dev.per == host.per).all()
    assert launched >= min_launches, "the kernels were launched %d times" % launched
    return dev


def equals_reference_in(dev, reads, patterns, K, r, a, b):
    """The hits of read r equal the naive tables of the stretch [a, b) where the stretch decides them: an end j needs the
    L + K bases before j - 1 inside it (or the read's first base) and j + 1 inside it (or the read's end); -> their number"""
    n, lmax = len(reads[r]), max(len(p) for p in patterns)
    first = 1 if a == 0 else a + lmax + K + 2
    last = n if b == n else b - 1
    want, _ = ref.scan([reads[r][a:b]], patterns, K)
    want = [(r, m, s, i + a, ln, e) for _, m, s, i, ln, e in want if first <= i + a + ln <= last]
    h = dev.hits
    end = h["start"] + h["length"]
    assert ref.as_tuples(h[(h["read"] == r) & (end >= first) & (end <= last)]) == want
    return len(want)


@pytest.mark.parametrize("K", [0, 1, 3, 7])
def test_read_lengths_around_words_stretches_and_tiles(K):
    rng = random.Random(K)
    patterns = [CENPB, acgt(rng, 32), acgt(rng, 33), "".join(rng.choice("ACGTRYSWKMBDHVN") for _ in range(64)), "ACGTTGCAAC"]
    motifs = [("m%d" % i, p) for i, p in enumerate(patterns)]
    ns = [0, 1, 17, 63, 64, 65, S - 1, S, S + 1, TILE - 1, TILE, TILE + 1, TILE + S + 40]
    reads = [text_of(rng, n) for n in ns]
    for r, n in enumerate(ns):   # instances anywhere, then one across the tile's end, then one that ends at the last base
        spots = [(p, rng.randrange(n - len(p))) for p in patterns if n > len(p) + 1]
        across, last = patterns[(r + 1) % len(patterns)], patterns[r % len(patterns)]
        spots += [(across, TILE - len(across) // 2)] if n >= TILE + 64 else []
        spots += [(last, None)] if n > len(last) + 1 else []
        for p, at in spots:
            inst = "".join(rng.choice(IUPAC[c]) for c in p)
            x = rng.randrange(2, len(inst) - 2)
            inst = [inst, inst[:x] + inst[x + 1:], inst[:x] + "A" + inst[x:]][rng.randrange(3) if K else 0]
            if rng.randrange(2):
                inst = "".join(COMP[c] for c in reversed(inst))
            reads[r] = plant(reads[r], n - len(inst) if at is None else min(at, n - len(inst)), inst)
    text, off, lens = layout(reads, rng)
    dev = dev_equals_host(text, off, lens, motifs, K)
    assert dev.per.sum() == len(dev.hits) >= 20
    key = [(int(h["read"]), int(h["motif"]), int(h["strand_edits"]) >> 7, int(h["start"]) + int(h["length"])) for h in dev.hits]
    assert key == sorted(key)   # the canonical order
    compared = 0
    for r, n in enumerate(ns):   # a thinned subset against the naive tables: the short reads whole, the long ones around their edges
        if n <= S + 1:
            compared += equals_reference_in(dev, reads, patterns, K, r, 0, n)
        else:
            compared += equals_reference_in(dev, reads, patterns, K, r, n - 260, n)
            compared += equals_reference_in(dev, reads, patterns, K, r, min(n, TILE + 60) - 300, min(n, TILE + 60))
            compared += equals_reference_in(dev, reads, patterns, K, r, 0, 200)
    assert compared >= 20


def planted_reads(rng, pattern, spots_of):
    """reads of random ACGT with an instance of one edit at every spot of spots_of(read) -> (reads, the hits expected on +)"""
    reads, want = [], []
    for r in range(64):
        s, at_before = acgt(rng, TILE + 300), None
        for k, at in enumerate(spots_of(r)):
            inst, e = one_edit(rng, pattern, (r + k) % 3)
            assert at >= 0 and (at_before is None or at > at_before + 2 * len(pattern))
            s, at_before = plant(s, at, inst), at
            want.append((r, 0, 0, at, len(inst), e))
        reads.append(s)
    return reads, want


@pytest.mark.parametrize("L", [17, 32, 33, 64])
def test_planted_edits_across_stretch_and_tile_ends(L):
    """64 reads, one per bit offset of the tile's last word.  In read `bit` an instance with one insertion, deletion or
    substitution starts at that bit of the tile's last word -- so it, or its look-ahead base, crosses the tile's end, which
    is a stretch's end -- and further instances are laid around the other stretch ends of the tile, every 64th stretch end
    in one read and every one in some read, shifted by the bit so that instance, warm-up (the L + K bases before a stretch) and look-ahead each cross a
    stretch end in some read.  Each is found exactly once, with the planted start and length, and nothing else is."""
    rng = random.Random(L)
    pattern = acgt(rng, L)
    stretches = TILE // S

    def spots_of(bit):
        ends = [1 + bit + 64 * k for k in range(stretches // 64)]   # over the 64 reads: every stretch end of the tile once
        return [e * S - L - 9 + (bit * (L + 12)) // 64 for e in ends if L + 9 <= e * S <= TILE - 4 * L - 64] + [TILE - 64 + bit]
    reads, want = planted_reads(rng, pattern, spots_of)
    text, off, lens = layout(reads, rng)
    dev = dev_equals_host(text, off, lens, [("p", pattern)], 1)
    got = ref.as_tuples(dev.hits)
    assert [h for h in got if h[2] == 0] == want and len(want) >= 4 * 64 - 8
    assert dev.per[:, 0, 0].tolist() == [sum(1 for h in want if h[0] == r) for r in range(64)]
    assert {h[4] for h in want} == {L - 1, L, L + 1}
    minus = [h for h in got if h[2] == 1]   # (a random read of 33 kb may hold the reverse complement of 17 codes with an edit)
    assert len(minus) <= 2 if L == 17 else not minus
    for r in (0, 31, 63):
        equals_reference_in(dev, reads, [pattern], 1, r, TILE - 200, TILE + 200)


@pytest.mark.parametrize("K", [0, 1, 3, 7])
def test_the_edit_budget(K):
    """sites of exactly K edits are hits with that count, sites of K + 2 substitutions are none"""
    rng = random.Random(20 + K)
    pattern = acgt(rng, 64)
    n = TILE + 500
    s = acgt(rng, n)

    def site(subs):
        inst = list(pattern)
        for x in rng.sample(range(4, 60, 4), subs):
            inst[x] = rng.choice([c for c in "ACGT" if c != inst[x]])
        return "".join(inst)
    ok, no = [70, TILE - 40, TILE + 200], [300, TILE - 200, n - 64]
    for at in ok:
        s = plant(s, at, site(K))
    for at in no:
        s = plant(s, at, site(K + 2))
    dev = dev_equals_host(s, [0], [n], [("p", pattern)], K)
    assert ref.as_tuples(dev.hits) == [(0, 0, 0, at, 64, K) for at in ok]
    assert equals_reference_in(dev, [s], [pattern], K, 0, 0, 400) == 1


def motifs_of(rng, n_strands):
    """motifs with n_strands pattern-strands: short degenerate patterns, one or two palindromes among them"""
    pal = ["GAATTC", "ACGT"][:2 - n_strands % 2]
    out = [("pal%d" % i, p) for i, p in enumerate(pal)]
    while 2 * (len(out) - len(pal)) + len(pal) < n_strands:
        p = "".join(rng.choice("ACGTRYSWKMBDHVN") for _ in range(rng.randrange(5, 9)))
        if sum(c != "N" for c in p) >= 3 and revcomp_sets(sets(p)) != sets(p) and p not in [q for _, q in out]:
            out.append(("m%d" % len(out), p))
    return out


@pytest.mark.parametrize("n_strands", [PB - 1, PB, PB + 1, 2 * PB + 1])
def test_pattern_blocks(n_strands):
    rng = random.Random(n_strands)
    motifs = motifs_of(rng, n_strands)
    strands = lib.motif_compile(motifs, 0)[2]
    assert len(strands) == n_strands and sum(s.palindrome for s in strands) in (1, 2)
    reads = [text_of(rng, TILE + 100), text_of(rng, 300), ""]
    text, off, lens = layout(reads, rng)
    dev = dev_equals_host(text, off, lens, motifs, 1)
    assert len(dev.hits) > 1000 and all(dev.per[:, m, 1].sum() == 0 for m, (name, _) in enumerate(motifs) if name.startswith("pal"))
    assert equals_reference_in(dev, reads, [p for _, p in motifs], 1, 1, 0, 300) >= 20


def test_a_call_of_several_launches():
    """more (tile, pattern block) units than one launch takes: the same arrays from several launches of each pass"""
    rng = random.Random(4)
    units = INFO["launch_wg"] + 40   # short reads, a tile each, one pattern block
    reads = [acgt(rng, rng.randrange(30, 90)) for _ in range(units)]
    for r in range(0, units, 7):
        reads[r] = plant(reads[r], 5, one_edit(rng, CENPB.replace("N", "A"), r % 3)[0])
    text, off, lens = layout(reads, rng)
    before = lib.motif_edits_info()["launches"]
    dev = dev_equals_host(text, off, lens, ["cenpb", "tel=TTAGGG"], 1)
    assert lib.motif_edits_info()["launches"] - before == 4   # two launches of each pass
    assert len(dev.hits) >= units // 7 and set(dev.hits["read"][dev.hits["motif"] == 0].tolist()) >= set(range(0, units, 7))
    for r in (0, units - 5, units - 1):
        equals_reference_in(dev, reads, [CENPB, "TTAGGG"], 1, r, 0, len(reads[r]))


def test_the_device_resident_form():
    """motif_edits_device on a DeviceReads of padded rows, on a caller's stream, into stale buffers, twice without a wait"""
    rng = random.Random(12)
    reads = [text_of(rng, n) for n in (300, 0, TILE + 65, 64, 1000)]
    for r in (0, 2, 4):
        inst = one_edit(rng, CENPB.replace("N", "C"), r % 3)[0]
        reads[r] = plant(reads[r], len(reads[r]) - len(inst), inst if r % 4 else "".join(COMP[c] for c in reversed(inst)))
    width = max(len(s) for s in reads) + 13
    rows = np.frombuffer(("".join(s + "A" * (width - len(s)) for s in reads)).encode(), dtype=np.uint8).reshape(len(reads), width)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        data = torch.from_numpy(rows.copy()).to("cuda:0", non_blocking=False)
        dr = lib.DeviceReads(data, [len(s) for s in reads])
    requests = ((["cenpb", "tel=TTAGGG"], 1), ([("w", "WSWSNNA"), ("pal", "GAATTC")], 2))
    hosts = [lib.motif_edits(reads, m, K, threads=THREADS) for m, K in requests]
    with torch.cuda.stream(side):
        stale_hits = [torch.full((len(h.hits) + 5, 16), 0x77, dtype=torch.uint8, device="cuda:0") for h in hosts]
        stale_per = [torch.full(h.per.shape, 77, dtype=torch.int64, device="cuda:0") for h in hosts]
    before = lib.motif_edits_info()["launches"]
    got = [lib.motif_edits_device(dr, m, K, stream=side, hits=stale_hits[i], per=stale_per[i]) for i, (m, K) in enumerate(requests)]   # no wait in between
    assert lib.motif_edits_info()["launches"] >= before + 4
    side.synchronize()
    for i, (m, K) in enumerate(requests):
        assert got[i].hits.is_cuda and got[i].hits.data_ptr() == stale_hits[i].data_ptr() and got[i].per.data_ptr() == stale_per[i].data_ptr()
        back = got[i].to_host()
        assert got[i].n_hits == len(hosts[i].hits) > 0 and back.hits.tobytes() == hosts[i].hits.tobytes() and (back.per == hosts[i].per).all()
        assert (stale_hits[i][got[i].n_hits:] == 0x77).all()   # nothing behind the last record
        fresh = lib.motif_edits(dr, m, K)   # torch's own buffers, the current stream
        assert fresh.hits.tobytes() == hosts[i].hits.tobytes() and (fresh.per == hosts[i].per).all()
    assert hosts[0].per[:, 0].sum() >= 3
    # a capacity one record short is refused with both numbers; host memory in the place of device memory is refused
    L = lib.load()
    names, patterns = lib.motif_request(requests[0][0])
    pats = lib._strs(patterns)
    err = C.create_string_buffer(512)
    n = C.c_int64(0)
    per = torch.empty(hosts[0].per.shape, dtype=torch.int64, device="cuda:0")
    hits = torch.full((len(hosts[0].hits), 16), 0x55, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    args = (C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, pats, len(names), 1, 0, None)
    assert L.sd_motif_edit_reads_size_dev(*args, C.c_void_p(per.data_ptr()), C.byref(n), err, 512) == lib.SD_OK and n.value == len(hosts[0].hits)
    rc = L.sd_motif_edit_reads_write_dev(*args, C.c_void_p(hits.data_ptr()), n.value - 1, err, 512)
    assert rc == lib.SD_ERR_PARAM and str(n.value).encode() in err.value and str(n.value - 1).encode() in err.value
    torch.cuda.synchronize()
    assert (hits == 0x55).all()   # nothing written
    with pytest.raises(lib.SdError) as e:
        lib.motif_edits_device(dr, requests[0][0], 1, hits=hits[:n.value - 1])
    assert str(n.value) in e.value.msg and str(n.value - 1) in e.value.msg
    hostbuf = np.zeros(16 * n.value, dtype=np.uint8)
    assert L.sd_motif_edit_reads_size_dev(*args, C.c_void_p(per.data_ptr()), C.byref(n), err, 512) == lib.SD_OK
    rc = L.sd_motif_edit_reads_write_dev(*args, C.c_void_p(hostbuf.ctypes.data), n.value, err, 512)
    assert rc == lib.SD_ERR_PARAM and b"not in device memory" in err.value
    other = (C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, pats, len(names), 2, 0, None)   # another budget than the size call's
    rc = L.sd_motif_edit_reads_write_dev(*other, C.c_void_p(hits.data_ptr()), n.value, err, 512)
    assert rc == lib.SD_ERR_PARAM and b"was not for these reads and motifs" in err.value


def test_the_two_searches_keep_separate_work_areas():
    """The Hamming search (sd_motif_*) and the edit search each have a work area of their own on a device: a size call of
    the one neither disturbs what the other's size call left nor answers for the other's write call."""
    rng = random.Random(21)
    motifs, budget = ["cenpb", "tel=TTAGGG"], 1
    names, patterns = lib.motif_request(motifs)
    pats = lib._strs(patterns)
    L = lib.load()
    err = C.create_string_buffer(512)

    def device_reads(seed_offset):
        reads = [text_of(rng, n) for n in (300, 0, 64 * lib.MOTIF_TILE_WORDS + 65, 64)]
        for r in (0, 2):
            inst = one_edit(rng, CENPB.replace("N", "C"), (r + seed_offset) % 3)[0]
            reads[r] = plant(reads[r], len(reads[r]) - len(inst), inst)
        width = max(len(s) for s in reads) + 13
        rows = np.frombuffer(("".join(s + "A" * (width - len(s)) for s in reads)).encode(), dtype=np.uint8).reshape(len(reads), width)
        dr = lib.DeviceReads(torch.from_numpy(rows.copy()).to("cuda:0"), [len(s) for s in reads])
        return reads, dr, (C.c_void_p(dr.ptr), dr.c_off, dr.c_lens, dr.n, pats, len(names), budget, 0, None)

    reads_a, dr_a, args_a = device_reads(0)
    reads_b, dr_b, args_b = device_reads(1)
    host_h = lib.motif(reads_a, motifs, budget, threads=THREADS)
    host_e = lib.motif_edits(reads_a, motifs, budget, threads=THREADS)
    assert len(host_h.hits) > 0 and len(host_e.hits) > 0
    per_h = torch.full(host_h.per.shape, 77, dtype=torch.int64, device="cuda:0")
    per_e = torch.full(host_e.per.shape, 77, dtype=torch.int64, device="cuda:0")
    n_h, n_e = C.c_int64(0), C.c_int64(0)
    torch.cuda.synchronize()
    # both size calls on A, then both write calls: the edit size call left the Hamming work area as it was
    assert L.sd_motif_reads_size_dev(*args_a, C.c_void_p(per_h.data_ptr()), C.byref(n_h), err, 512) == lib.SD_OK, err.value
    assert L.sd_motif_edit_reads_size_dev(*args_a, C.c_void_p(per_e.data_ptr()), C.byref(n_e), err, 512) == lib.SD_OK, err.value
    assert n_h.value == len(host_h.hits) and n_e.value == len(host_e.hits)
    hits_h = torch.full((n_h.value, 16), 0x55, dtype=torch.uint8, device="cuda:0")
    hits_e = torch.full((n_e.value, 16), 0x55, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert L.sd_motif_reads_write_dev(*args_a, C.c_void_p(hits_h.data_ptr()), n_h.value, err, 512) == lib.SD_OK, err.value
    assert L.sd_motif_edit_reads_write_dev(*args_a, C.c_void_p(hits_e.data_ptr()), n_e.value, err, 512) == lib.SD_OK, err.value
    torch.cuda.synchronize()
    assert hits_h.cpu().numpy().tobytes() == host_h.hits.tobytes() and (per_h.cpu().numpy() == host_h.per).all()
    assert hits_e.cpu().numpy().tobytes() == host_e.hits.tobytes() and (per_e.cpu().numpy() == host_e.per).all()
    # the edit search sized on A, the Hamming search on B: the Hamming size call does not answer for an edit write call on B
    assert L.sd_motif_edit_reads_size_dev(*args_a, C.c_void_p(per_e.data_ptr()), C.byref(n_e), err, 512) == lib.SD_OK, err.value
    assert L.sd_motif_reads_size_dev(*args_b, C.c_void_p(per_h.data_ptr()), C.byref(n_h), err, 512) == lib.SD_OK, err.value
    blank = torch.full((max(n_e.value, n_h.value) + 64, 16), 0x55, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = L.sd_motif_edit_reads_write_dev(*args_b, C.c_void_p(blank.data_ptr()), blank.shape[0], err, 512)
    assert rc == lib.SD_ERR_PARAM and b"was not for these reads and motifs" in err.value
    torch.cuda.synchronize()
    assert (blank == 0x55).all()   # nothing written


# ---- the command line --------------------------------------------------------------------------------------------------
OPTS = ["--motif", "cenpb", "--motif-edits", "1"]
OURS = ("final_decomposition_motif.tsv", "final_decomposition_motif_rows.tsv", "final_decomposition_motif_monomers.tsv")


def test_cli_files(tmp_path):
    """stringdecomposer --motif cenpb --motif-edits 1 on the test read: the three files equal those of the host form byte for
    byte, and boxes of 16 and 18 bases are among the hits; sd-motif alone writes the same hit file"""
    out, alone, host = (str(tmp_path / d) for d in ("flag", "alone", "host"))
    reads, mono = os.path.join(TD, "read.fa"), os.path.join(TD, "DXZ1_star_monomers.fa")
    for prog, extra, o in (("stringdecomposer", [mono], out), ("sd-motif", [], alone)):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog), reads] + extra + ["-o", o, "-t", str(THREADS)] + OPTS,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr
    from stringdecomposer_amd import motif as cli
    os.makedirs(host)
    args = argparse.Namespace(motif=["cenpb"], motif_file=None, motif_mismatches=0, motif_edits=1, sequences=reads, monomers=mono, lenient=False,
                              threads=THREADS)
    saved = cli.write(args, os.path.join(out, "final_decomposition.tsv"), host, "final_decomposition", None)   # device None: host threads
    assert [os.path.basename(f) for f in saved] == list(OURS)
    for f in OURS:
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(host, f), "rb").read(), f
    assert open(os.path.join(alone, OURS[0]), "rb").read() == open(os.path.join(out, OURS[0]), "rb").read()
    assert not os.path.exists(os.path.join(alone, OURS[1]))
    rows = formats.read_motif(os.path.join(out, OURS[0]))
    sizes = [r.end - r.start + 1 for r in rows]
    assert len(rows) == 163 and sizes.count(16) == 18 and sizes.count(18) == 18 and sizes.count(17) == 127
    assert sum(r.strand == "+" for r in rows) == 161 and sum(r.mismatches == 1 for r in rows) == 94
    log = open(os.path.join(out, "stringdecomposer.log")).read()
    assert all(f in log for f in OURS)
