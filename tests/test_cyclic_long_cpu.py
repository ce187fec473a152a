"""The team form of cyclic pairs (queries of 2 049 to 16 384 bp: a query across L lanes, K words each) without a GPU: the
host emulation of the kernel's schedule (sd_cyclic_pairs_team_host) against the host form, byte for byte, in all twelve
classes at the lane boundaries, at pad 0 and on strands shorter than the ramp; a thinned subset against the naive table of
tests/cyclic_ref.py; the class table; the symbols and limits of the header; the refusals."""
import os
import re

import pytest

import cyclic_long_cases as cases
import cyclic_ref as ref
from stringdecomposer_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sd_cyclic_pairs_team_host", "sd_cyclic_long_info", "sd_cyclic_long_kernel_bench")


def test_symbols_and_limits():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert getattr(L, name) is not None and name in lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
    assert re.search(r"#define SD_CYCLIC_QMAX_LONG 16384\b", header) and lib.CYCLIC_QMAX_LONG == 16384
    assert re.search(r"#define SD_CYCLIC_QMAX 2048\b", header) and lib.CYCLIC_QMAX == 2048 == lib.cyclic_info()["lmax_query"]
    info = lib.cyclic_long_info()
    assert info["lmax_query"] == lib.CYCLIC_QMAX_LONG == max(64 * K * L for K, L in lib.CYCLIC_TEAM_CLASSES)
    assert info["classes"] == len(lib.CYCLIC_TEAM_CLASSES) == len(cases.CLASSES) == 12 and sorted(lib.CYCLIC_TEAM_CLASSES) == sorted(cases.CLASSES)
    assert info["teams_per_wave"] == 64 // min(L for _, L in lib.CYCLIC_TEAM_CLASSES) == 4
    assert info["launches"] >= 0


def test_the_class_of_a_length():
    """the smallest K L that holds the words, the larger K of equal capacities; the header file has the same rule"""
    want = {1: (1, 16), 1024: (1, 16), 1025: (2, 16), 2048: (2, 16), 2049: (3, 16), 2054: (3, 16), 3072: (3, 16), 3073: (4, 16), 4096: (4, 16),
            4097: (3, 32), 6144: (3, 32), 6145: (4, 32), 8192: (4, 32), 8193: (3, 64), 12288: (3, 64), 12289: (4, 64), 16384: (4, 64), 16385: None}
    for n, c in want.items():
        assert lib.cyclic_team_class(n) == c, n
    for n in range(1, 16385, 61):
        K, L = lib.cyclic_team_class(n)
        words = (n + 63) // 64
        assert K * L >= words and not any(k * l >= words and (k * l, -k) < (K * L, -K) for k, l in lib.CYCLIC_TEAM_CLASSES), n


@pytest.mark.parametrize("K,L", cases.CLASSES)
def test_emulation_equals_the_host_form(K, L):
    seqs, q, t = cases.case(K, L)
    assert [len(seqs[a]) for a in q] == cases.query_lengths(K, L) and len(seqs[q[-1]]) == 64 * K * L
    assert [len(seqs[b]) for b in t[:-1]] == [1, 2, L - 1, L, L + 1, 171]
    got = lib.cyclic_pairs_team_host(seqs, q, t, K, L, threads=cases.THREADS)
    want = cases.host_arrays(K, L)
    cases.same_arrays(got, want)
    assert got.phase.tobytes() == want.phase.tobytes()
    # the related target: the longest query on strand -, five edits away at most
    assert got.strand[-1, -1] == 1 and got.dist[-1, -1] <= 5
    # a thread count does not show
    one = lib.cyclic_pairs_team_host(seqs, q[:3], t[:4], K, L, threads=1)
    assert one.dist.tobytes() == want.dist[:3, :4].tobytes() and one.end.tobytes() == want.end[:3, :4].tobytes()


def test_emulation_equals_the_table_on_a_thinned_subset():
    """every class once against the naive table: the query of 64 K (L - 1) + 1 bases, whose first row is the last row of the
    team's first lane, so that every lane boundary carries, against the target of 171 bases; in the classes of up to 2 048
    rows also the longest query against the related target.  Eleven pairs have a side over 2 048 bp."""
    strands, long_sides = set(), 0
    for K, L in cases.CLASSES:
        seqs, q, t = cases.case(K, L)
        got = lib.cyclic_pairs_team_host(seqs, q, t, K, L, threads=cases.THREADS)
        ql = cases.query_lengths(K, L)
        pairs = [(ql.index(64 * K * (L - 1) + 1), len(t) - 2)]
        if 64 * K * L <= 2048:
            pairs.append((len(q) - 1, len(t) - 1))
        for a, b in pairs:
            qs, ts = seqs[q[a]], seqs[t[b]]
            long_sides += max(len(qs), len(ts)) > 2048
            want = ref.pair(qs, ts)
            assert (int(got.dist[a, b]), int(got.end[a, b]), int(got.strand[a, b]), int(got.phase[a, b])) == want, (K, L, len(qs), len(ts))
            strands.add(want[2])
    assert strands == {0, 1} and long_sides <= 12


def test_refusals():
    seqs = ["ACGT" * 300, "ACGTTGCA"]   # 1 200 and 8 bases
    for K, L in ((0, 16), (5, 16), (1, 8), (4, 48), (4, 128), (16, 4)):
        for call in (lambda: lib.cyclic_pairs_team_host(seqs, [1], [1], K, L), lambda: lib.cyclic_long_kernel_bench(seqs, [1], [1], 0, K, L)):
            with pytest.raises(lib.SdError) as e:
                call()
            assert e.value.code == lib.SD_ERR_PARAM and "is no class of the team kernel" in e.value.msg and "\n" not in e.value.msg, e.value.msg
    for call in (lambda: lib.cyclic_pairs_team_host(seqs, [1, 0], [1], 1, 16), lambda: lib.cyclic_long_kernel_bench(seqs, [1, 0], [1], 0, 1, 16)):
        with pytest.raises(lib.SdError) as e:
            call()
        assert e.value.code == lib.SD_ERR_PARAM and "\n" not in e.value.msg
        assert e.value.msg.endswith("query 1 has 1200 bases, the class of 1 words x 16 lanes holds 1024"), e.value.msg
    # the library's own line, where the wrapper's check is not in the way
    import ctypes as C
    import numpy as np
    text, ro, rl = lib._reads_text(seqs)
    qi, out = np.array([0], dtype=np.int32), [np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint8)]
    err = C.create_string_buffer(512)
    rc = lib.load().sd_cyclic_pairs_team_host(text, ro.ctypes.data, rl.ctypes.data, 2, qi.ctypes.data, qi.ctypes.data, 1, 1, 1, 16, 1,
                                              out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, err, 512)
    assert rc == lib.SD_ERR_PARAM and err.value.decode() == "sd_cyclic_pairs_team_host: query 0 has 1200 bases, the class of 1 words x 16 lanes holds 1024"
    ms, info = (C.c_float * 1)(), (C.c_int64 * 4)()
    rc = lib.load().sd_cyclic_long_kernel_bench(text, ro.ctypes.data, rl.ctypes.data, 2, qi.ctypes.data, qi.ctypes.data, 1, 1, 0, 1, 16, 0, 1, ms, info,
                                                None, None, None)
    assert rc == lib.SD_ERR_PARAM   # (before any device work: this test runs without a device)
