"""The shapes that the CPU and the GPU tests of the team form of cyclic pairs share (sd_cyclic_pairs_long<K, L>, its host
emulation sd_cyclic_pairs_team_host): per class (K, L) the query lengths at the lane boundaries and at the class's capacity,
targets shorter than, as long as and longer than the ramp of L - 1 steps, and one related target.  The host form's arrays of
a class are computed once (host_arrays) and shared."""
import functools
import random

import cyclic_ref as ref
from stringdecomposer_amd import lib

THREADS = 16
CLASSES = [(K, L) for L in (16, 32, 64) for K in (1, 2, 3, 4)]


def query_lengths(K, L):
    """1, around the first lane boundary, around the last lane's first row, one below the capacity, and the capacity (pad 0)"""
    cap = 64 * K * L
    return sorted({n for n in (1, 64 * K - 1, 64 * K, 64 * K + 1, 64 * K * (L - 1) - 1, 64 * K * (L - 1) + 1, cap - 1, cap) if 1 <= n <= cap})


def target_lengths(L):
    """1, 2, and a strand of 2 |t| - 1 columns around the ramp; 171"""
    return [1, 2, L - 1, L, L + 1, 171]


@functools.lru_cache(maxsize=None)
def case(K, L):
    """(seqs, queries, targets): the class's sequences; the last target is a rotation on strand - of the longest query (the
    capacity: every lane at work, pad 0) with 5 spaced edits, so that distances are not all near |q|"""
    rng = random.Random(1000 * K + L)
    ql, tl = query_lengths(K, L), target_lengths(L)
    seqs = [ref.rnd(rng, n) for n in ql + tl]
    seqs.append(ref.edited(rng, ref.rotated(seqs[len(ql) - 1], 64 * K * L // 3, 1), 5))
    return seqs, list(range(len(ql))), list(range(len(ql), len(seqs)))


@functools.lru_cache(maxsize=None)
def host_arrays(K, L):
    """the host form on the class's case: formats.CyclicPairs, to be left as it is"""
    seqs, q, t = case(K, L)
    return lib.cyclic_pairs(seqs, q, t, threads=THREADS)


def same_arrays(got, want):
    """dist / end / strand byte for byte; got: a CyclicPairs or the dict of a bench call"""
    for name in ("dist", "end", "strand"):
        a = got[name] if isinstance(got, dict) else getattr(got, name)
        b = getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


def merge_seeds(seed=7, per_family=8):
    """(names, seqs, family per sequence): seeds of 2 054 bp from three unrelated planted families, each at a random
    rotation, on a random strand, with up to 4 % spaced edits, and a fourth family of 4 108-bp dimers of the first"""
    rng = random.Random(seed)
    fam = [ref.rnd(rng, 2054) for _ in range(3)]
    seqs, label = [], []
    for i in range(3 * per_family):
        f = i % 3
        s = ref.rotated(fam[f], rng.randrange(2054), rng.randrange(2))
        seqs.append(ref.edited(rng, s, rng.randrange(2054 * 4 // 100 + 1)))
        label.append(f)
    for _ in range(4):
        s = ref.rotated(fam[0] + fam[0], rng.randrange(4108), rng.randrange(2))
        seqs.append(ref.edited(rng, s, rng.randrange(40)))
        label.append(3)
    names = ["s%d count=%d" % (i, 1 + (i * 7) % 5) for i in range(len(seqs))]
    return names, seqs, label
