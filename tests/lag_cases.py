"""Inputs of the --lags tests: segments of a text in groups (the rows of a read), built so that the interesting pairs
occur -- shared by test_lags_cpu.py and test_gpu_lags.py."""
import random


def block_cols(K):
    """nw_block_cols of csrc/sd_nw.hpp: columns per register-resident block of the identity walk"""
    return 16 if K <= 1 else 12 if K == 2 else 9 if K == 3 else 6 if K == 4 else 4 if K <= 6 else 3


def words(tl):
    """64-bit words of a target's masks (5 and 7 run as 6 and 8)"""
    k = max(1, (tl + 63) // 64)
    return k if k <= 4 else 6 if k <= 6 else 8


def rand_seq(r, n, alphabet="ACGT"):
    return "".join(r.choice(alphabet) for _ in range(n))


def mutate(r, s, rate=0.08, alphabet="ACGT"):
    out = []
    for ch in s:
        x = r.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append(r.choice(alphabet))
        elif x < rate:
            out.append(ch)
            out.append(r.choice(alphabet))
        else:
            out.append(ch)
    return "".join(out)


def fit(r, s, n, alphabet="ACGT"):
    """s cut or extended to n symbols"""
    return s[:n] if len(s) >= n else s + rand_seq(r, n - len(s), alphabet)


def layout(groups, seed=0, gap=3):
    """groups: lists of segment strings -> (text, starts, ends, group_off); segments lie in text order with 0..gap bases
    between them; an empty string becomes an empty segment (end = start - 1)"""
    r = random.Random(seed)
    text, starts, ends, off = [], [], [], [0]
    at = 0
    for g in groups:
        for s in g:
            pad = rand_seq(r, r.randrange(gap + 1))
            text.append(pad)
            at += len(pad)
            starts.append(at)
            ends.append(at + len(s) - 1)
            text.append(s)
            at += len(s)
        off.append(len(starts))
    return "".join(text) or "N", starts, ends, off


def pool(seed=1, extra_byte=None):
    """A small pool of distinct segment strings: relatives of one 40-bp unit (so identities vary), segments with N, an
    exact duplicate (identical neighbours), a 1-bp segment, a 513-bp and a 1025-bp segment.  Drawing rows from a pool keeps
    the number of distinct pairs small, whatever the number of rows."""
    r = random.Random(seed)
    unit = rand_seq(r, 40)
    p = [unit, unit]
    p += [mutate(r, unit, 0.15) for _ in range(12)]
    p += [mutate(r, unit, 0.1, "ACGTN") for _ in range(4)]
    p += [unit[:17] + "NNN" + unit[20:], "N" * 9, "A", "T", rand_seq(r, 64), rand_seq(r, 65)]
    long_t = fit(r, mutate(r, unit * 13, 0.1), 513)
    long_q = fit(r, mutate(r, unit * 26, 0.1), 1025)
    p += [long_t, long_q, fit(r, mutate(r, long_t, 0.05), 500)]
    if extra_byte:
        p.append(unit[:10] + extra_byte + unit[11:])
    return p


def pooled_groups(sizes, pool_, seed=2):
    """groups of the given sizes, rows drawn from the pool; runs of equal rows do occur (the pool holds a duplicate)"""
    r = random.Random(seed)
    return [[r.choice(pool_) for _ in range(n)] for n in sizes]


def length_case(tl, n_pairs=100, seed=0, target=None):
    """One group [Q0, T0, Q1, T1, ...] for D = 1: pair (Qi -> Ti) has a target of tl bases and a query whose length walks
    through S - 1, S, S + 1, 2 S + 1 (S = the block columns of the target's word class), tl itself and 1024; pair
    (Ti -> Qi+1) has those as targets.  target: a function i -> the i-th target (default: relatives of one random unit)."""
    r = random.Random(1000 * tl + seed)
    S = block_cols(words(tl))
    qlens = [S - 1, S, S + 1, 2 * S + 1, tl, 1024, max(1, tl - 3), tl + 5]
    unit = rand_seq(r, tl)
    rows = []
    for i in range(n_pairs):
        t = target(i) if target else (unit if i % 7 == 0 else fit(r, mutate(r, unit, 0.1, "ACGTN" if i % 5 == 0 else "ACGT"), tl))
        assert len(t) == tl
        n = max(1, qlens[i % len(qlens)])
        q = fit(r, mutate(r, t.replace("N", "A") if i % 3 else t, 0.08), n)
        rows += [q, t]
    return [rows]
