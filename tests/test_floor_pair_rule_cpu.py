"""The floor level of a fill row by the previous and the current read symbol (sd_fast_fill.hpp, FastPlan::floor_pair).

A NumPy model of the lane recurrence as the narrow u16 fill runs it -- lazy carry K, KB = max(K, b), the floors applied in
place before the slot loop, cell 0 of a template without a keep move, pads that forward the last cell, the row maximum taken
from every lane's total with its template's end offset -- is run three times side by side: with the floor in every slot,
with the level of the row's read symbol, and with the level of the (previous, current) pair.  Every true cell max(L, K) and
every row maximum must agree, on random template sets, lane bounds, reads and the five scorings whose table is >= 0.
The levels are the exact ones (no groups of four slots), which is the hardest case: any group level is at or above them.

The second half checks lib.plan_floor_levels (host only): the matrix recomputed from the returned lane starts, its
identities, and the figures of the 12-monomer benchmark set.  No GPU anywhere."""
import random

import numpy as np
import pytest

from stringdecomposer_amd import lib, synth

NEG = -10 ** 9
SCORINGS = [(-1, -1, -1, 1), (-2, -3, -4, 2), (-1, -2, -2, 2), (-2, -2, -3, 1), (-1, -1, 0, 3)]   # (ins, del, mismatch, match)
ROWS = 400
CASES = 240


def _tv(c, b, sc):
    ins, dele, mm, ma = sc
    return (ma if (c == b and c < 4) else mm) - dele - ins


def _levels(lanes, sc):
    """Per-symbol and per-pair levels of a list of lanes (each a list of template codes), by the definition of the issue:
    the last slot q >= 1 where tbl_b[q] exceeds every earlier value of the lane and -- for the pair -- no earlier slot of the
    lane has tbl_a == tmax.  Behind an N the pair level is the symbol's."""
    tmax = max(sc[2], sc[3]) - sc[1] - sc[0]
    sym = [1] * 5
    pair = [[1] * 5 for _ in range(5)]
    for cells in lanes:
        for b in range(5):
            run = _tv(cells[0], b, sc)
            for q in range(1, len(cells)):
                val = _tv(cells[q], b, sc)
                if val > run:
                    run = val
                    sym[b] = max(sym[b], q)
                    for a in range(4):
                        if max(_tv(cells[x], a, sc) for x in range(q)) < tmax:
                            pair[a][b] = max(pair[a][b], q)
    pair[4] = list(sym)
    return sym, pair


def _random_bounds(rng, L, P):
    """Legal lane bounds of a template of L cells: ceil(L / P) lanes of 1..P cells, the first of at least two."""
    V = (L + P - 1) // P
    if V == 1:
        return [0, L]
    size = [2] + [1] * (V - 1)
    left = L - sum(size)
    while left > 0:
        u = rng.randrange(V)
        if size[u] < P:
            size[u] += 1
            left -= 1
    b = [0]
    for s in size:
        b.append(b[-1] + s)
    return b


def _random_template(rng, n):
    al = rng.sample(range(4), rng.choice([4, 4, 2, 3]))
    s = [rng.choice(al) for _ in range(n)]
    if rng.random() < 0.3:   # homopolymer prefix
        h = rng.randrange(1, min(n, 15))
        s[:h] = [rng.choice(al)] * h
    if rng.random() < 0.2:
        s[rng.randrange(n)] = 4
    return s


def _random_read(rng, T, rows):
    read = []
    while len(read) < rows:
        r = rng.random()
        if r < 0.6:     # a mutated template copy
            read += [c if rng.random() > 0.1 else rng.randrange(4) for c in rng.choice(T)]
        elif r < 0.8:   # a run
            read += [rng.randrange(4)] * rng.randrange(1, 12)
        elif r < 0.9:   # anything, N included
            read += [rng.choice([0, 1, 2, 3, 4]) for _ in range(rng.randrange(1, 10))]
        else:           # a two-letter stretch
            two = rng.sample(range(4), 2)
            read += [rng.choice(two) for _ in range(20)]
    return read[:rows]


def _run_case(seed, levels=None):
    rng = random.Random(seed)
    sc = SCORINGS[seed % len(SCORINGS)]
    P = [6, 8, 12, 16][(seed // len(SCORINGS)) % 4]
    ins, dele, mm, ma = sc
    assert min(mm, ma) - dele - ins >= 0 and dele <= 0
    T = [_random_template(rng, rng.randrange(14, 61)) for _ in range(rng.randrange(1, 6))]
    tmpl, first, cells = [], [], []
    for t, s in enumerate(T):
        b = _random_bounds(rng, len(s), P)
        for u in range(len(b) - 1):
            tmpl.append(t)
            first.append(u == 0)
            cells.append(s[b[u]:b[u + 1]])
    sym, pair = (levels or _levels)(cells, sc)
    assert all(pair[a][b] <= sym[b] for a in range(5) for b in range(5)) and all(pair[a][a] == sym[a] for a in range(5))
    read = _random_read(rng, T, ROWS)

    nl, nT = len(cells), len(T)
    tmpl = np.array(tmpl)
    first = np.array(first)
    # table [5][lane][slot], pads: min(tmin, 0) = 0 as in the u16 kernels
    tbl = np.zeros((5, nl, P), dtype=np.int64)
    for li, cs in enumerate(cells):
        for q, c in enumerate(cs):
            for b in range(5):
                tbl[b, li, q] = _tv(c, b, sc)
    endoff = np.array([(len(s) - 1) * dele + dele for s in T], dtype=np.int64)[tmpl]   # FLC_ENDALL + del: on every lane
    assert endoff.max() <= 0
    lane_u = np.zeros(nl, dtype=np.int64)   # index of the lane inside its template
    for li in range(1, nl):
        lane_u[li] = 0 if first[li] else lane_u[li - 1] + 1
    Vmax = int(lane_u.max()) + 1
    slot = np.arange(P)

    # three runs side by side: axis 0 = floors in every slot / by symbol / by pair
    Lc = np.full((3, nl, P), NEG, dtype=np.int64)
    K = np.full((3, nl), NEG, dtype=np.int64)
    bdel = np.zeros(3, dtype=np.int64)
    prev = 4
    for i, r in enumerate(read):
        if i == 0:
            lv = [P, P, P]                 # row 0 is another formula in the kernel: no level applies
        elif i == 1:
            lv = [P, sym[r], sym[r]]       # the row behind row 0 keeps the per-symbol level
        else:
            lv = [P, sym[r], pair[prev][r]]
        KB = np.maximum(K, bdel[:, None])                                    # [3, nl]
        # floors in place: L[q-1] = max(L[q-1], KB) for q = 1 .. level (q < P)
        fl = (slot[None, None, :] < np.array(lv)[:, None, None]) & (slot[None, None, :] < P - 1)
        Lc = np.where(fl, np.maximum(Lc, KB[:, :, None]), Lc)
        cand = np.empty_like(Lc)
        keep0 = np.where(first[None, :], NEG, Lc[:, :, 0])                   # cell 0 of a template has no keep move
        cand[:, :, 0] = np.maximum(np.maximum(KB + tbl[r, :, 0][None, :], keep0), K)   # the old carry joins the chain at slot 0
        cand[:, :, 1:] = np.maximum(Lc[:, :, :-1] + tbl[r, :, 1:][None, :, :], Lc[:, :, 1:])
        Lc = np.maximum.accumulate(cand, axis=2)
        tot = Lc[:, :, P - 1]                                                # lane totals
        bdel = (tot + endoff[None, :]).max(axis=1)                           # row maximum (+ del): the next row's start term
        # lazy carry: exclusive prefix maximum of the totals over the template's earlier lanes; it REPLACES the old one
        t2 = np.full((3, nT, Vmax + 1), NEG, dtype=np.int64)
        t2[:, tmpl, lane_u + 1] = tot
        K = np.maximum.accumulate(t2, axis=2)[:, tmpl, lane_u]
        true = np.maximum(Lc, K[:, :, None])
        if not (np.array_equal(true[0], true[1]) and np.array_equal(true[0], true[2])):
            return "row %d: cells differ (by symbol equal: %s, by pair equal: %s); sym %s pair %s" % (
                i, np.array_equal(true[0], true[1]), np.array_equal(true[0], true[2]), sym, pair)
        if not (bdel[0] == bdel[1] == bdel[2]):
            return "row %d: row maxima %s" % (i, bdel.tolist())
        prev = r
    return None


@pytest.mark.parametrize("block", range(8))
def test_pair_levels_keep_every_cell_and_row_maximum(block):
    per = CASES // 8
    for seed in range(block * per, (block + 1) * per):
        res = _run_case(seed)
        assert res is None, "case %d (scoring %s): %s" % (seed, SCORINGS[seed % len(SCORINGS)], res)


def test_model_notices_a_missing_floor():
    """The model is sensitive: with every level lowered to 1 (only slot 1 keeps its floor) some case differs."""
    ones = lambda lanes, sc: ([1] * 5, [[1] * 5 for _ in range(5)])
    assert any(_run_case(seed, levels=ones) is not None for seed in range(40))


# ---- lib.plan_floor_levels -------------------------------------------------------------------------------------------
_RC = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _matrix_from_layout(ms, starts, sc):
    """The plan's matrix restated: records per read symbol b (the plan compares plain match / mismatch scores; a template N
    meets a read N there), pairs for previous symbols A C G T, the symbol's level behind an N."""
    ins, dele, mm, ma = sc
    tmax = max(mm, ma)
    ms = [s.decode() if isinstance(s, bytes) else s for s in ms]
    tseq = list(ms) + ["".join(_RC[c] for c in reversed(s)) for s in ms]
    sym = [1] * 5
    pair = [[1] * 5 for _ in range(5)]
    for s, st in zip(tseq, starts):
        bnd = list(st) + [len(s)]
        for u in range(len(st)):
            codes = [_CODE.get(c, 4) for c in s[bnd[u]:bnd[u + 1]]]
            for b in range(5):
                run = ma if codes[0] == b else mm
                for q in range(1, len(codes)):
                    val = ma if codes[q] == b else mm
                    if val > run:
                        run = val
                        sym[b] = max(sym[b], q)
                        for a in range(4):
                            if all((ma if codes[x] == a else mm) < tmax for x in range(q)):
                                pair[a][b] = max(pair[a][b], q)
    pair[4] = list(sym)
    return sym, pair


def _check_identities(r):
    sym, pair = r["floor_sym"], r["floor_pair"]
    for a in range(5):
        assert pair[a][a] == sym[a]
        assert pair[4][a] == sym[a]
        for b in range(5):
            assert 1 <= pair[a][b] <= sym[b]


@pytest.mark.parametrize("n_mono,seed,scoring", [
    (12, 1, (-1, -1, -1, 1)), (12, 3, (-2, -3, -4, 2)), (12, 5, (-1, -2, -2, 2)), (6, 2, (-1, -1, 0, 3)), (16, 4, (-2, -2, -3, 1)),
    (20, 7, (-1, -1, -1, 1))])
def test_plan_floor_levels_matches_its_layout(n_mono, seed, scoring):
    _, ms = synth.make_monomers(n_mono, seed=seed)
    r = lib.plan_floor_levels(ms, scoring=scoring)
    assert r["family"] == "fast" and r["pair_rule"]
    assert len(r["lane_starts"]) == 2 * n_mono and all(st[0] == 0 for st in r["lane_starts"])
    P = r["cells_per_lane"]
    assert P == lib.plan_info(ms, scoring=scoring)["cells_per_lane"]
    for s, st in zip(list(ms) + list(ms), r["lane_starts"]):
        bnd = st + [len(s)]
        assert all(0 < bnd[u + 1] - bnd[u] <= P for u in range(len(st)))
    sym, pair = _matrix_from_layout(ms, r["lane_starts"], scoring)
    assert r["floor_sym"] == sym
    assert r["floor_pair"] == pair
    assert max(sym) == lib.plan_info(ms, scoring=scoring)["floor_slots"]
    _check_identities(r)


def test_plan_floor_levels_with_n_in_a_template():
    _, ms = synth.make_monomers(12, seed=9)
    ms = list(ms)
    ms[3] = ms[3][:40] + b"N" + ms[3][41:]
    r = lib.plan_floor_levels(ms)
    sym, pair = _matrix_from_layout(ms, r["lane_starts"], (-1, -1, -1, 1))
    assert r["floor_sym"] == sym and r["floor_pair"] == pair
    _check_identities(r)


@pytest.mark.parametrize("scoring", [(-1, -2, -4, 1), (-1, -1, -4, 1)])
def test_pair_levels_fall_back_to_symbol_levels(scoring):
    """A negative table value (mismatch below del + ins): a condition of the proof fails and every previous symbol gets the
    level of the current one.  (A positive deletion score, the other condition, never reaches the fast family.)"""
    _, ms = synth.make_monomers(12, seed=1)
    r = lib.plan_floor_levels(ms, scoring=scoring)
    assert r["family"] == "fast" and not r["pair_rule"]
    for a in range(5):
        assert r["floor_pair"][a] == r["floor_sym"]


def test_benchmark_set_matrix():
    """The 12-monomer set of the benchmark, default scoring: P = 35, per-symbol levels 16 / 15 / 10 / 6 and the pair matrix."""
    _, ms = synth.make_monomers(12, seed=1)
    r = lib.plan_floor_levels(ms)
    assert r["cells_per_lane"] == 35 and r["pair_rule"]
    assert r["floor_sym"] == [16, 15, 10, 6, 1]
    assert [row[:4] for row in r["floor_pair"][:4]] == [[16, 7, 5, 5], [6, 15, 8, 6], [4, 7, 10, 3], [4, 4, 4, 6]]
    assert r["floor_pair"][4] == [16, 15, 10, 6, 1]          # behind an N: the per-symbol level
    assert [row[4] for row in r["floor_pair"]] == [1] * 5    # an N row: slot 1 only
