"""The cases of tests/long_ident_cases.py without a GPU: they lie on the edges they exist for, the host identities
(sd_identity_segments, what the device route deals its split pairs to) equal the reference's edlib on every pair of every
call, the low-complexity pairs decide the traceback's ties, and the route counters have their documented layout."""
import numpy as np
import pytest

import edlib_ref
import long_ident_cases as lc
from stringdecomposer_amd import lib, synth


def test_edlib_is_the_reference():
    """The references below are the reference's vendored edlib itself, not a restatement of it."""
    assert edlib_ref.have_edlib()


def test_cases_lie_on_their_edges():
    lc.check_cases()
    assert [lc.qstar(max(v)) for v in lc.SETS.values()] == [5760, 4288, 3200, 3008, 2112, 1600]
    assert [lc.splits(q, t) for q, t in ((19584, 171), (19585, 171))] == [False, True]   # "~19.6 kb against 171 bp"


@pytest.mark.parametrize("homo", [False, True], ids=["plain", "homo"])
@pytest.mark.parametrize("name", list(lc.SETS))
def test_host_identities_equal_edlib_on_every_pair(name, homo):
    """Exact equality in (distance, matches, columns), all-vs-all and in the pair_tmpl forms."""
    assert edlib_ref.have_edlib()
    s = lc.long_set(name)
    for form in ("all", "pair", "one"):
        seq, starts, ends, pt, _ = s.call(form)
        got = lib.identity_segments(seq, starts, ends, s.templates, homo, threads=8, pair_tmpl=pt)
        for g, w, what in zip(got, lc.reference_of(name, form, homo), ("dist", "matches", "columns")):
            assert g.shape == w.shape and (g == w).all(), (name, homo, form, what, np.argwhere(g != w)[:5])
    d, m, c = lc.reference(name, homo)
    assert (d[0] == -1).all() and (m[0] == 0).all() and (c[0] == 0).all()      # the empty segment
    assert (d[1:] >= 0).all() and (c[1:] == d[1:] + m[1:]).all()


def test_host_identities_equal_edlib_on_the_rounds_case():
    r = lc.ROUNDS
    got = lib.identity_segments(r.seq, r.starts, r.ends, r.templates, False, threads=8)
    for g, w in zip(got, lc.reference("rounds", False)):
        assert (g == w).all()


def _walk(q, t, order):
    """(distance, '=' columns) of the unit-cost global alignment a full-matrix traceback from the bottom-right corner picks
    with the moves tried in `order`: "U" up (a query symbol against a gap), "L" left (a template symbol against a gap),
    "D" diagonal.  Rows are query symbols, columns template symbols, as edlib lays the matrix out."""
    n, m = len(q), len(t)
    qa, ta = np.frombuffer(q, dtype=np.uint8), np.frombuffer(t, dtype=np.uint8)
    D = np.zeros((n + 1, m + 1), dtype=np.int64)
    D[0, :] = np.arange(m + 1)
    ar = np.arange(m + 1)
    for i in range(1, n + 1):
        best = np.minimum(D[i - 1, :-1] + (ta != qa[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(np.concatenate([[i], best]) - ar) + ar      # the left moves: a running minimum
    i, j, matches = n, m, 0
    while i > 0 and j > 0:
        can = {"U": D[i - 1, j] + 1 == D[i, j], "L": D[i, j - 1] + 1 == D[i, j],
               "D": D[i - 1, j - 1] + (q[i - 1] != t[j - 1]) == D[i, j]}
        mv = next(x for x in order if can[x])
        if mv == "U":
            i -= 1
        elif mv == "L":
            j -= 1
        else:
            matches += q[i - 1] == t[j - 1]
            i, j = i - 1, j - 1
    return int(D[n, m]), int(matches)


def test_the_low_complexity_pairs_decide_the_traceback_ties():
    """Ten mutated 530-bp pairs of the low-complexity kinds: a plain walk with edlib's priority up > left > diagonal gives
    edlib's distance and match count on all of them; with the diagonal first the match count of at least five changes (measured: all
    ten, by 1 to 6 matches) -- so a kernel that prefers the diagonal does not pass on these texts."""
    st = synth.Stream(902, 1)
    changed = 0
    for k in range(10):
        t = lc.content(st, 1 + k % 4, 530)
        q = synth._to_ascii(synth.mutate(lc._codes(t), st, 0.06, 0.03, 0.03))
        e = edlib_ref.nw(q, t)
        assert _walk(q, t, "ULD") == e[:2], k
        other = _walk(q, t, "DUL")
        assert other[0] == e[0]
        changed += other[1] != e[1]
    assert changed >= 5, changed


def test_route_counter_layout():
    c = lib.nw_route_counts()
    assert tuple(c) == lib.NW_ROUTE_KEYS == ("long_calls", "long_pairs", "long_host_pairs", "long_rounds_max", "short_calls",
                                             "short_pairs", "declined_calls")
    assert set(lc.COUNT_KEYS) == set(lib.NW_ROUTE_KEYS) - {"long_rounds_max"}
    assert all(isinstance(v, int) and v >= 0 for v in c.values())
    assert lib.nw_route_counts() == c      # reading moves nothing
