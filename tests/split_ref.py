"""A numpy restatement of the rule of --split (the subfamilies of a monomer's instances), written from its definition and
not from the C++: rows are symbol vectors over 0..5 (A C G T N, deleted), H counts the columns in which two of them
differ, mode is the per-column most frequent symbol (ties: the smallest code), assign gives every row the centre of
smallest H (ties: the smallest centre index).  Plain and slow: the tests use small inputs."""
import numpy as np

NSYM = 6


def hamming(x, c):
    return int((np.asarray(x) != np.asarray(c)).sum())


def mode(rows):
    """per column the most frequent symbol of rows [n, L], ties to the smallest code"""
    rows = np.asarray(rows)
    counts = np.stack([(rows == s).sum(axis=0) for s in range(NSYM)], axis=0)   # [6, L]
    return counts.argmax(axis=0).astype(np.uint8)                               # (argmax: the first of equal maxima)


def assign(rows, centres):
    """-> assign, d1, d2 per row; d2 = the smallest distance to any other centre, -1 with one centre"""
    rows, centres = np.asarray(rows), np.asarray(centres)
    dist = (rows[:, None, :] != centres[None, :, :]).sum(axis=2)                # [n, k]
    a = dist.argmin(axis=1)                                                     # (the first of equal minima)
    d1 = dist[np.arange(len(rows)), a]
    if centres.shape[0] == 1:
        d2 = np.full(len(rows), -1)
    else:
        other = dist.copy()
        other[np.arange(len(rows)), a] = np.iinfo(dist.dtype).max
        d2 = other.min(axis=1)
    return a.astype(np.int32), d1.astype(np.int32), d2.astype(np.int32)


def lloyd_modes(rows, a, centres):
    """mode per cluster; a cluster without a member keeps its centre"""
    out = np.array(centres, copy=True)
    for c in range(len(centres)):
        if (a == c).any():
            out[c] = mode(rows[a == c])
    return out


def split(rows, R, K=64, S=8, I=16, trace=None):
    """-> dict(centres [k, L], assign, d1, d2, sizes, rounds, iters); trace (a list) receives one tuple per round:
    (seed row, its d1, "kept" | "rejected", the size of the new cluster)"""
    rows = np.asarray(rows, dtype=np.uint8)
    n = rows.shape[0]
    if n == 0:
        z = np.zeros(0, dtype=np.int32)
        return dict(centres=np.zeros((0, rows.shape[1]), dtype=np.uint8), assign=z, d1=z, d2=z, sizes=z, rounds=0, iters=0)
    centres = mode(rows)[None, :]
    cand = np.ones(n, dtype=bool)
    a, d1, d2 = assign(rows, centres)
    rounds = iters = 0
    while len(centres) < K and rounds < 4 * K:
        if not cand.any():
            break
        far = np.where(cand, d1, -1)
        i = int(far.argmax())                     # the largest d1, ties to the smallest row
        if d1[i] < R:
            break
        rounds += 1
        tc = np.concatenate([centres, rows[i][None, :]], axis=0)
        ta, t1, t2 = assign(rows, tc)
        for _ in range(I):
            tc = lloyd_modes(rows, ta, tc)
            na, t1, t2 = assign(rows, tc)
            iters += 1
            same = bool((na == ta).all())
            ta = na
            if same:
                break
        size = int((ta == len(tc) - 1).sum())
        if size < S:
            cand[i] = False
            if trace is not None:
                trace.append((i, int(d1[i]), "rejected", size))
            continue
        if trace is not None:
            trace.append((i, int(d1[i]), "kept", size))
        centres, a, d1, d2 = tc, ta, t1, t2
    sizes = np.array([(a == c).sum() for c in range(len(centres))], dtype=np.int32)
    return dict(centres=centres, assign=a, d1=d1, d2=d2, sizes=sizes, rounds=rounds, iters=iters)


def planted(rng, classes, per_class, L, divergence, noise, junk=0):
    """`classes` centres that differ from a random base in about `divergence` of the columns, `per_class` rows of each with
    `noise` of the columns replaced (substitutions, N and deletions), `junk` uniformly random rows; shuffled.
    -> (rows uint8 [n, L], label int [n], -1 for junk)"""
    base = rng.integers(0, 4, L)
    rows, label = [], []
    for c in range(classes):
        cen = base.copy()
        m = rng.random(L) < divergence
        cen[m] = (cen[m] + rng.integers(1, 4, int(m.sum()))) % 4
        for _ in range(per_class):
            x = cen.copy()
            e = rng.random(L) < noise
            x[e] = rng.integers(0, NSYM, int(e.sum()))
            rows.append(x)
            label.append(c)
    for _ in range(junk):
        rows.append(rng.integers(0, NSYM, L))
        label.append(-1)
    order = rng.permutation(len(rows))
    return np.asarray(rows, dtype=np.uint8)[order], np.asarray(label)[order]
