"""The rule of cyclic pairs and of the merge written naively from its text (include/sd_hip.h, "cyclic pairs and the merge of
seed monomers"): the text doubled and reverse-complemented explicitly, the table D column by column in numpy (the vertical
dependency as a minimum.accumulate of c_k - k), the end rule, the strand rule, the merge as one plain walk over all
sequences, the canonical record by trying every rotation.  No bit vectors, no blocks.  The tests of the cyclic pass compare
the library against it."""
import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def doubled(t, strand):
    """U = t^s t^s without its last base"""
    ts = revcomp(t) if strand else t
    return (ts + ts)[:-1]


def bottom_row(q, text):
    """D(j), j = 0 .. len(text) - 1: the smallest edit distance of q to a substring of text that ends at j inclusive"""
    m = len(q)
    qa = np.frombuffer(q.encode(), dtype=np.uint8)
    mis = {c: (qa != ord(c)).astype(np.int64) for c in "ACGT"}
    k = np.arange(m + 1, dtype=np.int64)
    col = k.copy()                       # before the first column: D[i] = i
    out = np.empty(len(text), dtype=np.int64)
    cand = np.empty(m + 1, dtype=np.int64)
    for j, c in enumerate(text):
        cand[0] = 0                      # the empty prefix costs nothing wherever it ends: a fit may start anywhere
        np.minimum(col[:-1] + mis[c], col[1:] + 1, out=cand[1:])   # substitution or match; an inserted text base
        col = np.minimum.accumulate(cand - k) + k                  # deleted query bases: D[i] = min_k cand[k] + (i - k)
        out[j] = col[m]
    return out


def strand_result(q, t, strand):
    """(dist_s, end_s): the minimum of D and the smallest j that attains it"""
    d = bottom_row(q, doubled(t, strand))
    j = int(np.argmin(d))                # (the first of equal minima)
    return int(d[j]), j


def pair(q, t):
    """(dist, end, strand, phase): that of +, unless dist_- is strictly smaller"""
    dp, ep = strand_result(q, t, 0)
    dm, em = strand_result(q, t, 1)
    if dm < dp:
        return dm, em, 1, (em + 1) % len(t)
    return dp, ep, 0, (ep + 1) % len(t)


def radius(P, m):
    return (100 - P) * m // 100


def merge(seqs, weights, P, pair_fn=pair):
    """The walk: by weight descending, then index ascending; a sequence close to no centre becomes the next one, any other
    joins the close centre of smallest dist, the earliest of equals.  -> (cluster, centre, dist, end, strand) per sequence
    and the number of clusters.  A centre: dist 0, end |c| - 1, strand 0."""
    n = len(seqs)
    order = sorted(range(n), key=lambda i: (-weights[i], i))
    centres = []
    res = [None] * n
    for i in order:
        q, R = seqs[i], radius(P, len(seqs[i]))
        best = None
        for c, ci in enumerate(centres):
            if abs(len(q) - len(seqs[ci])) > R:
                continue
            d, e, s, _ = pair_fn(q, seqs[ci])
            if d <= R and (best is None or d < best[2]):
                best = (c, ci, d, e, s)
        if best is None:
            centres.append(i)
            res[i] = (len(centres) - 1, i, 0, len(q) - 1, 0)
        else:
            res[i] = best
    return res, len(centres)


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------
def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rotated(c, r, strand):
    """the rotation by r of c on the strand: a query whose exact fit in c has that strand and phase r"""
    s = revcomp(c) if strand else c
    return s[r:] + s[:r]


def edited(rng, s, e):
    """s with e edits at evenly spaced places: substitution, insertion, deletion in turn"""
    s = list(s)
    for x in range(e):
        i = (2 * x + 1) * len(s) // (2 * e)
        kind = x % 3
        if kind == 0:
            s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
        elif kind == 1:
            s.insert(i, rng.choice("ACGT"))
        else:
            del s[i]
    return "".join(s)


ROTATIONS = lambda n: (0, 1, 63, 64, 65, n - 1)   # noqa: E731


def planted(seed, n):
    """(c, [(query, r, strand, edits)]): a random c of n bases and its rotations by ROTATIONS(n) on either strand, exact and
    with 1, 3 and 8 spaced edits"""
    import random
    rng = random.Random(seed)
    c = rnd(rng, n)
    cases = []
    for r in ROTATIONS(n):
        for strand in (0, 1):
            for e in (0, 1, 3, 8):
                cases.append((edited(rng, rotated(c, r, strand), e), r, strand, e))
    return c, cases


def families(seed, n=200, lens=(171, 171, 340), max_edit_percent=6):
    """(seqs, family per sequence): n sequences planted from unrelated random families, each at a random rotation, on a
    random strand, with 0 .. max_edit_percent % spaced edits"""
    import random
    rng = random.Random(seed)
    fam = [rnd(rng, m) for m in lens]
    seqs, label = [], []
    for _ in range(n):
        f = rng.randrange(len(fam))
        s = rotated(fam[f], rng.randrange(len(fam[f])), rng.randrange(2))
        seqs.append(edited(rng, s, rng.randrange(len(s) * max_edit_percent // 100 + 1)))
        label.append(f)
    return seqs, label, fam


def array_reads(seed=4, per_array=6, read_len=6000, periods=(171, 340)):
    """(names, reads, array per read): reads of two planted tandem arrays, copies 3 % apart, every read from a random phase,
    about half of them reverse-complemented.  The divergence is substitutions only, so that every read has the planted
    period exactly: with insertions and deletions among the copies a read's autocorrelation peaks one or two bases beside
    it (339 .. 342 for 340 at 0.5 % each, at 6 to 16 kb alike), and the tests of the command line ask for the period itself.
    Seeds with insertions and deletions are what families() is for."""
    from stringdecomposer_amd import synth
    names, reads, label = [], [], []
    for a, p in enumerate(periods):
        unit = synth._to_ascii(synth.Stream(seed, 7 + a).below(p, 4))
        _, rs = synth.make_reads([unit], per_array, read_len=read_len, seed=seed + a, psub=0.03, pins=0.0, pdel=0.0)
        for i, s in enumerate(rs):
            names.append("a%d_r%d" % (p, i))
            reads.append(s.decode())
            label.append(a)
    return names, reads, label


def same_partition(cluster, label):
    """is cluster the labelling under renaming"""
    return len(set(zip(cluster, label))) == len(set(cluster)) == len(set(label))


def canon(seq):
    """(record, rotation, strand): the smallest among all rotations of seq and of its reverse complement; the smallest
    rotation that gives it, strand 0 where both strands do"""
    best = None
    for strand, s in enumerate((seq, revcomp(seq))):
        for r in range(len(s)):
            rec = s[r:] + s[:r]
            if best is None or rec < best[0]:
                best = (rec, r, strand)
    return best
