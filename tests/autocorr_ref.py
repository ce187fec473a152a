"""The k-mer autocorrelation of --autocorr in plain numpy, written from the definition and not from the library: two
positions match when they hold the same byte and that byte is one of A C G T; position i is a hit at lag d when
0 <= i <= n - d - k and T[i + j] matches T[i + d + j] for j = 0 .. k - 1; A[w, d] counts the hits whose i lies in window
w = [w W, min(n, (w + 1) W)), W = 0 meaning one window.  Also the peak rule, the seed rule and the text of the two files."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bytes(seq):
    return np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)


def n_windows(n, W):
    return 1 if W <= 0 else max(1, -(-n // W))


def window(n, w, W):
    return (0, n) if W <= 0 else (w * W, min(n, (w + 1) * W))


def hits(seq, k, d):
    """bool [max(0, n - d - k + 1)]: position i is a hit at lag d"""
    t = _bytes(seq)
    n = len(t)
    m = n - d - k + 1
    if m <= 0:
        return np.zeros(0, dtype=bool)
    eq = (t[:n - d] == t[d:]) & np.isin(t[:n - d], ACGT)          # the equality mask of lag d
    run = np.concatenate(([0], np.cumsum(eq.astype(np.int64))))   # k-runs by a cumulative sum
    return (run[k:k + m] - run[:m]) == k


def spectrum(seq, k, D, W=0, lags=None):
    """int64 [windows, D] of one read; lags: compute only these (the others stay -1), to thin a large case"""
    n = len(seq)
    nw = n_windows(n, W)
    out = np.zeros((nw, D), dtype=np.int64)
    if lags is not None:
        out[:] = -1
    for d in (range(1, D + 1) if lags is None else lags):
        h = hits(seq, k, d)
        for w in range(nw):
            a, b = window(n, w, W)
            out[w, d - 1] = int(h[a:b].sum())
    return out


def spectra(reads, k, D, W=0, lags=None):
    """(counts [windows, D], win_off) of several reads"""
    parts = [spectrum(s, k, D, W, lags) for s in reads]
    off = np.concatenate(([0], np.cumsum([p.shape[0] for p in parts]))).astype(np.int64)
    return (np.concatenate(parts, axis=0) if parts else np.zeros((0, D), dtype=np.int64)), off


def positions(n, k, D, W=0):
    """brute force: the i of each window with i <= n - d - k"""
    nw = n_windows(n, W)
    out = np.zeros((nw, D), dtype=np.int64)
    for w in range(nw):
        a, b = window(n, w, W)
        for d in range(1, D + 1):
            out[w, d - 1] = sum(1 for i in range(a, b) if i <= n - d - k)
    return out


def peaks(A, LO, R, P):
    """A[d - 1] = the count of lag d -> [(lag, count)], at most P: d >= LO is a peak when A[d] > 0, no A[e] with e in
    [max(LO, d - R), min(D, d + R)] is larger and none with e < d is equal; by count descending, then lag ascending"""
    D = len(A)
    found = []
    for d in range(max(LO, 1), D + 1):
        c = int(A[d - 1])
        if c <= 0:
            continue
        es = range(max(LO, d - R), min(D, d + R) + 1)
        if all(c >= int(A[e - 1]) for e in es) and all(c > int(A[e - 1]) for e in es if e < d):
            found.append((d, c))
    found.sort(key=lambda x: (-x[1], x[0]))
    return found[:P]


def period(A, LO, R):
    p = peaks(A, LO, R, 1)
    return p[0] if p else (0, 0)


def seed(seq, k, p):
    """(s, run) of the longest run of consecutive hits at lag p, the first of equal runs; (-1, 0) without a hit"""
    best, s, cur = 0, -1, 0
    for i, h in enumerate(hits(seq, k, p).tolist()):
        cur = cur + 1 if h else 0
        if cur > best:
            best, s = cur, i - cur + 1
    return s, best


def seeds(reads, names, k, D, LO, R, min_count, whole=None):
    """whole: the reads' W = 0 spectra, where the caller has them already"""
    out = []
    for r, (seq, name) in enumerate(zip(reads, names)):
        A = spectrum(seq, k, D, 0)[0] if whole is None else whole[r]
        p, c = period(A, LO, R)
        if p <= 0 or c < min_count:
            continue
        s, _ = seed(seq, k, p)
        text = seq[s:s + p]
        text = text.decode() if isinstance(text, bytes) else text
        if len(text) != p or set(text) - set("ACGT"):
            continue
        out.append(("%s/%d_%d period=%d count=%d" % (name, s, s + p, p, c), text))
    return out


def summary_text(reads, names, k, D, W, LO, P, R, spectra=None):
    """the text of <out>_autocorr.tsv; spectra: the reads' spectrum(seq, k, D, W), where the caller has them already"""
    out = []
    for r, (seq, name) in enumerate(zip(reads, names)):
        n = len(seq)
        A = spectrum(seq, k, D, W) if spectra is None else spectra[r]
        for w in range(A.shape[0]):
            a, b = window(n, w, W)
            pk = peaks(A[w], LO, R, P)
            p, c = pk[0] if pk else (0, 0)
            pos = sum(1 for i in range(a, b) if i <= n - p - k) if p > 0 else 0
            out.append("\t".join([name] + [str(x) for x in (a, b, k, p, c, pos)] + ["%d:%d" % x for x in pk]) + "\n")
    return "".join(out)


def spectrum_text(reads, names, k, D, W, spectra=None):
    """the text of <out>_autocorr_spectrum.tsv"""
    out = []
    for r, (seq, name) in enumerate(zip(reads, names)):
        n = len(seq)
        A = spectrum(seq, k, D, W) if spectra is None else spectra[r]
        for w in range(A.shape[0]):
            a, b = window(n, w, W)
            for d in range(1, D + 1):
                if A[w, d - 1] > 0:
                    out.append("%s\t%d\t%d\t%d\t%d\t%d\n" % (name, a, b, d, A[w, d - 1], max(0, min(b, n - d - k + 1) - a)))
    return "".join(out)
