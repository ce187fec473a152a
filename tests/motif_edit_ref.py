"""The rule of --motif-edits written naively from its text (include/sd_hip.h, "IUPAC motif hits with insertions and
deletions"): the full Sellers table row by row, the hit test on its bottom row, and a second full table anchored at the end
for the start.  No bit vectors, no warm-up, no stretches.  The tests of --motif-edits compare the library against it."""
from motif_ref import revcomp_sets, sets


def matches(s, byte):
    """does the code (a set of bases, None for N) match the text byte"""
    return s is None or chr(byte) in s


def bottom_row(text, ps):
    """d(0 .. n): d[j] = the smallest edit distance of the pattern to any substring of text that ends just before j"""
    L, n = len(ps), len(text)
    col = list(range(L + 1))            # column j = 0: D[i][0] = i
    d = [L]
    for j in range(1, n + 1):
        new = [0] * (L + 1)             # D[0][j] = 0: a match may start anywhere
        for i in range(1, L + 1):
            new[i] = min(col[i - 1] + (0 if matches(ps[i - 1], text[j - 1]) else 1),   # substitution or match
                         new[i - 1] + 1,                                                # a deleted pattern code
                         col[i] + 1)                                                    # an inserted text byte
        col = new
        d.append(col[L])
    return d


def anchored_start(text, ps, j, d):
    """the largest s with ed(pattern, text[s .. j)) = d: global edit distance, suffix table from (L, j) backwards"""
    L = len(ps)
    lo = max(0, j - L - d)
    # G[i][t] = ed(pattern[i:], text[t:j]) for lo <= t <= j
    w = j - lo
    G = [[0] * (w + 1) for _ in range(L + 1)]
    for i in range(L, -1, -1):
        for t in range(w, -1, -1):
            if i == L and t == w:
                G[i][t] = 0
            elif i == L:
                G[i][t] = w - t
            elif t == w:
                G[i][t] = L - i
            else:
                G[i][t] = min(G[i + 1][t + 1] + (0 if matches(ps[i], text[lo + t]) else 1), G[i + 1][t] + 1, G[i][t + 1] + 1)
    for t in range(w, -1, -1):          # s = lo + t, largest first
        if G[0][t] == d:
            return lo + t
    raise AssertionError("no substring ending at %d has distance %d" % (j, d))


def scan_sets(text, ps, K):
    """[(start, length, edits)] of the pattern (as sets) against text (bytes), ends ascending"""
    n = len(text)
    d = bottom_row(text, ps)
    out = []
    for j in range(1, n + 1):
        nxt = d[j + 1] if j + 1 <= n else float("inf")
        if d[j] <= K and d[j] <= nxt and (d[j] < d[j - 1] or d[j] == 0):
            s = anchored_start(text, ps, j, d[j])
            out.append((s, j - s, d[j]))
    return out


def scan(reads, patterns, K):
    """hits in canonical order -- (read, motif, strand, start, length, edits) -- and per[read][motif][strand]"""
    hits, per = [], []
    for r, text in enumerate(reads):
        text = text.encode() if isinstance(text, str) else bytes(text)
        per.append([])
        for m, p in enumerate(patterns):
            fw = sets(p)
            rc = revcomp_sets(fw)
            per[r].append([0, 0])
            for strand, ps in ((0, fw), (1, rc)):
                if strand == 1 and rc == fw:   # a palindrome: + only
                    continue
                found = scan_sets(text, ps, K)
                per[r][m][strand] = len(found)
                hits += [(r, m, strand, s, ln, e) for s, ln, e in found]
    return hits, per


def as_tuples(h):
    """a lib edit-hit array -> the tuples of scan()"""
    return [(int(x["read"]), int(x["motif"]), int(x["strand_edits"]) >> 7, int(x["start"]), int(x["length"]), int(x["strand_edits"]) & 127)
            for x in h]
