"""The quantity of --lags stated in Python (include/sd_hip.h: sd_lag_segments): every segment against its next D
neighbours in the same group, each pair through tests/edlib_ref.nw (edlib's own path where python-edlib is installed, the
oracle's restatement otherwise), the sums per (group, lag) and the period rule in Python integers."""
import edlib_ref

_CACHE = {}


def pair(q, t):
    """(dist, matches) of query q against target t; (-1, 0) for an empty side"""
    k = (q, t)
    if k not in _CACHE:
        d, m, _ = edlib_ref.nw(q, t)
        _CACHE[k] = (d, m)
    return _CACHE[k]


def segments(text, starts, ends, group_off, D):
    """-> (dist, matches, sums) as nested lists: [n][D], [n][D], [groups][D][3]"""
    text = text.encode() if isinstance(text, str) else bytes(text)
    n = len(starts)
    seg = [text[s:e + 1] if e >= s else b"" for s, e in zip(starts, ends)]
    dist = [[-1] * D for _ in range(n)]
    matches = [[0] * D for _ in range(n)]
    sums = [[[0, 0, 0] for _ in range(D)] for _ in range(len(group_off) - 1)]
    for g in range(len(group_off) - 1):
        a, e = group_off[g], group_off[g + 1]
        for x in range(a, e):
            for d in range(1, D + 1):
                if x + d >= e:
                    break
                dd, mm = pair(seg[x], seg[x + d])
                dist[x][d - 1], matches[x][d - 1] = dd, mm
                if dd >= 0:
                    s = sums[g][d - 1]
                    s[0] += 1
                    s[1] += mm
                    s[2] += dd + mm
    return dist, matches, sums


def period(sums):
    """the lag (1-based) with the largest M / C among the lags with pairs, as a comparison of integers; ties to the
    smallest lag; 0 without pairs.  sums: [D][3]"""
    best = 0
    for d, (n, m, c) in enumerate(sums, 1):
        if n <= 0:
            continue
        if best == 0:
            best = d
            continue
        bm, bc = sums[best - 1][1], sums[best - 1][2]
        if m * bc > bm * c:
            best = d
    return best


def identity(d, m):
    return -1.0 if d < 0 else m / (d + m) * 100


def same(lags, ref):
    """a formats.Lags against segments()'s lists, exactly"""
    dist, matches, sums = ref
    assert lags.dist.tolist() == dist
    assert lags.matches.tolist() == matches
    assert lags.sums.tolist() == sums


def files_of_final(final_rows, reads, D):
    """The text of <out>_lags.tsv and <out>_period.tsv for the rows of a final TSV (formats.read_final) and the reads by
    name: the fold above, printed with '%.2f'."""
    groups = []
    for r in final_rows:
        if not groups or groups[-1][0] != r.read:
            groups.append((r.read, []))
        groups[-1][1].append(r)
    lag_text, per_text = [], []
    for name, rows in groups:
        seq = reads[name]
        st = [min(max(r.start, 0), len(seq)) for r in rows]
        en = [min(max(r.end + 1, s), len(seq)) - 1 for r, s in zip(rows, st)]
        dist, matches, sums = segments(seq, st, en, [0, len(rows)], D)
        for r, dd, mm in zip(rows, dist, matches):
            lag_text.append("%s\t%d\t%d\t%s\n" % (r.read, r.start, r.end, "\t".join("%.2f" % identity(d, m) for d, m in zip(dd, mm))))
        per_text.append("%s\t%d\t%d\t%s\n" % (name, len(rows), period(sums[0]),
                                             "\t".join("%.2f" % (m / c * 100 if n > 0 else -1.0) for n, m, c in sums[0])))
    return "".join(lag_text), "".join(per_text)
