"""The quantity of --heatmap stated in Python (include/sd_hip.h: sd_heat_segments): every segment of a group against
every earlier one (up to W rows back), each pair through lag_ref.pair and so through tests/edlib_ref.nw, the sums per
cell of the group's upper triangle of bins in Python integers, the closed forms of the layout, and the text of
<out>_heatmap.tsv for the rows of a final TSV."""
import lag_ref


def bins(n, B):
    return (n + B - 1) // B


def cell_index(nb, I, J):
    """cell (I, J), I <= J, of the row-major upper triangle of nb x nb bins"""
    assert 0 <= I <= J < nb
    return I * nb - I * (I - 1) // 2 + (J - I)


def pairs_of(n, W):
    """pairs (x, y), x < y, y - x <= W (W = 0: no limit) among n rows: counted, not from a formula"""
    return sum(min(y, W) if W > 0 else y for y in range(n))


def layout(group_off, B, W):
    """-> (cell_off, nb, cells, pairs) as Python lists / integers"""
    sizes = [b - a for a, b in zip(group_off, group_off[1:])]
    nb = [bins(n, B) for n in sizes]
    cell_off = [0]
    for k in nb:
        cell_off.append(cell_off[-1] + k * (k + 1) // 2)
    return cell_off, nb, cell_off[-1], sum(pairs_of(n, W) for n in sizes)


def segments(text, starts, ends, group_off, B, W=0, which=0):
    """-> sums [cells][3] as nested lists.  which = 1: only the pairs the kernel does not take (a target over 512 bp or a
    query over 1024 bp; the other reason, a pair edlib would split, needs longer rows than those limits allow)"""
    text = text.encode() if isinstance(text, str) else bytes(text)
    seg = [text[s:e + 1] if e >= s else b"" for s, e in zip(starts, ends)]
    cell_off, nb, cells, _ = layout(group_off, B, W)
    sums = [[0, 0, 0] for _ in range(cells)]
    todo = []
    for g in range(len(group_off) - 1):
        a, e = group_off[g], group_off[g + 1]
        for y in range(a, e):
            for x in range(a, y):
                if W > 0 and y - x > W:
                    continue
                q, t = seg[x], seg[y]
                if not q or not t:
                    continue
                if which == 1 and len(t) <= 512 and len(q) <= 1024:
                    continue
                todo.append((g, x - a, y - a, q, t))
    for g, x, y, q, t in todo:
        d, m = lag_ref.pair(q, t)
        assert d >= 0
        s = sums[cell_off[g] + cell_index(nb[g], x // B, y // B)]
        s[0] += 1
        s[1] += m
        s[2] += d + m
    return sums


def classes(text, starts, ends, group_off, W=0):
    """(kernel pairs, host pairs, pairs with an empty side) for a text in ACGTN"""
    ln = [max(0, e - s + 1) for s, e in zip(starts, ends)]
    dev = host = none = 0
    for g in range(len(group_off) - 1):
        a, e = group_off[g], group_off[g + 1]
        for y in range(a, e):
            for x in range(a, y):
                if W > 0 and y - x > W:
                    continue
                if ln[x] == 0 or ln[y] == 0:
                    none += 1
                elif ln[y] > 512 or ln[x] > 1024:
                    host += 1
                else:
                    dev += 1
    return dev, host, none


def pooled(n, m, c):
    return m / c * 100 if n > 0 else -1.0


def same(heat, ref):
    """a formats.Heat against segments()'s lists, exactly"""
    assert heat.sums.tolist() == ref


def text_of_final(final_rows, reads, B, W=0):
    """The text of <out>_heatmap.tsv for the rows of a final TSV (formats.read_final) and the reads by name: the fold
    above read by read, one line per cell with pairs, printed with '%.2f'."""
    groups = []
    for r in final_rows:
        if not groups or groups[-1][0] != r.read:
            groups.append((r.read, []))
        groups[-1][1].append(r)
    out = []
    for name, rows in groups:
        seq = reads[name]
        st = [min(max(r.start, 0), len(seq)) for r in rows]
        en = [min(max(r.end + 1, s), len(seq)) - 1 for r, s in zip(rows, st)]
        sums = segments(seq, st, en, [0, len(rows)], B, W)
        nb = bins(len(rows), B)
        for I in range(nb):
            for J in range(I, nb):
                n, m, c = sums[cell_index(nb, I, J)]
                if n == 0:
                    continue
                last = lambda k: rows[min((k + 1) * B, len(rows)) - 1]   # noqa: E731
                out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\n" % (name, I, J, rows[I * B].start, last(I).end, rows[J * B].start,
                                                                     last(J).end, n, pooled(n, m, c)))
    return "".join(out)
