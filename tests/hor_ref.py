"""The rule of --hor restated with Python dicts and lists, from its text alone (it shares no code with the library).

Rows of the final TSV in file order: read, start, end, key (2 m + s, -1 none), usable.  A row counts when it is usable and
has a key.  Two consecutive rows are adjacent when they have one read and one strand, both count, and 0 <= the bases
between them <= G.  An adjacent pair is a step from the earlier monomer to the later one on the forward strand and the
other way round on the reverse strand; T counts the steps.  succ / pred are the best successor and predecessor (most
steps, then smallest index) where that is at least C steps; an edge is kept when it is both.  Components with an edge are
the orders (cycles from their smallest monomer, paths from their head), numbered by their smallest monomer, unless longer
than 64.  A unit is a longest run of rows whose consecutive pairs are adjacent, on one order, and move forward along it
(backward on the reverse strand)."""
PMAX = 64


def analyse(read, start, end, key, usable, M, G=0, C=2):
    n = len(read)
    counts = [usable[i] and key[i] >= 0 for i in range(n)]
    mono = [key[i] // 2 if counts[i] else None for i in range(n)]
    strand = [key[i] % 2 if counts[i] else None for i in range(n)]

    def adjacent(i):   # rows i, i + 1
        return (i + 1 < n and counts[i] and counts[i + 1] and read[i] == read[i + 1] and strand[i] == strand[i + 1]
                and 0 <= start[i + 1] - end[i] - 1 <= G)

    steps, rows = {}, [0] * M
    for i in range(n):
        if counts[i]:
            rows[mono[i]] += 1
        if adjacent(i):
            e = (mono[i], mono[i + 1]) if strand[i] == 0 else (mono[i + 1], mono[i])
            steps[e] = steps.get(e, 0) + 1
    T = [[steps.get((a, b), 0) for b in range(M)] for a in range(M)]

    succ, pred = {}, {}
    for a in range(M):
        best = max(range(M), key=lambda b: (T[a][b], -b))
        if T[a][best] >= C:
            succ[a] = best
        best = max(range(M), key=lambda b: (T[b][a], -b))
        if T[best][a] >= C:
            pred[a] = best
    nxt = {a: b for a, b in succ.items() if pred.get(b) == a}
    prv = {b: a for a, b in nxt.items()}

    hor, pos, kinds, lens, long_ = [-1] * M, [0] * M, [], [], []
    done = set()
    for m in range(M):
        if m in done or (m not in nxt and m not in prv):
            continue
        walk, x = [m], nxt.get(m)   # forwards from m
        while x is not None and x != m:
            walk.append(x)
            x = nxt.get(x)
        cycle = x == m
        if not cycle:               # and backwards to the head
            x = prv.get(m)
            while x is not None:
                walk.insert(0, x)
                x = prv.get(x)
        done.update(walk)
        if len(walk) > PMAX:
            long_.append((walk[0], len(walk)))
            continue
        for i, x in enumerate(walk):
            hor[x], pos[x] = len(kinds), i + 1
        kinds.append(0 if cycle else 1)
        lens.append(len(walk))

    on = [counts[i] and hor[mono[i]] >= 0 for i in range(n)]
    row_unit, units = [-1] * n, []
    i = 0
    while i < n:
        if not on[i]:
            i += 1
            continue
        j = i
        while (adjacent(j) and on[j + 1] and hor[mono[j + 1]] == hor[mono[i]]
               and (pos[mono[j + 1]] > pos[mono[j]] if strand[i] == 0 else pos[mono[j + 1]] < pos[mono[j]])):
            j += 1
        mask = 0
        for x in range(i, j + 1):
            mask |= 1 << (pos[mono[x]] - 1)
            row_unit[x] = len(units)
        units.append((i, start[i], end[j], mask, read[i], j - i + 1, hor[mono[i]], strand[i]))
        i = j + 1
    return {"T": T, "rows": rows, "hor": hor, "pos": pos, "kinds": kinds, "lens": lens, "long": long_, "row_unit": row_unit,
            "units": units}


def name(mask):
    present = [p for p in range(1, 65) if mask >> (p - 1) & 1]
    runs = []
    for p in present:
        if runs and runs[-1][1] == p - 1:
            runs[-1][1] = p
        else:
            runs.append([p, p])
    return "_".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in runs)


def variants(units):
    """[(order, mask, units, rows, bases)] sorted by order, units descending, mask ascending"""
    acc = {}
    for first, s, e, mask, read, rows, order, strand in units:
        a = acc.setdefault((order, mask), [0, 0, 0])
        a[0] += 1
        a[1] += rows
        a[2] += e - s + 1
    return sorted(((o, m) + tuple(v) for (o, m), v in acc.items()), key=lambda t: (t[0], -t[2], t[1]))
