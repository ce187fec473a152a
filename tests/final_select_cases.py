"""Word sets for the final selection (sd_final_select_host / sd_final_select_dev) and an independent restatement, in plain
Python, of what the reference command line does with a decomposed read (its main.py: convert_read, classify, print_read)
once every identity is known -- here from (dist << 16) | matches words instead of alignments.

The words are drawn from a few (dist, matches) pairs, some of them different pairs of the same ratio, so that tied
maxima are the rule: among the keys (second best) and among the homopolymer ranks.  Rows with the identity exactly at
the threshold and just below it, rows no word decides (a 0 word, a 0xffffffff word, a segment long enough for edlib's
Hirschberg split) and reads without rows are part of every set."""
import random

import numpy as np

NONE = 0xFFFFFFFF
COEF = [-31.48494996, 0.41784018, 0.69186882]
# (dist, matches): 95 % three ways, 94 % and 96 % two ways each, 94.9 %, and a low one that a good second best turns '?'
PAIRS = [(5, 95), (10, 190), (1, 19), (6, 94), (12, 188), (51, 949), (4, 96), (8, 192), (30, 70)]
SPLIT_LEN, NO_SPLIT_LEN = 21000, 19000   # against a 171-bp monomer edlib splits the first and not the second


def monomers(n, seed=1):
    """n monomers of 171 bp; from three on, monomer 1 carries the name of the LAST one (one key, n_keys < T)."""
    rng = random.Random(seed)
    names = ["M%d" % i for i in range(n)]
    if n >= 3:
        names[1] = names[n - 1]
    return names, ["".join(rng.choice("ACGT") for _ in range(171)) for _ in range(n)]


def word(d, m):
    return (d << 16) | m


def make(n_mono, second_best, n_rows=2000, seed=3, empty_read=True, no_reads=False):
    """-> dict(rows [n, 4] int32, row_off, widx, words, hwords, read_len, names, seqs, second_best)."""
    rng = random.Random(seed * 1000 + n_mono + (500 if second_best else 0))
    names, seqs = monomers(n_mono)
    T = 2 * n_mono
    per = T if second_best else 1
    if no_reads:
        n_rows = 0
    counts = []
    left = n_rows
    while left > 0:
        c = min(left, rng.choice([1, 7, 300, 900]))
        counts.append(c)
        left -= c
    if len(counts) > 1 and counts[-1] < 2:   # (the two long segments below share the last read)
        counts[-2] += counts.pop()
    if empty_read and counts:
        counts.insert(len(counts) // 2, 0)
        counts.append(0)
    rows, read_len = [], []
    for c in counts:
        pos = rng.randrange(0, 50)
        for _ in range(c):
            ln = rng.randrange(150, 190)
            rows.append([rng.randrange(T), pos, pos + ln - 1, rng.randrange(100, 170)])
            pos += ln
        read_len.append(pos + rng.randrange(0, 30))
    rows = np.array(rows, dtype=np.int32).reshape(-1, 4)
    row_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_words = n_rows + 5
    order = list(range(n_words))
    rng.shuffle(order)
    widx = np.array(order[:n_rows], dtype=np.int64)   # a row's words lie somewhere else than at the row's index
    pick = lambda: word(*rng.choice(PAIRS))   # noqa: E731
    words = np.array([[pick() for _ in range(per)] for _ in range(n_words)], dtype=np.uint32).reshape(n_words, per)
    hwords = np.array([[pick() for _ in range(per)] for _ in range(n_words)], dtype=np.uint32).reshape(n_words, per)
    if n_rows >= 40:
        # the corners, at fixed rows of the first reads
        def own_col(b):   # the word that decides row b's identity
            if not second_best:
                return 0
            t = int(rows[b, 0])
            name = names[t] if t < n_mono else names[t - n_mono] + "'"
            il = [x for n in names for x in (n, n + "'")]
            return max(i for i, x in enumerate(il) if x == name)
        for b, (d, m) in ((3, (5, 95)), (4, (6, 94)), (5, (51, 949)), (6, (10, 190))):
            words[widx[b], own_col(b)] = word(d, m)
        words[widx[10], rng.randrange(per)] = 0
        words[widx[11], rng.randrange(per)] = NONE
        (hwords if second_best else words)[widx[12], rng.randrange(per)] = 0
        (hwords if second_best else words)[widx[13], rng.randrange(per)] = NONE
        # two long segments at the end of the last read that has rows
        last = max(r for r, c in enumerate(counts) if c)
        b1 = int(row_off[last + 1]) - 1
        s = int(rows[b1 - 1, 1])
        rows[b1 - 1, 2] = s + NO_SPLIT_LEN - 1
        rows[b1, 1] = s + NO_SPLIT_LEN
        rows[b1, 2] = s + NO_SPLIT_LEN + SPLIT_LEN - 1
        read_len[last] = int(rows[b1, 2]) + 1
    return dict(rows=rows, row_off=row_off, widx=widx, words=words, hwords=hwords if second_best else None,
                read_len=np.array(read_len, dtype=np.int64), names=names, seqs=seqs, second_best=second_best)


def ident(w):
    d, m = w >> 16, w & 0xFFFF
    a = 0.0
    a += m
    a /= (d + m)
    return a * 100


def splits(qlen, tlen):
    return 20 * ((qlen + 63) // 64) * tlen + 8 * tlen >= 1024 * 1024


def select(case, min_identity, coef=COEF):
    """-> (rows: list of tuples in final_dtype() field order, row_off, alt: list of lists or None, n_undecided, ties)
    where ties = (rows with a tied maximum among the other keys, rows with a tied homopolymer rank 0 or 1)."""
    names, sb = case["names"], case["second_best"]
    M = len(names)
    il = [x for n in names for x in (n, n + "'")]
    keys = list(dict.fromkeys(il))
    tmax = max(len(s) for s in case["seqs"])
    out, alt, off, und, tie_k, tie_h = [], ([] if sb else None), [0], 0, 0, 0
    for r in range(len(case["row_off"]) - 1):
        for b in range(int(case["row_off"][r]), int(case["row_off"][r + 1])):
            t, start, end, _ = (int(x) for x in case["rows"][b])
            w = [int(x) for x in case["words"][case["widx"][b]]]
            h = [int(x) for x in case["hwords"][case["widx"][b]]] if sb else []
            seg = len(range(int(case["read_len"][r]))[start:end + 1])
            if any(x in (0, NONE) for x in w + h) or splits(seg, tmax):
                und += 1
                continue
            monomer = names[t] if t < M else names[t - M] + "'"
            if not sb:
                score, second, s2, hb, hbs, hs, hss, scores = ident(w[0]), None, -1, None, -1, None, -1, {}
            else:
                scores = {}
                for i, m in enumerate(il):
                    scores[m] = ident(w[i])
                second, s2 = None, -1
                for m in scores:
                    if m != monomer:
                        if not second or s2 < scores[m]:
                            second, s2 = m, scores[m]
                homo = sorted([[m, ident(h[i])] for i, m in enumerate(il)], key=lambda x: -x[1])
                (hb, hbs), (hs, hss) = homo[0], homo[1]
                score = scores[monomer]
                others = [scores[m] for m in scores if m != monomer]
                tie_k += len(others) > 1 and others.count(max(others)) > 1
                hv = [x[1] for x in homo]
                tie_h += hv.count(hv[0]) > 1 or hv.count(hv[1]) > 1
            if not score >= min_identity:
                continue
            logit = (1.0 * coef[0] + score * coef[1]) + (score - s2) * coef[2]
            k = lambda n: -1 if n is None else keys.index(n)   # noqa: E731
            out.append((r, start, end, k(monomer), k(second), k(hb), k(hs), score, s2, hbs, hss, 1 if logit > 0 else 0))
            if sb:
                alt.append([scores[x] for x in keys])
        off.append(len(out))
    return out, off, alt, und, (tie_k, tie_h)
