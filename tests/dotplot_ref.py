"""The windowed k-mer identity of a read against itself (--dotplot) restated with Python sets and integers, for the tests:
nothing here shares code with the library.  include/sd_hip.h (sd_dotplot_*) holds the definition."""
import numpy as np

MASK = (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def h(x):
    """the splitmix64 finaliser"""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def codes(kmer):
    """(forward, reverse) codes of a k-mer of A C G T, None when it holds another byte"""
    if any(c not in CODE for c in kmer):
        return None
    f = r = 0
    for c in kmer:
        f = f * 4 + CODE[c]
    for c in reversed(kmer):
        r = r * 4 + 3 - CODE[c]
    return f, r


def n_windows(n, W):
    return -(-n // W)


def window_sets(s, k, W, M):
    """[(S_w, R_w, selected forward positions, selected reverse positions)] of a read"""
    out = []
    for w in range(n_windows(len(s), W)):
        S, R, nf, nr = set(), set(), 0, 0
        for i in range(w * W, min(len(s), (w + 1) * W)):
            if i + k > len(s):
                break
            fr = codes(s[i:i + k])
            if fr is None:
                continue
            if h(fr[0]) % M == 0:
                S.add(fr[0])
                nf += 1
            if h(fr[1]) % M == 0:
                R.add(fr[1])
                nr += 1
        out.append((S, R, nf, nr))
    return out


def row_first(i, B):
    return max(0, i - B) if B > 0 else 0


def layout(lens, W, B):
    win_off, cell_off = [0], [0]
    for n in lens:
        nw = n_windows(n, W)
        win_off.append(win_off[-1] + nw)
        cell_off.append(cell_off[-1] + sum(i - row_first(i, B) + 1 for i in range(nw)))
    return win_off, cell_off


def dotplot(reads, k, W, B=0, M=1, keep=None):
    """-> kmers, kmers_rc, shared, shared_rc (int64 arrays), win_off, cell_off.  keep(r, i, j): compute the cell (others
    hold -1), None = all"""
    win_off, cell_off = layout([len(s) for s in reads], W, B)
    kmers, kmers_rc, shared, shared_rc = [], [], [], []
    for r, s in enumerate(reads):
        sets = window_sets(s, k, W, M)
        kmers += [len(x[0]) for x in sets]
        kmers_rc += [len(x[1]) for x in sets]
        for i in range(len(sets)):
            for j in range(row_first(i, B), i + 1):
                if keep is None or keep(r, i, j):
                    shared.append(len(sets[i][0] & sets[j][0]))
                    shared_rc.append(len(sets[i][0] & sets[j][1]))
                else:
                    shared.append(-1)
                    shared_rc.append(-1)
    a = lambda x: np.array(x, dtype=np.int64)
    return a(kmers), a(kmers_rc), a(shared), a(shared_rc), win_off, cell_off


def identity(shared, a, b, k):
    """the float the text prints with %.2f"""
    return 100.0 * (shared / min(a, b)) ** (1.0 / k) if shared else 0.0


def revcomp(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(s))
