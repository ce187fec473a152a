"""Record lists for the piecewise seam merge (test_device_rows_cpu.py, test_gpu_device_rows.py): seeded random lists
whose records are 1-30 long and step back by up to 40 about a third of the time, and hand-made lists that put a jump of
the merge at every place a piece boundary (pieces of 8) could break it.  The expected rows come from lib.seam_merge, the
literal host merge."""
import random

import numpy as np

from stringdecomposer_amd import lib

LENGTHS = [0, 1, 2, 6, 7, 8, 9, 15, 16, 17, 23, 24, 25, 40, 64, 65, 100]
PER_LENGTH = 180          # 17 x 180 = 3060 lists
PIECES = [8, 9, 16, 64]


def random_list(rng, n):
    out, pos = [], 0
    for _ in range(n):
        ln = rng.randint(1, 30)
        if rng.random() < 0.35:
            pos = max(0, pos - rng.randint(0, 40))
        out.append((rng.randint(0, 23), pos, pos + ln - 1, rng.randint(-40, 300)))
        pos += ln
    return out


def _plain(n):
    """n records that never overlap: the merge keeps them all, one step at a time."""
    return [(k % 24, 100 * k, 100 * k + 49, 10 + k) for k in range(n)]


def handmade():
    """name -> list.  Record k of a plain list is (100k, 100k + 49); `cover(i, j)` makes b[i] cover more than half of
    b[j] and nothing between them, so the scan at i keeps b[i], drops b[i+1 .. j], keeps b[j+1] unchecked and goes on at
    j + 2."""
    out = {}

    def cover(lst, i, j):
        t, s, e, sc = lst[i]
        if j == i + 1:
            lst[i] = (t, s, s + 130, sc)           # reaches 30 into b[i+1]
        else:
            tj, _, _, scj = lst[j]
            lst[j] = (tj, s + 20, s + 60, scj)     # b[j] steps back into b[i]

    a = _plain(3)
    cover(a, 0, 2)                                  # j + 1 == N: nothing behind the dropped run
    out["jump_to_end"] = a
    a = _plain(9)
    cover(a, 2, 8)                                  # the same with j the last record of a second piece
    out["jump_to_end_two_pieces"] = a
    a = _plain(12)
    cover(a, 6, 7)                                  # kept b[8] is the first record of the next piece ...
    cover(a, 8, 9)                                  # ... and is not compared with b[9]: a scan from 8 would drop b[9]
    out["kept_unchecked_first_of_piece"] = a
    a = _plain(20)
    cover(a, 5, 6)                                  # goes on at 8: exactly the boundary
    out["lands_on_boundary"] = a
    a = _plain(20)
    cover(a, 7, 13)                                 # goes on at 15: boundary + 7
    out["lands_on_boundary_plus_7"] = a
    a = _plain(40)
    cover(a, 7, 13)
    cover(a, 15, 16)                                # entry 7 of piece 1, whose first step jumps again
    cover(a, 23, 29)                                # and from there to 31 = 24 + 7
    out["chained_jumps"] = a
    return out


def all_lists(seed=20240917):
    rng = random.Random(seed)
    lists = [random_list(rng, n) for n in LENGTHS for _ in range(PER_LENGTH)]
    hm = handmade()
    return lists + [hm[k] for k in sorted(hm)]


def pack(lists):
    """-> (recs [n, 4] int32, read_off int64)"""
    flat = [r for lst in lists for r in lst]
    recs = np.array(flat, dtype=np.int32).reshape(-1, 4)
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(lst) for lst in lists], out=off[1:])
    return recs, off


def expected(lists):
    return [lib.seam_merge(lst) for lst in lists]


def rows_of(rows, row_off, r):
    return [tuple(int(v) for v in x) for x in rows[int(row_off[r]):int(row_off[r + 1])]]
