"""Row sets for the tests of the device-final profiles (lib.final_profile_host / final_profile_device): segments cut from
one text as tests/test_gpu_profile.py cuts them, dealt to reads as rows in read coordinates with keep flags, and what
the existing host fold (lib.profile_segments(device=None)) makes of the kept ones."""
import random

import numpy as np

import profile_ref
from stringdecomposer_amd import lib


def segments(monos, n_seg, seed, max_extra=40, which=None):
    """(_segments of tests/test_gpu_profile.py; which: the monomer of every segment instead of a random one)
    Blocks of mutated monomer instances (either orientation) with flanks, cut from one text."""
    r = random.Random(seed)
    parts, st, en, pt, pos = [], [], [], [], 0
    for i in range(n_seg):
        m = r.randrange(len(monos)) if which is None else which[i]
        o = r.randrange(2)
        t = profile_ref.rc(monos[m]) if o else monos[m]
        s = list(t)
        for _ in range(len(s) // 12):
            k = r.randrange(len(s))
            x = r.random()
            if x < 0.4:
                s[k] = r.choice("ACGTN")
            elif x < 0.7:
                s[k] = ""
            else:
                s[k] = s[k] + "".join(r.choice("ACGT") for _ in range(r.randint(1, 6)))
        lead = "".join(r.choice("ACGT") for _ in range(r.randint(0, max_extra)))
        q = lead + "".join(s) + "".join(r.choice("ACGT") for _ in range(r.randint(0, max_extra)))
        parts.append(q)
        st.append(pos)
        en.append(pos + len(q) - 1)
        pt.append(2 * m + o)
        pos += len(q)
    return "".join(parts), st, en, pt


def as_rows(seq, st, en, pt, n_mono, cuts, keep, empty_read=None):
    """The segments as rows of reads: read k holds the segments [cuts[k], cuts[k + 1]); empty_read: the index at which a
    read without rows (40 bases of its own) is put in.  -> dict(text, read_off, rows, row_off, keep)."""
    text, read_off, rows, row_off = [], [0], [], [0]
    for k in range(len(cuts) - 1):
        if empty_read == k:
            text.append("ACGT" * 10)
            read_off.append(read_off[-1] + 40)
            row_off.append(row_off[-1])
        a, b = cuts[k], cuts[k + 1]
        lo = st[a] if a < b else 0
        hi = en[b - 1] + 1 if a < b else 0
        text.append(seq[lo:hi])
        for s in range(a, b):
            m, o = pt[s] >> 1, pt[s] & 1
            rows.append((m + o * n_mono, st[s] - lo, en[s] - lo, 0))
        read_off.append(read_off[-1] + hi - lo)
        row_off.append(len(rows))
    return dict(text="".join(text), read_off=np.array(read_off, dtype=np.int64),
                rows=np.array(rows, dtype=np.int32).reshape(-1, 4), row_off=np.array(row_off, dtype=np.int64),
                keep=np.array(keep, dtype=np.uint8))


def expected(case, monos, threads=8):
    """The host fold of the kept rows, their segments clamped here as Python's slicing clamps them.
    -> (counts, kept segments of 1 .. 1024 bases, kept segments longer than that)"""
    n_mono = len(monos)
    st, en, pt, short, long_ = [], [], [], 0, 0
    for r in range(len(case["read_off"]) - 1):
        r0, rl = int(case["read_off"][r]), int(case["read_off"][r + 1] - case["read_off"][r])
        for b in range(int(case["row_off"][r]), int(case["row_off"][r + 1])):
            if not case["keep"][b]:
                continue
            t, s, e, _ = (int(x) for x in case["rows"][b])
            s0 = min(max(s, 0), rl)
            e1 = min(max(e + 1, s0), rl)
            if e1 - s0 <= 0:
                continue
            st.append(r0 + s0)
            en.append(r0 + e1 - 1)
            pt.append(2 * t if t < n_mono else 2 * (t - n_mono) + 1)
            if e1 - s0 <= 1024:
                short += 1
            else:
                long_ += 1
    return lib.profile_segments(case["text"], st, en, monos, pt, threads=threads), short, long_


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape
        assert (x == y).all()
