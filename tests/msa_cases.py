"""Inputs shared by the --msa tests (CPU and GPU): mutated instances as tests/test_gpu_profile.py generates them, and
one hand-made set of the edges of a row."""
import random

import profile_ref


def segments(monos, n_seg, seed, max_extra=40, alphabet="ACGTN"):
    """Blocks of mutated monomer instances (either orientation) with flanks, cut from one text (the generator of
    test_gpu_profile._segments; substituted bases come from `alphabet`)."""
    r = random.Random(seed)
    parts, st, en, pt, pos = [], [], [], [], 0
    for _ in range(n_seg):
        m = r.randrange(len(monos))
        o = r.randrange(2)
        t = profile_ref.rc(monos[m]) if o else monos[m]
        s = list(t)
        for _ in range(max(1, len(s) // 12)):
            k = r.randrange(len(s))
            x = r.random()
            if x < 0.4:
                s[k] = r.choice(alphabet)
            elif x < 0.7:
                s[k] = ""
            else:
                s[k] = s[k] + "".join(r.choice("ACGT") for _ in range(r.randint(1, 6)))
        lead = "".join(r.choice("ACGT") for _ in range(r.randint(0, max_extra)))
        q = lead + "".join(s) + "".join(r.choice("ACGT") for _ in range(r.randint(0, max_extra)))
        if not q:
            q = r.choice("ACGT")
        parts.append(q)
        st.append(pos)
        en.append(pos + len(q) - 1)
        pt.append(2 * m + o)
        pos += len(q)
    return "".join(parts), st, en, pt


def random_monomer(length, seed):
    r = random.Random(seed)
    return "".join(r.choice("ACGT") for _ in range(length))


def edge_monomer():
    """171 bp whose ends and whose positions 79 / 80 make the hand-made edits below land in exactly one place: it
    begins AC, ends GT, and has C at 79 and G at 80."""
    m = list("AC" + random_monomer(167, 41) + "GT")
    m[79], m[80] = "C", "G"
    return "".join(m)


def edges(extra_byte=None):
    """(seq, starts, ends, pair_tmpl, monos, named): the pairs `named` = {what: index} are the edges the issue lists, each also
    against the reverse complement (what + "_rc").  extra_byte: a byte outside ACGTN put
    into one more pair (host form only)."""
    M = edge_monomer()
    monos = ["G", M, random_monomer(63, 1), random_monomer(64, 2), random_monomer(65, 3)]
    blocks, named = [], {}

    def add(what, q, il):
        named[what + ("_rc" if il & 1 else "")] = len(blocks)
        blocks.append((q, il))

    for o in (0, 1):
        t = profile_ref.rc(M) if o else M
        add("exact", t, 2 + o)
        add("ins_slot_0", ("T" if t[0] != "T" else "A") * 5 + t, 2 + o)       # before the first template base
        add("ins_slot_L", t + ("A" if t[-1] != "A" else "C") * 5, 2 + o)      # behind the last
        add("del_first", t[1:], 2 + o)
        add("del_last", t[:-1], 2 + o)
        add("ins_300", t[:80] + "A" * 300 + t[80:] if not o else t[:91] + "T" * 300 + t[91:], 2 + o)   # forward slot 80 either way
        add("one_base", t[40], 2 + o)
        add("with_N", t[:30] + "N" + t[31:100] + "NN" + t[102:], 2 + o)
    for m in (0, 2, 3, 4):
        for o in (0, 1):
            t = profile_ref.rc(monos[m]) if o else monos[m]
            add("len_%d" % len(monos[m]), t, 2 * m + o)
            add("len_%d_mut" % len(monos[m]), "C" + t[:len(t) // 2] + "A" + t[len(t) // 2 + 1:] + "T", 2 * m + o)
    if extra_byte is not None:
        add("other_byte", M[:50] + extra_byte + M[51:], 2)
    seq, st, en, pt, pos = [], [], [], [], 0
    for q, il in blocks:
        seq.append(q)
        st.append(pos)
        en.append(pos + len(q) - 1)
        pt.append(il)
        pos += len(q)
    named["empty"] = len(st)
    st.append(5)
    en.append(4)
    pt.append(3)
    return "".join(seq), st, en, pt, monos, named
