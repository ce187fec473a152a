"""Inputs of the lenient-mode tests, built from the committed goldens with a fixed seed (no fixtures of their own).

disguise(): what a soft-masked, IUPAC-coded file that went through another operating system looks like -- each base
lower-cased with probability 1/2, each N replaced by a random member of RYSWKMBDHVNryswkmbdhvn, lines wrapped at 60
columns, CRLF line ends.  A lenient job on it must give the bytes the unmodified reference gave on the canonical file.
fastq(): the same records as four-line FASTQ, the quality lines beginning with '@', '>' and '+' in turn."""
import random

AMBIGUITY = b"RYSWKMBDHV"
N_DISGUISES = b"RYSWKMBDHVNryswkmbdhvn"


def rule(data):
    """The normalisation rule, restated: -> (bytes, [lower folded, codes -> N, still outside ACGTN, examined])."""
    out, st = bytearray(), [0, 0, 0, len(data)]
    for c in bytes(data):
        if 0x61 <= c <= 0x7A:
            c -= 32
            st[0] += 1
        if c in AMBIGUITY:
            c = 0x4E
            st[1] += 1
        if c not in b"ACGTN":
            st[2] += 1
        out.append(c)
    return bytes(out), st


def read_records(path):
    """[(header line without '>', sequence bytes)] of a canonical FASTA file."""
    recs = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            if line.startswith(b">"):
                recs.append([line[1:], bytearray()])
            elif recs:
                recs[-1][1] += line
    return [(h, bytes(s)) for h, s in recs]


def disguise_seq(seq, rng):
    out = bytearray()
    for c in seq:
        if c == 0x4E:
            c = N_DISGUISES[rng.randrange(len(N_DISGUISES))]
        elif rng.random() < 0.5:
            c = c + 32
        out.append(c)
    return bytes(out)


def disguise(recs, seed=1, lower_only=False):
    rng = random.Random(seed)
    out = bytearray()
    for h, s in recs:
        s = s.lower() if lower_only else disguise_seq(s, rng)
        out += b">" + h + b"\r\n"
        for i in range(0, len(s), 60):
            out += s[i:i + 60] + b"\r\n"
    return bytes(out)


def fastq(recs, seed=None):
    """Four-line FASTQ; seed given: the sequences disguised and CRLF line ends (never wrapped: that is multi-line FASTQ)."""
    rng = random.Random(seed)
    nl = b"\n" if seed is None else b"\r\n"
    out = bytearray()
    for i, (h, s) in enumerate(recs):
        if seed is not None:
            s = disguise_seq(s, rng)
        q = (b"@>+I"[i % 4:i % 4 + 1] + b"@>+5I"[(i // 4) % 5:(i // 4) % 5 + 1] * len(s))[:len(s)]
        out += b"@" + h + nl + s + nl + b"+" + (h.split()[0] if i % 2 else b"") + nl + q + nl
    return bytes(out)


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)
