"""A naive scan for IUPAC motif hits, written from the definition (include/sd_hip.h, "IUPAC motif hits"): byte by byte, no
bit planes and no word step.  The tests of --motif compare the library against it."""
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def sets(pattern):
    """the pattern as a list of sets of bases; None for N (unconstrained)"""
    return [None if c == "N" else frozenset(IUPAC[c]) for c in pattern.upper()]


def revcomp_sets(ps):
    return [None if s is None else frozenset(COMP[b] for b in s) for s in reversed(ps)]


def scan_sets(text, ps, E):
    """[(start, mismatches)] of the pattern (as sets) against text (bytes), at most E mismatches"""
    L, out = len(ps), []
    con = [(j, frozenset(ord(b) for b in s)) for j, s in enumerate(ps) if s is not None]
    for i in range(len(text) - L + 1):
        mm = 0
        for j, s in con:
            if text[i + j] not in s:   # (a byte outside upper-case ACGT is in no set)
                mm += 1
                if mm > E:
                    break
        if mm <= E:
            out.append((i, mm))
    return out


def scan(reads, patterns, E):
    """hits in canonical order -- (read, motif, strand, start, mismatches) -- and per[read][motif][strand]"""
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
                found = scan_sets(text, ps, E)
                per[r][m][strand] = len(found)
                hits += [(r, m, strand, i, mm) for i, mm in found]
    return hits, per


def as_tuples(h):
    """a lib hit array -> the tuples of scan()"""
    return [(int(x["read"]), int(x["motif"]), int(x["strand"]), int(x["start"]), int(x["mismatches"])) for x in h]
