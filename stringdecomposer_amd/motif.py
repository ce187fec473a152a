"""--motif: the hits of IUPAC motifs -- the CENP-B box, telomeric repeats, any protein-binding site of up to 64 codes -- on
both strands of every read of the reads file, found on the device.  main.py runs the pass beside a decomposition
(stringdecomposer reads.fa monomers.fa --motif cenpb) and joins the hits with the rows of the final TSV on the host;
bin/sd-motif runs the scan alone (sd-motif reads.fa -o OUT --motif cenpb).

By default matches are Hamming matches: up to --motif-mismatches mismatches at the constrained positions, no insertions or
deletions.  --motif-edits K finds a box that a noisy read holds with an indel: up to K substitutions, inserted bases and
deleted codes (lib.motif_edits; csrc/sd_motif_edit.hpp holds the rule), written to the same three files with each hit's own
end and its edits in the sixth column.

The reads go to lib.motif in batches of whole reads, at most BATCH_BASES bases of text and lib.MOTIF_ITEMS_MAX (tile,
pattern-strand) items each, but at least one read; a request of so many motifs that one read exceeds the item cap goes in
blocks of motifs.  The hits of a batch are known only when the library has counted them: a batch it refuses for more than
lib.MOTIF_HITS_MAX hits is cut in two and tried again (scan_part)."""
import argparse
import os
import re
import sys

from . import formats, lib, shard

BATCH_BASES = 1 << 28
NAME = re.compile(r"[A-Za-z0-9_.-]+\Z")


def add_arguments(parser):
    parser.add_argument("--motif", action="append", default=None, metavar="SPEC",
                        help="also write <out-file>_motif.tsv: the hits of a motif on both strands of every read -- read, "
                             "start, end, strand, motif, mismatches, sequence.  SPEC is a built-in name (%s) or NAME=PATTERN, "
                             "PATTERN of 1 .. %d IUPAC codes (N matches anything); repeatable.  Beside a decomposition also "
                             "<out-file>_motif_rows.tsv (per row of <out-file>.tsv the motifs with a hit inside it) and "
                             "<out-file>_motif_monomers.tsv (per monomer and motif: rows, rows with a hit, hits).  Hamming "
                             "matches unless --motif-edits is given" % (", ".join(sorted(lib.MOTIF_BUILTIN)), lib.MOTIF_LMAX))
    parser.add_argument("--motif-file", dest="motif_file", default=None, metavar="FASTA",
                        help="motifs from a FASTA file, one pattern per record, after those of --motif")
    parser.add_argument("--motif-mismatches", dest="motif_mismatches", type=int, default=0, metavar="E",
                        help="mismatches allowed at the constrained positions of every motif (by default 0, at most %d)" % lib.MOTIF_EMAX)
    parser.add_argument("--motif-edits", dest="motif_edits", type=int, default=None, metavar="K",
                        help="match with up to K edits (0 .. %d) instead: substitutions at the constrained positions, inserted "
                             "bases and deleted codes.  A hit is the first end of every valley of the distance and every exact "
                             "occurrence, with the shortest substring that attains it; the sixth column of <out-file>_motif.tsv "
                             "holds the edits.  Not together with --motif-mismatches" % lib.MOTIF_KMAX)


def wanted(args):
    return bool(args.motif) or args.motif_file is not None


def _file_motifs(path):
    """(name, pattern) per record of a FASTA file, read here: a pattern is IUPAC text that the sequence readers refuse"""
    out, name, seq = [], None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    out.append((name, "".join(seq)))
                name, seq = (line[1:].split() or [""])[0], []
            elif line and name is not None:
                seq.append(line)
            elif line:
                raise ValueError("text before the first '>'")
    if name is not None:
        out.append((name, "".join(seq)))
    return out


def edits(args):
    """K of --motif-edits, None where the option is not given (or the namespace does not know it)"""
    return getattr(args, "motif_edits", None)


def request(args):
    """(names, patterns, E) of the options, or the text of the refusal"""
    specs = list(args.motif or [])
    try:
        names, patterns = lib.motif_request(specs)
    except lib.SdError as e:
        return "--motif: " + e.msg
    if args.motif_file is not None:
        try:
            more = _file_motifs(args.motif_file)
        except (OSError, ValueError) as e:
            return "--motif-file %s: %s" % (args.motif_file, e)
        if not more:
            return "--motif-file %s: no record" % args.motif_file
        names += [n for n, _ in more]
        patterns += [p for _, p in more]
    for n in names:
        if not NAME.match(n):
            return "--motif: the name '%s' must match [A-Za-z0-9_.-]+" % n
    try:
        lib.motif_compile(list(zip(names, patterns)), args.motif_mismatches)   # (host only: the library's own checks and texts)
    except lib.SdError as e:
        return "--motif: " + e.msg
    K = edits(args)
    if K is not None:
        if args.motif_mismatches:
            return "--motif-edits cannot be combined with --motif-mismatches %d: the edits are the budget" % args.motif_mismatches
        if not 0 <= K <= lib.MOTIF_KMAX:
            return "--motif-edits: K = %d, must be 0 .. %d" % (K, lib.MOTIF_KMAX)
        try:
            lib.motif_edits_request(list(zip(names, patterns)), K, "--motif-edits")   # (host only)
        except lib.SdError as e:
            return e.msg
    return names, patterns, args.motif_mismatches


def check(args, prog="stringdecomposer"):
    """--motif requests this process cannot serve end it here, with one line on stderr, before any work on a GPU."""
    def refuse(msg):
        sys.stderr.write("%s: %s\n" % (prog, msg))
        sys.exit(2)
    if shard.world()[2] > 1:
        refuse("--motif cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    req = request(args)
    if isinstance(req, str):
        refuse(req)
    return req


def files(out_dir, out_file):
    base = os.path.join(out_dir, out_file)
    return base + "_motif.tsv", base + "_motif_rows.tsv", base + "_motif_monomers.tsv"


def batches(lens, n_strands):
    """[(first read, end read)] of every call: whole reads, text and items bounded, at least one read"""
    tile = 64 * lib.MOTIF_TILE_WORDS
    at, out = 0, []
    while at < len(lens):
        e, bases, items = at, 0, 0
        while e < len(lens):
            it = -(-lens[e] // tile) * n_strands
            if e > at and (bases + lens[e] > BATCH_BASES or items + it > lib.MOTIF_ITEMS_MAX):
                break
            bases += lens[e]
            items += it
            e += 1
        out.append((at, e))
        at = e
    return out


def motif_blocks(n_motifs, tiles):
    """blocks of motifs so that tiles x 2 x block stays under the item cap"""
    per = max(1, min(n_motifs, lib.MOTIF_ITEMS_MAX // max(1, 2 * tiles)))
    return [(a, min(n_motifs, a + per)) for a in range(0, n_motifs, per)]


def _over_hit_cap(e):
    return e.code == lib.SD_ERR_PARAM and "MOTIF_HITS_MAX" in e.msg


def scan_part(reads, names, patterns, E, device, threads, K=None):
    """lib.motif -- with K, lib.motif_edits -- on some reads and some motifs -> (hits, per).  A call the library refuses for more than lib.MOTIF_HITS_MAX
    hits -- the one limit no batch can be sized for in advance -- is cut in two and tried again: the reads, or for one read
    the motifs; one read with one motif over the cap stays refused."""
    import numpy as np
    try:
        if K is None:
            m = lib.motif(reads, list(zip(names, patterns)), E, device=device, threads=threads)
        else:
            m = lib.motif_edits(reads, list(zip(names, patterns)), K, device=device, threads=threads)
        return m.hits, m.per
    except lib.SdError as e:
        if not _over_hit_cap(e) or (len(reads) == 1 and len(names) == 1):
            raise
    if len(reads) > 1:
        k = len(reads) // 2
        (h0, p0), (h1, p1) = (scan_part(r, names, patterns, E, device, threads, K) for r in (reads[:k], reads[k:]))
        h1["read"] += k
        return np.concatenate((h0, h1)), np.concatenate((p0, p1))
    k = len(names) // 2
    (h0, p0), (h1, p1) = (scan_part(reads, names[x], patterns[x], E, device, threads, K) for x in (slice(0, k), slice(k, None)))
    h1["motif"] += k
    return np.concatenate((h0, h1)), np.concatenate((p0, p1), axis=1)   # (one read: motif order is canonical order)


def scan(reads, motifs, E, device, threads, K=None):
    """lib.motif over the reads in batches -> formats.Motifs of all reads, hits in canonical order; with K, lib.motif_edits
    -> formats.MotifEdits (the batches are sized by the tile of --motif; that of the edit kernels is no smaller)"""
    import numpy as np
    names, patterns = lib.motif_request(motifs)
    lens = [len(s) for s in reads]
    tile = 64 * lib.MOTIF_TILE_WORDS
    dtype = lib.motif_hit_dtype() if K is None else lib.motif_edit_hit_dtype()
    hits, per = [], np.zeros((len(reads), len(names), 2), dtype=np.int64)
    for a, e in batches(lens, 2 * len(names)):
        tiles = sum(-(-n // tile) for n in lens[a:e])
        part = []
        for ma, me in motif_blocks(len(names), tiles):
            h, p = scan_part(reads[a:e], names[ma:me], patterns[ma:me], E, device, threads, K)
            h["read"] += a
            h["motif"] += ma
            per[a:e, ma:me] = p
            part.append(h)
        h = np.concatenate(part) if part else np.zeros(0, dtype=dtype)
        if len(part) > 1 and K is None:   # blocks of motifs: back into canonical order
            h = h[np.lexsort((h["start"], h["strand"], h["motif"], h["read"]))]
        elif len(part) > 1:
            h = h[np.lexsort((h["start"] + h["length"], h["strand_edits"] >> 7, h["motif"], h["read"]))]
        hits.append(h)
    allh = np.concatenate(hits) if hits else np.zeros(0, dtype=dtype)
    return formats.Motifs(allh, per, names, patterns, E) if K is None else formats.MotifEdits(allh, per, names, patterns, K)


def write(args, final_fn, out_dir, out_file, device):
    """The pass: the reads of args.sequences (lib.fasta_load: FASTA or FASTQ, --lenient honoured) through lib.motif on
    `device` -> <out>_motif.tsv; with final_fn (the final TSV of a decomposition) also <out>_motif_rows.tsv and
    <out>_motif_monomers.tsv.  Raises lib.SdError."""
    names, patterns, E = request(args)
    rn, rs, _ = lib.fasta_load(args.sequences, lenient=args.lenient)
    read_names = [n.split()[0] if n.split() else n for n in rn]   # (the TSVs name a read by its header's first token)
    K = edits(args)
    m = scan(rs, list(zip(names, patterns)), E, device, max(1, int(args.threads)), K)
    hit_fn, rows_fn, mono_fn = files(out_dir, out_file)
    formats.write_motif(hit_fn, (formats.motif_rows if K is None else formats.motif_edit_rows)(m, read_names, rs))
    if final_fn is None:
        return [hit_fn]
    final = formats.read_final(final_fn)
    if K is None:
        counts = formats.motif_row_counts(m.hits, final, m.lengths, read_names)
    else:
        counts = formats.motif_edit_row_counts(m.hits, final, len(names), read_names)
    formats.write_motif_rows(rows_fn, formats.motif_row_lines(counts, final, names))
    mono = [n.split()[0] if n.split() else n for n in lib.fasta_load(args.monomers, lenient=args.lenient)[0]]
    formats.write_motif_monomers(mono_fn, formats.motif_monomers(counts, final, names, mono))
    return [hit_fn, rows_fn, mono_fn]


def main(argv=None):
    parser = argparse.ArgumentParser(prog="sd-motif",
                                     description="hits of IUPAC motifs on both strands of every read: Hamming matches, or with "
                                                 "--motif-edits matches with insertions and deletions")
    parser.add_argument("sequences", help="fasta- or fastq-file with long reads or genomic sequences")
    parser.add_argument("-t", "--threads", help="number of host threads (by default 1)", default="1", required=False)
    parser.add_argument("-o", "--out-dir", help="output directory (by default .)", default=".", required=False)
    parser.add_argument("--out-file", help='prefix of the output files (by default "final_decomposition")',
                        default="final_decomposition", required=False)
    parser.add_argument("--device", type=int, default=0, help="HIP device ordinal (by default 0)")
    parser.add_argument("--lenient", action="store_true",
                        help="read the file leniently: lower case folded to upper case, IUPAC ambiguity codes read as N, the "
                             "CR of CRLF line ends dropped")
    add_arguments(parser)
    args = parser.parse_args(argv)
    if not wanted(args):
        args.motif = ["cenpb"]
    check(args, "sd-motif")
    os.makedirs(args.out_dir, exist_ok=True)
    try:
        for fn in write(args, None, args.out_dir, args.out_file, args.device):
            sys.stderr.write("sd-motif: saved " + fn + "\n")
    except lib.SdError as e:
        sys.stderr.write("--motif failed: " + e.msg + "\n")
        return e.code if 0 < e.code < 256 else 1
    return 0
