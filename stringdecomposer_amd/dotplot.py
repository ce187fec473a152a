"""--dotplot: the windowed k-mer identity of every read of the reads file against itself, on the device -- the read cut into
windows of W bases, every window scored against every earlier one by the k-mers they share, on both strands with
--dotplot-rc: where an array lies, how it is layered and where it flips, without a monomer file.  main.py runs the pass
beside a decomposition (stringdecomposer reads.fa monomers.fa --dotplot 2000); bin/sd-dotplot runs it alone
(sd-dotplot reads.fa --dotplot 2000).

The reads go to lib.dotplot in batches of whole reads, at most BATCH_BASES bases of text and BATCH_CELLS cells each, but at
least one read: a single read with more than lib.DOTPLOT_CELLS_MAX cells is refused by the library, with the numbers."""
import argparse
import os
import sys

from . import formats, lib, shard

BATCH_BASES = 1 << 28
BATCH_CELLS = 1 << 24


def add_arguments(parser):
    parser.add_argument("--dotplot", default=None, metavar="W[,B]",
                        help="also write <out-file>_dotplot.tsv: every read cut into windows of W bases (1 <= W <= 1073741824) "
                             "and every window compared with every earlier window of the read (with B: with the B windows "
                             "before it) by the distinct K-mers they share -- one line per pair that shares any: read, "
                             "start_i, end_i, start_j, end_j, kmers_i, kmers_j, shared, identity = 100 (shared / min(kmers_i, "
                             "kmers_j)) ^ (1 / K).  Needs no monomers")
    parser.add_argument("--dotplot-k", dest="dotplot_k", type=int, default=21, metavar="K",
                        help="the k-mer length, 1 <= K <= 32 (by default 21)")
    parser.add_argument("--dotplot-mod", dest="dotplot_mod", type=int, default=1, metavar="M",
                        help="compare only the k-mers whose hash is a multiple of M, 1 <= M <= 1048576 (by default 1: all); a "
                             "window may hold at most 4096 of them, so windows above 4096 bases need M > 1")
    parser.add_argument("--dotplot-rc", dest="dotplot_rc", action="store_true",
                        help="add the reverse strand: kmers_rc_j, shared_rc, identity_rc -- the k-mers of window i whose reverse "
                             "complement lies in window j, which shows inversions")
    parser.add_argument("--dotplot-min", dest="dotplot_min", type=int, default=0, metavar="P",
                        help="keep a line only when one of its identities reaches P percent (an integer 0 .. 100, by default 0)")


def _ints(text, lo, hi):
    """'A' or 'A,B' -> [A] or [A, B]; None when the text is neither"""
    parts = text.split(",")
    if not lo <= len(parts) <= hi or not all(x.strip().isdigit() for x in parts):
        return None
    return [int(x) for x in parts]


def request(args):
    """(W, B, K, M, rc, P) of the options, or the text of the refusal"""
    wb = _ints(args.dotplot, 1, 2)
    if wb is None or not 1 <= wb[0] <= lib.DOTPLOT_WMAX or (len(wb) == 2 and not 0 <= wb[1] <= lib.DOTPLOT_BMAX):
        return "--dotplot %s: expected W or W,B with 1 <= W <= %d the bases of a window and 0 <= B <= %d the windows before a " \
               "window it is compared with (0: all)" % (args.dotplot, lib.DOTPLOT_WMAX, lib.DOTPLOT_BMAX)
    if not 1 <= args.dotplot_k <= lib.DOTPLOT_KMAX:
        return "--dotplot-k %d: the k-mer length is 1 .. %d" % (args.dotplot_k, lib.DOTPLOT_KMAX)
    if not 1 <= args.dotplot_mod <= lib.DOTPLOT_MMAX:
        return "--dotplot-mod %d: the modulus is 1 .. %d" % (args.dotplot_mod, lib.DOTPLOT_MMAX)
    if not 0 <= args.dotplot_min <= 100:
        return "--dotplot-min %d: the smallest identity of a line is 0 .. 100 percent" % args.dotplot_min
    return wb[0], wb[1] if len(wb) == 2 else 0, args.dotplot_k, args.dotplot_mod, bool(args.dotplot_rc), args.dotplot_min


def check(args, prog="stringdecomposer"):
    """--dotplot requests this process cannot serve end it here, with one line on stderr, before any work on a GPU."""
    def refuse(msg):
        sys.stderr.write("%s: %s\n" % (prog, msg))
        sys.exit(2)
    if shard.world()[2] > 1:
        refuse("--dotplot cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    req = request(args)
    if isinstance(req, str):
        refuse(req)
    return req


def files(out_dir, out_file):
    return (os.path.join(out_dir, out_file) + "_dotplot.tsv",)


def _cells(n, W, B):
    nw = -(-n // W)
    return nw * (nw + 1) // 2 if B <= 0 or nw <= B + 1 else (B + 1) * (B + 2) // 2 + (nw - B - 1) * (B + 1)


def write(args, out_dir, out_file, device):
    """The pass: the reads of args.sequences (lib.fasta_load: FASTA or FASTQ, --lenient honoured) in batches through
    lib.dotplot on `device` -> <out>_dotplot.tsv.  Raises lib.SdError."""
    W, B, K, M, rc, P = request(args)
    rn, rs, _ = lib.fasta_load(args.sequences, lenient=args.lenient)
    names = [n.split()[0] if n.split() else n for n in rn]   # (the TSVs name a read by its header's first token)
    threads = max(1, int(args.threads))
    fn, = files(out_dir, out_file)
    with open(fn, "w", newline="") as f:
        at = 0
        while at < len(rs):   # a call's share: whole reads, text and cells bounded
            e, bases, cells = at, 0, 0
            while e < len(rs):
                c = _cells(len(rs[e]), W, B)
                if e > at and (bases + len(rs[e]) > BATCH_BASES or cells + c > BATCH_CELLS):
                    break
                bases += len(rs[e])
                cells += c
                e += 1
            dp = lib.dotplot(rs[at:e], K, W, B, M, rc, device=device, threads=threads)
            f.write(formats.format_dotplot(formats.dotplot_rows(dp, names[at:e], P)))
            at = e
    return [fn]


def main(argv=None):
    parser = argparse.ArgumentParser(prog="sd-dotplot",
                                     description="windowed k-mer identity of every read against itself, both strands on "
                                                 "request: the self-dotplot of a tandem array, without a monomer file")
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
    if args.dotplot is None:
        args.dotplot = "2000"
    check(args, "sd-dotplot")
    os.makedirs(args.out_dir, exist_ok=True)
    try:
        for fn in write(args, args.out_dir, args.out_file, args.device):
            sys.stderr.write("sd-dotplot: saved " + fn + "\n")
    except lib.SdError as e:
        sys.stderr.write("--dotplot failed: " + e.msg + "\n")
        return e.code if 0 < e.code < 256 else 1
    return 0
