"""--autocorr: the k-mer autocorrelation of every read of the reads file against itself, on the device -- where the tandem
arrays are and what their period is in bases, without a monomer file.  main.py runs the pass beside a decomposition
(stringdecomposer reads.fa monomers.fa --autocorr 8); bin/sd-autocorr runs it alone (sd-autocorr reads.fa --autocorr 8).

The reads go to lib.autocorr in batches of whole reads, at most BATCH_BASES bases of text and BATCH_CELLS counters
(windows x D) each -- 256 MB of text and 128 MB of counters at a time, whatever the file holds -- but at least one read: a
single read whose windows x D exceed lib.AUTOCORR_CELLS_MAX is refused by the library, with the numbers."""
import argparse
import os
import sys

from . import cyclic, formats, lib, shard

BATCH_BASES = 1 << 28
BATCH_CELLS = 1 << 24
PEAKS_MAX = 1024


def add_arguments(parser):
    parser.add_argument("--autocorr", default=None, metavar="K[,D]",
                        help="also write <out-file>_autocorr.tsv: per read (and window) the lags d = 1 .. D (by default 4096, at "
                             "most 1048576) at which its K-mers (1 <= K <= 32) recur most often -- one line per (read, "
                             "window): read, start, end, k, period (the lag of the first peak, 0 = none), count (positions "
                             "whose K-mer recurs that many bases on, neither copy holding a byte outside ACGT), positions "
                             "(how many could), then the peaks as lag:count.  Needs no monomers: the period is in bases")
    parser.add_argument("--autocorr-window", dest="autocorr_window", type=int, default=0, metavar="W",
                        help="count per window of W bases of a read (by default 0: one window, the whole read)")
    parser.add_argument("--autocorr-min-lag", dest="autocorr_min_lag", type=int, default=1, metavar="LO",
                        help="the smallest lag that can be a peak (by default 1)")
    parser.add_argument("--autocorr-peaks", dest="autocorr_peaks", default="8,8", metavar="P[,R]",
                        help="report up to P peaks per line; a lag is a peak when no lag within R of it counts more (by "
                             "default 8,8)")
    parser.add_argument("--autocorr-spectrum", dest="autocorr_spectrum", action="store_true",
                        help="also write <out-file>_autocorr_spectrum.tsv: read, start, end, lag, count, positions for every "
                             "lag of every window with a count")
    parser.add_argument("--autocorr-seeds", dest="autocorr_seeds", type=int, default=None, metavar="MINCOUNT",
                        help="also write <out-file>_autocorr_seeds.fa: for every read whose period counts at least MINCOUNT "
                             "positions, the period's worth of bases where the longest run of such positions starts -- a "
                             "monomer file for a second run with --profile, which polishes it")
    parser.add_argument("--autocorr-merge", dest="autocorr_merge", type=int, default=None, metavar="P",
                        help="with --autocorr-seeds, also write <out-file>_autocorr_merged.fa and <out-file>_autocorr_merge.tsv: "
                             "the seeds of all reads clustered up to rotation and strand -- a seed within 100 - P percent of "
                             "edits of a cluster's centre, and of its length, joins it; one record per cluster, and per seed "
                             "its cluster, distance, strand and phase")
    parser.add_argument("--autocorr-merge-min-size", dest="autocorr_merge_min_size", type=int, default=1, metavar="S",
                        help="leave clusters of fewer than S seeds out of <out-file>_autocorr_merged.fa (by default 1)")


def _ints(text, lo, hi):
    """'A' or 'A,B' -> [A] or [A, B]; None when the text is neither"""
    parts = text.split(",")
    if not lo <= len(parts) <= hi or not all(x.strip().isdigit() for x in parts):
        return None
    return [int(x) for x in parts]


def request(args):
    """(K, D, W, LO, P, R) of the options, or the text of the refusal"""
    kd = _ints(args.autocorr, 1, 2)
    if kd is None or not 1 <= kd[0] <= lib.AUTOCORR_KMAX or (len(kd) == 2 and not 1 <= kd[1] <= lib.AUTOCORR_DMAX):
        return "--autocorr %s: expected K or K,D with 1 <= K <= %d the k-mer length and 1 <= D <= %d the largest lag" % (
            args.autocorr, lib.AUTOCORR_KMAX, lib.AUTOCORR_DMAX)
    K, D = kd[0], kd[1] if len(kd) == 2 else 4096
    if not 0 <= args.autocorr_window < (1 << 62):
        return "--autocorr-window %d: the window is 0 (the whole read) or a number of bases" % args.autocorr_window
    if not 1 <= args.autocorr_min_lag <= D:
        return "--autocorr-min-lag %d: the smallest lag of a peak is 1 .. D = %d" % (args.autocorr_min_lag, D)
    pr = _ints(args.autocorr_peaks, 1, 2)
    if pr is None or not 0 <= pr[0] <= PEAKS_MAX or (len(pr) == 2 and not 0 <= pr[1] <= lib.AUTOCORR_DMAX):
        return "--autocorr-peaks %s: expected P or P,R with 0 <= P <= %d peaks per line and 0 <= R <= %d the radius of a peak" % (
            args.autocorr_peaks, PEAKS_MAX, lib.AUTOCORR_DMAX)
    if args.autocorr_seeds is not None and args.autocorr_seeds < 0:
        return "--autocorr-seeds %d: the smallest count of a seed's period is 0 or more" % args.autocorr_seeds
    if getattr(args, "autocorr_merge", None) is not None:
        if args.autocorr_seeds is None:
            return "--autocorr-merge %d: the merge clusters the seeds, it needs --autocorr-seeds" % args.autocorr_merge
        if cyclic.percent_error("--autocorr-merge", args.autocorr_merge):
            return cyclic.percent_error("--autocorr-merge", args.autocorr_merge)
        if args.autocorr_merge_min_size < 1:
            return "--autocorr-merge-min-size %d: the smallest cluster written is 1 or more seeds" % args.autocorr_merge_min_size
    return K, D, args.autocorr_window, args.autocorr_min_lag, pr[0], pr[1] if len(pr) == 2 else 8


def check(args, prog="stringdecomposer"):
    """--autocorr requests this process cannot serve end it here, with one line on stderr, before any work on a GPU."""
    def refuse(msg):
        sys.stderr.write("%s: %s\n" % (prog, msg))
        sys.exit(2)
    if shard.world()[2] > 1:
        refuse("--autocorr cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    req = request(args)
    if isinstance(req, str):
        refuse(req)
    return req


def refuse_merge_alone(args, prog="stringdecomposer"):
    """--autocorr-merge beside a decomposition without --autocorr: the pass that makes the seeds does not run (the other
    --autocorr-* options are ignored without it, as they always were; this one asks for files and is refused)"""
    sys.stderr.write("%s: --autocorr-merge %d: the merge clusters the seeds of --autocorr, it needs --autocorr and --autocorr-seeds\n" % (
        prog, args.autocorr_merge))
    sys.exit(2)


def files(out_dir, out_file):
    base = os.path.join(out_dir, out_file)
    return base + "_autocorr.tsv", base + "_autocorr_spectrum.tsv", base + "_autocorr_seeds.fa"


def merge_files(out_dir, out_file):
    base = os.path.join(out_dir, out_file)
    return base + "_autocorr_merged.fa", base + "_autocorr_merge.tsv"


def write(args, out_dir, out_file, device):
    """The pass: the reads of args.sequences (lib.fasta_load: FASTA or FASTQ, --lenient honoured) in batches through
    lib.autocorr on `device` -> <out>_autocorr.tsv, with --autocorr-spectrum <out>_autocorr_spectrum.tsv, with
    --autocorr-seeds <out>_autocorr_seeds.fa.  Raises lib.SdError."""
    K, D, W, LO, P, R = request(args)
    rn, rs, _ = lib.fasta_load(args.sequences, lenient=args.lenient)
    names = [n.split()[0] if n.split() else n for n in rn]   # (the TSVs name a read by its header's first token)
    threads = max(1, int(args.threads))
    sum_fn, spec_fn, seed_fn = files(out_dir, out_file)
    merged_fn, merge_fn = merge_files(out_dir, out_file)
    merge, seeds = getattr(args, "autocorr_merge", None), []
    fs = open(spec_fn, "w", newline="") if args.autocorr_spectrum else None
    fa = open(seed_fn, "w", newline="") if args.autocorr_seeds is not None else None
    try:
        with open(sum_fn, "w", newline="") as f:
            at = 0
            while at < len(rs):   # a call's share: whole reads, text and counters bounded
                e, bases, cells = at, 0, 0
                while e < len(rs):
                    c = max(1, -(-len(rs[e]) // W) if W > 0 else 1) * D
                    if e > at and (bases + len(rs[e]) > BATCH_BASES or cells + c > BATCH_CELLS):
                        break
                    bases += len(rs[e])
                    cells += c
                    e += 1
                reads, lens = rs[at:e], [len(s) for s in rs[at:e]]
                ac = lib.autocorr(reads, K, D, W, device=device, threads=threads)
                f.write(formats.format_autocorr(lib.autocorr_rows(ac, names[at:e], lens, LO, R, P)))
                if fs:
                    fs.write(formats.format_autocorr_spectrum(lib.autocorr_spectrum_rows(ac, names[at:e], lens)))
                if fa:
                    for name, seq in lib.autocorr_seeds(reads, names[at:e], ac, LO, args.autocorr_seeds, R):
                        fa.write(">%s\n%s\n" % (name, seq))
                        seeds.append((name, seq))
                at = e
    finally:
        if fs:
            fs.close()
        if fa:
            fa.close()
    saved = [sum_fn] + ([spec_fn] if fs else []) + ([seed_fn] if fa else [])
    if merge is not None:   # the seeds of all reads, clustered; a failure here leaves every other file
        try:
            cyclic.merge_files([n for n, _ in seeds], [s for _, s in seeds], merge, merged_fn, merge_fn, args.autocorr_merge_min_size,
                               device, threads)
            saved += [merged_fn, merge_fn]
        except lib.SdError as e:
            sys.stderr.write("--autocorr-merge failed: " + e.msg + "\n")
    return saved


def main(argv=None):
    parser = argparse.ArgumentParser(prog="sd-autocorr",
                                     description="k-mer autocorrelation of every read against itself: the period of its tandem "
                                                 "repeats in bases, without a monomer file")
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
    if args.autocorr is None:
        args.autocorr = "8"
    check(args, "sd-autocorr")
    os.makedirs(args.out_dir, exist_ok=True)
    try:
        for fn in write(args, args.out_dir, args.out_file, args.device):
            sys.stderr.write("sd-autocorr: saved " + fn + "\n")
    except lib.SdError as e:
        sys.stderr.write("--autocorr failed: " + e.msg + "\n")
        return e.code if 0 < e.code < 256 else 1
    return 0
