"""--hor: the higher-order repeat (HOR) of an array -- which monomers in which order --, where every copy lies and which
copies are variants (csrc/sd_hor.hpp holds the rule).  A post-pass over the rows of the final TSV, on host threads
(lib.hor_rows): transitions between adjacent reliable rows, mutual-best edges, the cycles and paths they form (the orders
H1, H2, ...), and the units -- maximal runs of adjacent rows that walk one order -- ->

  <out>_hor.tsv            one line per unit: read, start, end, strand, order, name, rows, complete
  <out>_hor_orders.tsv     one line per (order, position): order, kind, length, position, monomer, usable rows, edge count
  <out>_hor_variants.tsv   one line per (order, name): order, name, units, rows, bases

(formats.py describes the columns.)  The input meant for this pass is a position-specific monomer set, as --split writes
it: a monomer that sits at two positions of the HOR has two successors and breaks the mutual-best graph there."""
import os
import sys

from . import formats, lib, shard


def add_arguments(parser):
    parser.add_argument("--hor", action="store_true",
                        help="also annotate higher-order repeats: the monomers' cyclic orders (H1, H2, ...) from the transitions "
                             "between adjacent reliable rows of <out-file>.tsv, and every unit -- a run of adjacent rows that walks "
                             "one order.  Writes <out-file>_hor.tsv (per unit: read, start, end, strand, order, name such as 1-12 "
                             "or 1-4_7-12, rows, complete), <out-file>_hor_orders.tsv (per order and position: the monomer, its "
                             "rows, the count of the edge to the next position) and <out-file>_hor_variants.tsv (per order and "
                             "name: units, rows, bases).  Meant for position-specific monomers, e.g. <out-file>_split_monomers.fa "
                             "of a --split run")
    parser.add_argument("--hor-gap", dest="hor_gap", type=int, default=0, metavar="G",
                        help="rows of a read are adjacent when at most G bases lie between them (by default 0: contiguous rows; "
                             "a larger G bridges rows that -i dropped)")
    parser.add_argument("--hor-min-count", dest="hor_min_count", type=int, default=2, metavar="C",
                        help="an edge of an order needs at least C adjacent pairs (by default 2)")


def check(args, prog="stringdecomposer"):
    """--hor requests this process cannot serve end it here, with one line on stderr, before any work on a GPU."""
    def refuse(msg, code=2):
        sys.stderr.write("%s: %s\n" % (prog, msg))
        sys.exit(code)
    if shard.world()[2] > 1:
        refuse("--hor cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    if args.hor_gap < 0 or args.hor_gap >= (1 << 62):
        refuse("--hor-gap %d: a gap of 0 bases or more" % args.hor_gap)
    if args.hor_min_count < 1 or args.hor_min_count >= (1 << 62):
        refuse("--hor-min-count %d: 1 pair or more" % args.hor_min_count)
    if args.records:
        refuse("--hor cannot be combined with --records: it is a post-pass over the rows of the final TSV")
    try:
        names = lib.fasta_load(args.monomers)[0]
    except lib.SdError:
        return   # the job itself reports an unreadable monomer file
    if len(names) > lib.HOR_MMAX:
        refuse("--hor: %d monomers, at most %d are supported" % (len(names), lib.HOR_MMAX), lib.SD_ERR_UNSUPPORTED)
    seen = set()
    for n in names + [x + "'" for x in names]:
        if n in seen:
            refuse("--hor: monomer name %s is not unique: a row's key must name one monomer and strand" % n, lib.SD_ERR_PARAM)
        seen.add(n)


def files(out_dir, out_file):
    base = os.path.join(out_dir, out_file)
    return base + "_hor.tsv", base + "_hor_orders.tsv", base + "_hor_variants.tsv"


def columns(final_rows, mono_names):
    """The rows of a final TSV ([formats.FinalRow]) as the columns of lib.hor_rows -> (read_names, read, start, end, key,
    usable): a read is a run of rows with one name; key = 2 m + s by the monomer's name (s = 1 for name'), -1 for any other."""
    il = {}
    for m, n in enumerate(mono_names):
        for x in (n, n.split()[0]):
            il.setdefault(x, 2 * m)
            il.setdefault(x + "'", 2 * m + 1)
    read_names, read, start, end, key, usable = [], [], [], [], [], []
    for name, rows in formats.by_read(final_rows):
        for r in rows:
            read.append(len(read_names))
            start.append(r.start)
            end.append(r.end)
            key.append(il.get(r.monomer, -1))
            usable.append(1 if r.reliability == "+" else 0)
        read_names.append(name)
    return read_names, read, start, end, key, usable


def compute(args, final_fn):
    """-> (formats.Hor, read names, monomer names) of the final TSV just written"""
    mono_names = [n.split()[0] for n in lib.fasta_load(args.monomers, lenient=args.lenient)[0]]
    read_names, read, start, end, key, usable = columns(formats.read_final(final_fn), mono_names)
    hor = lib.hor_rows(read, start, end, key, usable, len(mono_names), int(args.hor_gap), int(args.hor_min_count),
                       threads=max(1, int(args.threads)))
    return hor, read_names, mono_names


def write(args, final_fn, out_dir, out_file, prog="stringdecomposer"):
    """The pass -> the three files written."""
    hor_fn, ord_fn, var_fn = files(out_dir, out_file)
    hor, read_names, mono_names = compute(args, final_fn)
    for first, n in hor.long:
        sys.stderr.write("%s: --hor: the order of %d monomers that begins at %s is longer than %d and is not numbered\n"
                         % (prog, n, mono_names[first], lib.HOR_PMAX))
    formats.write_hor(hor_fn, formats.hor_units(hor, read_names))
    formats.write_hor_orders(ord_fn, formats.hor_orders(hor, mono_names))
    formats.write_hor_variants(var_fn, formats.hor_variants(hor))
    return hor_fn, ord_fn, var_fn
