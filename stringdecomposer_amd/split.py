"""--split: the subfamilies of every monomer's instances -- the step from a coarse monomer set to the array's own monomers
(csrc/sd_split.hpp holds the rule).  A post-pass over the rows of the final TSV: the rows of --msa are computed read by
read on the device (lib.msa_segments), kept, and clustered per forward monomer (lib.split_msa) ->

  <out>_split.tsv           one line per row of <out>.tsv: read, start, end, monomer, subfamily, d1, d2, columns
  <out>_split_monomers.fa   a monomer file for a second run: per forward monomer, in file order, every subfamily
                            "><name>.<j>" with its consensus; a monomer without instances unchanged as "<name>.0"
  <out>_split_summary.tsv   per subfamily: monomer, subfamily, size, sum of d1, largest d1, nearest subfamily, distance

(formats.py describes the columns.)"""
import os
import sys

from . import formats, lib, shard

K_DEFAULT = 64


def add_arguments(parser):
    parser.add_argument("--split", default=None, metavar="P[,K]",
                        help="also split every monomer's instances (the rows of <out-file>.tsv, by monomer column, as --msa "
                             "shows them) into at most K subfamilies (by default 64, at most 64): an instance that differs from "
                             "its subfamily's centre in P percent of the monomer's columns or more (1 <= P <= 100) seeds a new "
                             "one.  Writes <out-file>_split.tsv (per row: read, start, end, monomer, subfamily, d1, d2, "
                             "columns), <out-file>_split_monomers.fa (the subfamilies' consensus sequences, a monomer file for "
                             "a second run) and <out-file>_split_summary.tsv")
    parser.add_argument("--split-min-size", dest="split_min_size", type=int, default=8, metavar="S",
                        help="a new subfamily needs at least S instances (by default 8)")
    parser.add_argument("--split-iters", dest="split_iters", type=int, default=16, metavar="I",
                        help="at most I rounds of (consensus per subfamily, reassignment) after a subfamily is added (by default 16)")


def request(args):
    """(P, K, S, I) of the options, or the text of the refusal"""
    parts = args.split.split(",")
    ok = 1 <= len(parts) <= 2 and all(x.strip().isdigit() for x in parts)
    pk = [int(x) for x in parts] if ok else None
    if pk is None or not 1 <= pk[0] <= 100 or (len(pk) == 2 and not 1 <= pk[1] <= lib.SPLIT_KMAX):
        return "--split %s: expected P or P,K with 1 <= P <= 100 the radius in percent of a monomer's length and 1 <= K <= %d the " \
               "most subfamilies of a monomer" % (args.split, lib.SPLIT_KMAX)
    if not 1 <= args.split_min_size < (1 << 31):
        return "--split-min-size %d: a subfamily has 1 instance or more" % args.split_min_size
    if not 1 <= args.split_iters < (1 << 31):
        return "--split-iters %d: 1 iteration or more" % args.split_iters
    return pk[0], pk[1] if len(pk) == 2 else K_DEFAULT, args.split_min_size, args.split_iters


def check(args, prog="stringdecomposer"):
    """--split requests this process cannot serve end it here, with one line on stderr, before any work on a GPU."""
    def refuse(msg, code=2):
        sys.stderr.write("%s: %s\n" % (prog, msg))
        sys.exit(code)
    if shard.world()[2] > 1:
        refuse("--split cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    req = request(args)
    if isinstance(req, str):
        refuse(req)
    if args.records:
        refuse("--split cannot be combined with --records: it is a post-pass over the rows of the final TSV")
    try:
        names = lib.fasta_load(args.monomers)[0]
    except lib.SdError:
        return req   # the job itself reports an unreadable monomer file
    seen = set()
    for n in names + [x + "'" for x in names]:
        if n in seen:
            refuse("--split: monomer name %s is not unique: a row's key must name one template" % n, lib.SD_ERR_PARAM)
        seen.add(n)
    return req


def files(out_dir, out_file):
    base = os.path.join(out_dir, out_file)
    return base + "_split.tsv", base + "_split_monomers.fa", base + "_split_summary.tsv"


def collect(args, final_fn, device):
    """The rows of --msa of every row of the final TSV, by the path --msa takes, as one formats.Msa -> (msa, pair_tmpl,
    meta, inserted, names, seqs): meta = (read, start, end, monomer) per row, inserted = {row: {slot: bases}} for the rows
    that insert, names / seqs = the forward monomers."""
    import numpy as np
    rn, rs, _ = lib.fasta_load(args.sequences, lenient=args.lenient)
    mn, ms, _ = lib.fasta_load(args.monomers, lenient=args.lenient)
    reads, il = {}, {}
    for n, s in zip(rn, rs):   # (the TSV names a read by its header's first token)
        reads.setdefault(n, s.upper())
        reads.setdefault(n.split()[0], s.upper())
    ms = [s.upper() for s in ms]
    for m, n in enumerate(mn):
        for x in (n, n.split()[0]):
            il.setdefault(x, 2 * m)
            il.setdefault(x + "'", 2 * m + 1)
    parts, ats, stats, pts, meta, inserted, base = [], [], [], [], [], {}, 0
    for read, rows in formats.by_read(formats.read_final(final_fn)):
        seq = reads[read]
        st = [min(max(r.start, 0), len(seq)) for r in rows]
        en = [min(max(r.end + 1, s), len(seq)) - 1 for r, s in zip(rows, st)]   # (an empty segment: end = start - 1)
        pt = [il[r.monomer] for r in rows]
        msa = lib.msa_segments(seq or b"N", st, en, ms, pt, threads=max(1, int(args.threads)), device=device)
        for i, x in enumerate(pt):
            if int(msa.status[i]) == 1 and formats.msa_row(msa, i, x)[1].any():
                got = formats.msa_inserted(msa, i, x, seq[st[i]:en[i] + 1])
                if got:
                    inserted[len(meta) + i] = got
        parts.append(np.asarray(msa.rows))
        ats.append(np.asarray(msa.row_at[:-1], dtype=np.int64) + base)
        base += int(msa.row_at[-1])
        stats.append(np.asarray(msa.status))
        pts += pt
        meta += [(r.read, r.start, r.end, r.monomer) for r in rows]
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)   # noqa: E731
    row_at = np.concatenate([cat(ats, np.int64), np.asarray([base], dtype=np.int64)])
    msa = formats.Msa(cat(parts, np.uint8), row_at, cat(stats, np.uint8), [len(s) for s in ms])
    return msa, pts, meta, inserted, [n.split()[0] for n in mn], [s if isinstance(s, str) else s.decode() for s in ms]


def write(args, final_fn, out_dir, out_file, device):
    """The pass -> the three files written."""
    P, K, S, I = request(args)
    split_fn, fa_fn, sum_fn = files(out_dir, out_file)
    msa, pt, meta, inserted, names, seqs = collect(args, final_fn, device)
    splits = lib.split_msa(msa, pt, msa.tlen, P, K, S, I, device=device, threads=max(1, int(args.threads)))
    formats.write_split(split_fn, formats.split_rows(msa, pt, names, splits, meta))
    with open(fa_fn, "w", newline="") as f:
        for m, (name, seq, sp) in enumerate(zip(names, seqs, splits)):
            for sub, _, sq in formats.split_consensus(msa, pt, m, name, seq, sp, inserted):
                f.write(">%s\n%s\n" % (sub, sq or seq))
    formats.write_split_summary(sum_fn, formats.split_summary(names, splits))
    return split_fn, fa_fn, sum_fn
