"""The merge of seed monomers: which sequences of a FASTA file are the same monomer up to rotation, strand and a few
percent of edits (lib.cyclic_merge; csrc/sd_cyclic.hpp has the rule).  autocorr.py runs it on the seeds of a run
(--autocorr-merge P); bin/sd-merge runs it on any FASTA file (sd-merge seeds.fa -o OUT --merge 85): seed files of several
runs, or monomer sets of different origin whose phases differ.

Two files come out: <base>merged.fa, one record per cluster in cluster order -- the canonical record of the cluster's
centre, the same whichever read supplied it -- and <base>merge.tsv, one line per input sequence (formats.MergeRow)."""
import argparse
import os
import sys

from . import formats, lib, shard


def weight_of(header):
    """the N of the header's count=N token, else 0"""
    for tok in header.split()[1:]:
        if tok.startswith("count=") and tok[6:].isdigit():
            return int(tok[6:])
    return 0


def read_fasta(path, lenient=False):
    """(headers, sequences) of a FASTA file, the headers whole -- lib.fasta_load keeps a record's name only, and the weight
    is in the rest of the line.  lenient: lower case folded to upper case, the CR of CRLF line ends dropped; nothing else is
    changed, so any other byte reaches the merge's own check and is refused there with the sequence's name."""
    names, parts = [], []
    try:
        with open(path, "rb") as f:
            for line in f:
                line = line.rstrip(b"\n")
                if lenient:
                    line = line.rstrip(b"\r")
                if line.startswith(b">"):
                    names.append(line[1:].decode(errors="replace"))
                    parts.append([])
                elif line and not names:
                    raise lib.SdError(lib.SD_ERR_FORMAT, "%s: sequence data before the first header" % path)
                elif line:
                    parts[-1].append(line.upper() if lenient else line)
    except OSError as e:
        raise lib.SdError(lib.SD_ERR_IO, "%s: %s" % (path, e.strerror))
    return names, [b"".join(p) for p in parts]


def percent_error(option, P):
    """the text of the refusal of a P that is not 1 .. 100, else None"""
    if not lib._is_int(P) or not 1 <= P <= 100:
        return "%s %s: the identity of a cluster is 1 .. 100 percent" % (option, P)
    return None


def merge_files(names, seqs, P, fa_path, tsv_path, min_size=1, device=None, threads=1, block=None):
    """names (FASTA headers) and seqs -> the two files; weights from the headers' count= tokens.  min_size leaves smaller
    clusters out of fa_path only.  -> the formats.CyclicMerge.  Raises lib.SdError."""
    weights = [weight_of(n) for n in names]
    m = lib.cyclic_merge(seqs, weights, P, block=block, device=device, threads=threads, names=[formats._token(n) for n in names])
    recs = formats.merged_records(m, names, seqs, weights, lib.cyclic_canon, min_size)
    with open(fa_path, "w", newline="") as f:
        f.write(formats.format_merged(recs))
    formats.write_merge(tsv_path, formats.merge_rows(m, names, [len(s) for s in seqs]))
    return m


def main(argv=None):
    parser = argparse.ArgumentParser(prog="sd-merge",
                                     description="cluster the sequences of a FASTA file up to rotation and strand: one record "
                                                 "per monomer from the seed files of several runs")
    parser.add_argument("sequences", help="fasta-file with seed monomers (upper-case ACGT; a count=N token of a header is its weight)")
    parser.add_argument("-t", "--threads", help="number of host threads (by default 1)", default="1", required=False)
    parser.add_argument("-o", "--out-dir", help="output directory (by default .)", default=".", required=False)
    parser.add_argument("--out-file", help='prefix of the output files (by default "final_decomposition")',
                        default="final_decomposition", required=False)
    parser.add_argument("--device", type=int, default=0, help="HIP device ordinal (by default 0)")
    parser.add_argument("--lenient", action="store_true",
                        help="read the file leniently: lower case folded to upper case, the CR of CRLF line ends dropped (any "
                             "byte outside ACGT that remains is refused with the sequence's name)")
    parser.add_argument("--merge", type=int, default=85, metavar="P",
                        help="sequences within 100 - P percent of edits of a cluster's centre, at any rotation and on either "
                             "strand, and within that share of its length, join the cluster (by default 85)")
    parser.add_argument("--merge-min-size", dest="merge_min_size", type=int, default=1, metavar="S",
                        help="leave clusters of fewer than S sequences out of <out>_merged.fa (by default 1)")
    args = parser.parse_args(argv)

    def refuse(msg):
        sys.stderr.write("sd-merge: %s\n" % msg)
        sys.exit(2)
    if shard.world()[2] > 1:
        refuse("--merge cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    if percent_error("--merge", args.merge):
        refuse(percent_error("--merge", args.merge))
    if args.merge_min_size < 1:
        refuse("--merge-min-size %d: the smallest cluster written is 1 or more sequences" % args.merge_min_size)
    os.makedirs(args.out_dir, exist_ok=True)
    base = os.path.join(args.out_dir, args.out_file)
    try:
        names, seqs = read_fasta(args.sequences, args.lenient)
        m = merge_files(names, seqs, args.merge, base + "_merged.fa", base + "_merge.tsv", args.merge_min_size, args.device,
                        max(1, int(args.threads)))
    except lib.SdError as e:
        sys.stderr.write("--merge failed: " + e.msg + "\n")
        return e.code if 0 < e.code < 256 else 1
    sys.stderr.write("sd-merge: %d sequences in %d clusters; saved %s_merged.fa, %s_merge.tsv\n" % (len(names), m.n_clusters, base, base))
    return 0
