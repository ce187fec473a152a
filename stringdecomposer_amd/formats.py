"""On-disk formats of StringDecomposer as a small library API.

Three tab-separated text files make up the contract with downstream tools (centroFlye, HORmon):

  <out>_raw.tsv   7 columns, written by the DP stage (reference main.cpp:272-285, SaveBatch):
                  read, monomer, start, end, score ("%f" of a float), gap to the previous row of the
                  same read (start - previous end; the first row of a read: its start), end - start
  <out>.tsv       12 columns, README.md:77-83 of the reference / main.py:153-160:
                  read, best monomer, start, end, identity, second best monomer, its identity,
                  homopolymer-compressed best monomer, its identity, homo second best, its identity,
                  reliability ('+' or '?')
  <out>_alt.tsv   6 columns (main.py:161-165): read, monomer, start, end, identity, '*' for the
                  monomer reported in <out>.tsv else '-'

Two more text files are this package's own (opt-in, `--profile`):

  <out>_profile.tsv   the column profile of every monomer over the rows of <out>.tsv: a header line, then per
                      monomer (FASTA order) rows g = 0..L of 16 columns -- name, g, ref (the monomer's base at g, '-' at
                      g = L), n (instances), A C G T N (read bases aligned to position g), del, ins_n (instances with
                      an insertion in slot g, i.e. before position g), insA insC insG insT insN (the inserted bases).
                      Instances of m' are folded into m (reverse-complemented).  read_profile / write_profile below.
  <out>_consensus.fa  one record per monomer, ">name instances=n", the consensus of its profile (consensus below).

  <out>_msa.tsv       (`--msa`) one line per row of <out>.tsv, in its order, behind a header line: read, start, end,
                      monomer (as printed there), columns (one character per position of the FORWARD monomer over
                      ACGTN-: the read base aligned there, '-' a deleted position; '.' throughout for a row that is no
                      instance), insertions ("slot:count,..." -- count read bases inserted before position slot, 255
                      meaning 255 or more -- or '.').  Instances of m' are reverse-complemented onto m, as in the
                      profile, so the lines of one monomer are a multiple alignment.  read_msa / write_msa below.

  <out>_screen.tsv    (`--screen THR`) one line per region that was decomposed, no header: read, start, end (0-based,
                      inclusive), chunks (passing chunks the region was made of), best_distance (the smallest infix
                      edit distance of a monomer or reverse complement against one of them), best_template (its name,
                      with ' for a reverse complement).  read_screen / write_screen below.

  <out>_autocorr.tsv  (`--autocorr K[,D]`) one line per (read, window), no header: read, start, end (the window's bases
                      [start, end), 0-based), k, period (the lag of the first peak, 0 = none), count (positions whose k-mer
                      recurs `period` bases on), positions (how many could), then up to P columns lag:count, the peaks.
                      <out>_autocorr_spectrum.tsv (`--autocorr-spectrum`): read, start, end, lag, count, positions for
                      every lag of every window with a count.  read_autocorr / read_autocorr_spectrum below.

  <out>_dotplot.tsv   (`--dotplot W[,B]`) one line per pair of windows of a read that share a k-mer, no header: read,
                      start_i, end_i, start_j, end_j, kmers_i, kmers_j, shared, identity; with `--dotplot-rc` kmers_rc_j,
                      shared_rc, identity_rc.  read_dotplot / write_dotplot below.

  <out>_split.tsv     (`--split P[,K]`) one line per row of <out>.tsv, no header: read, start, end, monomer, subfamily
                      ("<name>.<j>", '*' for a row that is no instance), d1, d2 (columns in which the row differs from its
                      subfamily's centre and from the nearest other one), columns (as in <out>_msa.tsv).
                      <out>_split_summary.tsv: monomer, subfamily, size, sum of d1, largest d1, nearest subfamily, distance.
                      read_split / read_split_summary below; <out>_split_monomers.fa is a monomer file.

  <out>_hor.tsv       (`--hor`) one line per higher-order repeat unit, no header: read, start, end, strand ('+' / '-'),
                      order (H1, H2, ...), name (the positions of the order present, as ranges: 1-12, 1-4_7-12, 3), rows,
                      complete (1 when every position is present, else 0).
                      <out>_hor_orders.tsv, one line per (order, position): order, kind (cycle / path), length, position,
                      monomer, usable rows of the monomer, count of the edge to the next position (0 at a path's end).
                      <out>_hor_variants.tsv, one line per (order, name): order, name, units, rows, bases.
                      read_hor / read_hor_orders / read_hor_variants below.

  <out>_autocorr_merge.tsv  (`--autocorr-merge P`; `<out>_merge.tsv` of bin/sd-merge) one line per seed, no header: seed,
                      length, cluster (M1, M2, ...), centre (the seed that is the cluster's centre), distance, identity
                      ("%.2f" of 100 (length - distance) / length, printf's rounding), strand, phase.  <out>_autocorr_merged.fa / <out>_merged.fa: one record per cluster, its canonical
                      record.  read_merge / write_merge / merged_records below.

A fourth, binary, file is this package's own (the reference has no counterpart; opt-in, `--records`):

  <out>_raw.sdr   the rows of <out>_raw.tsv as 16-byte records per read (read_records / write_records below;
                  layout in csrc/sd_records.hpp, C-ABI sd_write_records / sd_read_records in include/sd_hip.h).
                  records_to_raw_tsv(read_records(path)) is the raw TSV byte for byte.

Readers return lists of named tuples with numeric fields converted; writers reproduce the reference's
text exactly (round trip = identity on files the reference or this package wrote), so a tool can
filter / merge decompositions without re-deriving the formatting rules.
"""
from collections import namedtuple

RawRow = namedtuple("RawRow", "read monomer start end score gap length")
FinalRow = namedtuple("FinalRow", "read monomer start end identity second_best second_best_identity "
                                   "homo_best homo_best_identity homo_second_best "
                                   "homo_second_best_identity reliability")
AltRow = namedtuple("AltRow", "read monomer start end identity best")


class FormatError(ValueError):
    def __init__(self, path, lineno, msg):
        super().__init__("%s:%d: %s" % (path, lineno, msg))
        self.path, self.lineno = path, lineno


def _lines(path_or_text, is_text):
    if is_text:
        data = path_or_text
    else:
        with open(path_or_text, "r", newline="") as f:
            data = f.read()
    if not data:
        return []
    body = data[:-1] if data.endswith("\n") else data
    return body.split("\n")


def _parse(path_or_text, is_text, ncol, conv, cls):
    name = "<text>" if is_text else str(path_or_text)
    out = []
    for no, ln in enumerate(_lines(path_or_text, is_text), 1):
        f = ln.split("\t")
        if len(f) != ncol:
            raise FormatError(name, no, "expected %d tab-separated columns, found %d" % (ncol, len(f)))
        try:
            out.append(cls(*[c(x) for c, x in zip(conv, f)]))
        except ValueError as e:
            raise FormatError(name, no, str(e))
    return out


def _ident(x):
    return x


# ---- raw ------------------------------------------------------------------------------------------
def read_raw(path):
    return _parse(path, False, 7, (_ident, _ident, int, int, float, int, int), RawRow)


def parse_raw(text):
    return _parse(text, True, 7, (_ident, _ident, int, int, float, int, int), RawRow)


def format_raw(rows):
    """SaveBatch (main.cpp:272-285): '%f' of the score; gap / length columns are stored, not recomputed."""
    return "".join("%s\t%s\t%d\t%d\t%f\t%d\t%d\n" % (r.read, r.monomer, r.start, r.end, r.score, r.gap,
                                                    r.length) for r in rows)


def raw_rows(read, triples):
    """Rows of one read from (monomer, start, end, score) in position order, with the derived
    columns filled in as SaveBatch does (prev_end starts at 0 for every read)."""
    out, prev_end = [], 0
    for monomer, start, end, score in triples:
        out.append(RawRow(read, monomer, int(start), int(end), float(score), int(start) - prev_end,
                          int(end) - int(start)))
        prev_end = int(end)
    return out


# ---- final ----------------------------------------------------------------------------------------
_FINAL_CONV = (_ident, _ident, int, int, float, _ident, float, _ident, float, _ident, float, _ident)


def read_final(path):
    return _parse(path, False, 12, _FINAL_CONV, FinalRow)


def parse_final(text):
    return _parse(text, True, 12, _FINAL_CONV, FinalRow)


def format_final(rows):
    """main.py:153-160: identities with '{:.2f}'."""
    f2 = "{:.2f}".format
    return "".join("\t".join([r.read, r.monomer, str(r.start), str(r.end), f2(r.identity), r.second_best,
                              f2(r.second_best_identity), r.homo_best, f2(r.homo_best_identity),
                              r.homo_second_best, f2(r.homo_second_best_identity), r.reliability]) + "\n"
                   for r in rows)


# ---- alt ------------------------------------------------------------------------------------------
def _star(x):
    if x not in ("*", "-"):
        raise ValueError("last column must be '*' or '-', found %r" % x)
    return x == "*"


def read_alt(path):
    return _parse(path, False, 6, (_ident, _ident, int, int, float, _star), AltRow)


def parse_alt(text):
    return _parse(text, True, 6, (_ident, _ident, int, int, float, _star), AltRow)


def format_alt(rows):
    f2 = "{:.2f}".format
    return "".join("\t".join([r.read, r.monomer, str(r.start), str(r.end), f2(r.identity),
                              "*" if r.best else "-"]) + "\n" for r in rows)


def final_rows(final, read_names, keys):
    """The rows of a final-mode stream job (lib.Stream(final=True).collect(): a FinalRows, or its (rows, row_off, alt);
    a lib.DeviceFinalRows of a device_final stream is copied to the host first)
    as the command line would write them: ([FinalRow], [AltRow]) -- format_final / format_alt of these are the text of
    <out>.tsv / <out>_alt.tsv.  read_names: the job's reads in submit order; keys: Stream.keys().  The _alt list is
    empty without second_best (alt None).

    This is the host route, a Python loop over every row and key.  The same bytes without it: lib.format_final_device /
    Stream.collect_final_text_device format a DeviceFinalRows on its device (lib.format_raw_device / collect_text_device:
    a DeviceRows), lib.format_final_host / format_raw_host are the compiled host twin."""
    if hasattr(final, "n_rows") and hasattr(final.rows, "cpu"):   # a lib.DeviceFinalRows: copied to the host first
        final = final.to_host()
    rows, _, alt = final
    name = lambda k: keys[k] if k >= 0 else "None"   # noqa: E731
    fin, alts = [], []
    for i, r in enumerate(rows.tolist()):
        read, start, end, best, second, hb, hs, ident, sid, hid, hsid, rel = r
        fin.append(FinalRow(read_names[read], keys[best], start, end, ident, name(second), sid, name(hb), hid, name(hs),
                            hsid, "+" if rel else "?"))
        if alt is not None:
            for k, v in enumerate(alt[i].tolist()):
                alts.append(AltRow(read_names[read], keys[k], start, end, v, k == best))
    return fin, alts


def by_read(rows):
    """Group consecutive rows by read name, preserving file order: [(read, [rows])]."""
    out = []
    for r in rows:
        if not out or out[-1][0] != r.read:
            out.append((r.read, []))
        out[-1][1].append(r)
    return out


# ---- binary record stream (<out>_raw.sdr) -------------------------------------------------------------
# Pure Python (struct only): a downstream tool needs neither the HIP library nor numpy to consume it.  The native
# reader / writer of the same bytes is sd_read_records / sd_write_records (lib.read_records / lib.write_records).
import struct

RECORDS_MAGIC = b"SDRECS1\n"
Records = namedtuple("Records", "scoring part_size overlap ed_thr templates reads")
"""scoring = (ins, del, mismatch, match); templates = names as in column 2 of the raw TSV (monomers, then monomers
+ "'"); reads = [(name, read_len or -1, [(template index, start, end, score), ...])] in file order."""


def _pad8(n):
    return (-n) & 7


def write_records(path, rec):
    """Records -> file.  Layout: csrc/sd_records.hpp."""
    head = bytearray(RECORDS_MAGIC)
    head += struct.pack("<II", 0, 0)
    head += struct.pack("<7i", *(list(rec.scoring) + [rec.part_size, rec.overlap, rec.ed_thr]))
    head += struct.pack("<I", len(rec.templates))
    for t in rec.templates:
        b = t.encode()
        head += struct.pack("<I", len(b)) + b
    head += b"\0" * _pad8(len(head))
    struct.pack_into("<I", head, 8, len(head))
    nt = len(rec.templates)
    total = 0
    with open(path, "wb") as f:
        f.write(head)
        for name, rlen, rows in rec.reads:
            b = name.encode()
            f.write(struct.pack("<IIqq", len(b), 0, -1 if rlen is None else int(rlen), len(rows)))
            f.write(b + b"\0" * _pad8(len(b)))
            for t, s, e, sc in rows:
                if not 0 <= t < nt:
                    raise ValueError("template index %d outside the template table" % t)
                f.write(struct.pack("<4i", t, s, e, int(sc)))
            total += len(rows)
        f.write(struct.pack("<IIqq", 0xFFFFFFFF, 0, len(rec.reads), total))


def read_records(path):
    """file -> Records; FormatError for anything that is not a complete, consistent record stream."""
    with open(path, "rb") as f:
        d = f.read()

    def bad(msg):
        return FormatError(str(path), 0, msg)

    if len(d) < 48 or d[:8] != RECORDS_MAGIC:
        raise bad("not a record stream (bad magic)")
    hb, _ = struct.unpack_from("<II", d, 8)
    v = struct.unpack_from("<7i", d, 16)
    (nt,) = struct.unpack_from("<I", d, 44)
    at = 48
    templates = []
    for _ in range(nt):
        if at + 4 > len(d):
            raise bad("truncated template table")
        (l,) = struct.unpack_from("<I", d, at)
        at += 4
        if at + l > len(d):
            raise bad("truncated template table")
        templates.append(d[at:at + l].decode())
        at += l
    at += _pad8(at)
    if at != hb or hb > len(d):
        raise bad("header size does not match the template table")
    reads, total = [], 0
    while True:
        if at + 8 > len(d):
            raise bad("truncated: no trailer (the writer did not finish)")
        nl, _ = struct.unpack_from("<II", d, at)
        at += 8
        if nl == 0xFFFFFFFF:
            if at + 16 > len(d):
                raise bad("truncated trailer")
            nr, nrow = struct.unpack_from("<qq", d, at)
            at += 16
            if nr != len(reads) or nrow != total:
                raise bad("trailer totals do not match the read blocks")
            if at != len(d):
                raise bad("bytes after the trailer")
            return Records(tuple(v[:4]), v[4], v[5], v[6], templates, reads)
        if at + 16 > len(d):
            raise bad("truncated read block")
        rlen, n = struct.unpack_from("<qq", d, at)
        at += 16
        if n < 0 or at + nl > len(d):
            raise bad("truncated read block")
        name = d[at:at + nl].decode()
        at += nl + _pad8(nl)
        if at + 16 * n > len(d):
            raise bad("truncated read block")
        flat = struct.unpack_from("<%di" % (4 * n), d, at)
        at += 16 * n
        rows = [tuple(flat[4 * i:4 * i + 4]) for i in range(n)]
        for r in rows:
            if not 0 <= r[0] < nt:
                raise bad("record with a template index outside the template table")
        reads.append((name, rlen, rows))
        total += n


def records_to_raw_rows(rec):
    """Records -> [RawRow] exactly as SaveBatch derives them (gap from the previous end of the same read, length)."""
    out = []
    for name, _, rows in rec.reads:
        out.extend(raw_rows(name, [(rec.templates[t], s, e, sc) for t, s, e, sc in rows]))
    return out


def records_to_raw_tsv(rec):
    """Records -> the text of <out>_raw.tsv (main.cpp:272-285)."""
    return format_raw(records_to_raw_rows(rec))


def raw_to_records(rows, templates, scoring=(-1, -1, -1, 1), part_size=5000, overlap=500, ed_thr=-1, read_lens=None):
    """[RawRow] (+ the template names in the DP's order: monomers, then monomers + "'") -> Records.  A repeated template
    name maps to its first index, which is what the raw TSV can tell."""
    idx = {}
    for i, t in enumerate(templates):
        idx.setdefault(t, i)
    reads = []
    for name, rr in by_read(rows):
        reads.append((name, -1 if read_lens is None else read_lens.get(name, -1),
                      [(idx[r.monomer], r.start, r.end, int(r.score)) for r in rr]))
    return Records(tuple(scoring), part_size, overlap, ed_thr, list(templates), reads)


# ---- column profiles (--profile) -------------------------------------------------------------------------------------
PROFILE_COLUMNS = ("A", "C", "G", "T", "N", "del", "ins_n", "insA", "insC", "insG", "insT", "insN")
PROFILE_NCOLS = len(PROFILE_COLUMNS)
PROFILE_HEADER = "name\tg\tref\tn\t" + "\t".join(PROFILE_COLUMNS) + "\n"
# names, seqs (forward monomers, FASTA order) and counts: per monomer an int64 array [len(seq) + 1, PROFILE_NCOLS] (or,
# from lib.last_run_profile(numpy=False), the same rows as lists of ints -- every function below takes either)
Profile = namedtuple("Profile", "names seqs counts")


def split_counts(lens, flat, numpy=True):
    """The flat counter vector of the C-ABI (monomer after monomer, (L + 1) x 12 each) -> a list of [L + 1, 12] arrays
    (numpy=False: lists of row lists)."""
    out, at = [], 0
    for L in lens:
        k = (int(L) + 1) * PROFILE_NCOLS
        if numpy:
            import numpy as np
            out.append(np.asarray(flat[at:at + k], dtype=np.int64).reshape(int(L) + 1, PROFILE_NCOLS))
        else:
            out.append([[int(v) for v in flat[at + g * PROFILE_NCOLS:at + (g + 1) * PROFILE_NCOLS]] for g in range(int(L) + 1)])
        at += k
    return out


def profile_from_counts(names, seqs, flat, numpy=True):
    return Profile(list(names), list(seqs), split_counts([len(x) for x in seqs], flat, numpy=numpy))


def profile_instances(c):
    """n of one monomer's counters: the instances (NW is global, so A..del sum to n at every position)."""
    return sum(int(v) for v in c[0][:6]) if len(c) > 1 else 0


def format_profile(prof):
    out = [PROFILE_HEADER]
    for name, seq, c in zip(prof.names, prof.seqs, prof.counts):
        n = profile_instances(c)
        for g in range(len(seq) + 1):
            ref = seq[g] if g < len(seq) else "-"
            out.append("%s\t%d\t%s\t%d\t%s\n" % (name, g, ref, n, "\t".join(str(int(v)) for v in c[g])))
    return "".join(out)


def write_profile(path, prof):
    with open(path, "w") as f:
        f.write(format_profile(prof))


def read_profile(path):
    """<out>_profile.tsv -> Profile (the sequences are rebuilt from the ref column)."""
    import numpy as np
    names, seqs, rows = [], [], []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            if lineno == 1 and line == PROFILE_HEADER:
                continue
            x = line.rstrip("\n").split("\t")
            if len(x) != 4 + PROFILE_NCOLS:
                raise FormatError(path, lineno, "expected %d columns, got %d" % (4 + PROFILE_NCOLS, len(x)))
            if int(x[1]) == 0:
                names.append(x[0])
                seqs.append([])
                rows.append([])
            elif not names or x[0] != names[-1] or int(x[1]) != len(rows[-1]):
                raise FormatError(path, lineno, "rows of a monomer must run g = 0, 1, ..., L")
            if x[2] != "-":
                seqs[-1].append(x[2])
            rows[-1].append([int(v) for v in x[4:]])
    return Profile(names, ["".join(q) for q in seqs], [np.asarray(r, dtype=np.int64).reshape(-1, PROFILE_NCOLS) for r in rows])


def _argmax_first(vals):
    best = 0
    for i in range(1, len(vals)):
        if vals[i] > vals[best]:
            best = i
    return best


def consensus(prof):
    """[(name, n, sequence)]: per slot g = 0..L, the most frequent inserted base when more than half of the instances
    insert there (ties: first of ACGTN), then for g < L the most frequent of A C G T N del (ties: the monomer's own
    base if it is among them, else the first in that order; del emits nothing).  n = 0 keeps the monomer's sequence."""
    out = []
    for name, seq, c in zip(prof.names, prof.seqs, prof.counts):
        n = profile_instances(c)
        if n == 0:
            out.append((name, 0, seq))
            continue
        s = []
        for g in range(len(seq) + 1):
            row = [int(x) for x in c[g]]
            if 2 * row[6] > n:
                s.append("ACGTN"[_argmax_first(row[7:12])])
            if g == len(seq):
                break
            v = row[:6]
            top = max(v)
            r = "ACGTN".find(seq[g])
            k = r if r >= 0 and v[r] == top else v.index(top)
            if k < 5:
                s.append("ACGTN"[k])
        out.append((name, n, "".join(s)))
    return out


def format_consensus(prof):
    return "".join(">%s instances=%d\n%s\n" % (name, n, sq) for name, n, sq in consensus(prof))


def write_consensus(path, prof):
    with open(path, "w") as f:
        f.write(format_consensus(prof))


# ---- one row per instance (--msa) ------------------------------------------------------------------------------------
MSA_DEL, MSA_NONE = 5, 7            # SD_MSA_DEL, SD_MSA_NONE (include/sd_hip.h)
MSA_COLUMNS = ("A", "C", "G", "T", "N", "del", "ins_n", "ins_bases")
MSA_HEADER = "read\tstart\tend\tmonomer\tcolumns\tinsertions\n"
_MSA_CHARS = "ACGTN-?."             # the column byte -> its character ('.' = MSA_NONE)
# rows: the flat bytes of the C-ABI (uint8), row_at: n + 1 offsets, status: n bytes (0 no instance, 1 computed, 2 left
# out by a device-resident call), tlen: the lengths of the FORWARD monomers.  Pair i against interleaved template il
# owns rows[row_at[i]:row_at[i + 1]]: tlen[il >> 1] column bytes, then tlen[il >> 1] + 1 insertion counts, then padding.
Msa = namedtuple("Msa", "rows row_at status tlen")
MsaRow = namedtuple("MsaRow", "read start end monomer columns insertions")   # a line of <out>_msa.tsv; insertions: ((slot, count), ...)


def msa_pitch(L):
    """SD_MSA_PITCH: the bytes of a row of a monomer of L bases."""
    return (2 * int(L) + 1 + 15) & ~15


def msa_row(msa, i, il):
    """(columns [L], insertions [L + 1]) of pair i (uint8 views)."""
    L = int(msa.tlen[int(il) >> 1])
    at = int(msa.row_at[i])
    return msa.rows[at:at + L], msa.rows[at + L:at + 2 * L + 1]


def msa_matrix(msa, pair_tmpl, m):
    """The [n, L] column matrix of monomer m's computed rows (either orientation), in the pairs' order."""
    import numpy as np
    L = int(msa.tlen[m])
    pick = [i for i, il in enumerate(pair_tmpl) if int(il) >> 1 == m and int(msa.status[i]) == 1]
    out = np.zeros((len(pick), L), dtype=np.uint8)
    for k, i in enumerate(pick):
        out[k] = msa_row(msa, i, pair_tmpl[i])[0]
    return out


def msa_counts(msa, pair_tmpl, n_mono):
    """The computed rows summed per monomer: a list of int64 [L + 1, 8] arrays (MSA_COLUMNS) -- columns 0..6 are those
    of the job's profile, ins_bases the sum of its columns 7..11 wherever no row's count saturated."""
    import numpy as np
    out = [np.zeros((int(msa.tlen[m]) + 1, len(MSA_COLUMNS)), dtype=np.int64) for m in range(n_mono)]
    for i, il in enumerate(pair_tmpl):
        if int(msa.status[i]) != 1:
            continue
        c = out[int(il) >> 1]
        col, ins = msa_row(msa, i, il)
        L = len(col)
        np.add.at(c, (np.arange(L), col.astype(np.int64)), 1)
        c[:, 6] += ins > 0
        c[:, 7] += ins
    return out


def msa_rows(msa, pair_tmpl, meta):
    """The lines of <out>_msa.tsv: meta = (read, start, end, monomer) per pair."""
    out = []
    for i, (il, (read, start, end, monomer)) in enumerate(zip(pair_tmpl, meta)):
        col, ins = msa_row(msa, i, il)
        if int(msa.status[i]) != 1:
            out.append(MsaRow(read, int(start), int(end), monomer, "." * len(col), ()))
            continue
        out.append(MsaRow(read, int(start), int(end), monomer, "".join(_MSA_CHARS[v] for v in col.tolist()),
                          tuple((g, v) for g, v in enumerate(ins.tolist()) if v)))
    return out


def msa_from_rows(rows, mono_names, mono_lens):
    """The inverse of msa_rows: lines of <out>_msa.tsv -> (Msa, pair_tmpl).  A name with a trailing ' is the reverse
    complement's: its line is already on the forward monomer."""
    import numpy as np
    idx = {}
    for m, n in enumerate(mono_names):
        idx[n], idx[n + "'"] = 2 * m, 2 * m + 1
    pt = [idx[r.monomer] for r in rows]
    at = np.zeros(len(rows) + 1, dtype=np.int64)
    for i, il in enumerate(pt):
        at[i + 1] = at[i] + msa_pitch(mono_lens[il >> 1])
    data = np.zeros(int(at[-1]), dtype=np.uint8)
    status = np.zeros(len(rows), dtype=np.uint8)
    for i, (r, il) in enumerate(zip(rows, pt)):
        L = int(mono_lens[il >> 1])
        if len(r.columns) != L:
            raise ValueError("row %d: %d columns for a monomer of %d bases" % (i, len(r.columns), L))
        o = int(at[i])
        data[o:o + L] = [_MSA_CHARS.index(ch) for ch in r.columns]
        status[i] = 0 if r.columns == "." * L and L > 0 else 1
        for g, v in r.insertions:
            data[o + L + g] = v
    return Msa(data, at, status, [int(x) for x in mono_lens]), pt


def format_msa(rows, header=True):
    return (MSA_HEADER if header else "") + "".join("%s\t%d\t%d\t%s\t%s\t%s\n" % (
        r.read, r.start, r.end, r.monomer, r.columns, ",".join("%d:%d" % x for x in r.insertions) or ".") for r in rows)


def write_msa(path, rows):
    with open(path, "w") as f:
        f.write(format_msa(rows))


def _msa_ins(x):
    if x == ".":
        return ()
    out = []
    for item in x.split(","):
        g, v = item.split(":")
        out.append((int(g), int(v)))
    return tuple(out)


def read_msa(path):
    """<out>_msa.tsv -> [MsaRow]."""
    out = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            if lineno == 1 and line == MSA_HEADER:
                continue
            x = line.rstrip("\n").split("\t")
            if len(x) != 6:
                raise FormatError(path, lineno, "expected 6 columns, got %d" % len(x))
            try:
                if x[4].strip("ACGTN-") and x[4] != "." * len(x[4]):
                    raise ValueError("columns must be over ACGTN- or all '.', found %r" % x[4])
                out.append(MsaRow(x[0], int(x[1]), int(x[2]), x[3], x[4], _msa_ins(x[5])))
            except ValueError as e:
                raise FormatError(path, lineno, str(e))
    return out


# ---- lags -----------------------------------------------------------------------------------------
# --lags D: <out>_lags.tsv, one line per row of <out>.tsv -- read, start, end, then the identity of the row's segment (the
# query) to that of each of its next D neighbours in the same read (the target), "-1.00" where the read ends first -- and
# <out>_period.tsv, one line per read -- read, rows, period, then the D pooled identities (sum of matches / sum of columns
# over the read's pairs at that lag, "-1.00" for a lag without pairs).  No headers; D is the number of identity columns.
Lags = namedtuple("Lags", "dist matches sums")
"""lib.lag_segments / final_lags_host / DeviceLags.to_host(): dist, matches = int32 [n, D] (dist -1: no partner, -2: left out
by a device-resident call), sums = int64 [groups, D, 3] = (pairs, sum of matches, sum of dist + matches)."""
LagRow = namedtuple("LagRow", "read start end identities")          # a line of <out>_lags.tsv
PeriodRow = namedtuple("PeriodRow", "read rows period identities")  # a line of <out>_period.tsv
# (the identities of a Lags: lib.lag_identities(dist, matches); periods and pooled identities: lib.lag_periods(sums))


def lag_period(sums):
    """The period of a read from its sums ([D][3] = pairs, sum of matches, sum of columns per lag): the lag with the largest
    pooled identity M / C among the lags with pairs, compared as integers (M1 * C2 > M2 * C1, never in floating point), ties
    to the smallest lag; 0 when no lag has a pair.  A [groups][D][3] array gives a list."""
    rows = sums.tolist() if hasattr(sums, "tolist") else sums
    if rows and rows[0] and isinstance(rows[0][0], (list, tuple)):
        return [lag_period(r) for r in rows]
    best = 0
    for d, (n, m, c) in enumerate(rows, 1):
        if n <= 0 or c <= 0:
            continue
        if best == 0 or int(m) * int(rows[best - 1][2]) > int(rows[best - 1][1]) * int(c):
            best = d
    return best


def format_lags(rows):
    f2 = "{:.2f}".format
    return "".join("%s\t%d\t%d\t%s\n" % (r.read, r.start, r.end, "\t".join(f2(v) for v in r.identities)) for r in rows)


def format_periods(rows):
    f2 = "{:.2f}".format
    return "".join("%s\t%d\t%d\t%s\n" % (r.read, r.rows, r.period, "\t".join(f2(v) for v in r.identities)) for r in rows)


def write_lags(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_lags(rows))


def write_periods(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_periods(rows))


def _read_lag_file(path, make):
    out = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            x = line.rstrip("\n").split("\t")
            if len(x) < 4 or (out and len(x) != 3 + len(out[0].identities)):
                raise FormatError(path, lineno, "expected 3 columns and the same number of identities on every line, got %d" % len(x))
            try:
                out.append(make(x[0], int(x[1]), int(x[2]), tuple(float(v) for v in x[3:])))
            except ValueError as e:
                raise FormatError(path, lineno, str(e))
    return out


def read_lags(path):
    """<out>_lags.tsv -> [LagRow]."""
    return _read_lag_file(path, LagRow)


def read_periods(path):
    """<out>_period.tsv -> [PeriodRow]."""
    return _read_lag_file(path, PeriodRow)


# ---- heatmap --------------------------------------------------------------------------------------
# --heatmap B[,W]: <out>_heatmap.tsv, one line per cell with pairs -- read, bin_i, bin_j (bin_i <= bin_j), start and end of
# bin i (the start of its first row, the end of its last row, as <out>.tsv prints them), start and end of bin j, the number
# of pairs, and their pooled identity (sum of matches / sum of columns, "%.2f").  Lines in the order read, bin_i, bin_j.
class Heat:
    """lib.heat_segments / final_heat_host / DeviceHeat.to_host(): sums = int64 [cells, 3] = (pairs, sum of matches, sum of
    dist + matches) per cell; group g owns nb[g] bins of B rows and the cells cell_off[g] .. cell_off[g + 1], the row-major
    upper triangle of its nb x nb bins: cell (I, J), I <= J, at I * nb - I * (I - 1) // 2 + (J - I).  W: the largest row
    distance of a pair, 0 = no limit.  classes (where the call counts them): (kernel pairs, host pairs, pairs with an
    empty side)."""

    def __init__(self, sums, cell_off, nb, B, W=0):
        self.sums, self.cell_off, self.nb, self.B, self.W = sums, cell_off, nb, int(B), int(W)
        self.classes = None

    def index(self, g, I, J):
        nb = int(self.nb[g])
        if not 0 <= I <= J < nb:
            raise IndexError("cell (%d, %d) of a group of %d bins" % (I, J, nb))
        return int(self.cell_off[g]) + I * nb - I * (I - 1) // 2 + (J - I)

    def cell(self, g, I, J):
        """(pairs, sum of matches, sum of dist + matches) of cell (I, J), I <= J, of group g, as Python integers"""
        return tuple(int(v) for v in self.sums[self.index(g, I, J)])

    def matrix(self, g):
        """dense nb x nb float64 array of the pooled identities in percent of group g, the upper triangle mirrored, nan
        where a cell has no pair"""
        import numpy as np
        nb = int(self.nb[g])
        out = np.full((nb, nb), np.nan, dtype=np.float64)
        for I in range(nb):
            for J in range(I, nb):
                n, m, c = self.cell(g, I, J)
                if n > 0 and c > 0:
                    out[I, J] = out[J, I] = heat_pooled(m, c)
        return out


HeatRow = namedtuple("HeatRow", "read bin_i bin_j start_i end_i start_j end_j pairs identity")   # a line of <out>_heatmap.tsv


def heat_pooled(m, c):
    """the identity column's arithmetic on the sums of a cell: 0.0 + m, / c, * 100 in doubles"""
    a = 0.0
    a += m
    a /= c
    return a * 100


def heat_rows(heat, g, read, rows):
    """The HeatRows of group g of a Heat: rows = the group's (start, end) pairs in row order; cells without pairs are left out"""
    out = []
    nb, B = int(heat.nb[g]), heat.B
    for I in range(nb):
        for J in range(I, nb):
            n, m, c = heat.cell(g, I, J)
            if n > 0:
                out.append(HeatRow(read, I, J, rows[I * B][0], rows[min((I + 1) * B, len(rows)) - 1][1], rows[J * B][0],
                                   rows[min((J + 1) * B, len(rows)) - 1][1], n, heat_pooled(m, c) if c > 0 else -1.0))
    return out


def format_heatmap(rows):
    return "".join("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\n" % tuple(r) for r in rows)


def write_heatmap(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_heatmap(rows))


def read_heatmap(path):
    """<out>_heatmap.tsv -> [HeatRow]."""
    out = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            x = line.rstrip("\n").split("\t")
            if len(x) != 9:
                raise FormatError(path, lineno, "expected 9 columns, got %d" % len(x))
            try:
                out.append(HeatRow(x[0], *[int(v) for v in x[1:8]], float(x[8])))
            except ValueError as e:
                raise FormatError(path, lineno, str(e))
    return out


# ---- autocorr -------------------------------------------------------------------------------------
# --autocorr K[,D]: <out>_autocorr.tsv, one line per (read, window) -- read, start, end (the window's bases [start, end),
# 0-based), k, period (the lag of the first peak, 0 = none), count (hits at the period), positions (the i of the window that
# could be a hit at the period), then up to P further columns lag:count, the peaks in their order.  Lines in the order
# read, window.  <out>_autocorr_spectrum.tsv (--autocorr-spectrum): read, start, end, lag, count, positions for every lag
# of every window with count > 0, in the order read, window, lag.
class Autocorr:
    """lib.autocorr / DeviceAutocorr.to_host(): counts = int64 [windows, D], counts[w, d - 1] = the hits at lag d whose first
    position lies in window w (include/sd_hip.h: sd_autocorr_*); read r owns the windows win_off[r] .. win_off[r + 1], window
    w covers the bases [win_start[w], win_end[w]) of its read; k: the k-mer length."""

    def __init__(self, counts, win_off, win_start, win_end, k):
        self.counts, self.win_off, self.win_start, self.win_end, self.k = counts, win_off, win_start, win_end, int(k)

    @property
    def D(self):
        return int(self.counts.shape[1])

    def windows(self, r):
        return range(int(self.win_off[r]), int(self.win_off[r + 1]))

    def spectrum(self, r):
        """the whole-read spectrum of read r: the sum of its windows, int64 [D]"""
        return self.counts[int(self.win_off[r]):int(self.win_off[r + 1])].sum(axis=0)


AutocorrRow = namedtuple("AutocorrRow", "read start end k period count positions peaks")   # a line of <out>_autocorr.tsv
AutocorrSpectrumRow = namedtuple("AutocorrSpectrumRow", "read start end lag count positions")   # ... of <out>_autocorr_spectrum.tsv


def format_autocorr(rows):
    return "".join("%s\t%d\t%d\t%d\t%d\t%d\t%d%s\n" % (tuple(r)[:7] + ("".join("\t%d:%d" % tuple(p) for p in r.peaks),)) for r in rows)


def write_autocorr(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_autocorr(rows))


def read_autocorr(path):
    """<out>_autocorr.tsv -> [AutocorrRow]; peaks = a tuple of (lag, count)."""
    out = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            x = line.rstrip("\n").split("\t")
            if len(x) < 7:
                raise FormatError(path, lineno, "expected at least 7 columns, got %d" % len(x))
            try:
                peaks = []
                for p in x[7:]:
                    lag, _, count = p.partition(":")
                    peaks.append((int(lag), int(count)))
                out.append(AutocorrRow(x[0], *[int(v) for v in x[1:7]], tuple(peaks)))
            except ValueError as e:
                raise FormatError(path, lineno, str(e))
    return out


def format_autocorr_spectrum(rows):
    return "".join("%s\t%d\t%d\t%d\t%d\t%d\n" % tuple(r) for r in rows)


def write_autocorr_spectrum(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_autocorr_spectrum(rows))


def read_autocorr_spectrum(path):
    """<out>_autocorr_spectrum.tsv -> [AutocorrSpectrumRow]."""
    out = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            x = line.rstrip("\n").split("\t")
            if len(x) != 6:
                raise FormatError(path, lineno, "expected 6 columns, got %d" % len(x))
            try:
                out.append(AutocorrSpectrumRow(x[0], *[int(v) for v in x[1:]]))
            except ValueError as e:
                raise FormatError(path, lineno, str(e))
    return out


# ---- dotplot --------------------------------------------------------------------------------------
# --dotplot W[,B]: <out>_dotplot.tsv, one line per cell (i, j), j <= i, of a read's windows of W bases whose shared or
# shared_rc is not 0, no header -- read, start_i, end_i, start_j, end_j (the windows' bases, 0-based, end exclusive),
# kmers_i, kmers_j (distinct selected k-mers of the two windows), shared (those in both), identity; with --dotplot-rc
# kmers_rc_j, shared_rc, identity_rc follow (the k-mers of window i whose reverse complement lies in window j).  Lines in
# the order read, i, j.  The identity is the one conversion below, printed %.2f.
def dotplot_identity(shared, a, b, k):
    """100 * (shared / min(a, b)) ** (1 / k): containment of the smaller set turned into a per-base identity, the conversion
    ModDotPlot uses; 0 when nothing is shared"""
    return 100.0 * (shared / min(a, b)) ** (1.0 / k) if shared > 0 else 0.0


def dotplot_reaches(shared, a, b, k, P):
    """dotplot_identity(shared, a, b, k) >= P, decided in integers: shared * 100^k >= P^k * min(a, b)"""
    return P <= 0 or (shared > 0 and shared * 100 ** k >= P ** k * min(a, b))


class Dotplot:
    """lib.dotplot / DeviceDotplot.to_host(): kmers, kmers_rc = int32 [windows], shared, shared_rc = int32 [cells] (the two
    reverse-strand arrays None without rc); read r owns the windows win_off[r] .. win_off[r + 1] and the cells
    cell_off[r] .. cell_off[r + 1], ordered by i, then j, j = max(0, i - B) .. i when B > 0, j = 0 .. i otherwise
    (include/sd_hip.h: sd_dotplot_*)."""

    def __init__(self, kmers, kmers_rc, shared, shared_rc, win_off, cell_off, read_lens, k, W, B=0, M=1):
        self.kmers, self.kmers_rc, self.shared, self.shared_rc = kmers, kmers_rc, shared, shared_rc
        self.win_off, self.cell_off, self.read_lens = win_off, cell_off, read_lens
        self.k, self.W, self.B, self.M = int(k), int(W), int(B), int(M)

    @property
    def rc(self):
        return self.shared_rc is not None

    def n_windows(self, r):
        return int(self.win_off[r + 1] - self.win_off[r])

    def first(self, i):
        """the smallest j of row i"""
        return max(0, i - self.B) if self.B > 0 else 0

    def cell(self, r, i, j):
        """the index of the cell (i, j) of read r in shared / shared_rc"""
        B = self.B
        if not 0 <= i < self.n_windows(r) or not self.first(i) <= j <= i:
            raise IndexError("read %d has no cell (%d, %d)" % (r, i, j))
        before = i * (i + 1) // 2 if B <= 0 or i <= B + 1 else (B + 1) * (B + 2) // 2 + (i - B - 1) * (B + 1)
        return int(self.cell_off[r]) + before + j - self.first(i)

    def matrix(self, r, rc=False):
        """int32 [nw, nw]: shared (rc: shared_rc) of read r at [i, j], j <= i; -1 where there is no cell"""
        import numpy as np
        nw = self.n_windows(r)
        out = np.full((nw, nw), -1, dtype=np.int32)
        src = self.shared_rc if rc else self.shared
        for i in range(nw):
            a = self.cell(r, i, self.first(i))
            out[i, self.first(i):i + 1] = src[a:a + i - self.first(i) + 1]
        return out


DotplotRow = namedtuple("DotplotRow", "read start_i end_i start_j end_j kmers_i kmers_j shared identity kmers_rc_j shared_rc identity_rc")


def dotplot_rows(dp, names, min_identity=0):
    """The lines of <out>_dotplot.tsv for a Dotplot -> [DotplotRow] (the last three fields None without rc): the cells whose
    shared or shared_rc is not 0 and, with min_identity = P > 0, one of whose identities reaches P (dotplot_reaches)."""
    out = []
    k, W, P = dp.k, dp.W, int(min_identity)
    for r, name in enumerate(names):
        n, w0, at = int(dp.read_lens[r]), int(dp.win_off[r]), int(dp.cell_off[r])
        for i in range(dp.n_windows(r)):
            ki = int(dp.kmers[w0 + i])
            for j in range(dp.first(i), i + 1):
                s, kj = int(dp.shared[at]), int(dp.kmers[w0 + j])
                s2, kr = (int(dp.shared_rc[at]), int(dp.kmers_rc[w0 + j])) if dp.rc else (0, 0)
                at += 1
                if (s == 0 and s2 == 0) or not (dotplot_reaches(s, ki, kj, k, P) or (dp.rc and dotplot_reaches(s2, ki, kr, k, P))):
                    continue
                tail = (kr, s2, dotplot_identity(s2, ki, kr, k)) if dp.rc else (None, None, None)
                out.append(DotplotRow(name, i * W, min(n, (i + 1) * W), j * W, min(n, (j + 1) * W), ki, kj, s,
                                      dotplot_identity(s, ki, kj, k), *tail))
    return out


def format_dotplot(rows):
    return "".join(("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f" % tuple(r)[:9]) + ("\t%d\t%d\t%.2f" % tuple(r)[9:] if r.shared_rc is not None else "") + "\n"
                   for r in rows)


def write_dotplot(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_dotplot(rows))


def read_dotplot(path):
    """<out>_dotplot.tsv -> [DotplotRow]; the identities as printed."""
    with open(path) as f:
        return read_dotplot_text(f.read(), path)


def read_dotplot_text(text, path="<text>"):
    """the text of an <out>_dotplot.tsv (format_dotplot) -> [DotplotRow]"""
    out = []
    for lineno, line in enumerate(text.splitlines(), 1):
        x = line.split("\t")
        if len(x) not in (9, 12):
            raise FormatError(path, lineno, "expected 9 or 12 columns, got %d" % len(x))
        try:
            tail = (int(x[9]), int(x[10]), float(x[11])) if len(x) == 12 else (None, None, None)
            out.append(DotplotRow(x[0], *[int(v) for v in x[1:8]], float(x[8]), *tail))
        except ValueError as e:
            raise FormatError(path, lineno, str(e))
    return out


# ---- subfamilies (--split) -------------------------------------------------------------------------
# --split P[,K]: <out>_split.tsv, one line per row of <out>.tsv in its order, no header -- read, start, end, monomer (as
# printed there), subfamily ("<name>.<j>" on the forward monomer's name, '*' for a row that is no instance), d1 (columns
# in which the row differs from its subfamily's centre), d2 (from the nearest other centre; -1: none, or no instance),
# columns (as in <out>_msa.tsv).  <out>_split_summary.tsv, one line per subfamily, integers -- monomer, subfamily, size,
# sum of d1, largest d1, nearest (the other subfamily of the monomer whose centre is closest, '*' when alone), distance
# (the columns in which the two centres differ, -1 when alone).  <out>_split_monomers.fa: a monomer file.
Split = namedtuple("Split", "centres assign d1 d2 sizes rounds iters")
"""lib.split_rows / split_msa: centres = uint8 [k, L] (0..4 = A C G T N, 5 = deleted), assign / d1 / d2 = int32 [n] per
member row in the given order (d2 -1: one centre), sizes = int32 [k], rounds and iters = the rounds and Lloyd iterations
that ran (csrc/sd_split.hpp)."""
SplitRow = namedtuple("SplitRow", "read start end monomer subfamily d1 d2 columns")            # a line of <out>_split.tsv
SplitSummaryRow = namedtuple("SplitSummaryRow", "monomer subfamily size sum_d1 max_d1 nearest distance")   # ... of <out>_split_summary.tsv


def split_members(msa, pair_tmpl, m):
    """The pairs that are members of forward monomer m, in order: status 1 and either strand of m."""
    return [i for i, il in enumerate(pair_tmpl) if int(il) >> 1 == m and int(msa.status[i]) == 1]


def split_rows(msa, pair_tmpl, mono_names, splits, meta):
    """The lines of <out>_split.tsv: splits = one Split per forward monomer over split_members, meta = (read, start, end,
    monomer) per pair."""
    sub, d1, d2 = {}, {}, {}
    for m, sp in enumerate(splits):
        for x, i in enumerate(split_members(msa, pair_tmpl, m)):
            sub[i], d1[i], d2[i] = "%s.%d" % (mono_names[m], int(sp.assign[x])), int(sp.d1[x]), int(sp.d2[x])
    out = []
    for i, (il, (read, start, end, monomer)) in enumerate(zip(pair_tmpl, meta)):
        col = msa_row(msa, i, il)[0]
        if i in sub:
            out.append(SplitRow(read, int(start), int(end), monomer, sub[i], d1[i], d2[i], "".join(_MSA_CHARS[v] for v in col.tolist())))
        else:
            out.append(SplitRow(read, int(start), int(end), monomer, "*", -1, -1, "." * len(col)))
    return out


def format_split(rows):
    return "".join("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\n" % tuple(r) for r in rows)


def write_split(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_split(rows))


def read_split(path):
    """<out>_split.tsv -> [SplitRow]."""
    out = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            x = line.rstrip("\n").split("\t")
            if len(x) != 8:
                raise FormatError(path, lineno, "expected 8 columns, got %d" % len(x))
            try:
                if x[7].strip("ACGTN-") and x[7] != "." * len(x[7]):
                    raise ValueError("columns must be over ACGTN- or all '.', found %r" % x[7])
                out.append(SplitRow(x[0], int(x[1]), int(x[2]), x[3], x[4], int(x[5]), int(x[6]), x[7]))
            except ValueError as e:
                raise FormatError(path, lineno, str(e))
    return out


def split_summary(mono_names, splits):
    """The lines of <out>_split_summary.tsv -> [SplitSummaryRow]; the nearest other centre, ties to the smallest index."""
    out = []
    for name, sp in zip(mono_names, splits):
        k = len(sp.centres)
        for j in range(k):
            mine = [int(v) for v, a in zip(sp.d1, sp.assign) if int(a) == j]
            best, at = -1, -1
            for o in range(k):
                if o != j:
                    h = int((sp.centres[j] != sp.centres[o]).sum())
                    if at < 0 or h < best:
                        best, at = h, o
            out.append(SplitSummaryRow(name, "%s.%d" % (name, j), len(mine), sum(mine), max(mine) if mine else 0,
                                       "%s.%d" % (name, at) if at >= 0 else "*", best))
    return out


def format_split_summary(rows):
    return "".join("%s\t%s\t%d\t%d\t%d\t%s\t%d\n" % tuple(r) for r in rows)


def write_split_summary(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_split_summary(rows))


def read_split_summary(path):
    """<out>_split_summary.tsv -> [SplitSummaryRow]."""
    out = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            x = line.rstrip("\n").split("\t")
            if len(x) != 7:
                raise FormatError(path, lineno, "expected 7 columns, got %d" % len(x))
            try:
                out.append(SplitSummaryRow(x[0], x[1], int(x[2]), int(x[3]), int(x[4]), x[5], int(x[6])))
            except ValueError as e:
                raise FormatError(path, lineno, str(e))
    return out


# ---- higher-order repeat units (--hor; csrc/sd_hor.hpp holds the rule) ------------------------------------------------
Hor = namedtuple("Hor", "T rows hor pos kinds lens long row_unit units")
"""lib.hor_rows / final_hor_host: T = int64 [M, M] transitions, rows = int64 [M] usable rows per monomer, hor / pos = int32
[M] the order (0-based, -1: none) and position (1-based, 0: none) of a monomer, kinds (0 cycle, 1 path) / lens per order,
long = [(first monomer, length)] of the orders too long to number, row_unit = int32 [n_rows] (-1: in no unit), units = a
numpy array of lib.hor_unit_dtype() (first_row, start, end, mask, read, n_rows, order, strand)."""
HorUnitRow = namedtuple("HorUnitRow", "read start end strand order name rows complete")        # a line of <out>_hor.tsv
HorOrderRow = namedtuple("HorOrderRow", "order kind length position monomer rows count")       # ... of <out>_hor_orders.tsv
HorVariantRow = namedtuple("HorVariantRow", "order name units rows bases")                     # ... of <out>_hor_variants.tsv
HOR_KINDS = ("cycle", "path")


def hor_mask_name(mask):
    """The name of a unit's mask: the positions present (bit pos - 1), ascending, as ranges joined by '_'."""
    out, p, mask = [], 1, int(mask)
    while mask >> (p - 1):
        if not (mask >> (p - 1)) & 1:
            p += 1
            continue
        q = p
        while (mask >> q) & 1:
            q += 1
        out.append("%d-%d" % (p, q) if q > p else "%d" % p)
        p = q + 1
    return "_".join(out)


def hor_mask_of(name):
    """The mask of a name (the inverse of hor_mask_name)."""
    mask = 0
    for part in name.split("_"):
        lo, _, hi = part.partition("-")
        lo, hi = int(lo), int(hi or lo)
        if not 1 <= lo <= hi <= 64:
            raise ValueError("a range of positions must lie in 1 .. 64, found %r" % part)
        for p in range(lo, hi + 1):
            mask |= 1 << (p - 1)
    if hor_mask_name(mask) != name:
        raise ValueError("%r is not the name of a set of positions" % name)
    return mask


def hor_units(hor, read_names):
    """The lines of <out>_hor.tsv -> [HorUnitRow]; read_names: the reads by index."""
    lens = [int(x) for x in hor.lens]
    out = []
    for first_row, start, end, mask, read, n_rows, order, strand in hor.units.tolist():
        out.append(HorUnitRow(read_names[read], start, end, "-" if strand else "+", "H%d" % (order + 1), hor_mask_name(mask), n_rows,
                              1 if mask == (1 << lens[order]) - 1 else 0))
    return out


def hor_orders(hor, mono_names):
    """The lines of <out>_hor_orders.tsv -> [HorOrderRow]; count = T[monomer][the next position's], 0 at a path's end."""
    at = {}
    for m, (h, p) in enumerate(zip(hor.hor.tolist(), hor.pos.tolist())):
        if h >= 0:
            at[(h, p)] = m
    out = []
    for o, (kind, n) in enumerate(zip([int(x) for x in hor.kinds], [int(x) for x in hor.lens])):
        for p in range(1, n + 1):
            m = at[(o, p)]
            nxt = at[(o, p + 1)] if p < n else (at[(o, 1)] if kind == 0 else None)
            out.append(HorOrderRow("H%d" % (o + 1), HOR_KINDS[kind], n, p, mono_names[m], int(hor.rows[m]),
                                   int(hor.T[m][nxt]) if nxt is not None else 0))
    return out


def hor_variants(hor):
    """The lines of <out>_hor_variants.tsv -> [HorVariantRow]: per (order, mask) its units, rows and bases, sorted by order,
    then units descending, then mask ascending."""
    acc = {}
    for first_row, start, end, mask, read, n_rows, order, strand in hor.units.tolist():
        a = acc.setdefault((order, mask), [0, 0, 0])
        a[0] += 1
        a[1] += n_rows
        a[2] += end - start + 1
    keys = sorted(acc, key=lambda k: (k[0], -acc[k][0], k[1]))
    return [HorVariantRow("H%d" % (o + 1), hor_mask_name(mask), *acc[(o, mask)]) for o, mask in keys]


def format_hor(rows):
    return "".join("%s\t%d\t%d\t%s\t%s\t%s\t%d\t%d\n" % tuple(r) for r in rows)


def format_hor_orders(rows):
    return "".join("%s\t%s\t%d\t%d\t%s\t%d\t%d\n" % tuple(r) for r in rows)


def format_hor_variants(rows):
    return "".join("%s\t%s\t%d\t%d\t%d\n" % tuple(r) for r in rows)


def _write_text(path, text):
    with open(path, "w", newline="") as f:
        f.write(text)


def write_hor(path, rows):
    _write_text(path, format_hor(rows))


def write_hor_orders(path, rows):
    _write_text(path, format_hor_orders(rows))


def write_hor_variants(path, rows):
    _write_text(path, format_hor_variants(rows))


def _hor_order_name(x):
    if not (x.startswith("H") and x[1:].isdigit() and int(x[1:]) >= 1):
        raise ValueError("an order is H1, H2, ..., found %r" % x)
    return x


def _hor_name(x):
    hor_mask_of(x)
    return x


def _hor_choice(*allowed):
    def conv(x):
        if x not in allowed:
            raise ValueError("expected one of %s, found %r" % (", ".join(allowed), x))
        return x
    return conv


def read_hor(path):
    """<out>_hor.tsv -> [HorUnitRow]."""
    return _parse(path, False, 8, (_ident, int, int, _hor_choice("+", "-"), _hor_order_name, _hor_name, int, int), HorUnitRow)


def read_hor_orders(path):
    """<out>_hor_orders.tsv -> [HorOrderRow]."""
    return _parse(path, False, 7, (_hor_order_name, _hor_choice(*HOR_KINDS), int, int, _ident, int, int), HorOrderRow)


def read_hor_variants(path):
    """<out>_hor_variants.tsv -> [HorVariantRow]."""
    return _parse(path, False, 5, (_hor_order_name, _hor_name, int, int, int), HorVariantRow)


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def msa_inserted(msa, i, il, segment):
    """The bases a pair inserts, by slot, read back from its row and its stretch of the read (`segment`, as it stands in
    the read): {slot: bases} on the forward monomer.  None when the row does not say -- a saturated count (255), or a row
    that does not add up to the stretch."""
    col, ins = msa_row(msa, i, il)
    seg = segment if isinstance(segment, str) else segment.decode()
    if int(il) & 1:
        seg = "".join(_COMP.get(c, c) for c in reversed(seg))
    cols, counts = col.tolist(), ins.tolist()
    if max(counts) >= 255 or sum(counts) + sum(1 for v in cols if v != MSA_DEL) != len(seg):
        return None
    out, at = {}, 0
    for g in range(len(counts)):
        if counts[g]:
            out[g] = seg[at:at + counts[g]]
            at += counts[g]
        if g < len(cols) and cols[g] != MSA_DEL:
            at += 1
    return out


def split_profile(msa, pair_tmpl, m, name, seq, split, inserted=None):
    """The column profile of every subfamily of monomer m (Profile of "<name>.<j>", all with the monomer's sequence): per
    subfamily the msa_counts of its rows, columns 0..6 those of --profile; the inserted bases (columns 7..11) come from
    `inserted` = {pair: msa_inserted(...)}, for the pairs that insert."""
    import numpy as np
    L = int(msa.tlen[m])
    k = len(split.centres)
    counts = [np.zeros((L + 1, PROFILE_NCOLS), dtype=np.int64) for _ in range(k)]
    for x, i in enumerate(split_members(msa, pair_tmpl, m)):
        c = counts[int(split.assign[x])]
        col, ins = msa_row(msa, i, pair_tmpl[i])
        np.add.at(c, (np.arange(L), col.astype(np.int64)), 1)
        c[:, 6] += ins > 0
        for g, bases in ((inserted or {}).get(i) or {}).items():
            for ch in bases:
                c[g, 7 + "ACGTN".index(ch if ch in "ACGT" else "N")] += 1
    return Profile(["%s.%d" % (name, j) for j in range(k)], [seq] * k, counts)


def split_consensus(msa, pair_tmpl, m, name, seq, split, inserted=None):
    """[(subfamily name, rows, sequence)] of monomer m: the rule of consensus() on split_profile, so insertions are
    honoured as --profile honours them.  A monomer without instances: [("<name>.0", 0, seq)]."""
    if len(split.centres) == 0:
        return [("%s.0" % name, 0, seq)]
    return consensus(split_profile(msa, pair_tmpl, m, name, seq, split, inserted))


# ---- screen ---------------------------------------------------------------------------------------
ScreenRow =namedtuple("ScreenRow", "read start end chunks best_distance best_template")   # a line of <out>_screen.tsv


def format_screen(rows):
    """One line per region: read, start, end (0-based, inclusive), passing chunks, the smallest infix edit distance of
    a template against one of them, and that template's name (' marks a reverse complement).  No header."""
    return "".join("%s\t%d\t%d\t%d\t%d\t%s\n" % (r.read, r.start, r.end, r.chunks, r.best_distance, r.best_template)
                   for r in rows)


def write_screen(path, rows):
    with open(path, "w", newline="") as f:
        f.write(format_screen(rows))


def parse_screen(text):
    return _parse(text, True, 6, (_ident, int, int, int, int, _ident), ScreenRow)


def read_screen(path):
    """<out>_screen.tsv -> [ScreenRow]."""
    return _parse(path, False, 6, (_ident, int, int, int, int, _ident), ScreenRow)


def screen_rows(regions, read_names, mono_names):
    """lib.screen_regions' array -> [ScreenRow]; template j >= len(mono_names) is the reverse complement of j - len."""
    n = len(mono_names)
    out = []
    for g in regions:
        j = int(g["best_key"]) & 0xffff
        out.append(ScreenRow(read_names[int(g["read"])], int(g["start"]), int(g["end_incl"]), int(g["n_chunks"]),
                             int(g["best_key"]) >> 16, mono_names[j] if j < n else mono_names[j - n] + "'"))
    return out


# ---- motif hits (--motif): <out>_motif.tsv, <out>_motif_rows.tsv, <out>_motif_monomers.tsv -----------------------------------
# <out>_motif.tsv: read, start, end (inclusive, like the final TSV), strand, motif, mismatches, sequence -- the matched
# bases as the read has them, on - their reverse complement (a byte outside ACGT complements to N) -- in the order read,
# start, motif (request order), strand.  <out>_motif_rows.tsv: one line per row of the final TSV: read, start, end, monomer,
# then name:count of the motifs with a hit inside the row, in request order, comma-separated, * for none.
# <out>_motif_monomers.tsv: monomer, motif, rows, rows with a hit, hits -- per monomer name as the final TSV prints it
# (monomer-file order, forward before ') and per motif in request order.
class Motifs:
    """lib.motif / DeviceMotifs.to_host(): hits = a numpy record array (start, read, motif, strand, mismatches: sd_motif_hit
    of include/sd_hip.h) in canonical order -- read, motif in request order, + before -, start; per = int64 [reads, motifs,
    2], the hits per read, motif and strand; names, patterns: the request; E: the mismatches allowed."""

    def __init__(self, hits, per, names, patterns, E):
        self.hits, self.per, self.names, self.patterns, self.E = hits, per, list(names), list(patterns), int(E)

    @property
    def lengths(self):
        return [len(p) for p in self.patterns]


class MotifEdits:
    """lib.motif_edits / DeviceMotifEdits.to_host(): hits = a numpy record array (start, read, motif, length, strand_edits:
    sd_motif_edit_hit of include/sd_hip.h) in canonical order -- read, motif in request order, + before -, end; per = int64
    [reads, motifs, 2]; names, patterns: the request; K: the edits allowed."""

    def __init__(self, hits, per, names, patterns, K):
        self.hits, self.per, self.names, self.patterns, self.K = hits, per, list(names), list(patterns), int(K)

    @property
    def strand(self):
        return self.hits["strand_edits"] >> 7

    @property
    def edits(self):
        return self.hits["strand_edits"] & 127

    @property
    def end(self):
        """one past the last base of every hit"""
        return self.hits["start"] + self.hits["length"]


MotifRow = namedtuple("MotifRow", "read start end strand motif mismatches sequence")   # a line of <out>_motif.tsv
MotifRowsRow = namedtuple("MotifRowsRow", "read start end monomer counts")              # ... of <out>_motif_rows.tsv; counts: ((motif, n), ...)
MotifMonomerRow = namedtuple("MotifMonomerRow", "monomer motif rows rows_hit hits")     # ... of <out>_motif_monomers.tsv

_MOTIF_RC = bytes.maketrans(b"ACGT", b"TGCA")


def motif_sequence(seq, strand):
    """the matched bases of a hit as a str: as they stand on +, the reverse complement on - (outside ACGT: N)"""
    b = bytes(seq)
    if strand in (1, "-"):
        b = bytes(c if c in b"ACGT" else 78 for c in b).translate(_MOTIF_RC)[::-1]
    return b.decode("latin-1")


def motif_rows(motifs, read_names, reads):
    """The lines of <out>_motif.tsv for a Motifs -> [MotifRow], in the order read, start, motif, strand"""
    import numpy as np
    h = motifs.hits
    order = np.lexsort((h["strand"], h["motif"], h["start"], h["read"]))
    lens = motifs.lengths
    out = []
    for x in h[order].tolist():   # (start, read, motif, strand, mismatches)
        start, r, m, strand, mm = x
        seq = reads[r]
        seq = seq.encode() if isinstance(seq, str) else seq
        out.append(MotifRow(read_names[r], start, start + lens[m] - 1, "-" if strand else "+", motifs.names[m], mm,
                            motif_sequence(seq[start:start + lens[m]], strand)))
    return out


def motif_edit_rows(motifs, read_names, reads):
    """The lines of <out>_motif.tsv for a MotifEdits -> [MotifRow] with end = start + length - 1 and the edits in the sixth
    column, in the order read, start, end, motif, strand"""
    import numpy as np
    h = motifs.hits
    strand, end = motifs.strand, h["start"] + h["length"].astype(np.int64) - 1
    order = np.lexsort((strand, h["motif"], end, h["start"], h["read"]))
    out = []
    for start, r, m, length, se in h[order].tolist():
        seq = reads[r]
        seq = seq.encode() if isinstance(seq, str) else seq
        out.append(MotifRow(read_names[r], start, start + length - 1, "-" if se >> 7 else "+", motifs.names[m], se & 127,
                            motif_sequence(seq[start:start + length], se >> 7)))
    return out


def format_motif(rows):
    return "".join("%s\t%d\t%d\t%s\t%s\t%d\t%s\n" % tuple(r) for r in rows)


def write_motif(path, rows):
    _write_text(path, format_motif(rows))


def _strand(x):
    if x not in ("+", "-"):
        raise ValueError("a strand is + or -, found %r" % x)
    return x


def read_motif(path):
    """<out>_motif.tsv -> [MotifRow]."""
    return _parse(path, False, 7, (_ident, int, int, _strand, _ident, int, _ident), MotifRow)


def motif_row_counts(hits, final_rows, lengths, read_names=None):
    """Per row of the final TSV and per motif, the hits that lie wholly inside the row: row.start <= start and end <=
    row.end, with end = start + lengths[motif] - 1 -> int64 [rows, motifs].  A hit across a row boundary belongs to no row.
    final_rows: FinalRow-like tuples (read, monomer, start, end, ...) whose read is an index into the job's reads, or a name
    of read_names; the rows of a read ascending and disjoint, as the final TSV has them.  Plain numpy over two sorted
    lists: the rows by (read, start), and for every hit the last row that starts at or before it."""
    import numpy as np
    lengths = np.asarray(lengths, dtype=np.int64)
    return _motif_row_join(hits, lengths[hits["motif"].astype(np.int64)] if len(hits) else lengths[:0], len(lengths), final_rows, read_names)


def motif_edit_row_counts(hits, final_rows, n_motifs, read_names=None):
    """motif_row_counts for sd_motif_edit_hit records: every hit has its own length, end = start + hit.length - 1."""
    import numpy as np
    return _motif_row_join(hits, hits["length"].astype(np.int64), n_motifs, final_rows, read_names)


def _motif_row_join(hits, hit_len, n_motifs, final_rows, read_names):
    """the join of motif_row_counts; hit_len: the bases of every hit"""
    import numpy as np
    index = {n: i for i, n in enumerate(read_names)} if read_names is not None else None
    n = len(final_rows)
    rr = np.fromiter(((index[r[0]] if index is not None else r[0]) for r in final_rows), dtype=np.int64, count=n)
    rs = np.fromiter((r[2] for r in final_rows), dtype=np.int64, count=n)
    re_ = np.fromiter((r[3] for r in final_rows), dtype=np.int64, count=n)
    out = np.zeros((n, n_motifs), dtype=np.int64)
    if n == 0 or len(hits) == 0:
        return out
    order = np.lexsort((rs, rr))
    key = (rr[order] << 42) + rs[order]
    hs = hits["start"].astype(np.int64)
    hm = hits["motif"].astype(np.int64)
    at = np.searchsorted(key, (hits["read"].astype(np.int64) << 42) + hs, side="right") - 1
    row = order[np.maximum(at, 0)]
    inside = (at >= 0) & (rr[row] == hits["read"]) & (rs[row] <= hs) & (hs + hit_len - 1 <= re_[row])
    np.add.at(out, (row[inside], hm[inside]), 1)
    return out


def motif_row_lines(counts, final_rows, names):
    """The lines of <out>_motif_rows.tsv -> [MotifRowsRow], one per row of the final TSV"""
    return [MotifRowsRow(r[0], r[2], r[3], r[1], tuple((names[m], int(c)) for m, c in enumerate(counts[i]) if c > 0))
            for i, r in enumerate(final_rows)]


def motif_monomers(counts, final_rows, names, mono_names=None):
    """The lines of <out>_motif_monomers.tsv -> [MotifMonomerRow]: per monomer name as the final rows print it and per
    motif, the rows, the rows with a hit and the hits.  Order: mono_names (the monomer file's), each forward then with ',
    then any other name as it first appears; motifs in request order."""
    import numpy as np
    seen = {}
    for i, r in enumerate(final_rows):
        seen.setdefault(r[1], []).append(i)
    order = []
    for m in (mono_names or ()):
        order += [x for x in (m, m + "'") if x in seen]
    order += [x for x in seen if x not in set(order)]
    out = []
    for mono in order:
        c = np.asarray(counts)[seen[mono]]
        for m, name in enumerate(names):
            out.append(MotifMonomerRow(mono, name, len(seen[mono]), int((c[:, m] > 0).sum()), int(c[:, m].sum())))
    return out


def format_motif_rows(rows):
    return "".join("%s\t%d\t%d\t%s\t%s\n" % (r.read, r.start, r.end, r.monomer, ",".join("%s:%d" % c for c in r.counts) or "*")
                   for r in rows)


def write_motif_rows(path, rows):
    _write_text(path, format_motif_rows(rows))


def _motif_counts(x):
    if x == "*":
        return ()
    out = []
    for item in x.split(","):
        name, sep, c = item.rpartition(":")
        if not sep or not name or int(c) < 1:
            raise ValueError("expected name:count, found %r" % item)
        out.append((name, int(c)))
    return tuple(out)


def read_motif_rows(path):
    """<out>_motif_rows.tsv -> [MotifRowsRow]."""
    return _parse(path, False, 5, (_ident, int, int, _ident, _motif_counts), MotifRowsRow)


def format_motif_monomers(rows):
    return "".join("%s\t%s\t%d\t%d\t%d\n" % tuple(r) for r in rows)


def write_motif_monomers(path, rows):
    _write_text(path, format_motif_monomers(rows))


def read_motif_monomers(path):
    """<out>_motif_monomers.tsv -> [MotifMonomerRow]."""
    return _parse(path, False, 5, (_ident, _ident, int, int, int), MotifMonomerRow)


# ---- the merge of seed monomers (--autocorr-merge, bin/sd-merge) ---------------------------------------
# <out>_autocorr_merge.tsv / <out>_merge.tsv, one line per sequence in input order, no header: seed (the header's first
# token), length, cluster (M1, M2, ... in order of creation), centre (the seed that is the cluster's centre), distance (the
# cyclic edit distance of the seed in its centre), identity = "%.2f" of 100 (length - distance) / length, strand and phase of the fit
# (a centre: 0, 100.00, +, 0).  <out>_autocorr_merged.fa / <out>_merged.fa: one record per cluster, its canonical record.
CyclicPairs = namedtuple("CyclicPairs", "dist end strand phase")   # [queries, targets] each; strand 0 = +, 1 = -
CyclicMerge = namedtuple("CyclicMerge", "cluster centre dist end strand phase n_clusters")   # per sequence; cluster 0-based
MergeRow = namedtuple("MergeRow", "seed length cluster centre distance identity strand phase")
MergedRecord = namedtuple("MergedRecord", "name sequence cluster size count centre rotation strand")


def _token(name):
    return name.split()[0] if name.split() else name


def merge_identity(length, distance):
    """100 (length - distance) / length as "%.2f" prints it: the integer 100 (length - distance) divided by the integer
    length in one correctly rounded double division, then printf's rounding of that double (an exact tie such as 90.625
    goes to the even digit: 90.62)"""
    return "%.2f" % (100 * (length - distance) / length)


def merge_rows(merge, names, lens):
    """The lines of the merge TSV for a CyclicMerge of the sequences `names` (headers) of lengths `lens` -> [MergeRow]"""
    return [MergeRow(_token(names[i]), int(lens[i]), "M%d" % (int(merge.cluster[i]) + 1), _token(names[int(merge.centre[i])]), int(merge.dist[i]),
                     merge_identity(int(lens[i]), int(merge.dist[i])), "-" if merge.strand[i] else "+", int(merge.phase[i]))
            for i in range(len(names))]


def format_merge(rows):
    return "".join("%s\t%d\t%s\t%s\t%d\t%s\t%s\t%d\n" % tuple(r) for r in rows)


def write_merge(path, rows):
    _write_text(path, format_merge(rows))


def _merge_identity(x):
    float(x)
    return x


def read_merge(path):
    """the merge TSV -> [MergeRow] (identity stays the text it was written as)"""
    return _parse(path, False, 8, (_ident, int, _ident, _ident, int, _merge_identity, _strand, int), MergeRow)


def merged_records(merge, names, seqs, weights, canon, min_size=1):
    """One MergedRecord per cluster of at least min_size sequences, in cluster order: name = the FASTA header
    "M{k} period={length of the centre} seeds={size} count={sum of weights} centre={seed} rotation={r} strand={+|-}",
    sequence = the canonical record of the centre.  canon(seq) -> (record, rotation, strand): lib.cyclic_canon."""
    out = []
    size, count, centre = [0] * merge.n_clusters, [0] * merge.n_clusters, [0] * merge.n_clusters
    for i in range(len(names)):
        c = int(merge.cluster[i])
        size[c] += 1
        count[c] += int(weights[i])
        centre[c] = int(merge.centre[i])
    for c in range(merge.n_clusters):
        if size[c] < min_size:
            continue
        rec, rot, strand = canon(seqs[centre[c]])
        seed = _token(names[centre[c]])
        sign = "-" if strand else "+"
        out.append(MergedRecord("M%d period=%d seeds=%d count=%d centre=%s rotation=%d strand=%s" % (c + 1, len(rec), size[c], count[c], seed, rot, sign),
                                rec, c, size[c], count[c], seed, rot, sign))
    return out


def format_merged(records):
    return "".join(">%s\n%s\n" % (r.name, r.sequence) for r in records)
