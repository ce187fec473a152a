#!/usr/bin/env python3
"""Drop-in command line of StringDecomposer on MI355X.

Mirrors the reference driver stringdecomposer/main.py (same positional arguments, options,
defaults, output files and log line), with the one process boundary of the reference --
`subprocess.run([SD_BIN, ...], stdout=raw_file)` at main.py:194 -- replaced by a ctypes call into
libsd_hip.so (HIP kernels for gfx950).  Post-processing of the raw TSV into
final_decomposition.tsv / _alt.tsv follows main.py:29-184 without Bio / python-edlib / pandas.

Documented difference: the reference CLI silently ignores -s/--scoring (it always launches the
binary with 10 arguments, and main.cpp:381 parses scores only when argc == 10, i.e. 9 arguments).
Here -s is honoured (the documented intent, README / main.py:210); pass --ref-compat to reproduce
the reference CLI's effective behaviour (default scores whatever -s says).

The command line runs natively end to end (lib.run_files -> sd_run_files): FASTA ingest, DP, raw TSV,
identities (device kernel) and the final / _alt TSVs are produced batch by batch inside the library.
convert_read / print_read / convert_tsv below are the same post-processing written on numpy arrays:
the module-level API of the reference, kept importable and used by the tests as a second implementation.
"""
import argparse
import logging
import os
import pathlib
import sys



class _LazyNumpy:
    """numpy is only needed by the module-level convert_* API (the Python implementation of the post-processing,
    kept for the tests and for callers of the reference's functions); the command line runs natively and should
    not pay ~0.1-0.2 s of import time for it."""

    def __getattr__(self, name):
        import numpy
        globals()["np"] = numpy
        return getattr(numpy, name)


np = _LazyNumpy()

from . import autocorr
from . import motif
from . import dotplot
from . import split
from . import hor
from . import lib
from . import shard

CUR_DIR = os.path.dirname(os.path.abspath(__file__))
LOGREG_FILE = os.path.join(CUR_DIR, "models", "ont_logreg_model.txt")
# main.py:25-26 -- intercept, coef(identity), coef(identity - second best)
DEFAULT_LR = [-31.48494996, 0.41784018, 0.69186882]


def _lr_coef():
    if os.path.isfile(LOGREG_FILE):
        with open(LOGREG_FILE) as f:
            return list(map(float, f.readline().strip().split()))
    return list(DEFAULT_LR)


def get_logger(filename, logger_name="StringDecomposer", level=logging.INFO, filemode="a", stdout=True):
    """py/standard_logger.py:5-28."""
    logger = logging.getLogger(logger_name)
    logger.setLevel(level)
    for h in list(logger.handlers):
        logger.removeHandler(h)
    fh = logging.FileHandler(filename, mode=filemode)
    formatter = logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    fh.setFormatter(formatter)
    logger.addHandler(fh)
    if stdout:
        sh = logging.StreamHandler(sys.stdout)
        sh.setFormatter(formatter)
        logger.addHandler(sh)
    return logger


class Record:
    """The three SeqRecord attributes main.py uses: .id/.name (first header token) and .seq."""
    __slots__ = ("id", "name", "seq")

    def __init__(self, rid, seq, name=None):
        self.id = rid
        self.name = name if name is not None else rid
        self.seq = seq


def read_fasta(filename):
    """Bio.SeqIO.parse(filename, 'fasta') + .upper() (main.py:63-74): id = first word of the
    title, sequence = remaining lines with whitespace removed, upper-cased."""
    recs = []
    name, chunks = None, []
    with open(filename) as f:
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    recs.append(Record(name, "".join(chunks).upper()))
                title = line[1:].rstrip()
                name = title.split(None, 1)[0] if title.split() else ""
                chunks = []
            elif name is not None:
                chunks.append("".join(line.split()))
    if name is not None:
        recs.append(Record(name, "".join(chunks).upper()))
    return recs


def load_fasta(filename, tp="list"):
    recs = read_fasta(filename)
    if tp == "map":
        d = {}
        for r in recs:
            if r.id in d:
                raise ValueError("Duplicate key '%s'" % r.id)
            d[r.id] = r
        return d
    return recs


_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def add_rc_monomers(monomers):
    """main.py:81-86: interleaved m0, m0', m1, m1', ..."""
    res = []
    for m in monomers:
        res.append(m)
        res.append(Record(m.id + "'", m.seq.translate(_COMP)[::-1], m.name + "'"))
    return res


def convert_to_homo(seq):
    """main.py:87-92: homopolymer compression."""
    res = []
    prev = None
    for c in seq:
        if c != prev:
            res.append(c)
            prev = c
    return "".join(res)


def _strip_star(p):
    return p[:-1] if p.endswith("*") else p


def aai_batch(pairs, threads):
    """main.py:38-60 for a list of (query, target): percent identity from the NW alignment."""
    q = [_strip_star(a) for a, _ in pairs]
    t = [_strip_star(b) for _, b in pairs]
    res = lib.nw_identity_batch(q, t, threads=threads)
    out = []
    for ed, matches, cols in res:
        if ed == -1:
            out.append(0)
        else:
            a = 0.0
            a += matches       # sum of the '=' run lengths (integers; exact in a double)
            a /= cols
            out.append(a * 100)
    return out


def _identity_percent(dist, matches, cols):
    """main.py:38-60 on arrays: 0 for an empty side (edist -1), else '=' columns / CIGAR columns * 100."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = matches.astype(np.float64) / cols
        a = a * 100
    return np.where(dist == -1, 0.0, a)


def classify(score, second_best_score, coef):
    """main.py:95-104 (pandas DataFrame.dot == numpy dot over [1, score, score - second_best]):
    True where the block keeps '+', False where it becomes '?'."""
    s = np.asarray(score, dtype=np.float64)
    s2 = np.asarray(second_best_score, dtype=np.float64)
    if s.size == 0:
        return np.zeros(0, dtype=bool)
    X = np.stack([np.ones_like(s), s, s - s2], axis=1)
    return X.dot(np.array(coef, dtype=np.float64)) > 0


def _identities(seq, starts, ends, monomers, light, threads, own_names=None):
    """The NW identities convert_read needs for the blocks [starts, ends] of `seq`:
    light -> (scores,) against each block's own monomer; else -> (vals, hvals) against all monomers,
    plain and homopolymer-compressed."""
    seqs = [m.seq for m in monomers]
    if light:
        by_name = {}
        for x, m in enumerate(monomers):
            by_name[m.name] = x  # the reference keeps the last monomer of a given name
        pair = np.array([by_name[nm] for nm in own_names], dtype=np.int32)
        return (_identity_percent(*lib.identity_segments(seq, starts, ends, seqs, False, threads, pair_tmpl=pair)),)
    return (_identity_percent(*lib.identity_segments(seq, starts, ends, seqs, False, threads)),
            _identity_percent(*lib.identity_segments(seq, starts, ends, seqs, True, threads)))


def _convert_read_arrays(decomposition, read, monomers, light, threads, coef, pre=None):
    """main.py:107-150 on arrays: one entry per block.  Returns a dict of columns (lists / arrays).
    `pre` = this read's slice of identities computed for a batch of reads (see convert_tsv)."""
    n = len(decomposition)
    starts = np.array([d["start"] for d in decomposition], dtype=np.int64)
    ends = np.array([d["end"] for d in decomposition], dtype=np.int64)
    own_names = [d["m"] for d in decomposition]
    col = {"m": own_names, "start": starts, "end": ends, "alt_keys": None}
    if pre is None:
        pre = _identities(read.seq, starts, ends, monomers, light, threads, own_names)
    if light:
        col["score"] = pre[0]
        col["second_best"] = ["None"] * n
        col["second_best_score"] = np.full(n, -1.0)
        col["homo_best"] = ["None"] * n
        col["homo_best_score"] = np.full(n, -1.0)
        col["homo_second_best"] = ["None"] * n
        col["homo_second_best_score"] = np.full(n, -1.0)
    else:
        names = [m.name for m in monomers]
        vals, hvals = pre
        # scores is a dict keyed by monomer name in the reference: a repeated name keeps its first
        # position and its last value
        first, last = {}, {}
        for x, nm in enumerate(names):
            first.setdefault(nm, x)
            last[nm] = x
        keys = list(first)
        kidx = {k: x for x, k in enumerate(keys)}
        kcol = np.array([last[k] for k in keys], dtype=np.int64)
        kvals = vals[:, kcol]                                  # [n, len(keys)] in dict order
        for nm in own_names:
            if nm not in kidx:
                raise KeyError(nm)
        own = np.array([kidx[nm] for nm in own_names], dtype=np.int64)
        rows = np.arange(n)
        masked = kvals.copy()
        masked[rows, own] = -np.inf
        if len(keys) > 1 and "" not in kidx:
            sb = np.argmax(masked, axis=1)                     # first maximum among the other names
            col["second_best"] = [keys[x] for x in sb.tolist()]
            col["second_best_score"] = masked[rows, sb]
        else:  # `not secondbest` quirk of main.py:127 for an empty name / a single key
            sbn, sbs = [], []
            for i in range(n):
                secondbest, secondbest_score = None, -1
                for kx, m in enumerate(keys):
                    if kx != own[i]:
                        if not secondbest or secondbest_score < kvals[i, kx]:
                            secondbest, secondbest_score = m, float(kvals[i, kx])
                sbn.append(str(secondbest))
                sbs.append(secondbest_score)
            col["second_best"] = sbn
            col["second_best_score"] = np.array(sbs, dtype=np.float64)
        horder = np.argsort(-hvals, axis=1, kind="stable")
        h0, h1 = horder[:, 0], horder[:, 1]
        col["score"] = kvals[rows, own]
        col["homo_best"] = [names[x] for x in h0.tolist()]
        col["homo_best_score"] = hvals[rows, h0]
        col["homo_second_best"] = [names[x] for x in h1.tolist()]
        col["homo_second_best_score"] = hvals[rows, h1]
        col["alt_keys"], col["alt_vals"], col["own_key"] = keys, kvals, own
    keep = classify(col["score"], col["second_best_score"], coef)
    col["q"] = ["+" if k else "?" for k in keep.tolist()]
    return col


def convert_read(decomposition, read, monomers, light, threads, coef):
    """main.py:107-150.  Returns the list of per-block dicts of the reference (scores as floats)."""
    if not decomposition:
        return []
    c = _convert_read_arrays(decomposition, read, monomers, light, threads, coef)
    res = []
    for i in range(len(decomposition)):
        res.append({"m": c["m"][i], "start": str(int(c["start"][i])), "end": str(int(c["end"][i])),
                    "score": float(c["score"][i]),
                    "second_best": c["second_best"][i],
                    "second_best_score": -1 if light else float(c["second_best_score"][i]),
                    "homo_best": c["homo_best"][i], "homo_best_score": -1 if light else float(c["homo_best_score"][i]),
                    "homo_second_best": c["homo_second_best"][i],
                    "homo_second_best_score": -1 if light else float(c["homo_second_best_score"][i]),
                    "alt": {} if c["alt_keys"] is None else (c["alt_keys"], c["alt_vals"][i]), "q": c["q"][i]})
    return res


def print_read(fout, fout_alt, dec, read, monomers, identity_th, light, threads, coef, pre=None, alt_acc=None):
    """main.py:153-165.  With alt_acc (a list) the _alt rows are not written but appended to it as
    (read name, keys, starts, ends, own key, values) for one formatting call per batch of reads."""
    if not dec:
        return
    c = _convert_read_arrays(dec, read, monomers, light, threads, coef, pre)
    keep = np.nonzero(c["score"] >= identity_th)[0]
    f2 = "{:.2f}".format
    ks = keep.tolist()
    sc = [f2(x) for x in c["score"][keep].tolist()]
    s2 = [f2(x) for x in c["second_best_score"][keep].tolist()]
    h1 = [f2(x) for x in c["homo_best_score"][keep].tolist()]
    h2 = [f2(x) for x in c["homo_second_best_score"][keep].tolist()]
    st = c["start"][keep].tolist()
    en = c["end"][keep].tolist()
    name = read.name
    m, sbn, hb, hsb, q = c["m"], c["second_best"], c["homo_best"], c["homo_second_best"], c["q"]
    fout.write("".join(["%s\t%s\t%d\t%d\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n" %
                        (name, m[i], st[j], en[j], sc[j], sbn[i], s2[j], hb[i], h1[j], hsb[i], h2[j], q[i])
                        for j, i in enumerate(ks)]))
    if c["alt_keys"] is not None and len(ks) and alt_acc is not None:
        alt_acc.append((name, c["alt_keys"], c["start"][keep], c["end"][keep], c["own_key"][keep], c["alt_vals"][keep]))
    elif c["alt_keys"] is not None and len(ks):  # one row per block and monomer name, formatted natively
        fout_alt.write(lib.format_alt_rows(name, c["alt_keys"], c["start"][keep], c["end"][keep],
                                           c["own_key"][keep], c["alt_vals"][keep],
                                           max(1, min(threads, len(ks) // 512))))


def convert_tsv(decomposition, reads, monomers, outfile, identity_th, light, threads=1):
    """main.py:168-184.  Reads are post-processed in the order of the raw file; the NW identities are
    computed for batches of reads at a time (one native call per ~64 k blocks instead of one per read)."""
    coef = _lr_coef()
    per_read = []            # [(read name, [block dicts])] in file order
    prev_read = None
    for ln in decomposition.split("\n")[:-1]:
        read, monomer, start, end = ln.split("\t")[:4]
        read = read.split()[0]
        monomer = monomer.split()[0]
        if read != prev_read:
            per_read.append((read, []))
        prev_read = read
        per_read[-1][1].append({"m": monomer, "start": int(start), "end": int(end)})
    with open(outfile[:-len(".tsv")] + "_alt.tsv", "w") as fout_alt:
        with open(outfile, "w") as fout:
            i = 0
            while i < len(per_read):
                j, blocks = i, 0
                while j < len(per_read) and (j == i or blocks + len(per_read[j][1]) <= 65536):
                    blocks += len(per_read[j][1])
                    j += 1
                batch = per_read[i:j]
                # one sequence for the batch: blocks never cross a read, so shifted coordinates are exact
                seqs, off, pos = [], [], 0
                for name, _ in batch:
                    sq = reads[name].seq
                    off.append(pos)
                    seqs.append(sq)
                    pos += len(sq)
                starts = np.array([d["start"] + o for (_, dec), o in zip(batch, off) for d in dec], dtype=np.int64)
                ends = np.array([d["end"] + o for (_, dec), o in zip(batch, off) for d in dec], dtype=np.int64)
                own = [d["m"] for _, dec in batch for d in dec]
                pre = _identities("".join(seqs), starts, ends, monomers, light, threads, own)
                at = 0
                alt_acc = []
                for name, dec in batch:
                    sl = slice(at, at + len(dec))
                    print_read(fout, fout_alt, dec, reads[name], monomers, identity_th, light, threads, coef,
                               tuple(p[sl] for p in pre), alt_acc)
                    at += len(dec)
                if alt_acc:  # the key list is the same for every read (it depends on the monomers only)
                    fout_alt.write(lib.format_alt_rows(
                        [a[0] for a in alt_acc], alt_acc[0][1], np.concatenate([a[2] for a in alt_acc]),
                        np.concatenate([a[3] for a in alt_acc]), np.concatenate([a[4] for a in alt_acc]),
                        np.concatenate([a[5] for a in alt_acc]), threads,
                        row_read=np.concatenate([np.full(len(a[2]), x, dtype=np.int32) for x, a in enumerate(alt_acc)])))
                i = j


def run(sequences, monomers, num_threads, scoring, batch_size, raw_file, ed_thr, overlap, logger,
        ref_compat=False, device=0, kernel=0, final_file=None, min_identity=0, second_best=False, records_file=None,
        devices=None, profile=False, screen=None, screen_file=None, lenient=False):
    """main.py:186-197 with the subprocess replaced by libsd_hip.so.

    Single process with final_file given: ONE native call (sd_run_files) streams the job through the
    device and writes the raw, final and _alt TSVs batch by batch -- nothing is re-read, returns True.
    devices (a list of ordinals, --gpus / --devices): the same call with one pipeline per entry
    (sd_run_files_devices); `device` is then ignored.
    Otherwise (a multi-GPU launch, or no final_file): writes the raw TSV and returns its text (rank 0)."""
    ins, dels, mm, match = [int(x) for x in scoring.split(",")]
    if ref_compat:
        ins, dels, mm, match = -1, -1, -1, 1  # what the reference binary does with 10 argv (main.cpp:381)
    try:
        lib.load()
    except lib.SdError as e:
        logger.info("The HIP library of String Decomposer is not available. Did you forget to run `make`? Aborting. (%s)" % e.msg)
        sys.exit(1)
    logger.info(" ".join(["Run", lib.LIB_PATH, "with parameters", sequences, monomers, str(num_threads),
                          str(batch_size), str(overlap), scoring]))
    if devices is not None:
        logger.info("HIP devices of this process: " + ",".join(str(d) for d in devices))
    rank, local_rank, ws = shard.world()
    if ws > 1:
        # launched with `python -m torch.distributed.run --nproc-per-node G bin/stringdecomposer ...`:
        # one process per GPU, each takes a contiguous range of the global chunk table (shard.py);
        # every rank writes the rows of its own range into the output (shard._assemble_by_ranks) -- no device collective.
        dist = shard.init_process_group("gloo")
        dev = local_rank % max(lib.device_count(), 1)
        common = dict(scoring=(ins, dels, mm, match), part_size=int(batch_size), overlap=int(overlap), ed_thr=int(ed_thr),
                      threads=int(num_threads), kernel=kernel, device=dev, flags=lib.FLAG_PROGRESS)
        try:
            ok = None
            if final_file is not None:
                # a set of reads: every rank runs its group of reads completely (DP + post-processing + text)
                ok = shard.run_files_sharded(sequences, monomers, raw_file, final_file,
                                             final_file[:-len(".tsv")] + "_alt.tsv", dist, min_identity=min_identity,
                                             second_best=second_best, lr_coef=_lr_coef(), **common)
            if ok is True:
                return True if rank == 0 else None
            # a single huge sequence (or no final file wanted): shard by chunk range; every rank makes the raw TSV text
            # of its own range (seam merge across the range boundaries from exchanged edges) and writes it at its offset
            asm_stats = {}
            ok = shard.decompose_files_sharded(sequences, monomers, raw_file, dist, assemble_stats=asm_stats, **common)
            if asm_stats:
                logger.info("raw TSV: this rank wrote %d bytes of it (merge + text %.1f ms before, %.1f ms after the exchange of "
                            "edges, write %.1f ms)" % (asm_stats["text_bytes"], asm_stats["begin_ms"], asm_stats["text_ms"],
                                                       asm_stats["write_ms"]))
            if final_file is not None:
                # ... and convert_tsv (main.py:168-184) is shared again: every rank converts the rows of its byte range of
                # the raw file (identities on its own GPU), the parts are copied into the final / _alt files
                shard.barrier(dist)   # the raw file is complete
                shard.convert_sharded(raw_file, sequences, monomers, final_file, final_file[:-len(".tsv")] + "_alt.tsv", dist,
                                      min_identity=min_identity, second_best=second_best, lr_coef=_lr_coef(), device=dev,
                                      threads=max(1, int(num_threads)))
                return True if rank == 0 else None
        finally:
            shard.barrier(dist)
            dist.destroy_process_group()
        return "raw file written" if ok else None
    if final_file is not None:
        lib.run_files(sequences, monomers, raw_file, final_file, final_file[:-len(".tsv")] + "_alt.tsv",
                      min_identity=min_identity, second_best=second_best, lr_coef=_lr_coef(),
                      scoring=(ins, dels, mm, match), part_size=int(batch_size), overlap=int(overlap),
                      ed_thr=int(ed_thr), threads=int(num_threads), device=device, kernel=kernel,
                      # the dp binary's progress lines on stderr (main.cpp:82,115,393); --profile: the counters stay in the
                      # library until main() writes them (lib.last_run_profile(numpy=False): no numpy import on this path)
                      flags=lib.FLAG_PROGRESS | (lib.FLAG_PROFILE if profile else 0),
                      records_out=records_file, devices=devices, screen=screen, screen_tsv_out=screen_file,
                      lenient=lenient)
        _log_input_stats(logger)
        if screen is not None:
            c = lib.last_run_screen()
            logger.info("Screen (threshold %d): %d reads, %d with a region, %d bases read, %d bases decomposed"
                        % (screen, c["reads"], c["reads_with_region"], c["bases_read"], c["bases_decomposed"]))
        return True
    lib.decompose_files(sequences, monomers, raw_file, scoring=(ins, dels, mm, match),
                        part_size=int(batch_size), overlap=int(overlap), ed_thr=int(ed_thr),
                        threads=int(num_threads), device=devices[0] if devices else device, kernel=kernel,
                        lenient=lenient)
    _log_input_stats(logger)
    with open(raw_file, "r") as f:
        raw_decomposition = "".join(f.readlines())
    return raw_decomposition


def _log_input_stats(logger):
    """One line with what the file indexes met (lib.last_run_input_stats), when any count is non-zero."""
    c = lib.last_run_input_stats()
    if any(c[k] for k in ("lower", "ambiguity", "cr", "copied", "fastq")):
        logger.info("Input%s: %d lower-case bases folded, %d ambiguity codes read as N, %d CRs dropped, %d records copied, "
                    "%d FASTQ records" % (" (--lenient)" if c["lenient"] else "", c["lower"], c["ambiguity"], c["cr"],
                                          c["copied"], c["fastq"]))


MAX_DEVICE_ENTRIES = 16   # sd_run_files_devices


def _refuse(msg, code=2):
    """A request this process cannot serve ends it here: one line on stderr, before any work on a GPU."""
    sys.stderr.write("stringdecomposer: %s\n" % msg)
    sys.exit(code)


def _device_list(args):
    """--gpus / --devices -> None (the single-device path of --device) or the list of ordinals for sd_run_files_devices.
    A request this process cannot serve ends it here, with one line on stderr, before any work on a GPU."""
    if args.gpus is None and args.devices is None:
        return None
    if args.devices is not None:
        items = args.devices.split(",")
        if not all(x.strip().isdigit() for x in items):
            _refuse("--devices %s: expected a comma-separated list of device ordinals, e.g. 0,2,5" % args.devices)
        devs = [int(x) for x in items]
        what = "--devices %s" % args.devices
    else:
        if args.gpus < 1:
            _refuse("--gpus %d: at least one device" % args.gpus)
        if args.gpus == 1:
            return None   # today's single-device path, exactly
        devs = list(range(args.gpus))
        what = "--gpus %d" % args.gpus
    if len(devs) > MAX_DEVICE_ENTRIES:
        _refuse("%s: at most %d device entries in one process" % (what, MAX_DEVICE_ENTRIES))
    if len(devs) > 1 and shard.world()[2] > 1:
        _refuse("%s: several devices per process cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)"
                % (what, shard.world()[2]))
    try:
        count = lib.device_count()
    except lib.SdError as e:
        _refuse("%s: the HIP library is not available (%s)" % (what, e.msg))
    bad = [d for d in devs if d >= count]
    if bad and args.devices is None:
        _refuse("%s: %d devices asked for, %d HIP device%s visible" % (what, len(devs), count, "" if count == 1 else "s"))
    if bad:
        _refuse("%s: device %d does not exist (%d HIP device%s visible)" % (what, bad[0], count, "" if count == 1 else "s"))
    return devs


def _check_profile(args, flag="--profile", why="a profile needs one template per name"):
    """--profile (and --msa) requests this process cannot serve end it here, with one line on stderr, before any work on a
    GPU."""
    if shard.world()[2] > 1:
        sys.stderr.write("stringdecomposer: %s cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)\n"
                         % (flag, shard.world()[2]))
        sys.exit(2)
    try:
        names = lib.fasta_load(args.monomers)[0]
    except lib.SdError:
        return   # the job itself reports an unreadable monomer file
    seen = set()
    for n in names + [x + "'" for x in names]:
        if n in seen:
            sys.stderr.write("stringdecomposer: %s: monomer name %s is not unique: %s\n" % (flag, n, why))
            sys.exit(lib.SD_ERR_PARAM)
        seen.add(n)


def _check_screen(args):
    """--screen requests this process cannot serve end it here, with one line on stderr, before any work on a GPU."""
    if shard.world()[2] > 1:
        _refuse("--screen cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    if args.screen < 0:
        _refuse("--screen %d: the threshold is an edit distance, at least 0" % args.screen)
    if args.records:
        _refuse("--screen cannot be combined with --records: the record stream holds whole reads")
    if args.overlap.isdigit() and args.batch_size.isdigit() and int(args.overlap) >= int(args.batch_size):
        _refuse("--screen needs -v/--overlap smaller than -b/--batch-size (the regions of a read must not overlap)")


def _check_lags(args):
    """--lags requests this process cannot serve end it here, with one line on stderr, before any work on a GPU."""
    if shard.world()[2] > 1:
        _refuse("--lags cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    if not 1 <= args.lags <= lib.LAG_DMAX:
        _refuse("--lags %d: the number of neighbours is 1 .. %d" % (args.lags, lib.LAG_DMAX))
    if args.records:
        _refuse("--lags cannot be combined with --records: it is a post-pass over the rows of the final TSV")


def _heatmap_arg(text):
    """'B' or 'B,W' -> (B, W), None when the text is neither"""
    parts = text.split(",")
    if not 1 <= len(parts) <= 2 or not all(x.strip().isdigit() for x in parts):
        return None
    return int(parts[0]), int(parts[1]) if len(parts) == 2 else 0


def _check_heatmap(args):
    """--heatmap requests this process cannot serve end it here, with one line on stderr, before any work on a GPU."""
    if shard.world()[2] > 1:
        _refuse("--heatmap cannot be combined with a torch.distributed launch (WORLD_SIZE=%d)" % shard.world()[2])
    bw = _heatmap_arg(args.heatmap)
    if bw is None or not 1 <= bw[0] <= lib.HEAT_BMAX or bw[1] >= (1 << 62):
        _refuse("--heatmap %s: expected B or B,W with 1 <= B <= %d rows per bin and W >= 0 (0: no limit) the largest row "
                "distance of a pair" % (args.heatmap, lib.HEAT_BMAX))
    if args.heatmap_max_pairs < 0:
        _refuse("--heatmap-max-pairs %d: the cap is 0 (no limit) or more" % args.heatmap_max_pairs)
    if args.records:
        _refuse("--heatmap cannot be combined with --records: it is a post-pass over the rows of the final TSV")


def _check_lenient(args):
    """--lenient requests this process cannot serve end it here, with one line on stderr, before any work."""
    if args.ref_compat:
        _refuse("--lenient cannot be combined with --ref-compat, whose purpose is the reference's behaviour (its error for "
                "lower case, IUPAC codes and CRLF included): drop one of the two, or convert the input to upper-case ACGTN first",
                lib.SD_ERR_PARAM)
    if shard.world()[2] > 1:
        _refuse("--lenient cannot be combined with a torch.distributed launch (WORLD_SIZE=%d): the ranks' convert step reads "
                "the files strictly; use --gpus N / --devices LIST, several GPUs in one process" % shard.world()[2], lib.SD_ERR_PARAM)


def _reads_by_name(args):
    """The reads of the job, upper case, by header and by the header's first token (what the TSV names a read by); the
    first of equal names holds."""
    rn, rs, _ = lib.fasta_load(args.sequences, lenient=args.lenient)
    reads = {}
    for n, s in zip(rn, rs):
        reads.setdefault(n, s.upper())
        reads.setdefault(n.split()[0], s.upper())
    return reads


def _write_msa(args, final_fn, msa_fn, device):
    """--msa: one line per row of the final TSV just written (formats.MSA_HEADER), the rows computed read by read on
    `device` (lib.msa_segments: the row kernel, the host form for the pairs it does not take)."""
    from . import formats
    reads = _reads_by_name(args)
    mn, ms, _ = lib.fasta_load(args.monomers, lenient=args.lenient)
    ms, il = [s.upper() for s in ms], {}
    for m, n in enumerate(mn):
        for x in (n, n.split()[0]):
            il.setdefault(x, 2 * m)
            il.setdefault(x + "'", 2 * m + 1)
    with open(msa_fn, "w") as f:
        f.write(formats.MSA_HEADER)
        for read, rows in formats.by_read(formats.read_final(final_fn)):
            seq = reads[read]
            seg = [lib.segment_clamp(r.start, r.end, len(seq)) for r in rows]
            st, en = [x[0] for x in seg], [x[1] for x in seg]
            pt = [il[r.monomer] for r in rows]
            msa = lib.msa_segments(seq or b"N", st, en, ms, pt, threads=max(1, int(args.threads)), device=device)
            f.write(formats.format_msa(formats.msa_rows(msa, pt, [(r.read, r.start, r.end, r.monomer) for r in rows]),
                                       header=False))


def _write_lags(args, final_fn, lags_fn, period_fn, device):
    """--lags D: the identity of every row of the final TSV just written to its next D neighbours in the same read
    (lib.lag_segments on `device`: the lane kernel, the host form for the pairs it does not take) -> <out>_lags.tsv, one
    line per row, and <out>_period.tsv, one line per read."""
    from . import formats
    D = int(args.lags)
    reads = _reads_by_name(args)
    groups = formats.by_read(formats.read_final(final_fn))
    with open(lags_fn, "w", newline="") as fl, open(period_fn, "w", newline="") as fp:
        at = 0
        while at < len(groups):   # a call's share: whole reads, rows x D and text bounded
            text, st, en, off, rows, base, e = [], [], [], [0], [], 0, at
            while e < len(groups) and (e == at or ((len(rows) + len(groups[e][1])) * D < (1 << 26) and base < (1 << 28))):
                seq = reads[groups[e][0]]
                seq = seq if isinstance(seq, bytes) else seq.encode()
                for r in groups[e][1]:
                    s0, e0 = lib.segment_clamp(r.start, r.end, len(seq))
                    st.append(base + s0)
                    en.append(base + e0)
                    rows.append((r.read, r.start, r.end))
                text.append(seq)
                base += len(seq)
                off.append(len(rows))
                e += 1
            lags = lib.lag_segments(b"".join(text) or b"N", st, en, off, D, device=device, threads=max(1, int(args.threads)))
            ident = lib.lag_identities(lags.dist, lags.matches).tolist()
            period, pooled = lib.lag_periods(lags.sums)
            fl.write(formats.format_lags(formats.LagRow(r[0], r[1], r[2], v) for r, v in zip(rows, ident)))
            fp.write(formats.format_periods(formats.PeriodRow(g[0], len(g[1]), int(p), v)
                                            for g, p, v in zip(groups[at:e], period.tolist(), pooled.tolist())))
            at = e


def _write_heatmap(args, final_fn, heat_fn, device):
    """--heatmap B[,W]: the identity of every row of the final TSV just written to every earlier row of the same read
    (up to W rows back), pooled per pair of bins of B rows (lib.heat_segments on `device`: the kernel, the host form for
    the pairs it does not take) -> <out>_heatmap.tsv, one line per cell with pairs, read by read."""
    from . import formats
    B, W = _heatmap_arg(args.heatmap)
    cap = int(args.heatmap_max_pairs)
    reads = _reads_by_name(args)
    groups = formats.by_read(formats.read_final(final_fn))
    for read, rows in groups:   # every read's size first: a refusal leaves no half-written file
        _, _, cells, pairs = lib.heat_layout([0, len(rows)], B, W)
        if cells > lib.HEAT_CELLS_MAX:
            raise lib.SdError(lib.SD_ERR_PARAM, "read %s: %d rows in bins of %d give %d cells, the cap is %d: use more rows per bin"
                              % (read, len(rows), B, cells, lib.HEAT_CELLS_MAX))
        if cap > 0 and pairs > cap:
            raise lib.SdError(lib.SD_ERR_PARAM, "read %s: %d rows give %d pairs, the cap is %d (--heatmap-max-pairs): give a row "
                              "distance limit (--heatmap B,W) or raise the cap" % (read, len(rows), pairs, cap))
    with open(heat_fn, "w", newline="") as f:
        for read, rows in groups:
            seq = reads[read]
            seq = seq if isinstance(seq, bytes) else seq.encode()
            seg = [lib.segment_clamp(r.start, r.end, len(seq)) for r in rows]
            st, en = [x[0] for x in seg], [x[1] for x in seg]
            heat = lib.heat_segments(seq or b"N", st, en, [0, len(rows)], B, W, device=device, threads=max(1, int(args.threads)),
                                     max_pairs=cap)
            f.write(formats.format_heatmap(formats.heat_rows(heat, 0, read, [(r.start, r.end) for r in rows])))


def main(argv=None):
    parser = argparse.ArgumentParser(description="Decomposes string into blocks alphabet")
    parser.add_argument("sequences", help="fasta-file with long reads or genomic sequences")
    parser.add_argument("monomers", help="fasta-file with monomers")
    parser.add_argument("-t", "--threads", help="number of threads (by default 1)", default="1", required=False)
    parser.add_argument("-o", "--out-dir", help="output directory (by default .)", default=".", required=False)
    parser.add_argument("--out-file", help='output tsv-file (by default "final_decomposition")',
                        default="final_decomposition", required=False)
    parser.add_argument("-i", "--min-identity",
                        help="only monomer alignments with percent identity >= MIN_IDENTITY are printed (by default MIN_IDENTITY=0)",
                        type=int, default=0, required=False)
    parser.add_argument("-s", "--scoring",
                        help='set scoring scheme for SD in the format "insertion,deletion,mismatch,match" (by default "-1,-1,-1,1")',
                        default="-1,-1,-1,1", required=False)
    parser.add_argument("-b", "--batch-size", help="set size of the batch in parallelization (by default 5000)",
                        type=str, default="5000", required=False)
    parser.add_argument("--second-best", dest="second_best",
                        help="generate second best monomer and homopolymer scores", action="store_true")
    parser.add_argument("--ed_thr",
                        help="align only monomers with edit distance less then ed_thr for each segment (by default align all monomers)",
                        default=-1, type=int, required=False)
    parser.add_argument("-v", "--overlap", help="set size of batch overlap (by default 500)", type=str,
                        default="500", required=False)
    # opt-in extras of this build (never change defaults)
    parser.add_argument("--ref-compat", action="store_true",
                        help="reproduce the reference CLI exactly: -s/--scoring is ignored (default scores)")
    parser.add_argument("--device", type=int, default=0, help="HIP device ordinal (by default 0)")
    dg = parser.add_mutually_exclusive_group()
    dg.add_argument("--gpus", type=int, default=None, metavar="N",
                    help="use HIP devices 0..N-1 in this process (by default 1: the --device ordinal)")
    dg.add_argument("--devices", default=None, metavar="LIST",
                    help="comma-separated HIP device ordinals to use in this process, e.g. 0,2,5 (repeats allowed: 0,0 runs "
                         "two pipelines on device 0)")
    parser.add_argument("--kernel", choices=["auto", "generic", "fast"], default="auto",
                        help="device kernel family (by default auto)")
    parser.add_argument("--records", action="store_true",
                        help="also write <out-file>_raw.sdr: the rows of the raw tsv as a binary record stream "
                             "(stringdecomposer_amd.formats.read_records)")
    parser.add_argument("--profile", action="store_true",
                        help="also write <out-file>_profile.tsv (per-monomer column profiles of the rows of <out-file>.tsv) "
                             "and <out-file>_consensus.fa (their consensus sequences)")
    parser.add_argument("--msa", action="store_true",
                        help="also write <out-file>_msa.tsv: one line per row of <out-file>.tsv with the read's bases by column "
                             "of the forward monomer (ACGTN, '-' = deleted) and its insertions as slot:count (a count of 255 "
                             "means 255 or more)")
    parser.add_argument("--lags", type=int, default=None, metavar="D",
                        help="also write <out-file>_lags.tsv (one line per row of <out-file>.tsv: read, start, end, then the "
                             "identity of the row's stretch of the read to that of each of its next D neighbours in the same "
                             "read, -1.00 where the read ends; nothing is reverse-complemented, so a pair across an inversion "
                             "scores low) and <out-file>_period.tsv (one line per read: read, rows, the lag with the largest "
                             "pooled identity, then the D pooled identities); 1 <= D <= 255")
    parser.add_argument("--heatmap", default=None, metavar="B[,W]",
                        help="also write <out-file>_heatmap.tsv: the identity of every row of <out-file>.tsv to every other row "
                             "of the same read (with W: to the rows up to W rows away), pooled in bins of B consecutive rows; "
                             "one line per pair of bins with pairs: read, bin_i, bin_j, start_i, end_i, start_j, end_j, pairs, "
                             "identity (sum of matches / sum of alignment columns).  The earlier row is the query; nothing is "
                             "reverse-complemented.  1 <= B <= 1048576; at most 33554432 cells per read")
    parser.add_argument("--heatmap-max-pairs", dest="heatmap_max_pairs", type=int, default=4000000000, metavar="N",
                        help="refuse a read whose heatmap needs more than N pairs (by default 4000000000, about 8 s of device "
                             "time on 171-bp blocks; 0: no limit)")
    autocorr.add_arguments(parser)
    dotplot.add_arguments(parser)
    split.add_arguments(parser)
    hor.add_arguments(parser)
    motif.add_arguments(parser)
    parser.add_argument("--screen", type=int, default=None, metavar="THR",
                        help="decompose only the stretches where a monomer occurs: a chunk (-b, -v) is kept when some monomer "
                             "or reverse complement lies within infix edit distance THR of it, runs of kept chunks are "
                             "decomposed as reads of their own (positions stay those of the whole read); also writes "
                             "<out-file>_screen.tsv, one line per stretch")
    parser.add_argument("--lenient", action="store_true",
                        help="read both files leniently: lower-case (soft-masked) bases are folded to upper case, the IUPAC "
                             "ambiguity codes RYSWKMBDHV are read as N (which matches N only), and the CR of CRLF line ends is "
                             "dropped.  Without it such input ends with the reference's error.  FASTQ (four lines per "
                             "record) is read with or without it")
    args = parser.parse_args(argv)
    if args.lenient:
        _check_lenient(args)
    if args.screen is not None:
        _check_screen(args)
    if args.lags is not None:
        _check_lags(args)
    if args.heatmap is not None:
        _check_heatmap(args)
    if args.autocorr is not None:
        autocorr.check(args)
    elif args.autocorr_merge is not None:
        autocorr.refuse_merge_alone(args)
    if args.dotplot is not None:
        dotplot.check(args)
    if args.split is not None:
        split.check(args)
    if args.hor:
        hor.check(args)
    if motif.wanted(args):
        motif.check(args)
    if args.profile:
        _check_profile(args)
    if args.msa:
        _check_profile(args, "--msa", "a row's key must name one template")
    devices = _device_list(args)
    pathlib.Path(args.out_dir).mkdir(parents=True, exist_ok=True)

    logfn = os.path.join(args.out_dir, "stringdecomposer.log")
    if shard.world()[0] == 0:
        logger = get_logger(logfn, logger_name="StringDecomposer")
    else:  # ranks > 0 of a multi-GPU launch compute their share and stay silent
        logger = logging.getLogger("StringDecomposer.rank%d" % shard.world()[0])
        logger.addHandler(logging.NullHandler())
        logger.propagate = False
    logger.info(f"cmd: {sys.argv}")

    raw_decomp_fn = os.path.join(args.out_dir, args.out_file + "_raw.tsv")
    convert_tsv_fn = os.path.join(args.out_dir, args.out_file + ".tsv")
    records_fn = os.path.join(args.out_dir, args.out_file + "_raw.sdr") if args.records else None
    kernel = {"auto": 0, "generic": 1, "fast": 2}[args.kernel]
    try:
        raw_decomposition = run(args.sequences, args.monomers, args.threads, args.scoring, args.batch_size,
                                raw_decomp_fn, args.ed_thr, args.overlap, logger,
                                ref_compat=args.ref_compat, device=args.device, kernel=kernel,
                                final_file=convert_tsv_fn, min_identity=int(args.min_identity),
                                second_best=args.second_best,
                                records_file=records_fn if shard.world()[2] == 1 else None, devices=devices,
                                profile=args.profile, screen=args.screen, lenient=args.lenient,
                                screen_file=os.path.join(args.out_dir, args.out_file + "_screen.tsv") if args.screen is not None else None)
    except lib.SdError as e:
        # the reference dies with CalledProcessError after the binary printed its message on stderr
        sys.stderr.write(e.msg + "\n")
        logger.info("String Decomposer failed: " + e.msg)
        sys.exit(e.code if 0 < e.code < 256 else 1)
    if raw_decomposition is None:
        return  # not rank 0
    logger.info("Saved raw decomposition to " + raw_decomp_fn)
    if records_fn and shard.world()[2] > 1:
        # a multi-GPU launch: the ranks wrote text parts; rank 0 restates the finished raw file as the record stream
        from . import formats
        names = lib.fasta_load(args.monomers)[0]
        sc = (-1, -1, -1, 1) if args.ref_compat else tuple(int(x) for x in args.scoring.split(","))
        formats.write_records(records_fn, formats.raw_to_records(
            formats.read_raw(raw_decomp_fn), names + [n + "'" for n in names], scoring=sc,
            part_size=int(args.batch_size), overlap=int(args.overlap), ed_thr=int(args.ed_thr)))
    if records_fn:
        logger.info("Saved the binary record stream to " + records_fn)
    if args.screen is not None:
        logger.info("Saved the screened regions to " + os.path.join(args.out_dir, args.out_file + "_screen.tsv"))
    logger.info("Transforming raw alignments...")
    if raw_decomposition is not True:
        # multi-GPU launch: rank 0 holds the raw TSV of the whole job; convert_tsv (main.py:168-184) natively,
        # identities on this rank's GPU
        try:
            lib.convert_raw_tsv(raw_decomp_fn, args.sequences, args.monomers, convert_tsv_fn,
                                convert_tsv_fn[:-len(".tsv")] + "_alt.tsv", int(args.min_identity), args.second_best,
                                _lr_coef(), device=shard.world()[1] % max(lib.device_count(), 1),
                                threads=max(1, int(args.threads)))
        except lib.SdError as e:
            sys.stderr.write("post-processing failed: " + e.msg + "\n")
            logger.info("Transformation failed (%s); the raw decomposition is in %s" % (e.msg, raw_decomp_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
    logger.info("Transformation finished. Results can be found in " + convert_tsv_fn)
    if args.profile:
        from . import formats
        prof = lib.last_run_profile(numpy=False)
        prof_fn = os.path.join(args.out_dir, args.out_file + "_profile.tsv")
        cons_fn = os.path.join(args.out_dir, args.out_file + "_consensus.fa")
        formats.write_profile(prof_fn, prof)
        formats.write_consensus(cons_fn, prof)
        logger.info("Saved the monomer column profiles to " + prof_fn)
        logger.info("Saved the monomer consensus sequences to " + cons_fn)

    if args.msa:
        msa_fn = os.path.join(args.out_dir, args.out_file + "_msa.tsv")
        try:
            _write_msa(args, convert_tsv_fn, msa_fn, devices[0] if devices else args.device)
        except lib.SdError as e:
            sys.stderr.write("--msa failed: " + e.msg + "\n")
            logger.info("--msa failed (%s); the decomposition is in %s" % (e.msg, convert_tsv_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
        logger.info("Saved the per-instance monomer columns to " + msa_fn)

    if args.lags is not None:
        lags_fn = os.path.join(args.out_dir, args.out_file + "_lags.tsv")
        period_fn = os.path.join(args.out_dir, args.out_file + "_period.tsv")
        try:
            _write_lags(args, convert_tsv_fn, lags_fn, period_fn, devices[0] if devices else args.device)
        except lib.SdError as e:
            sys.stderr.write("--lags failed: " + e.msg + "\n")
            logger.info("--lags failed (%s); the decomposition is in %s" % (e.msg, convert_tsv_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
        logger.info("Saved the identities against lag to " + lags_fn + " and the periods to " + period_fn)

    if args.heatmap is not None:
        heat_fn = os.path.join(args.out_dir, args.out_file + "_heatmap.tsv")
        try:
            _write_heatmap(args, convert_tsv_fn, heat_fn, devices[0] if devices else args.device)
        except lib.SdError as e:
            sys.stderr.write("--heatmap failed: " + e.msg + "\n")
            logger.info("--heatmap failed (%s); the decomposition is in %s" % (e.msg, convert_tsv_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
        logger.info("Saved the binned all-against-all identities to " + heat_fn)

    if args.autocorr is not None:
        try:
            saved = autocorr.write(args, args.out_dir, args.out_file, devices[0] if devices else args.device)
        except lib.SdError as e:
            sys.stderr.write("--autocorr failed: " + e.msg + "\n")
            logger.info("--autocorr failed (%s); the decomposition is in %s" % (e.msg, convert_tsv_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
        logger.info("Saved the k-mer autocorrelation of the reads to " + ", ".join(saved))

    if args.dotplot is not None:
        try:
            saved = dotplot.write(args, args.out_dir, args.out_file, devices[0] if devices else args.device)
        except lib.SdError as e:
            sys.stderr.write("--dotplot failed: " + e.msg + "\n")
            logger.info("--dotplot failed (%s); the decomposition is in %s" % (e.msg, convert_tsv_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
        logger.info("Saved the windowed k-mer identities of the reads to " + ", ".join(saved))

    if args.split is not None:
        try:
            saved = split.write(args, convert_tsv_fn, args.out_dir, args.out_file, devices[0] if devices else args.device)
        except lib.SdError as e:
            sys.stderr.write("--split failed: " + e.msg + "\n")
            logger.info("--split failed (%s); the decomposition is in %s" % (e.msg, convert_tsv_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
        logger.info("Saved the subfamilies of the monomers' instances to " + ", ".join(saved))

    if args.hor:
        try:
            saved = hor.write(args, convert_tsv_fn, args.out_dir, args.out_file)
        except lib.SdError as e:
            sys.stderr.write("--hor failed: " + e.msg + "\n")
            logger.info("--hor failed (%s); the decomposition is in %s" % (e.msg, convert_tsv_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
        logger.info("Saved the higher-order repeat units to " + ", ".join(saved))

    if motif.wanted(args):
        try:
            saved = motif.write(args, convert_tsv_fn, args.out_dir, args.out_file, devices[0] if devices else args.device)
        except lib.SdError as e:
            sys.stderr.write("--motif failed: " + e.msg + "\n")
            logger.info("--motif failed (%s); the decomposition is in %s" % (e.msg, convert_tsv_fn))
            sys.exit(e.code if 0 < e.code < 256 else 1)
        logger.info("Saved the motif hits of the reads to " + ", ".join(saved))

    logger.info("Thank you for using StringDecomposer!")


if __name__ == "__main__":
    main()
