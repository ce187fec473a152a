/*
 * sd_hip.h -- C-ABI of libsd_hip.so: the MI355X-native StringDecomposer DP hot path.
 *
 * Drop-in boundary.  The reference crosses from Python into native code exactly once, by running
 * its `dp` binary as a subprocess with stdout redirected to <out>_raw.tsv:
 *     stringdecomposer/main.py:194   subprocess.run([SD_BIN, sequences, monomers, num_threads,
 *                                     batch_size, overlap, ins, dels, mm, match, str(ed_thr)], stdout=f)
 *     stringdecomposer/src/main.cpp:374-402   (argv contract of that binary)
 * This header is what an FFI for that call binds instead (INTEGRATION.md shows the ctypes stub).
 * Plain C types only; no torch/HIP types in any signature (a HIP stream is passed as void*).
 *
 * There is NO CPU fallback behind these entry points: every compute call needs a gfx950 device
 * and fails with SD_ERR_NO_DEVICE otherwise.
 */
#ifndef SD_HIP_H
#define SD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define SD_OK 0
#define SD_ERR_IO 2           /* cannot open / write a file                                      */
#define SD_ERR_FORMAT 3       /* malformed FASTA (no header, header without name)                */
#define SD_ERR_PARAM 4        /* bad parameter                                                   */
#define SD_ERR_EMPTY 6        /* empty read or monomer (the reference segfaults, main.cpp:115)   */
#define SD_ERR_INTERNAL 7
#define SD_ERR_NO_DEVICE 8    /* no usable HIP device: the product path never falls back to CPU  */
#define SD_ERR_UNSUPPORTED 9  /* input outside what the device kernels support (documented)      */
#define SD_ERR_HIP 10         /* a HIP runtime call failed (message in errbuf)                   */
#define SD_ERR_SYMBOL 255     /* undefined symbol in a sequence: reference exit(-1), main.cpp:335 */

/* ---- parameters: the argv of the reference binary (main.cpp:374-402) ----------------------- */
typedef struct sd_params {
    int32_t ins, del, mismatch, match; /* argv[6..9]; defaults -1,-1,-1,1 (main.cpp:380)          */
    int32_t part_size;                 /* argv[4] (-b/--batch-size, main.py:212): chunk step, bp   */
    int32_t overlap;                   /* argv[5] (-v/--overlap,   main.py:216)                    */
    int32_t ed_thr;                    /* argv[10] (--ed_thr): -1 = off; >=0 = per-chunk prefilter */
    int32_t threads;                   /* argv[3] (-t): host threads for parse / format            */
    int32_t device;                    /* HIP device ordinal                                      */
    int32_t kernel;                    /* 0 auto, 1 generic family (int32, workgroup per chunk), 2 fast family (packed 16-bit cells, wave(s) per chunk) */
    int32_t max_batch_rows;            /* 0 = size device batches from free HBM; >0 = cap on chunk rows per batch */
    /* Switches that have no counterpart in the reference's argv (all 0 = the defaults):
     *   reserved[0]  kernel streams of the batch pipeline: 0 default (SD_PIPE_* below), else mode + 1
     *                (1: every kernel in order on one stream, 2: traceback on a second stream, 3: fills alternating too)
     *   reserved[1]  SD_FLAG_* bits
     *   reserved[2]  fp16 range guard of the fills: magnitude limit (0 = 2040); a smaller value makes the guard trip
     *                on ordinary input -- the test hook of the guard and of the re-run with integer cells
     *   reserved[3..4] must be 0 */
    int32_t reserved[5];
} sd_params;
#define SD_FLAG_NO_F16 1           /* no fp16 cell format: integer cells (or the generic family)                   */
#define SD_FLAG_NO_U16 128         /* narrow layout: no biased-u16 cells (fp16 where the range allows, as in rounds 1-5; A/B) */
#define SD_FLAG_FULL_FLOOR 2       /* fills that take the start-term maximum in every slot (A/B of the FL variants) */
#define SD_FLAG_NO_EDTHR_COMPACT 4 /* --ed_thr with > 128 templates: every chunk on the W-wave ranked kernel (a set
                                    * beyond eight waves, whose only fast form is the compacted one: generic family)   */
#define SD_FLAG_FILTER_GENERAL 8   /* --ed_thr: the general prefilter kernel instead of the uniform one             */
#define SD_FLAG_NO_STREAM_IDENT 16 /* sd_run_files, final-mode streams: identities from the read text (round 2)     */
#define SD_FLAG_TRACE_V1 64        /* the one-block int32 traceback (sd_fast_trace) where the packed two-block form would run */
#define SD_FLAG_NO_IDENT_PRUNE 256 /* sd_run_files --second-best: every homopolymer-compressed pair aligned in full (rounds 3-5; A/B) */
#define SD_FLAG_PROGRESS 32        /* sd_run_files: the reference binary's progress lines on stderr ("Scores: ...",
                                      "Prepared reads", "<p>%: Aligned <read>", main.cpp:82,115,393); the command line sets it */
#define SD_FLAG_PROFILE 512        /* sd_run_files*, final-mode streams: per-monomer column profiles of the kept rows
                                      (sd_last_run_profile / sd_stream_profile); a repeated monomer name is SD_ERR_PARAM */

#define SD_FLAG_DEVICE_ROWS 1024   /* raw-mode streams with one device entry: the rows of a job are assembled on the device and
                                      stay there (sd_stream_peek_dev / sd_stream_collect_dev); no record crosses to the host */
#define SD_FLAG_DEVICE_FINAL 2048  /* final-mode streams with one device entry: the rows of final_decomposition.tsv / _alt.tsv are
                                      selected on the device and stay there (sd_stream_peek_final_dev / sd_stream_collect_final_dev) */
#define SD_FLAG_DEVICE_PROFILE 4096 /* SD_FLAG_DEVICE_FINAL streams: the column profiles of the kept rows are folded on the device
                                      from the job's text in HBM (sd_stream_profile / sd_stream_profile_dev) */
#define SD_FLAG_LENIENT 8192       /* every entry point that opens the two files: the lenient reading of both (below); the
                                      default, without it, reproduces the reference's errors byte for byte */

/* ---- lenient input (a documented superset of the reference, never the default) -------------------------------
 * The rule for a sequence byte (csrc/sd_normalize.hpp, one text for host and device): a-z becomes the upper-case
 * letter; then any of R Y S W K M B D H V becomes N; every other byte stays, so U, digits, '*', '-', a stray CR and
 * bytes >= 0x80 are still reported by the checks that exist, in their words.  N keeps the reference's meaning: an
 * ordinary symbol that matches N only (main.cpp:190) -- a monomer that holds an ambiguity code matches a read's N
 * there and nothing else.
 * Files (SD_FLAG_LENIENT): besides the rule, a CR directly in front of a newline is dropped from header and sequence
 * lines.  A record the rule changes gets a buffer of its own; a canonical one-line record stays in the mapping.
 * FASTQ needs no flag: a file whose first non-blank byte is '@' is read as four-line records (name = first whitespace
 * token behind '@'; the third line must begin with '+' -- multi-line FASTQ is SD_ERR_FORMAT; the fourth must have the
 * sequence's length and is never looked at otherwise).  Its sequences are strict without the flag, lenient with it.
 * Not read: gzip / BGZF. */

/* out[0, n) = the rule applied to in[0, n); out may equal in.  stats (may be NULL) are ADDED to: [0] lower-case bytes
 * folded, [1] ambiguity codes turned into N, [2] bytes still outside A C G T N afterwards, [3] bytes examined.
 * SD_ERR_PARAM for n < 0 or a NULL buffer with n > 0. */
int sd_normalize_host(const char* in, char* out, int64_t n, uint64_t stats[4]);
/* The same for reads that lie in the memory of `device`: read r = the read_lens[r] bytes at d_in + read_off[r] (host
 * arrays, as in sd_stream_submit_dev: gaps, padding and any order are allowed, overlapping reads are not), written at
 * d_out + read_off[r].  Only the bytes of the reads are read or written; d_out == d_in normalises in place, otherwise
 * the two must not overlap.  d_stats (may be NULL): four uint64 counters in device memory, added to as above.  The
 * kernel is enqueued on hip_stream and the call returns without waiting for it.
 * SD_ERR_PARAM for a bad argument or memory that is not device memory (or reads that end outside the allocation),
 * SD_ERR_UNSUPPORTED for another device's memory, SD_ERR_NO_DEVICE without a device. */
int sd_normalize_dev(const void* d_in, void* d_out, const int64_t* read_off, const int64_t* read_lens,
                     int32_t n_reads, int32_t device, void* hip_stream, uint64_t* d_stats,
                     char* errbuf, size_t errlen);
/* What the file indexes of the last call of this process that opened a reads and a monomers file met, summed over the
 * two: [0] lower-case bases folded, [1] ambiguity codes turned into N, [2] CRs dropped, [3] records copied because the
 * rule changed them, [4] FASTQ records, [5] 1 if the call was lenient, [6..7] 0. */
void sd_last_run_input_stats(int64_t out[8]);

void sd_params_default(sd_params* p); /* -1,-1,-1,1 / 5000 / 500 / -1 / 1 / 0 / auto */

/* One monomer alignment = one raw TSV row (MonomerAlignment, main.cpp:37-49), chunk-local or
 * read-global coordinates depending on the call.  score = dp at the monomer end minus the
 * between-monomers score at its start (main.cpp:255), always integral. */
typedef struct sd_rec {
    int32_t tmpl;  /* template index: 0..M-1 monomers in file order, M..2M-1 their reverse complements */
    int32_t start;
    int32_t end;
    int32_t score;
} sd_rec;

const char* sd_version(void);
int sd_device_count(void);           /* number of visible HIP devices (0 if none / no runtime)   */
void sd_free(void* p);               /* frees anything this library returned                     */
/* Engines return their large device buffers to a process-wide cache instead of the driver (hipMalloc /
 * hipFree of the multi-GB workspaces can take longer than the kernels); this hands the cached buffers
 * back.  Environment SD_DEVICE_POOL=0 disables the cache.
 * The file and chunk-range entry points (sd_run_files*, sd_decompose_files*, sd_decompose_chunk_range) also keep the
 * device pipeline of a finished job -- engines, streams, pinned staging and their device buffers, i.e. GIGABYTES of
 * HBM that other users of the GPU in this process or on this device do not see as free -- for the next job with the
 * same parameters and monomer set (at most two pipelines per device entry, none above SD_PIPE_CACHE_GB [96] GB, none whose engines had
 * to leave their layout; SD_PIPE_CACHE_OFF=1 disables it).  sd_release_cache() destroys them too; nothing of either
 * cache is torn down at process exit. */
void sd_release_cache(void);

/* ---- one-shot entry points (replace main.py:194) ------------------------------------------- */

/* reads.fa + monomers.fa -> raw TSV file, byte-identical to `dp ... > raw_tsv_out`
 * (SaveBatch, main.cpp:272-285; reads in input order).  Error text for bad symbols equals the
 * reference's stderr line (main.cpp:335). */
int sd_decompose_files(const char* reads_fa, const char* monomers_fa, const sd_params* p,
                       const char* raw_tsv_out, char* errbuf, size_t errlen);

/* In-memory variant: monomers WITHOUT reverse complements (appended here as main.cpp:364-371).
 * *tsv is malloc'ed (sd_free). */
int sd_decompose(const char* const* read_names, const char* const* read_seqs,
                 const int64_t* read_lens, int32_t n_reads, const char* const* mono_names,
                 const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                 const sd_params* p, char** tsv, size_t* tsv_len, char* errbuf, size_t errlen);

/* The whole CLI job in one call (main.py:186-197 `run` + :168-184 `convert_tsv`): both FASTA files are
 * mapped and indexed by all host threads, the chunks stream through the device in batches, and every
 * batch's rows are written three ways -- raw TSV (as sd_decompose_files), final TSV (main.py:157-160) and
 * _alt TSV (:161-165, empty without second_best) -- with the identities of main.py:29-60 computed by the
 * device kernel of sd_identity_segments_dev.  lr_coef = the three logistic-regression coefficients of
 * main.py:25-26.  Nothing is re-read from the raw file. */
int sd_run_files(const char* reads_fa, const char* monomers_fa, const sd_params* p, const char* raw_tsv_out,
                 const char* final_tsv_out, const char* alt_tsv_out, int32_t min_identity, int32_t second_best,
                 const double* lr_coef, char* errbuf, size_t errlen);

/* The same for one rank of a multi-process launch: the read set is split into `world` contiguous groups of
 * reads with about equal chunk counts and this call runs group `rank` completely (DP, identities, the three
 * TSV texts of its reads) into its own files, which the launcher concatenates in rank order.  Only the
 * reads of the group are alphabet-checked.  info (may be NULL): [0] first read, [1] one past the last,
 * [2] reads in the file, [3] chunks of this rank.  SD_ERR_UNSUPPORTED (nothing written) when the read set
 * cannot be split by reads -- one read holds more than half a rank's share, e.g. a single chromosome --
 * then shard by chunk range (sd_decompose_files_range). */
int sd_run_files_range(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank,
                       int32_t world, const char* raw_tsv_out, const char* final_tsv_out,
                       const char* alt_tsv_out, int32_t min_identity, int32_t second_best,
                       const double* lr_coef, int64_t* info, char* errbuf, size_t errlen);
/* Stage times (ms) of the last sd_run_files / sd_run_files_range call of this process: [0] fill, [1] traceback,
 * [2] compaction, [3] in-stream identity kernels (HIP events, summed over the batches), [4] identity pairs computed
 * in-stream, [5] device batches, [6] DP rows, [7] pack + enqueue, [8] waits for the device, [9] raw text,
 * [10] post-processing, [11] file writes, [12] text-based identities (0 when they all came in-stream), [13] final /
 * _alt text, [14] whole call, [15] device / pinned allocations, [16] engine / pipeline set-up, [17] per-read assembly,
 * [18] homopolymer-compressed pairs of the job (--second-best), [19] those of them that were aligned in full (the pruned pass
 * aligns only the pairs whose identity bounds reach a record's two best), [20..23] 0.  Measurement only (bench.py, tools/). */
void sd_last_run_stats(double out[24]);
/* Batches of this process that were repeated with integer cells because the fp16 range guard of a fill tripped
 * (0 unless sd_params.reserved[2] lowers the limit, or the layout plan's range bound is wrong). */
int64_t sd_guard_trips(void);

/* convert_tsv (main.py:168-184) alone: an existing raw TSV + the two FASTA files -> final TSV and _alt TSV,
 * streamed in batches of reads.  device < 0: host identities (sd_identity_segments). */
int sd_convert_raw_tsv(const char* raw_tsv, const char* reads_fa, const char* monomers_fa,
                       const char* final_tsv_out, const char* alt_tsv_out, int32_t min_identity,
                       int32_t second_best, const double* lr_coef, int32_t device, int32_t threads,
                       char* errbuf, size_t errlen);
/* The same for one rank of a multi-process launch: the rows of the raw TSV that begin in this rank's byte range (world
 * ranges cut at line starts) into this rank's own part files; rows are independent (main.py:95-150), so the parts
 * concatenated in rank order are the files sd_convert_raw_tsv writes (shard.convert_sharded does that). */
int sd_convert_raw_tsv_range(const char* raw_tsv, const char* reads_fa, const char* monomers_fa,
                             const char* final_tsv_out, const char* alt_tsv_out, int32_t min_identity,
                             int32_t second_best, const double* lr_coef, int32_t device, int32_t threads,
                             int32_t rank, int32_t world, char* errbuf, size_t errlen);

/* ---- on-disk binary record stream ---------------------------------------
 * The reference's only hand-over between its DP stage and everything downstream is text: <out>_raw.tsv, written by
 * SaveBatch (main.cpp:272-285) and re-read line by line by convert_tsv (main.py:168-184; column spec README.md:77-83).
 * The record stream holds the same rows -- per read, in read order -- as 16-byte sd_rec records, so a consumer
 * skips the text round trip; the raw TSV is a pure function of it (sd_records_to_raw_tsv gives SaveBatch's bytes).
 * Layout: csrc/sd_records.hpp and stringdecomposer_amd/formats.py (read_records / write_records, pure Python).
 * Template names are column 2 of the raw TSV: the monomers in file order, then their names + "'" (main.cpp:364-371). */
typedef struct sd_records {
    int32_t ins, del, mismatch, match, part_size, overlap, ed_thr;   /* the job's argv (main.cpp:374-402)           */
    int32_t n_templates;
    char** tmpl_names;
    int32_t n_reads;
    char** read_names;
    int64_t* read_lens;    /* -1 where the writer did not know it                                              */
    int64_t* row_off;      /* n_reads + 1: read r owns rows[row_off[r] .. row_off[r+1]), read-global coordinates */
    int64_t n_rows;
    sd_rec* rows;
} sd_records;
/* Host only.  rows / row_off as sd_stream_collect returns them (or any rows in SaveBatch order). */
int sd_write_records(const char* path, const sd_params* p, const char* const* tmpl_names, int32_t n_templates,
                     const char* const* read_names, const int64_t* read_lens, int32_t n_reads, const sd_rec* rows,
                     const int64_t* row_off, char* errbuf, size_t errlen);
/* Host only.  Checks the file (magic, bounds, template indices, the trailer's totals: a stream whose writer did not
 * finish is SD_ERR_FORMAT); *out is filled with malloc'ed arrays, released by sd_records_free. */
int sd_read_records(const char* path, sd_records* out, char* errbuf, size_t errlen);
void sd_records_free(sd_records* r);
/* Host only: the raw TSV of a record stream, byte for byte what `dp` prints for the same job. */
int sd_records_to_raw_tsv(const char* records_path, const char* raw_tsv_out, int32_t threads, char* errbuf,
                          size_t errlen);
/* sd_decompose_files with the record stream as its output (no text is made anywhere). */
int sd_decompose_files_records(const char* reads_fa, const char* monomers_fa, const sd_params* p,
                               const char* records_out, char* errbuf, size_t errlen);
/* sd_run_files that also writes the record stream, read by read as the batches complete (records_out == NULL:
 * exactly sd_run_files).  Single process only. */
int sd_run_files_records(const char* reads_fa, const char* monomers_fa, const sd_params* p, const char* raw_tsv_out,
                         const char* final_tsv_out, const char* alt_tsv_out, const char* records_out,
                         int32_t min_identity, int32_t second_best, const double* lr_coef, char* errbuf,
                         size_t errlen);
/* The whole CLI job on several devices of this process: one batch pipeline per entry of devices[0 .. n_devices)
 * (p->device is ignored), the job's batches dealt to whichever pipeline frees a slot first, their records consumed
 * strictly in batch order by the one per-read assembler and writer.  The three TSVs (and the record stream when
 * records_out != NULL) are byte-identical to sd_run_files / sd_run_files_records with the same parameters.
 * 1 <= n_devices <= 16; every ordinal must exist and be a gfx950 device, checked before any work starts on any of
 * them (SD_ERR_PARAM / SD_ERR_NO_DEVICE, errbuf names the ordinal).  An ordinal may repeat: {0, 0} runs two
 * pipelines on device 0 (how the form is tested on a machine with one GPU).  The single-device calls are this route
 * with one entry, driven on the calling thread; n_devices == 1 is sd_run_files_records on devices[0].  A HIP failure
 * on one of several devices ends the job with SD_ERR_HIP naming the device; the other pipelines are drained first. */
int sd_run_files_devices(const char* reads_fa, const char* monomers_fa, const sd_params* p, const int32_t* devices,
                         int32_t n_devices, const char* raw_tsv_out, const char* final_tsv_out, const char* alt_tsv_out,
                         const char* records_out, int32_t min_identity, int32_t second_best, const double* lr_coef,
                         char* errbuf, size_t errlen);
/* Per device entry of the last sd_run_files* call of this process (one entry for the single-device calls): batches
 * dealt to it and its device busy time in ms (HIP-event spans of its batches), up to cap entries; returns the number
 * of entries. */
int sd_last_run_device_stats(int64_t* batches, double* busy_ms, int32_t cap);

/* ---- chunk-range form: one job sharded over several GPUs, one process per GPU ---------------
 * The chunks of a read set (main.cpp:70-81, all reads, input order) form one global table; a chunk's
 * DP depends on nothing but its own bases and the template set (main.cpp:88-96), so rank g runs the
 * contiguous range [lo_g, hi_g) of the table -- a single 200-Mb sequence splits like a million reads --
 * and one rank turns the concatenated records into the raw TSV.  No collective on the data path. */
int64_t sd_chunk_table_size(const int64_t* read_lens, int32_t n_reads, int32_t part_size, int32_t overlap);

/* Records (chunk-local coordinates, as sd_engine_fetch) of chunks [chunk_lo, chunk_hi); batched and
 * pipelined on the device like sd_decompose.  *recs / *rec_off (chunk_hi - chunk_lo + 1 entries) are
 * malloc'ed (sd_free). */
int sd_decompose_chunk_range(const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads,
                             const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                             const sd_params* p, int64_t chunk_lo, int64_t chunk_hi, sd_rec** recs,
                             int64_t** rec_off, char* errbuf, size_t errlen);

/* File forms, for the multi-process command line: every rank maps + indexes the FASTA (sequences are not
 * copied), runs its share block_range(n_chunks, rank, world) of the chunk table and validates only the reads
 * that share touches; rank 0 then turns the gathered records into the raw TSV file. */
int sd_decompose_files_range(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank,
                             int32_t world, sd_rec** recs, int64_t** rec_off, int64_t* chunk_lo, int64_t* chunk_hi,
                             int64_t* n_chunks_total, char* errbuf, size_t errlen);
int sd_assemble_files_tsv(const char* reads_fa, const char* monomers_fa, const sd_params* p, const sd_rec* recs,
                          const int64_t* rec_off, int64_t n_chunks, const char* raw_tsv_out, char* errbuf,
                          size_t errlen);

/* Host only: records of ALL chunks in table order -> raw TSV (chunk offsets main.cpp:109-111, seam
 * merge :287-302, SaveBatch :272-285).  The bytes equal sd_decompose's. */
int sd_assemble_tsv(const char* const* read_names, const int64_t* read_lens, int32_t n_reads,
                    const char* const* mono_names, int32_t n_mono, const sd_params* p,
                    const sd_rec* recs, const int64_t* rec_off, int64_t n_chunks, char** tsv,
                    size_t* tsv_len, char* errbuf, size_t errlen);

/* ---- one read over several ranks: every rank makes the text of its own chunk range --------------------
 * The gather above leaves the seam merge and the text of a whole chromosome to rank 0 (46 ms for 200 Mb, whatever
 * the number of GPUs).  The merge (main.cpp:287-302) is a scan whose state is one index, so a rank can run it on its
 * own records once it knows where the scan enters them -- which follows from a few records either side of every
 * range boundary (csrc/sd_seam.hpp).  Protocol, host only, no record leaves its rank:
 *   1. sd_range_assemble_begin[_files]: chunk offsets, the merge and text of the reads that lie completely inside
 *      [chunk_lo, chunk_hi), the scan of the crossing pieces from an assumed entry, the text of their middle part;
 *      fills `edge` (POD, 160 bytes) for the exchange;
 *   2. the caller all-gathers the edges (torch.distributed all_gather_object in shard.py);
 *   3. sd_range_assemble_text(h, edges, world, rank, &bytes): the real entry from the chain of edges, the first
 *      and last rows of the crossing pieces; SD_ERR_UNSUPPORTED when some rank's edge has ok == 0 (an empty share or
 *      a crossing piece of fewer than 32 rows): gather on rank 0 instead;
 *   4. the caller all-gathers `bytes` and every rank calls sd_range_assemble_write(h, path, offset of its text,
 *      total bytes).
 * The concatenation of the ranks' texts is byte for byte what sd_assemble_tsv makes of all records. */
typedef struct sd_seam_edge {
    int32_t ok;          /* 0: this share cannot take part */
    int32_t has_front;   /* the share begins inside a read (its first records continue the previous rank's last read) */
    int32_t has_back;    /* the share ends inside a read */
    int32_t through;     /* both, and it is the same read: the share lies inside one read */
    int32_t head[8][2];  /* start, end (read coordinates) of the first eight records of the front piece */
    int32_t tail[8][2];  /* ... of the last eight records of the back piece */
    int8_t exit_of[8];   /* position 0..7 at which the scan reaches the last eight records, by entry position 0..7 */
    int64_t reserved;
} sd_seam_edge;
typedef struct sd_range_asm sd_range_asm;
int sd_range_assemble_begin(const char* const* read_names, const int64_t* read_lens, int32_t n_reads,
                            const char* const* mono_names, int32_t n_mono, const sd_params* p, int64_t chunk_lo,
                            int64_t chunk_hi, const sd_rec* recs, const int64_t* rec_off, sd_seam_edge* edge,
                            sd_range_asm** h, char* errbuf, size_t errlen);
/* names and lengths from the FASTA index; the range is block_range(n_chunks, rank, world) as in
 * sd_decompose_files_range */
int sd_range_assemble_begin_files(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank,
                                  int32_t world, const sd_rec* recs, const int64_t* rec_off, sd_seam_edge* edge,
                                  sd_range_asm** h, char* errbuf, size_t errlen);
int sd_range_assemble_text(sd_range_asm* h, const sd_seam_edge* edges, int32_t world, int32_t rank, int64_t* text_bytes,
                           char* errbuf, size_t errlen);
/* The text into the file `path` at byte `offset`.  file_bytes >= 0: the file is created if missing and set to that
 * size first (the sum of all ranks' text_bytes: every rank passes the same value, so no rank has to wait for another);
 * file_bytes < 0: an existing file, size untouched.  sd_range_assemble_copy: the text into `buf` (text_bytes of room). */
int sd_range_assemble_write(sd_range_asm* h, const char* path, int64_t offset, int64_t file_bytes, char* errbuf,
                            size_t errlen);
int sd_range_assemble_copy(sd_range_asm* h, char* buf, int64_t room);
/* DP + step 1 in one call (the FASTA is mapped and indexed once, the records never leave the library): what
 * sd_decompose_files_range followed by sd_range_assemble_begin_files does.  sd_range_assemble_records lends the
 * share's records (valid until sd_range_assemble_free) for the gather on rank 0 when step 3 refuses. */
int sd_decompose_files_range_begin(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank,
                                   int32_t world, sd_seam_edge* edge, sd_range_asm** h, int64_t* chunk_lo,
                                   int64_t* chunk_hi, int64_t* n_chunks_total, char* errbuf, size_t errlen);
int sd_range_assemble_records(sd_range_asm* h, const sd_rec** recs, const int64_t** rec_off, int64_t* n_chunks);
/* stage times of this handle in ms: [0] begin, [1] of it merge + text of complete reads, [2] assumed scans + text
 * made ahead, [3] sd_range_assemble_text, [4] rows printed by it (repaired head + tail), [5] 1 if the real scan joined
 * the assumed one too late and the piece was formatted again, [6] write */
void sd_range_assemble_stats(sd_range_asm* h, double out[8]);
void sd_range_assemble_free(sd_range_asm* h);

/* ---- engine: device-resident batches (what bench.py and the parity tests drive) ------------ */
typedef struct sd_engine sd_engine;

/* Templates = monomers followed by their reverse complements (built here).  Uploads the template
 * tables to HBM and picks the kernel family (p->kernel). */
int sd_engine_create(sd_engine** out, const sd_params* p, const char* const* mono_seqs,
                     const int32_t* mono_lens, int32_t n_mono, char* errbuf, size_t errlen);
void sd_engine_destroy(sd_engine* e);

/* Chunk the reads (main.cpp:70-81), pack them 2-bit (+N mask) and copy them to HBM.
 * Replaces any previously loaded batch.  Returns the chunk count via *n_chunks. */
int sd_engine_load_reads(sd_engine* e, const char* const* read_seqs, const int64_t* read_lens,
                         int32_t n_reads, int64_t* n_chunks, char* errbuf, size_t errlen);

/* The same from reads that already lie in DEVICE memory: read r = d_bases[read_off[r] .. read_off[r] + read_lens[r])
 * (read_off / read_lens are host arrays), packed by a HIP kernel -- no base passes through the host.  Arguments,
 * ordering with hip_stream and the alphabet check as sd_stream_submit_dev below; the call returns when the batch is
 * packed, and a byte outside A C G T N is reported by sd_engine_fetch (SD_ERR_SYMBOL). */
int sd_engine_load_reads_dev(sd_engine* e, const void* d_bases, const int64_t* read_off, const int64_t* read_lens,
                             int32_t n_reads, void* hip_stream, int64_t* n_chunks, char* errbuf, size_t errlen);

/* One pass of the hot path over the loaded batch: DP fill + traceback + record compaction, all
 * on `hip_stream` (a hipStream_t cast to void*, NULL = default stream).  Asynchronous. */
int sd_engine_run(sd_engine* e, void* hip_stream, char* errbuf, size_t errlen);

/* Wait for the last run and copy the compact records to the host.  rec_off has n_chunks+1
 * entries; chunk c owns recs[rec_off[c] .. rec_off[c+1]) in read order, chunk-local coordinates.
 * Both arrays are malloc'ed (sd_free). */
int sd_engine_fetch(sd_engine* e, sd_rec** recs, int64_t** rec_off, char* errbuf, size_t errlen);

/* Per-read assembly of fetched records: chunk offsets added (main.cpp:109-111) and the seam merge
 * PostProcessing (main.cpp:287-302) applied; read r owns rows[row_off[r] .. row_off[r+1]). */
int sd_engine_assemble(sd_engine* e, const sd_rec* recs, const int64_t* rec_off, sd_rec** rows,
                       int64_t** row_off, char* errbuf, size_t errlen);

/* The same assembly on the DEVICE, straight on the compact records of the last run (csrc/sd_rows_dev.hip): after the
 * call -- which waits for the run as sd_engine_fetch does, a guard trip's repeat included -- d_rows[0 .. *n_rows) holds the
 * rows sd_engine_assemble makes of sd_engine_fetch's records (scores in the caller's scale) and d_row_off the n_reads + 1
 * offsets.  Both are DEVICE buffers of the caller's, on the engine's device.  Every kernel is enqueued on hip_stream (the
 * stream the buffers are used on), so later work on it follows; the call returns when the host knows *n_rows (one 8-byte
 * copy).  cap_rows < *n_rows: SD_ERR_PARAM, *n_rows set, nothing written, and the call may be repeated with room: the
 * assembly of a run is made once, the repeat only copies -- so a first call with cap_rows = 0 (d_rows NULL) is how a
 * caller learns the exact size without any record crossing to the host. */
int sd_engine_rows_dev(sd_engine* e, sd_rec* d_rows, int64_t cap_rows, int64_t* d_row_off, void* hip_stream, int64_t* n_rows,
                       char* errbuf, size_t errlen);

/* HIP-event timings (ms) of the last completed sd_engine_run, measured on its stream:
 * [0] fill kernel(s)  [1] traceback kernel(s)  [2] compaction  [3] whole run.  */
int sd_engine_timings(sd_engine* e, float ms[4]);

/* Static facts about the engine / loaded batch (for roofline arithmetic in bench.py):
 * [0] n_templates [1] sum of template lengths [2] n_chunks [3] sum of chunk rows
 * [4] low byte: kernel family actually used (1 generic, 2 fast); bits 8..: cell arithmetic of the fill
 *     (0 int32, 1 packed int16, 2 packed fp16 [exact small integers], 3 wide: int16 cells / int8 table,
 *      4 wide: fp16 cells / bf8 table, 5 multi-wave wide: fp16 cells / template codes in LDS, > 128 templates,
 *      6 tiled multi-wave: as 5 with a template over several virtual lanes -- templates longer than 224 bp in sets
 *      beyond one wave of the narrow layout, 7 / 8: as 5 / 6 with int16 cells and int8 table bytes -- scorings beyond
 *      the fp16 range, or after a tripped fp16 guard)
 * [5] generic: cells-per-thread parameter Q; fast: slots per lane P in bits 0..15, bits 16..: the last slot
 *     of a lane whose diagonal input needs the maximum with the start term (0 = every slot takes it)
 * [6] bytes of HBM workspace allocated [7] bits 0..15: number of fill launches per run; bits 16..: traceback of the
 *     fast family: 1 = one block per step, int32 cells (sd_fast_trace), 2 = two blocks per step, packed 16-bit cells
 *     (sd_fast_trace_pk: layouts with one wave per chunk, templates <= 256 bp, unless SD_FLAG_TRACE_V1) */
int sd_engine_info(sd_engine* e, int64_t info[8]);

/* Host only (no device needed): the layout sd_engine_create would choose for this monomer set and scoring.
 * info: [0] kernel family of "auto" (2 fast, 1 generic; generic: the reason is in errbuf, rc is still SD_OK)
 * [1] slots per lane P [2] cell arithmetic code (as sd_engine_info [4] >> 8) [3] last slot of a lane that needs
 * the maximum with the start term [4] low byte: waves per chunk; bits 8..39: the proven bound on the magnitude of a
 * stored cell (fp16 cell formats are chosen when it is <= 2040; tests/test_host_cpu.py checks it against the
 * recurrence itself); bits 40..: rows between two rebases of the stored cells (128, or 64 where only that keeps
 * the set inside the fp16 range) [5] cells in the shortest first lane of a template
 * [6] cells in the fullest lane [7] bits 0..15: common factor divided out of the four scores; bits 16..23: registers per
 * lane of the packed two-block traceback at its widest level (0 = the one-block int32 traceback runs); bits 24..55: the
 * proven bound on |E' - base| of that traceback's 16-bit words (tests/test_host_cpu.py checks it against the
 * recurrence); bit 56: the narrow fill takes its carry scan through ds_bpermute. */
int sd_plan_info(const sd_params* p, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                 int64_t info[8], char* errbuf, size_t errlen);

/* Host only: the floor levels of that layout -- per read symbol A C G T N the last slot of a lane whose diagonal input needs
 * the maximum with the start term (floor_sym), the same by previous and current read symbol (floor_pair[5 * previous +
 * current], <= floor_sym[current]) -- and the lanes they were computed over: the templates are the monomers followed by
 * their reverse complements, template j has the lanes lane_off[j] .. lane_off[j + 1] - 1 (lane_off: 2 * n_mono + 1 words),
 * and lane_start[] is the first template cell of each (lane_cap words; the sum of the template lengths always suffices).
 * info: [0] kernel family of "auto" as in sd_plan_info (generic: everything else is 0) [1] slots per lane P [2] 1 where the
 * scoring meets the conditions of the pair levels, else floor_pair[a][b] == floor_sym[b] [3] number of lanes. */
int sd_plan_floor_levels(const sd_params* p, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                         int32_t floor_sym[5], int32_t floor_pair[25], int32_t* lane_off, int32_t* lane_start, int64_t lane_cap,
                         int64_t info[4], char* errbuf, size_t errlen);

/* ---- streaming form: sequences in host memory -> rows in host memory ------------------------
 * AlignReadsSet (main.cpp:67-122) without the text: chunk table (:70-81), DP + traceback per chunk
 * (:84-102), per-read flush with chunk offsets and seam merge (:104-117).  A stream keeps up to three device
 * batches in flight: every submitted job (a read set) is cut into `sub_batches` device batches of
 * consecutive chunks; while the device works on one batch the host packs and uploads the next ones (pinned
 * staging, asynchronous copies) and assembles the previous one, across job boundaries.  A caller whose jobs
 * are one batch each keeps the device busiest with TWO jobs outstanding before it collects the oldest (the
 * traceback of a batch runs at low priority beside the next fill and ends with it: with one job outstanding
 * the job after that is enqueued late).  This is the
 * region SURVEY.md 8(d) defines the throughput metric on, and what bench.py times.
 * Sequences are NOT validated here (they went through sd_fasta_load / sd_decompose's check). */
typedef struct sd_stream sd_stream;
int sd_stream_create(sd_stream** out, const sd_params* p, const char* const* mono_seqs,
                     const int32_t* mono_lens, int32_t n_mono, int32_t sub_batches, char* errbuf,
                     size_t errlen);
void sd_stream_destroy(sd_stream* s);
/* Packs, uploads and enqueues the job's batches; returns while the last ones are still running.  The
 * read buffers are no longer needed when it returns. */
int sd_stream_submit(sd_stream* s, const char* const* read_seqs, const int64_t* read_lens,
                     int32_t n_reads, char* errbuf, size_t errlen);
/* sd_stream_submit for reads that already lie in DEVICE memory (a basecaller's output, a torch tensor, an earlier GPU
 * stage): read r = d_bases[read_off[r] .. read_off[r] + read_lens[r]); read_off and read_lens are HOST arrays, and
 * gaps, padding and any order of the offsets are allowed.  The bytes are packed into the 2-bit words by a HIP kernel
 * (csrc/sd_pack_dev.hip) on the stream's copy streams; no base is copied to the host (final mode: only the reads whose
 * blocks take the fallback identities, when the rows come back, from a device copy the job keeps).  The rows are those
 * of sd_stream_submit on the same bytes.  Works on a raw or final-mode stream, with or without a device list.
 *
 * ORDERING AND BUFFER LIFETIME.  hip_stream (a hipStream_t cast to void*, NULL = the null stream) is the stream on which
 * the caller produced the bytes.  The library records an event on it and makes its own streams wait for that event
 * before the first packer, and before this call returns it makes hip_stream wait for an event recorded behind the
 * job's last packer.  Work the caller enqueues on hip_stream AFTER the call -- overwriting the buffer, a stream-ordered
 * free of it -- is therefore ordered behind the library's last read of it; there is no host-side wait.  Work on OTHER
 * streams is not ordered.  As sd_stream_submit in raw mode, the call returns once every batch of the job is packed,
 * which here means: its packer is enqueued.
 *
 * Checked before any work: SD_ERR_PARAM for a NULL handle, NULL d_bases with n_reads > 0, n_reads < 0, or a d_bases that
 * hipPointerGetAttributes does not report as device memory; SD_ERR_EMPTY for a read of length <= 0;
 * SD_ERR_UNSUPPORTED when the memory belongs to another device than one of the stream's entries (errbuf names both
 * ordinals; {0, 0} is fine, copies between devices are not made).
 * The alphabet is checked by the packer: a byte outside A C G T N fails the stream with SD_ERR_SYMBOL -- errbuf gives
 * the read's index within the job, the 0-based position and the byte -- under the stream's failure rule: the submit
 * or collect that meets it reports it, and every outstanding job is dropped.  (The byte is packed under the same
 * masked 2-bit formula as any other, so it cannot cause an out-of-range access on the device.) */
int sd_stream_submit_dev(sd_stream* s, const void* d_bases, const int64_t* read_off, const int64_t* read_lens,
                         int32_t n_reads, void* hip_stream, char* errbuf, size_t errlen);
/* Rows of the oldest submitted job (FIFO): read r owns rows[row_off[r] .. row_off[r+1]), read-global
 * coordinates, seam-merged.  Both arrays are malloc'ed (sd_free). */
int sd_stream_collect(sd_stream* s, sd_rec** rows, int64_t** row_off, int64_t* n_rows, char* errbuf,
                      size_t errlen);
/* ---- rows that stay on the device (SD_FLAG_DEVICE_ROWS in sd_params.reserved[1] at create) ---------------------
 * The counterpart of sd_stream_submit_dev: every batch's compact records are appended, on the device and behind the
 * batch's compaction, to a record store the job keeps in HBM (chunk offsets added, scores in the caller's scale); after
 * the job's last batch the seam merge runs there in pieces (csrc/sd_seam_dev.hpp, sd_rows_dev.hip).  No record is copied
 * to the host and no host thread assembles anything (sd_stream_stats [9] stays 0); the per-chunk record counts still
 * come back, as they always did.  A read that spans several batches is just a longer record list.
 * Raw mode with ONE device entry only: the flag is SD_ERR_PARAM at sd_stream_create_final* (final rows are selected on
 * the host; SD_FLAG_DEVICE_FINAL, below, selects them on the device) and with a device list of more than one entry (a job's batches would lie on several devices).
 * sd_stream_collect on such a stream and sd_stream_collect_dev on a plain one are SD_ERR_PARAM.
 *
 * sd_stream_peek_dev waits for the oldest job (FIFO) and gives what its buffers need: *n_reads, and *max_rows = its
 * record count before the merge, an upper bound on its rows.  The job stays.
 * sd_stream_collect_dev hands the oldest job over: d_rows[0 .. *n_rows) = its rows, read-global and seam-merged, as
 * sd_stream_collect gives them; d_row_off = the n_reads + 1 offsets.  Both are DEVICE buffers of the caller's on the
 * stream's device (checked for d_rows: SD_ERR_PARAM / SD_ERR_UNSUPPORTED as in sd_stream_submit_dev).  hip_stream (NULL =
 * the null stream) is the stream the caller uses the buffers on: the library's copy into them is enqueued on hip_stream
 * itself, behind an event of its own stream's assembly, so it follows what the caller enqueued before (the allocation,
 * an earlier use) and precedes what the caller enqueues afterwards -- no host-side wait for it.  The call returns when the
 * host knows *n_rows, which takes one 8-byte copy.  cap_rows < *n_rows: SD_ERR_PARAM with *n_rows set, nothing is written
 * and the job stays collectable.  The buffers are the caller's alone from then on: a later job does not touch them. */
int sd_stream_peek_dev(sd_stream* s, int32_t* n_reads, int64_t* max_rows, char* errbuf, size_t errlen);
int sd_stream_collect_dev(sd_stream* s, sd_rec* d_rows, int64_t cap_rows, int64_t* d_row_off, void* hip_stream,
                          int64_t* n_rows, char* errbuf, size_t errlen);
/* Accumulated over all collected batches: [0] fill [1] traceback [2] compaction [3] whole-run HIP-event
 * ms (per-batch spans; batches on the two streams overlap, so these do not add up to wall time),
 * [4] fill launches [5] batches [6] chunk rows, host ms: [7] pack+enqueue [8] wait for the device
 * [9] assembly [10] inside submit [11] inside collect, [12] jobs [13] sub_batches [14] row budget, [15] 0
 * (the identity figures of a final-mode stream: sd_stream_final_stats). */
int sd_stream_stats(sd_stream* s, double out[16]);
int sd_stream_info(sd_stream* s, int64_t info[8]);   /* as sd_engine_info, of the stream's engine */

/* ---- final mode of the stream: the rows of final_decomposition.tsv / _alt.tsv in host memory -----------------
 * The same jobs, but collect returns what the command line writes (main.py:107-165) as typed rows instead of the raw
 * DP rows.  The identities come from the in-stream kernels (csrc/sd_ident.hip) that run on the 2-bit reads already
 * on the device behind each batch's compaction; pairs those kernels do not take (a segment over their length limit, a
 * pair edlib aligns by Hirschberg's split, a batch whose identity outputs had no room) take the fallback of the file
 * path (sd_identity_segments_dev, then the host).  The selection rules are the ones sd_run_files formats with.
 *
 * One kept block (a row of final_decomposition.tsv).  Names are key indices into sd_stream_keys (-1: "None"); the
 * identities are the doubles the text prints with "%.2f" (-1 where it prints -1.00). */
typedef struct sd_final_row {
    int32_t read;                    /* read index within its job                                           */
    int64_t start, end;              /* read-global, inclusive (as in the raw TSV)                            */
    int32_t best, second, homo_best, homo_second;
    double ident, second_ident, homo_ident, homo_second_ident;
    int8_t reliable;                 /* 1: '+', 0: '?' (classify, main.py:95-104)                             */
} sd_final_row;
/* sd_stream_create's arguments plus the monomer names (the first header token: names are the keys, a repeated name
 * is one key), main.py's -i (min_identity), --second-best and the three logistic-regression coefficients.
 * SD_ERR_PARAM before any device work for a missing name, n_mono <= 0 or lr_coef NULL.
 * sd_stream_submit of a final-mode stream COPIES the reads (the buffers are still free on return, as in the raw mode):
 * the fallback identities of a batch need the read text when its rows come back, which can be at a later submit or
 * at collect.  (Keeping the caller's buffers alive until collect instead would make a raw-mode rule depend on the
 * mode; the copy is one memcpy per read, on the stream's host threads.) */
int sd_stream_create_final(sd_stream** out, const sd_params* p, const char* const* mono_names,
                           const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                           int32_t sub_batches, int32_t min_identity, int32_t second_best,
                           const double* lr_coef, char* errbuf, size_t errlen);
/* Kept rows of the oldest submitted job (FIFO), in read order: read r owns rows[row_off[r] .. row_off[r+1]).
 * alt (may be NULL; NULL is returned without second_best): n_rows x n_keys identities in key order, the _alt rows
 * of each kept block (main.py:161-165; the block's own key is `best`).  All arrays malloc'ed (sd_free).
 * SD_ERR_PARAM on a stream made by sd_stream_create (and sd_stream_collect on a final-mode stream). */
int sd_stream_collect_final(sd_stream* s, sd_final_row** rows, int64_t** row_off, int64_t* n_rows, double** alt,
                            char* errbuf, size_t errlen);
/* ---- final rows that stay on the device (SD_FLAG_DEVICE_FINAL in sd_params.reserved[1] at sd_stream_create_final) ------
 * The chain sd_stream_submit_dev -> final rows with nothing crossing to the host: every batch's compact records are
 * appended to the job's record store in HBM as with SD_FLAG_DEVICE_ROWS, and the batch's identity words (csrc/sd_ident.hip)
 * are kept beside them at the same index, device to device.  Behind the job's last batch the seam merge runs, one kernel
 * writes which record each merged row is, and the selection kernels (csrc/sd_final_dev.hip) apply the rule of
 * main.py:107-165 -- its arithmetic and the end of the rule are csrc/sd_final_dev.hpp, one text for the host's
 * PostProcessor::select and the kernels; the maximum searches are lane reductions there -- to every merged row: best
 * monomer, identity, second best, homopolymer ranks, '+' / '?', the min_identity filter; the kept rows are counted and
 * scanned.  The rows have the bytes sd_stream_collect_final returns, padding included.  No record, no identity word and
 * no host thread's assembly is involved (sd_stream_stats [9] stays 0).
 * Accepted by sd_stream_create_final and by sd_stream_create_final_devices with exactly one entry.  SD_ERR_PARAM, before
 * any device is touched: at sd_stream_create / sd_stream_create_devices (a raw-mode stream), with a device list of more
 * than one entry, together with SD_FLAG_PROFILE (the profile pass reads the kept rows and the text on the host), and
 * together with SD_FLAG_DEVICE_ROWS.  sd_stream_submit, sd_stream_submit_dev, sd_stream_keys, sd_stream_stats and
 * sd_stream_final_stats work unchanged.
 *
 * The text-based path.  Rows the words cannot decide are counted by the kernels, not guessed: a missing word (a pair the
 * identity kernels left out), a segment long enough for edlib's Hirschberg split against the longest monomer (about 19.6 kb
 * against 171 bp: -b >= 19000), a batch whose identity outputs had no room (its words are stored as zeroes).  A job with
 * such a row, and every job of a stream whose engines compute no identities (SD_FLAG_NO_STREAM_IDENT, a monomer set
 * the in-stream kernels do not take), is finished by the host instead: its merged raw rows and row offsets come to the
 * host, its reads too (the job keeps its copy, as every final-mode job does), the post-processor of the file path
 * computes every identity from the text, and the rows are copied into the caller's buffers on the caller's stream, which
 * the host waits for.  Correct and slow; sd_stream_final_stats [2] counts the blocks of such jobs.
 *
 * sd_stream_peek_final_dev waits for the oldest job (FIFO) and gives what its buffers need: *n_reads, *n_rows = the EXACT
 * number of kept rows (16 bytes from the device once the selection has run; min_identity can drop most rows and alt is
 * n_rows x n_keys doubles, so an upper bound would not do) and *n_keys.  The job stays.
 * sd_stream_collect_final_dev hands the oldest job over: d_rows[0 .. *n_rows), d_row_off (n_reads + 1) and, with
 * second_best, d_alt (n_rows x n_keys, key order; may be NULL and is ignored without second_best) -- DEVICE buffers of the
 * caller's on the stream's device (SD_ERR_PARAM / SD_ERR_UNSUPPORTED as in sd_stream_collect_dev).  Ordering on
 * hip_stream and ownership are those of sd_stream_collect_dev: the copy is enqueued on hip_stream behind an event of
 * the library's selection, nothing waits on the host beyond the count, and the buffers are the caller's alone afterwards.
 * cap_rows < *n_rows: SD_ERR_PARAM with *n_rows set, nothing is written and the job stays collectable.
 * The wrong collect for a stream's mode is SD_ERR_PARAM and leaves the job in place: sd_stream_collect,
 * sd_stream_collect_final and sd_stream_collect_dev on such a stream, these two calls on any other.
 * Out of scope: several device entries, SD_FLAG_PROFILE, and sd_engine (which has no final mode). */
int sd_stream_peek_final_dev(sd_stream* s, int32_t* n_reads, int64_t* n_rows, int32_t* n_keys, char* errbuf, size_t errlen);
int sd_stream_collect_final_dev(sd_stream* s, sd_final_row* d_rows, int64_t cap_rows, int64_t* d_row_off, double* d_alt,
                                void* hip_stream, int64_t* n_rows, char* errbuf, size_t errlen);
/* The distinct monomer names in key order (m0, m0', m1, m1', ... first occurrences): up to cap pointers, valid
 * until sd_stream_destroy; *n_keys = the number of keys.  SD_ERR_PARAM on a stream not in final mode. */
int sd_stream_keys(sd_stream* s, const char** keys, int32_t cap, int32_t* n_keys);
/* Identities of a final-mode stream, accumulated over its collected batches: [0] in-stream identity kernels, ms (HIP
 * events, as sd_last_run_stats [3]), [1] pairs computed in-stream (as [4]), [2] blocks whose identities came from
 * the fallback, [3] kept rows.  All 0 on a stream not in final mode. */
int sd_stream_final_stats(sd_stream* s, double out[4]);
/* A final-mode stream created with SD_FLAG_PROFILE: the profile summed over the jobs collected so far, in the form of
 * sd_last_run_profile.  reset != 0 (with counts given) zeroes it after the copy.  SD_ERR_PARAM on a raw-mode stream
 * or one created without the flag. */
int sd_stream_profile(sd_stream* s, int32_t reset, int32_t* n_monomers, int64_t* n_counts, int64_t* text_bytes,
                      char* text, uint64_t* counts);
/* ---- profiles folded on the device (SD_FLAG_DEVICE_PROFILE, with SD_FLAG_DEVICE_FINAL, at sd_stream_create_final) ------
 * A mode of its own beside SD_FLAG_PROFILE, whose pass reads the kept rows and the read text on the host (and stays
 * refused on a device-final stream).  Here, behind the selection of a job and on the same stream, one kernel plans the
 * pair of every kept row -- the segment the selection measured (the read's place in the job's text plus the clamped
 * [start, end]; length 0 is no instance) against the row's own interleaved template; csrc/sd_final_prof_dev.hpp, one
 * text for host and device -- the pairs of the fold kernel (set's longest template <= 512 bp, segment of 1 .. 1024 bp,
 * no Hirschberg split) are counted per forward monomer and scattered into groups, the others are compacted into a list
 * of 16 bytes each, and 4 (monomers + 2) bytes of summary reach pinned memory with the selection's counts.
 * sd_stream_collect_final_dev then sizes checkpoints, work items and grid from the summary and enqueues the fold kernel
 * of sd_profile_segments_dev on a stream the sd_stream owns, reading the job's own text in HBM -- the copy a
 * sd_stream_submit_dev job has anyway; a job submitted from host memory uploads its reads once, asynchronously -- and
 * adding into the stream's 64-bit counters in HBM.  No base, record or row crosses to the host.  The fold outlives the
 * collect: the job's workspace and text are not reused before the host has seen an event behind it, and
 * sd_stream_destroy waits for it.  Rows, row offsets and alt are byte for byte those of the stream without the flag.
 * What the host still folds, into counters of its own: the listed pairs (only their segments' text is fetched; a job
 * from host memory reads its own copy), and every job finished by the text-based path (above), through the pass of
 * SD_FLAG_PROFILE.  Totals = device counters + host counters.
 * SD_ERR_PARAM before any device is touched, in words that name both flags: on a raw-mode stream, without
 * SD_FLAG_DEVICE_FINAL, with a device list of more than one entry, with SD_FLAG_PROFILE, with a repeated monomer name.
 *
 * sd_stream_profile works on such a stream: it waits for the folds of the jobs whose sd_stream_collect_final_dev has
 * returned, copies the device counters down and adds the host's; reset zeroes both (the device's in order on the
 * stream's own stream).  A fold that ran out of checkpoints -- they are sized by the longest segment: it cannot -- is
 * SD_ERR_INTERNAL.
 * sd_stream_profile_dev places the same totals (*n_counts of them, the layout of sd_profile_segments) in d_counts, a
 * DEVICE buffer of the caller's on the stream's device with room for cap_counts, ordered on hip_stream: work enqueued
 * there afterwards sees them.  cap_counts too small (or d_counts NULL): SD_ERR_PARAM with *n_counts set and a message
 * that names the exact size; nothing is written.
 * sd_stream_profile_stats: [0] pairs folded on the device, [1] pairs folded on the host (listed pairs and the kept rows
 * of text-based jobs), [2] bytes of read text the profile fetched to the host, [3] fold kernels, ms (HIP events, of
 * the folds that have completed).  All 0 on any other stream. */
int sd_stream_profile_dev(sd_stream* s, int32_t reset, uint64_t* d_counts, int64_t cap_counts, void* hip_stream,
                          int64_t* n_counts, char* errbuf, size_t errlen);
int sd_stream_profile_stats(sd_stream* s, double out[4]);
/* The plan / group / fold alone, in the manner of sd_final_select_dev / _host: text = the reads back to back, read r =
 * text[read_off[r] .. read_off[r + 1]) (n_reads + 1 offsets); rows[row_off[r] .. row_off[r + 1]) = the rows of read r
 * (tmpl in the DP's order: monomer t, T + t = its reverse complement; start / end in read coordinates, clamped as the
 * selection clamps them), keep[b] != 0 = row b is a kept row; templates = the T FORWARD monomers.  counts (the layout
 * of sd_profile_segments) is overwritten; pairs[0] = pairs the fold kernel takes, pairs[1] = pairs left to the host.
 * _dev uploads its inputs (HOST arrays) and runs exactly the kernels the stream runs, then folds the listed pairs on
 * host threads; _host runs the same plan text on the host and folds every pair there (device is ignored). */
int sd_final_profile_dev(const char* text, const int64_t* read_off, int32_t n_reads, const sd_rec* rows, const int64_t* row_off,
                         const uint8_t* keep, const char* const* templates, const int32_t* tlen, int32_t T, int32_t device,
                         int32_t threads, uint64_t* counts, int64_t pairs[2]);
int sd_final_profile_host(const char* text, const int64_t* read_off, int32_t n_reads, const sd_rec* rows, const int64_t* row_off,
                          const uint8_t* keep, const char* const* templates, const int32_t* tlen, int32_t T, int32_t device,
                          int32_t threads, uint64_t* counts, int64_t pairs[2]);

/* ---- the TSV text of device rows, formatted on the device (csrc/sd_text_dev.hip) -------------------------------------
 * The last link of the device chain: the bytes of final_decomposition.tsv / _alt.tsv from the rows of
 * sd_stream_collect_final_dev, and of _raw.tsv from the rows of sd_stream_collect_dev / sd_engine_rows_dev, written into
 * DEVICE buffers of the caller's.  The bytes are those of the existing formatters (sd_format_rows for a raw row; the
 * twelve columns of main.py:153-160 and the six of :161-165, identities with "%.2f", "None" for key -1, '+' / '?', '*' /
 * '-'); csrc/sd_text_dev.hpp is their one text for the kernels and the _host calls below.
 *
 * Name tables.  An sd_text_tables holds the read names of a job (n_reads of them, the job's reads in submit order) and
 * the column names -- the keys of sd_stream_keys for final rows (n_cols = n_keys; "None" is added by the library), the
 * DP templates (monomers, then monomers + "'") for raw rows -- as byte strings plus offsets.  Creating one touches no
 * device; the first _dev call uploads it to that call's device, later calls reuse the upload (another device:
 * SD_ERR_PARAM), so a caller formatting many jobs of the same reads and monomers uploads once.  The object also owns
 * the small scratch of the size calls (tile sums, counters, 32 pinned bytes): calls on one object take turns, and
 * nothing is allocated per call once its buffers have grown.  The destroy call waits for the last write call's kernels.
 *
 * Two calls per job, both enqueued on hip_stream (NULL = the null stream) of `device`:
 *   1. the size call: a length pass over the rows, an exclusive int64 scan, and the positions --
 *      d_row_pos[n_rows + 1] (where the text of row i begins; for _alt: d_alt_pos, where the n_keys lines of final row
 *      i begin), d_read_pos[n_reads + 1] (where the text of read r begins: row_pos[row_off[r]]; _alt: d_alt_read_pos),
 *      and for raw rows d_row_read[n_rows] (the read of every row) -- all DEVICE scratch of the caller's, which the
 *      write call reads.  The host waits for 32 bytes and nothing else: *final_bytes / *alt_bytes (*text_bytes), the
 *      count of unprintable identities and the count of failed checks.
 *   2. the write call, with text buffers of exactly those sizes: returns without waiting; work enqueued on hip_stream
 *      afterwards sees the text.  Nothing is written at or behind final_bytes / alt_bytes / text_bytes.  rows, alt and
 *      the positions must be what the size call saw.
 * d_alt NULL (a job without second_best): no _alt text, d_alt_pos / d_alt_read_pos / d_alt_text are ignored.
 * Checked by the host before any kernel runs (SD_ERR_PARAM): NULL arguments, n_keys != the table's n_cols, a buffer that
 * is not device memory (SD_ERR_UNSUPPORTED: of another device, as in sd_stream_collect_dev).  Checked by the length
 * pass, which follows no index it has not checked, so before any byte of text is written (the size call returns
 * SD_ERR_PARAM): a read, key or template index outside its table, a final row outside its read's rows, row offsets that
 * do not rise from 0 to n_rows.  An identity that is infinite, NaN or >= 2^40 in size is printed by snprintf on the host;
 * the device counts it and the size call returns SD_ERR_UNSUPPORTED (no row the library produces holds one).
 * Without a device: SD_ERR_NO_DEVICE.  Every offset is 64-bit; a text of more than 4 GB per call is not tested. */
typedef struct sd_text_tables sd_text_tables;
int sd_text_tables_create(sd_text_tables** out, const char* const* read_names, int32_t n_reads, const char* const* col_names,
                          int32_t n_cols, char* errbuf, size_t errlen);
void sd_text_tables_destroy(sd_text_tables* t);
int sd_text_final_size_dev(sd_text_tables* t, const sd_final_row* d_rows, int64_t n_rows, const int64_t* d_row_off, const double* d_alt,
                           int32_t n_keys, int32_t device, void* hip_stream, int64_t* d_row_pos, int64_t* d_alt_pos,
                           int64_t* d_read_pos, int64_t* d_alt_read_pos, int64_t* final_bytes, int64_t* alt_bytes, char* errbuf,
                           size_t errlen);
int sd_text_final_write_dev(sd_text_tables* t, const sd_final_row* d_rows, int64_t n_rows, const double* d_alt, int32_t n_keys,
                            int32_t device, void* hip_stream, const int64_t* d_row_pos, const int64_t* d_alt_pos, char* d_final_text,
                            int64_t final_bytes, char* d_alt_text, int64_t alt_bytes, char* errbuf, size_t errlen);
int sd_text_raw_size_dev(sd_text_tables* t, const sd_rec* d_rows, int64_t n_rows, const int64_t* d_row_off, int32_t device,
                         void* hip_stream, int32_t* d_row_read, int64_t* d_row_pos, int64_t* d_read_pos, int64_t* text_bytes,
                         char* errbuf, size_t errlen);
int sd_text_raw_write_dev(sd_text_tables* t, const sd_rec* d_rows, int64_t n_rows, const int64_t* d_row_off, int32_t device,
                          void* hip_stream, const int32_t* d_row_read, const int64_t* d_row_pos, char* d_text, int64_t text_bytes,
                          char* errbuf, size_t errlen);
/* The same text from HOST arrays on `threads` host threads, without a device: *final_text / *alt_text / *text are
 * malloc'ed (sd_free) and hold *final_bytes / *alt_bytes / *text_bytes bytes; row_pos, alt_pos (n_rows + 1), read_pos
 * and alt_read_pos (n_reads + 1) may be NULL, else they are filled as the size calls fill theirs.  alt NULL: no _alt
 * text.  The same checks (SD_ERR_PARAM, nothing returned); unprintable identities are printed by snprintf. */
int sd_text_final_host(sd_text_tables* t, const sd_final_row* rows, int64_t n_rows, const int64_t* row_off, const double* alt,
                       int32_t n_keys, int32_t threads, char** final_text, int64_t* final_bytes, char** alt_text, int64_t* alt_bytes,
                       int64_t* row_pos, int64_t* alt_pos, int64_t* read_pos, int64_t* alt_read_pos, char* errbuf, size_t errlen);
int sd_text_raw_host(sd_text_tables* t, const sd_rec* rows, int64_t n_rows, const int64_t* row_off, int32_t threads, char** text,
                     int64_t* text_bytes, int64_t* row_pos, int64_t* read_pos, char* errbuf, size_t errlen);

/* ---- a stream on several devices of this process ----------------------------------------------------------------
 * sd_stream_create / sd_stream_create_final with a device list: one batch pipeline per entry of devices[0 .. n_devices)
 * (repeats allowed, as in sd_run_files_devices; p->device is ignored).  1 <= n_devices <= 16; every ordinal must exist
 * and be a gfx950 device, checked before any work starts on any of them (the checks and messages of
 * sd_run_files_devices; without a device SD_ERR_NO_DEVICE).  n_devices == 1 is the plain stream on devices[0]: driven
 * on the calling thread, no thread of its own.
 * With several entries each pipeline is driven by a thread of its own, bound to its device for the life of the stream.
 * A job is cut into at least 2 x n_devices batches (and sub_batches); the batches are numbered across jobs, each entry
 * takes the lowest one no entry has, and their records are assembled strictly in batch order, so the rows are those of
 * a single-device stream, in both modes.  Entries on the same device share its free HBM.  The other sd_stream_* calls
 * work unchanged, jobs are collected in FIFO order, and stats sum over the entries.  sd_stream_submit of a raw-mode
 * stream returns once every batch of the job has been packed by its entry (the read buffers are then free, as with one
 * device: no copy, but submit waits for the entries to have room for the job); a final-mode stream copies the reads
 * and returns at once.  The fallback identities run on devices[0].  The first push or pop failure of any stream, on one
 * entry or several, fails it: the batches in flight on every entry are drained, every outstanding job is dropped, and
 * the submit or collect that meets the failure reports it (with several entries the message is prefixed "device N: ").
 * sd_stream_destroy joins every thread. */
int sd_stream_create_devices(sd_stream** out, const sd_params* p, const int32_t* devices, int32_t n_devices,
                             const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, int32_t sub_batches,
                             char* errbuf, size_t errlen);
int sd_stream_create_final_devices(sd_stream** out, const sd_params* p, const int32_t* devices, int32_t n_devices,
                                   const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens,
                                   int32_t n_mono, int32_t sub_batches, int32_t min_identity, int32_t second_best,
                                   const double* lr_coef, char* errbuf, size_t errlen);
/* Per entry of a stream (one for a stream made without a device list): batches dealt to it and its device busy time
 * in ms (HIP-event spans of its batches, as sd_last_run_device_stats), up to cap entries; returns the number of
 * entries (0 for a NULL stream). */
int sd_stream_device_stats(sd_stream* s, int64_t* batches, double* busy_ms, int32_t cap);

/* ---- host-side pieces of the path, exported for CPU-only tests ----------------------------- */

/* chunk plan of one read (main.cpp:70-81): up to cap (offset,len) pairs; returns the count */
int32_t sd_chunk_plan(int64_t read_len, int32_t part_size, int32_t overlap, int64_t* off,
                      int32_t* len, int32_t cap);
/* PostProcessing seam merge (main.cpp:287-302), in place; returns the new count */
int32_t sd_seam_merge(sd_rec* recs, int32_t n);
/* SaveBatch text of one read's rows (main.cpp:272-285); *txt malloc'ed (sd_free) */
int sd_format_rows(const char* read_name, const char* const* tmpl_names, const sd_rec* rows,
                   int32_t n_rows, char** txt, size_t* txt_len);
/* 2-bit packing of a chunk as the device reads it (16 bases per dword, base i at bits 2*(i&15), A,C,G,T
 * = 0..3, N = 0 + a set bit in the optional 1-bit mask); returns 1 if the chunk holds an N, -1 on bad
 * arguments.  words: (n+15)/16 dwords, nmask (may be NULL): (n+31)/32 dwords. */
int32_t sd_pack_bases(const char* seq, int64_t n, uint32_t* words, uint32_t* nmask);
/* The device packer alone, results on the host (for tests): chunk c = d_bases[chunk_off[c] .. chunk_off[c] + chunk_len[c])
 * in the memory of `device`, packed on hip_stream.  bases2: the chunks' words back to back ((len+15)/16 dwords each);
 * nmask: (len+31)/32 dwords per chunk back to back, written ONLY for the chunks that hold an N (the others keep what the
 * caller put there); has_n[c] (may be NULL): 1 / 0; *first_bad (may be NULL): the smallest offset into d_bases of a
 * byte outside A C G T N, or -1.  SD_ERR_PARAM for bad arguments or memory that is not device memory,
 * SD_ERR_UNSUPPORTED when it belongs to another device. */
int sd_pack_bases_dev(const void* d_bases, const int64_t* chunk_off, const int32_t* chunk_len, int32_t n_chunks,
                      int32_t device, void* hip_stream, uint32_t* bases2, uint32_t* nmask, int32_t* has_n,
                      int64_t* first_bad);
/* The assembly kernels alone (for tests): read r = d_recs[d_read_off[r] .. d_read_off[r + 1]), records already in
 * read-global coordinates, d_read_off[0] = 0; all four arrays in the memory of `device`, d_rows with room for every
 * record.  piece = records per piece of the merge, 0 = the production value, 1..7 SD_ERR_PARAM (a step of the merge
 * reaches 8 records ahead).  Runs on hip_stream and returns when it is done.  SD_ERR_NO_DEVICE without a device. */
int sd_seam_merge_dev(const sd_rec* d_recs, const int64_t* d_read_off, int32_t n_reads, int32_t piece, int32_t device,
                      void* hip_stream, sd_rec* d_rows, int64_t* d_row_off, int64_t* n_rows);
/* Host only: the same piece functions (exit tables, their composition, keep flags) run by the host, read by read; the
 * rows must equal sd_seam_merge's.  Arguments as above, in host memory. */
int sd_seam_pieces_selftest(const sd_rec* recs, const int64_t* read_off, int32_t n_reads, int32_t piece, sd_rec* rows,
                            int64_t* row_off, int64_t* n_rows);
/* The device prefix scan of the post-pass units alone (for tests; csrc/sd_scan_dev.hpp): out[i] = values[0] + .. +
 * values[i - 1] for i = 0 .. n, so out holds n + 1 entries and out[n] is the total; values and out in host memory,
 * 0 <= n < 2^31.  tile_sums_32 != 0: the sums per tile of 256 values are kept as int32 (the form of the units that
 * count flags), else as int64.  Returns when it is done.  SD_ERR_NO_DEVICE without a device. */
int sd_scan_selftest(const int64_t* values, int64_t n, int32_t tile_sums_32, int32_t device, int64_t* out);
/* The selection kernels alone (for tests): the rows of n_reads reads (read r = d_rows[d_row_off[r] .. d_row_off[r + 1]),
 * read-global, already merged), row b's identity words at d_words / d_hwords + d_widx[b] * per (plain / homopolymer-
 * compressed; per = 1, the word of the row's own monomer, or with second_best 2 * n_mono, one per interleaved template
 * m0, m0', m1, ...; 0 <= d_widx[b] < n_word_rows) and d_read_len (may be NULL: segments are not clamped to their read),
 * all in the memory of `device`.  The tables are built from the monomers, min_identity, second_best and lr_coef the way
 * a final-mode stream builds them.  d_out (room for every row), d_out_off (n_reads + 1) and d_alt (every row x n_keys,
 * second_best only) receive the kept rows; *n_rows = how many, *n_undecided = the rows the words do not decide (a word
 * 0 or 0xffffffff, a segment edlib aligns by Hirschberg's split), which are counted and not kept.  Runs on hip_stream and
 * returns when it is done.  SD_ERR_PARAM for bad arguments (offsets, word indices and templates are checked on the
 * host before any kernel runs), SD_ERR_NO_DEVICE without a device. */
int sd_final_select_dev(const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                        int32_t min_identity, int32_t second_best, const double* lr_coef, const sd_rec* d_rows,
                        const int64_t* d_row_off, int32_t n_reads, const int64_t* d_widx, const uint32_t* d_words,
                        const uint32_t* d_hwords, int64_t n_word_rows, int32_t per, const int64_t* d_read_len, int32_t device,
                        void* hip_stream, sd_final_row* d_out, int64_t* d_out_off, double* d_alt, int64_t* n_rows,
                        int64_t* n_undecided);
/* Host only: the same arguments in host memory, answered by the host's selection (PostProcessor::select) itself. */
int sd_final_select_host(const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                         int32_t min_identity, int32_t second_best, const double* lr_coef, const sd_rec* rows,
                         const int64_t* row_off, int32_t n_reads, const int64_t* widx, const uint32_t* words,
                         const uint32_t* hwords, int64_t n_word_rows, int32_t per, const int64_t* read_len,
                         sd_final_row* out, int64_t* out_off, double* alt, int64_t* n_rows, int64_t* n_undecided);
/* The --ed_thr prefilter's result alone, on the host (for tests): valid after sd_engine_fetch of a batch run with
 * ed_thr > -1, else SD_ERR_PARAM.  dist[chunk][T]: the infix edit distance of every template against every chunk, chunks
 * in the order of sd_engine_fetch; rank[chunk][T]: the template's position in the chunk's filtered order (by distance,
 * then index; the first and every distance <= ed_thr kept), 0xffff = dropped -- decoded here from the table the engine's
 * kernel family reads (rank table, per-lane constants, or compacted kept list); after a batch that a guard trip made the
 * engine repeat, the tables of the repeat.  cap: entries each array has room for (>= n_chunks x T, both returned through
 * n_chunks / n_templates, which may be NULL).  Launches nothing; the copies happen inside this call only. */
int sd_engine_filter_result(sd_engine* e, int32_t* dist, uint16_t* rank, int64_t cap, int64_t* n_chunks,
                            int32_t* n_templates, char* errbuf, size_t errlen);
/* Self-test of the file writer behind sd_run_files (no device): n_parts parts of part_bytes bytes appended to
 * `path` in two calls, read back and compared.  fail_reserve != 0 makes the page reservation of the mapped
 * (tmpfs) path fail, as on a full /dev/shm -- the text must then arrive through the pwritev loop, which reports
 * ENOSPC as SD_ERR_IO instead of dying of SIGBUS.  out (may be NULL): [0] bytes written, [1] 1 on tmpfs / ramfs. */
int sd_write_parts_selftest(const char* path, int32_t n_parts, int64_t part_bytes, int32_t threads,
                            int32_t fail_reserve, int64_t out[2]);
/* Host only (CPU test): the pipeline-cache key (which jobs share cached engines) and the batch planner (how a job is cut
 * into device batches) against their contracts, without a device; SD_OK, or SD_ERR_INTERNAL with the broken property. */
int sd_pipeline_logic_selftest(char* errbuf, size_t errlen);
/* Self-test of the batch dealing of sd_run_files_devices (no device): the plan of 1..16 device entries cuts a chunk
 * table into contiguous, covering batches of equal share, at least 2 x entries of them where the chunks allow; batches
 * that complete on several threads in shuffled order are consumed strictly in batch order, slice by slice; a batch that
 * fails on one pipeline (pushed, popped, or popped while it drains) ends the job on every driver thread with an in-order
 * prefix consumed, and an aborted job releases every waiter.  SD_OK, or SD_ERR_INTERNAL with the broken property in errbuf. */
int sd_multi_device_selftest(char* errbuf, size_t errlen);
/* Rates of the host stages alone (no device): out[0] = chunk table + 2-bit packing, bp/s; out[1] = per-read
 * assembly (chunk offsets, seam merge) + raw TSV text of one synthetic record per 171 bases, bp/s; out[2] =
 * TSV rows/s; out[3] = bytes of text per pass.  p->threads host threads, `iters` passes over the reads. */
int sd_host_stage_rates(const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads,
                        const sd_params* p, int32_t iters, double out[4]);
/* FASTA validation + load with the reference's semantics (main.cpp:314-346).  Arrays malloc'ed,
 * free with sd_fasta_free. */
typedef struct sd_fasta {
    int32_t n;
    char** names;
    char** seqs;
    int64_t* lens;
    int32_t has_n;
} sd_fasta;
int sd_fasta_load(const char* path, sd_fasta* out, char* errbuf, size_t errlen);
/* The same with flags: SD_FLAG_LENIENT reads the file leniently (above); sd_fasta_load is flags == 0.  Both read FASTQ. */
int sd_fasta_load_ex(const char* path, int32_t flags, sd_fasta* out, char* errbuf, size_t errlen);
void sd_fasta_free(sd_fasta* f);

/* ---- post-processing helper (host): identity of a read segment vs a template ---------------
 * What main.py:29-60 (edist + aai) obtains from python-edlib: unit-cost global alignment
 * (edlib mode "NW", task "path"), number of '=' columns and total CIGAR columns.  Traceback from
 * the bottom-right corner with priority up (consume query, 'I') > left (consume target, 'D') >
 * diagonal, i.e. edlib's obtainAlignmentTraceback (edlib.cpp:945-1150); pairs whose traceback data would
 * reach 1 MB (~19.6 kb against a 171-bp target) by Hirschberg's split of the target as edlib does
 * (edlib.cpp:1186-1400).  Any byte alphabet (a symbol matches itself only), sequences of up to 2^27.
 * matches[i] = columns[i] = 0 and dist[i] = -1 if either sequence is empty (main.py:30-33).
 * Multi-threaded over pairs (threads >= 1). */
int sd_nw_identity_batch(const char* const* queries, const int32_t* qlens,
                         const char* const* targets, const int32_t* tlens, int64_t n_pairs,
                         int32_t threads, int32_t* dist, int32_t* matches, int32_t* columns);

/* The forms convert_read needs (main.py:107-150): segment s = seq[starts[s] .. ends[s]] (inclusive,
 * as in the raw TSV) is the query, a template the target.
 *   pair_tmpl == NULL: all-vs-all (--second-best), result index s * T + t;
 *   pair_tmpl != NULL: segment s against template pair_tmpl[s] only (light mode), result index s.
 * homo != 0 compresses homopolymer runs on both sides first (convert_to_homo, main.py:87-92).
 * Multi-threaded over segments. */
int sd_identity_segments(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends,
                         int64_t n_seg, const char* const* tmpl, const int32_t* tlen, int32_t T,
                         const int32_t* pair_tmpl, int32_t homo, int32_t threads, int32_t* dist,
                         int32_t* matches, int32_t* columns);

/* The same on the device (csrc/sd_nw.hip, Myers bit-vectors and edlib's traceback priority): identical results.
 * The route follows the longest template AFTER the homopolymer compression of a homo call:
 *   up to 512 bp   one lane per (segment, template) pair, a per-lane delta history in HBM.  The call as a whole is
 *                  SD_ERR_UNSUPPORTED when the longest segment against the longest template (lengths before
 *                  compression) is long enough for edlib's Hirschberg split: 20 * ceil(q / 64) * t + 8 * t >= 2^20.
 *   513 .. 2048 bp a pair across 16 or 32 lanes (csrc/sd_nw_long.hip).  The pairs are dealt one by one, by their
 *                  lengths before compression: a pair edlib would split, and every pair of a segment longer than 8192
 *                  symbols, is aligned by host threads inside the same call (under the kernel); the others go to
 *                  the device.  The results are the same wherever a pair went.
 *   beyond 2048 bp SD_ERR_UNSUPPORTED.
 * Also SD_ERR_UNSUPPORTED: a symbol outside ACGTN in a template or the text, a segment longer than 65000 bp, no
 * device memory for the call's buffers.  Callers then use sd_identity_segments.
 * SD_ERR_NO_DEVICE without a GPU.  Device buffers are kept between calls (sd_nw_release_cache frees them). */
int sd_identity_segments_dev(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends,
                             int64_t n_seg, const char* const* tmpl, const int32_t* tlen, int32_t T,
                             const int32_t* pair_tmpl, int32_t homo, int32_t device, int32_t threads,
                             int32_t* dist, int32_t* matches, int32_t* columns);
void sd_nw_release_cache(void);

/* Which route the device identity calls of this process took (sd_identity_segments_dev and every caller of the same
 * driver: the file job's post-processing, the stream's fallback).  Cumulative, read-only, never reset:
 *   [0] long_calls       calls that took the 513 .. 2048 bp route
 *   [1] long_pairs       pairs of those calls handed to the kernel of csrc/sd_nw_long.hip
 *   [2] long_host_pairs  pairs of those calls dealt to host threads (pairs with an empty side are in neither count)
 *   [3] long_rounds_max  the most rounds of pairs a workgroup of one long launch took: ceil(pairs / (grid * slots))
 *   [4] short_calls      calls that took the route of templates up to 512 bp
 *   [5] short_pairs      their pairs (all of them: that route deals nothing to the host)
 *   [6] declined_calls   calls that returned SD_ERR_UNSUPPORTED
 *   [7] 0 (reserved) */
void sd_nw_route_counts(int64_t out[8]);

/* ---- monomer column profiles (--profile) -----------------------------------------------------------------------
 * The alignment behind a row's identity (edlib NW path of the block against its monomer, Hirschberg's split where
 * edlib takes it), folded into the FORWARD monomer: a pair against rc(m) (length L) counts rc position q at L-1-q,
 * insertion slot h at L-h, and its bases complemented.  Per monomer, SD_PROFILE_COLS counters for every slot
 * g = 0..L, in this order:
 *   [0..4] read bases A C G T N aligned to template position g (g < L)   [5] deletions of position g (g < L)
 *   [6] instances with at least one read base inserted in slot g (bases before position g, after g - 1)
 *   [7..11] the inserted bases of slot g, A C G T N
 * Monomer t's block starts at sum over t' < t of (tlen[t'] + 1) * SD_PROFILE_COLS.  A pair with an empty side is not
 * an instance.  Read bases other than ACGT count as N. */
#define SD_PROFILE_COLS 12

/* Segment s = seq[starts[s] .. ends[s]] (inclusive) against monomer pair_tmpl[s] >> 1, its reverse complement when
 * pair_tmpl[s] & 1 (the interleaved order m0, m0', m1, m1', ...).  tmpl / tlen / T: the FORWARD monomers.  counts
 * (sum of (tlen + 1) * SD_PROFILE_COLS) is overwritten.  Host threads (sd_profile_segments) or the device
 * (sd_profile_segments_dev: the profile kernel of csrc/sd_nw.hip, with the host form for the pairs it does not take
 * -- monomers over 512 bp, segments over 1024 bp, pairs edlib splits). */
int sd_profile_segments(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                        const char* const* tmpl, const int32_t* tlen, int32_t T, const int32_t* pair_tmpl,
                        int32_t threads, uint64_t* counts);
int sd_profile_segments_dev(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends,
                            int64_t n_seg, const char* const* tmpl, const int32_t* tlen, int32_t T,
                            const int32_t* pair_tmpl, int32_t device, int32_t threads, uint64_t* counts);
/* ---- one row per instance (--msa): the same alignment, not summed ------------------------------------------------
 * The per-instance counterpart of the profile: the row of a pair (segment, interleaved template il) against the
 * FORWARD monomer il >> 1 of length L, SD_MSA_PITCH(L) bytes:
 *   [0, L)       per forward position g: 0..4 = the read base aligned there (A C G T N), SD_MSA_DEL = the position is
 *                deleted, SD_MSA_NONE = the pair is no instance or was not computed
 *   [L, 2L + 1)  per insertion slot g = 0..L: the read bases inserted before position g, saturating at 255
 *   padding      0, up to a multiple of 16 bytes
 * A pair against rc(m) lands reversed and complemented, exactly as in the profile (position p at L-1-p, slot h at L-h).
 * Per pair a status byte: 0 = no instance (an empty side), 1 = computed, 2 = left out by a device-resident call (the row
 * is then SD_MSA_NONE / 0).  The rows of a job, summed per monomer, are its profile: columns 0..6 exactly, and the
 * inserted bases as one number (the sum of columns 7..11) wherever no count saturated. */
#define SD_MSA_DEL 5
#define SD_MSA_NONE 7
#define SD_MSA_PITCH(L) ((2 * (L) + 1 + 15) & ~15)

/* row_at[0 .. n_seg]: where the row of each pair begins when the rows lie back to back in the pairs' order (tlen / T:
 * the FORWARD monomers, pair_tmpl: interleaved).  Returns the total bytes (row_at[n_seg]), or -SD_ERR_PARAM for a
 * template out of range. */
int64_t sd_msa_row_offsets(const int32_t* tlen, int32_t T, const int32_t* pair_tmpl, int64_t n_seg, int64_t* row_at);
/* The arguments of sd_profile_segments[_dev]; rows (sd_msa_row_offsets' total bytes), row_at (n_seg + 1) and status
 * (n_seg) are overwritten.  Host threads (sd_msa_segments: every pair, any length, any byte alphabet -- a read byte
 * outside ACGT counts as N) or the device (sd_msa_segments_dev: the row kernel of csrc/sd_msa.hip, and under it the host
 * form for the pairs it does not take -- a set with a monomer over 512 bp, segments over 1024 bp, pairs edlib splits, a
 * text outside ACGTN).  Every status is 0 or 1 and the two calls give the same bytes. */
int sd_msa_segments(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                    const char* const* tmpl, const int32_t* tlen, int32_t T, const int32_t* pair_tmpl, int32_t threads,
                    uint8_t* rows, int64_t* row_at, uint8_t* status);
int sd_msa_segments_dev(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                        const char* const* tmpl, const int32_t* tlen, int32_t T, const int32_t* pair_tmpl, int32_t device,
                        int32_t threads, uint8_t* rows, int64_t* row_at, uint8_t* status);

/* Developer entry (tools/msa_bench.py): the arguments of sd_msa_segments_dev; on the pairs the row kernel takes, the row
 * kernel and the profile kernel run warmup + reps times in turn, each launch between two HIP events: ms_msa[reps],
 * ms_profile[reps]; info = K, grid, work items, pairs, LDS bytes of the row kernel, rows staged in LDS (1) or written
 * through (0), LDS bytes of the profile kernel, checkpoint slots per lane.  SD_ERR_UNSUPPORTED when no pair is the kernels'. */
int sd_msa_kernel_bench(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                        const char* const* tmpl, const int32_t* tlen, int32_t T, const int32_t* pair_tmpl, int32_t device,
                        int32_t warmup, int32_t reps, float* ms_msa, float* ms_profile, int64_t info[8]);

/* ---- the rows of a device-final job, device to device ----------------------------------------------------------------
 * The last link of the chain sd_stream_submit_dev -> sd_stream_collect_final_dev: the final rows in HBM and the reads'
 * text in HBM give the rows of --msa in the caller's device buffers, in the manner of sd_text_final_size_dev /
 * sd_text_final_write_dev.  An sd_msa_tables holds what does not change between jobs: key_il[k] = the interleaved
 * template that key k (sd_stream_keys) names -- a key must name ONE template, so a set with a repeated monomer name has
 * no such table -- and the FORWARD monomers; the first size pass uploads them to its device.  The object also owns the
 * plan between a size pass and its write pass, so the two are called in pairs, one pair at a time per object; a size
 * pass waits for the object's previous write pass.  Destroy waits for the last write pass.
 *
 * sd_msa_final_size_dev: d_rows[0 .. n_rows) as sd_stream_collect_final_dev delivers them; d_text / read_off / read_lens
 * (host arrays, n_reads each) as sd_stream_submit_dev takes them: read r is d_text[read_off[r] .. + read_lens[r]), complete
 * on hip_stream.  On hip_stream: the reads are copied back to back into the object's own text, one kernel plans each
 * row's pair -- the segment the selection measured (csrc/sd_final_prof_dev.hpp: final_prof_pair, the same clamp and
 * limits) against the row's own template keys[best] -- and the pitches are scanned into d_row_at (n_rows + 1, the
 * caller's).  *total_bytes and classes[3] = rows that are no instance (status 0), pairs of the row kernel (status 1),
 * pairs the kernel does not take (a set with a monomer over 512 bp, a segment over 1024 bp, a pair edlib splits: status 2)
 * come to the host: the only wait.  SD_ERR_PARAM for a row whose read or key index lies outside its table.
 * sd_msa_final_write_dev (same d_rows, n_rows, device): groups the kernel's pairs by forward monomer on the device
 * (csrc/sd_final_prof_dev.hip) and runs the row kernel (csrc/sd_msa.hip) into d_out (cap bytes, 16-byte aligned) at
 * d_row_at, with d_status (n_rows); rows of status 0 and 2 are filled with SD_MSA_NONE / 0 -- counted, never guessed
 * (sd_msa_segments on the host computes them).  Everything is ordered on hip_stream and nothing waits on the host.
 * cap < *total_bytes: SD_ERR_PARAM with the exact size in the message, nothing written.  Buffers that are not device
 * memory: SD_ERR_PARAM; another device's: SD_ERR_UNSUPPORTED. */
typedef struct sd_msa_tables sd_msa_tables;
int sd_msa_tables_create(sd_msa_tables** out, const int32_t* key_il, int32_t n_keys, const char* const* mono_seqs,
                         const int32_t* mono_lens, int32_t n_mono, char* errbuf, size_t errlen);
void sd_msa_tables_destroy(sd_msa_tables* t);
int sd_msa_final_size_dev(sd_msa_tables* t, const sd_final_row* d_rows, int64_t n_rows, const void* d_text, const int64_t* read_off,
                          const int64_t* read_lens, int32_t n_reads, int32_t device, void* hip_stream, int64_t* d_row_at,
                          int64_t* total_bytes, int64_t classes[3], char* errbuf, size_t errlen);
int sd_msa_final_write_dev(sd_msa_tables* t, const sd_final_row* d_rows, int64_t n_rows, int32_t device, void* hip_stream,
                           const int64_t* d_row_at, uint8_t* d_out, int64_t cap, uint8_t* d_status, char* errbuf, size_t errlen);

/* ---- identity against lag (--lags): every row against its next D neighbours in the same read ---------------------------
 * Rows in file order; a read (group) owns rows x = 0 .. n-1.  For 1 <= d <= D and x + d < n the pair (x, d) aligns
 * query = the segment of row x against target = the segment of row x + d -- both as they stand in the read, nothing is
 * reverse-complemented, so a pair across an inversion scores low -- and yields (dist, matches) exactly as
 * sd_nw_identity_batch defines them.  Result index s * D + (d - 1) for segment s:
 *   dist >= 0   computed              dist = -1, matches = 0   no partner at that lag (the read ends), or an empty side
 *   dist = -2, matches = 0            left out by a device-resident call (below)
 * sums[(g * D + d - 1) * 3 + {0, 1, 2}] = over the pairs of group g at lag d with dist >= 0: their number n, the sum M of
 * matches, the sum C of dist + matches.  The pooled identity of a lag is M / C; a read's period is the lag with the largest
 * pooled identity among the lags with n > 0, compared by 128-bit cross products, ties to the smallest lag, 0 when the read
 * has fewer than two rows (csrc/sd_lags.hpp: one text for host and device).  1 <= D <= 255, else SD_ERR_PARAM before any
 * device work.  segments x D must stay below 2^31 (SD_ERR_UNSUPPORTED).
 *
 * sd_lag_segments: host threads, any length, any byte alphabet.  Segment s = seq[starts[s] .. ends[s]] (inclusive);
 * segments group_off[g] .. group_off[g + 1] are the rows of one read (group_off[0] = 0, group_off[n_groups] = n_seg).
 * dist / matches (n_seg x D) and sums (n_groups x D x 3) are overwritten.
 * sd_lag_segments_dev: the lane kernel of csrc/sd_lags.hip -- one lane per pair, which builds the match masks of its own
 * target in LDS and runs the identity kernel's walk on them -- for targets up to 512 bp and queries up to 1024 bp that
 * edlib does not split, over a text in ACGTN; the host form under it for every other pair.  The same arrays byte for byte,
 * no -2 ever appears. */
int sd_lag_segments(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                    const int64_t* group_off, int32_t n_groups, int32_t D, int32_t threads, int32_t* dist, int32_t* matches,
                    int64_t* sums);
int sd_lag_segments_dev(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                        const int64_t* group_off, int32_t n_groups, int32_t D, int32_t device, int32_t threads, int32_t* dist,
                        int32_t* matches, int64_t* sums);
/* The device-resident form, the last link of sd_stream_submit_dev -> sd_stream_collect_final_dev: d_rows[0 .. n_rows) as
 * sd_stream_collect_final_dev delivers them (rows of a read adjacent; partners are found from sd_final_row.read), d_text /
 * read_off / read_lens (host arrays, n_reads each) as sd_stream_submit_dev takes them.  A row's segment is the one its
 * identity column measured (read[start : end + 1] as Python clamps it).  d_dist / d_matches (n_rows x D int32) and d_sums
 * (n_reads x D x 3 int64) are the caller's, on `device`.  Everything is ordered on hip_stream; the host waits once, for
 * classes[3] = entries with dist -1 / pairs of the lane kernel / pairs left out as -2 (they add up to n_rows x D), which
 * also size the kernel's launches.  The call returns with the kernels in flight; its workspace is kept per device, and the
 * next call on that device first waits for them.  Buffers not in device memory: SD_ERR_PARAM; another device's:
 * SD_ERR_UNSUPPORTED; a row whose read index lies outside the reads: SD_ERR_PARAM.
 * sd_lag_final_host: the same from host arrays (text: the reads at read_off), every pair computed, no device needed. */
int sd_lag_final_dev(const sd_final_row* d_rows, int64_t n_rows, const void* d_text, const int64_t* read_off,
                     const int64_t* read_lens, int32_t n_reads, int32_t D, int32_t device, void* hip_stream, int32_t* d_dist,
                     int32_t* d_matches, int64_t* d_sums, int64_t classes[3], char* errbuf, size_t errlen);
int sd_lag_final_host(const sd_final_row* rows, int64_t n_rows, const char* text, const int64_t* read_off, const int64_t* read_lens,
                      int32_t n_reads, int32_t D, int32_t threads, int32_t* dist, int32_t* matches, int64_t* sums);
/* What the two files of --lags print: out[i] = the identity in percent of (dist[i], matches[i]) by the identity column's
 * arithmetic, -1 for dist < 0; period[g] and pooled[g * D + d - 1] (-1 for a lag without pairs) of each group's sums. */
void sd_lag_identities(const int32_t* dist, const int32_t* matches, int64_t n, double* out);
void sd_lag_periods(const int64_t* sums, int64_t n_groups, int32_t D, int32_t* period, double* pooled);
/* Developer entry (tools/lags_bench.py): the arguments of sd_lag_segments_dev; warmup + reps times each, between two HIP
 * events: ms_group = plan + scan + scatter, ms_pairs = the lane kernels with their reduction, ms_walk = the same without
 * it, ms_ident = the light identity kernel (csrc/sd_nw.hip) on as many pairs -- the same queries against one target of the
 * most frequent word class.  info = lane-kernel pairs, host pairs, K of the most frequent class, its pairs, checkpoint
 * slots and grid of the yardstick, grid and checkpoint slots of that class.  SD_ERR_UNSUPPORTED when no pair is the kernel's. */
int sd_lag_kernel_bench(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                        const int64_t* group_off, int32_t n_groups, int32_t D, int32_t device, int32_t warmup, int32_t reps,
                        float* ms_group, float* ms_pairs, float* ms_walk, float* ms_ident, int64_t info[8]);

/* ---- all-against-all identity in bins (--heatmap): every row against every earlier row of the same read -----------------
 * Rows in file order; a read (group) owns rows x = 0 .. n-1.  B rows per bin (1 <= B <= 2^20): row x lies in bin x / B, the
 * group has nb = ceil(n / B) bins.  The pairs of a group are all (x, y) with x < y, and with y - x <= W when W > 0 (W = 0:
 * no limit).  Query = the segment of row x, the earlier one; target = the segment of row y; (dist, matches) exactly as
 * sd_nw_identity_batch defines them, so pair (x, y) is the pair (x, d = y - x) of sd_lag_segments bit for bit.  A pair with
 * an empty side does not exist.  Cell (I, J), I <= J, of a group holds {n, M, C}: the number of pairs with x in bin I and y
 * in bin J, the sum of their matches, the sum of their dist + matches.  The cells of a group are the row-major upper
 * triangle, cell I * nb - I (I - 1) / 2 + (J - I); group g starts at cell_off[g], the prefix sum of nb (nb + 1) / 2:
 * sums[(cell_off[g] + cell) * 3 + {0, 1, 2}].  The pooled identity of a cell is M / C by the identity column's arithmetic,
 * -1 for a cell without pairs (sd_heat_identities).  No per-pair result exists anywhere: memory is O(rows + cells).
 * Refused with SD_ERR_PARAM and the numbers in errbuf, before any pair is aligned: B, W or max_pairs out of range; more
 * than SD_HEAT_CELLS_MAX cells in the call (805 MB of sums); more pairs than max_pairs (0: no limit).
 *
 * sd_heat_layout: the closed forms, host only: cell_off[0 .. n_groups] (may be NULL), the cells and the pairs of the groups.
 * sd_heat_segments: host threads, any length, any byte alphabet; segments and groups as sd_lag_segments takes them.
 * which = 0: every pair; which = 1: only the pairs the kernel does not take (below).  sums (cells x 3) is overwritten.
 * sd_heat_segments_dev: the kernel of csrc/sd_heat.hip -- a wave per (target, strip of up to 64 consecutive queries): the
 * wave builds the target's match masks once, in LDS, every lane walks its own query against them, and the wave reduces
 * {1, matches, dist + matches} per cell before one triple of 64-bit atomic adds -- for targets up to 512 bp and queries up to
 * 1024 bp that edlib does not split, over a text in ACGTN; the host form with which = 1 added to it.  The same bytes as
 * sd_heat_segments(which = 0).  classes = {pairs of the kernel, pairs of the host, pairs with an empty side}. */
#define SD_HEAT_CELLS_MAX ((int64_t)1 << 25)
int sd_heat_layout(const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int64_t* cell_off, int64_t* cells_total,
                   int64_t* pairs);
int sd_heat_segments(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                     const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int64_t max_pairs, int32_t which,
                     int32_t threads, int64_t* sums, char* errbuf, size_t errlen);
int sd_heat_segments_dev(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                         const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int64_t max_pairs, int32_t device,
                         int32_t threads, int64_t* sums, int64_t classes[3], char* errbuf, size_t errlen);
/* The device-resident form, behind sd_stream_submit_dev -> sd_stream_collect_final_dev: d_rows, d_text, read_off and
 * read_lens as sd_lag_final_dev takes them; a group is a read, its rows adjacent and the reads ascending (else
 * SD_ERR_PARAM).  d_sums (n_cells x 3 int64) is the caller's, on `device`; n_cells must be what sd_heat_layout gives for
 * the rows per read (else SD_ERR_PARAM: nothing is written).  Everything is ordered on hip_stream.  The host waits twice:
 * for the rows per read and their lengths (the closed forms, the two refusals and classes), then for the work items per
 * word class, which size the launches.  The pairs the kernel does not take are left out and counted in classes[1].  The
 * call returns with the kernels in flight; its workspace is kept per device, and the next call on that device first waits
 * for them.
 * sd_heat_final_host: the same from host arrays, with the `which` of sd_heat_segments: the device sums plus the sums of
 * which = 1 are the sums of which = 0. */
int sd_heat_final_dev(const sd_final_row* d_rows, int64_t n_rows, const void* d_text, const int64_t* read_off,
                      const int64_t* read_lens, int32_t n_reads, int64_t B, int64_t W, int64_t max_pairs, int32_t device,
                      void* hip_stream, int64_t* d_sums, int64_t n_cells, int64_t classes[3], char* errbuf, size_t errlen);
int sd_heat_final_host(const sd_final_row* rows, int64_t n_rows, const char* text, const int64_t* read_off, const int64_t* read_lens,
                       int32_t n_reads, int64_t B, int64_t W, int64_t max_pairs, int32_t which, int32_t threads, int64_t* sums,
                       int64_t n_cells, int64_t classes[3], char* errbuf, size_t errlen);
/* out[i] = the pooled identity in percent of cell i (sums + 3 i), -1 for a cell without pairs. */
void sd_heat_identities(const int64_t* sums, int64_t n_cells, double* out);
/* Developer entry (tools/heat_bench.py): the arguments of sd_heat_segments_dev; warmup + reps times each, between two HIP
 * events: ms_group = plan + scatter + scan, ms_pairs = the pair kernels, ms_walk = the same with the masks built once per
 * wave and without the reduction (the walk alone; its sums mean nothing).  info = kernel pairs, host pairs, K of the word
 * class with most work items, work items, cells, work items / grid / checkpoint slots of that class. */
int sd_heat_kernel_bench(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                         const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int32_t device, int32_t warmup,
                         int32_t reps, float* ms_group, float* ms_pairs, float* ms_walk, int64_t info[8]);

/* ---- k-mer autocorrelation of every read against itself (--autocorr): no monomer file, a period in bases ----------------
 * A read is a text T[0 .. n).  Two positions match when they hold the same byte and that byte is one of A C G T; N and
 * every other byte match nothing, themselves included.  For 1 <= k <= SD_AUTOCORR_KMAX and a lag d >= 1, position i is a hit
 * at lag d when 0 <= i <= n - d - k and T[i + j] matches T[i + d + j] for j = 0 .. k - 1: the k-mer at i recurs at i + d
 * and neither copy holds an N.  With a window length W in bases (W = 0: one window, the whole read) read r has
 * max(1, ceil(n / W)) windows, window w = [w W, min(n, (w + 1) W)), and starts at window win_off[r] of the call.
 * counts[(win_off[r] + w) * D + d - 1], d = 1 .. D, is the number of hits at lag d whose i lies in window w; the partner
 * at i + d may lie beyond the window, so the windows of a read sum to its W = 0 spectrum.  Lags above n - k count 0.
 * Reads are text + read_off[r], read_lens[r] bytes each: any byte alphabet, gaps, padding and any order of offsets, as
 * sd_stream_submit_dev takes them.  Every count is an exact integer; host and device forms return the same bytes.
 * Refused with SD_ERR_PARAM and the numbers in errbuf, before any device work: k outside 1 .. SD_AUTOCORR_KMAX, D outside
 * 1 .. SD_AUTOCORR_DMAX, W < 0, more than SD_AUTOCORR_CELLS_MAX cells (windows x D) in the call (1 GB of counters).
 *
 * sd_autocorr_layout: host only: win_off[0 .. n_reads] (may be NULL) and the windows of the call.
 * sd_autocorr_host: host threads.  counts (windows x D) is overwritten.
 * sd_autocorr_dev: the kernels of csrc/sd_autocorr.hip -- the text becomes three bit planes (code low bit, code high bit,
 * valid), 64 bases per word; a workgroup takes a tile of a window and a block of lags, a lane one lag: per tile word it
 * shifts the partner planes by its lag, forms the equality word, finds the starts of k-runs by shift-and doubling and adds
 * a population count; one 64-bit atomic add per (window, lag) and workgroup.  The reads are uploaded, the counts come
 * back; every cell is the kernel's (threads is unused).  No launch exceeds a fixed amount of work (sd_autocorr_info). */
#define SD_AUTOCORR_KMAX 32
#define SD_AUTOCORR_DMAX (1 << 20)
#define SD_AUTOCORR_CELLS_MAX ((int64_t)1 << 27)
int sd_autocorr_layout(const int64_t* read_lens, int32_t n_reads, int64_t W, int64_t* win_off, int64_t* windows_total);
int sd_autocorr_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D,
                     int64_t W, int32_t threads, int64_t* counts, char* errbuf, size_t errlen);
int sd_autocorr_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D,
                    int64_t W, int32_t device, int32_t threads, int64_t* counts, char* errbuf, size_t errlen);
/* The device-resident form: d_text is device memory of `device` (read_off and read_lens HOST arrays), d_counts (windows x D
 * int64) the caller's, on `device`, zeroed by the call whatever it held.  Everything is ordered on hip_stream; the host
 * waits for nothing and the call returns with the kernels in flight.  Its workspace (planes, tables) is kept per device,
 * and the next call on that device first waits for them.  SD_ERR_PARAM for a buffer that is not device memory,
 * SD_ERR_UNSUPPORTED for another device's. */
int sd_autocorr_reads_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k,
                          int64_t D, int64_t W, int32_t device, void* hip_stream, int64_t* d_counts, char* errbuf, size_t errlen);
/* positions[(win_off[r] + w) * D + d - 1] = the number of i in window w with i <= n - d - k: what a count is out of. */
int sd_autocorr_positions(const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D, int64_t W, int64_t* positions);
/* Peaks, integers only (csrc/sd_autocorr.hpp).  In a spectrum A[1 .. D] with smallest lag LO >= 1 and radius R >= 0, lag
 * d >= LO is a peak when A[d] > 0, A[d] >= A[e] for every e in [max(LO, d - R), min(D, d + R)], and A[d] > A[e] for every
 * such e < d (ties go to the smaller lag).  Peaks are ordered by count descending, then lag ascending; the first P of
 * each of the n_windows spectra of counts go to lag / count [n_windows x P], the tails filled with 0.  The period of a
 * spectrum is its first peak's lag, 0 when it has none. */
int sd_autocorr_peaks(const int64_t* counts, int64_t n_windows, int64_t D, int64_t LO, int64_t R, int64_t P, int64_t* lag,
                      int64_t* count);
/* The seed of a read with period p: with E[i] = 1 where i is a hit at lag p, the longest run of consecutive ones in E (of
 * equal runs the first) starts at *start and has *run ones; T[*start .. *start + p) is the seed.  *start = -1, *run = 0
 * when no position is a hit.  Host only. */
int sd_autocorr_seed(const char* text, int64_t n, int32_t k, int64_t p, int64_t* start, int64_t* run);
/* info = {bases of a tile, lags of a workgroup, the most base-lag products one launch of the pair kernel takes, launches
 * of the pair kernel in this process so far}. */
void sd_autocorr_info(int64_t info[4]);
/* Developer entry (tools/autocorr_bench.py): the arguments of sd_autocorr_dev; warmup + reps times each, between two HIP
 * events: ms_prep = the plane kernel, ms_pairs = every launch of the pair kernel.  info = launches, workgroups, cells,
 * plane words. */
int sd_autocorr_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k,
                             int64_t D, int64_t W, int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_pairs,
                             int64_t info[4]);

/* ---- windowed k-mer identity of every read against itself (--dotplot): no monomer file, both strands -------------------
 * A read is a text T[0 .. n).  The k-mer at i (1 <= k <= SD_DOTPLOT_KMAX) exists when i + k <= n and T[i .. i + k) are all
 * A C G T (the byte rule of sd_autocorr_*).  Its forward code f is the 2k-bit number with A C G T = 0 1 2 3, first base most
 * significant; its reverse code r is the code of its reverse complement.  Window w of a read covers the positions
 * [w W, min(n, (w + 1) W)), nw = ceil(n / W) (a read of 0 bases has none), 1 <= W <= SD_DOTPLOT_WMAX; a k-mer belongs to the
 * window its start lies in.  h is the splitmix64 finaliser (csrc/sd_dotplot.hpp: dotplot_hash); with the modulus M,
 * 1 <= M <= SD_DOTPLOT_MMAX, a code x is selected when h(x) % M == 0 -- always the value that is compared: S_w is the set of
 * distinct selected forward codes of window w, R_w the set of distinct selected reverse codes (selected by h(r)).
 * For windows j <= i of a read, with i - j <= B when a band 0 < B <= SD_DOTPLOT_BMAX is given (B = 0: all), the cell (i, j)
 * holds shared = |S_i & S_j| and, with rc != 0, shared_rc = |S_i & R_j|, the diagonal included.  Read r owns the windows
 * win_off[r] .. win_off[r + 1] and the cells cell_off[r] .. cell_off[r + 1] of the call, its cells ordered by i, then j.
 * Results, all int32: kmers[windows] = |S_w|, kmers_rc[windows] = |R_w|, shared[cells], shared_rc[cells]; with rc == 0
 * kmers_rc and shared_rc are not touched and may be NULL.  Every number is an exact integer; host and device forms return the
 * same bytes.  Reads are text + read_off[r], read_lens[r] bytes each, as sd_autocorr_* takes them.
 * Refused with SD_ERR_PARAM and the numbers in errbuf: k, W, M or B out of range and more than SD_DOTPLOT_CELLS_MAX cells in
 * the call, before any device work; a window with more than SD_DOTPLOT_SET_MAX selected positions on a strand, counted
 * before duplicates are removed -- the refusal names the read, the window, the count and the cap and advises a larger M; the
 * counting pass is the only device work before it (W <= 4096 with M = 1 cannot hit it).
 *
 * sd_dotplot_layout: host only: win_off, cell_off [0 .. n_reads] (each may be NULL) and the totals.
 * sd_dotplot_host: host threads: sets by sort and unique, cells by merge.
 * sd_dotplot_dev: the kernels of csrc/sd_dotplot.hip -- a counting pass per tile of 1 024 positions, one scan for the sets'
 * offsets, a gather, a sort of 64-bit keys in LDS per (window, strand), and the pair kernel: a workgroup holds S_i sorted in
 * LDS and looks the elements of S_j (and R_j) up in it, a ballot and a population count per 64 of them, one store per cell.
 * No kernel uses an atomic.  The reads are uploaded, the arrays come back.  No launch of the pair kernel exceeds a fixed
 * amount of work (sd_dotplot_info). */
#define SD_DOTPLOT_KMAX 32
#define SD_DOTPLOT_WMAX (1 << 30)
#define SD_DOTPLOT_MMAX (1 << 20)
#define SD_DOTPLOT_BMAX (1 << 30)
#define SD_DOTPLOT_CELLS_MAX ((int64_t)1 << 27)
#define SD_DOTPLOT_SET_MAX 4096
int sd_dotplot_layout(const int64_t* read_lens, int32_t n_reads, int64_t W, int64_t B, int64_t* win_off, int64_t* cell_off,
                      int64_t* windows_total, int64_t* cells_total);
int sd_dotplot_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t W,
                    int64_t B, int64_t M, int32_t rc, int32_t threads, int32_t* kmers, int32_t* kmers_rc, int32_t* shared,
                    int32_t* shared_rc, char* errbuf, size_t errlen);
int sd_dotplot_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t W,
                   int64_t B, int64_t M, int32_t rc, int32_t device, int32_t* kmers, int32_t* kmers_rc, int32_t* shared,
                   int32_t* shared_rc, char* errbuf, size_t errlen);
/* The device-resident form: d_text is device memory of `device` (read_off and read_lens HOST arrays), the four result
 * arrays the caller's, on `device`, every element written by the call.  Everything is ordered on hip_stream.  The host
 * waits once, for the counting pass's summary (four numbers: the total and the largest count, which size the sets and bound
 * the launches, and the first window over the cap); the call returns with the other kernels in flight.  Its workspace is
 * kept per device, and the next call on that device first waits for them.  SD_ERR_PARAM for a buffer that is not device
 * memory, SD_ERR_UNSUPPORTED for another device's. */
int sd_dotplot_reads_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k,
                         int64_t W, int64_t B, int64_t M, int32_t rc, int32_t device, void* hip_stream, int32_t* d_kmers,
                         int32_t* d_kmers_rc, int32_t* d_shared, int32_t* d_shared_rc, char* errbuf, size_t errlen);
/* info = {positions of a tile of the counting pass, cells of a row a workgroup of the pair kernel takes, SD_DOTPLOT_SET_MAX,
 * the most pair-elements (elements looked up, counted with the call's largest set) of one launch of the pair kernel,
 * SD_DOTPLOT_CELLS_MAX, launches of the pair kernel in this process so far}. */
void sd_dotplot_info(int64_t info[6]);
/* h(x), the splitmix64 finaliser the selection uses. */
uint64_t sd_dotplot_hash(uint64_t x);
/* Developer entry (tools/dotplot_bench.py): the arguments of sd_dotplot_dev; warmup + reps times each, between two HIP
 * events: ms_count = the counting pass and the scan, ms_sets = gather and sort, ms_pairs = every launch of the pair kernel.
 * info = launches, workgroups, cells, windows, selected positions, the largest set before duplicates are removed. */
int sd_dotplot_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k,
                            int64_t W, int64_t B, int64_t M, int32_t rc, int32_t device, int32_t warmup, int32_t reps,
                            float* ms_count, float* ms_sets, float* ms_pairs, int64_t info[6]);

/* ---- subfamilies of a monomer's instances (--split; csrc/sd_split.hpp holds the rule) ---------------------------------
 * The member rows of one forward monomer of L bases -- rows of --msa with status 1, bytes [0, L): 0..4 = A C G T N,
 * SD_MSA_DEL; insertion slots take no part -- are clustered by column distance H.  centres = [per-column mode of all
 * members] (ties: the smallest code); then rounds while fewer than K centres and fewer than 4 K rounds: the candidate row
 * farthest from its centre (ties: the smallest row) is tried as a new centre when its distance is at least the radius R:
 * assign (ties: the smallest centre), then at most I times (mode per cluster -- an empty one keeps its centre --, assign)
 * until nothing changes; a new cluster of fewer than S rows discards the trial and retires the row as a candidate.
 * Results: centres (k rows of L symbol bytes, K x L allocated), per row assign, d1 (its distance) and d2 (the smallest
 * distance to another centre, -1 with one centre), sizes (K), info = {k, rounds, Lloyd iterations, 1 when kernels ran}.
 * n = 0 gives k = 0.  Refused with SD_ERR_PARAM and the numbers in errbuf: R, S, I < 1, K outside 1 .. SD_SPLIT_KMAX,
 * more than SD_SPLIT_NMAX member rows of one monomer.
 *
 * sd_split_host: host threads, any L >= 1; sym is n rows of `pitch` >= L bytes.
 * sd_split_dev: the same call on a device (csrc/sd_split.hip): rows become three bit planes; a lane per row measures
 * popcount((a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2)) against the centres in LDS; the modes come from ballots over rows grouped
 * by cluster.  Per pass 16 bytes reach the host.  L > SD_SPLIT_LMAX is computed by the host form, with the same results. */
#define SD_SPLIT_KMAX 64
#define SD_SPLIT_LMAX 512
#define SD_SPLIT_NMAX ((int64_t)1 << 26)
int sd_split_host(const uint8_t* sym, int64_t n, int64_t pitch, int32_t L, int32_t R, int32_t K, int32_t S, int32_t I, int32_t threads,
                  uint8_t* centres, int32_t* assign, int32_t* d1, int32_t* d2, int32_t* sizes, int64_t info[4], char* errbuf, size_t errlen);
int sd_split_dev(const uint8_t* sym, int64_t n, int64_t pitch, int32_t L, int32_t R, int32_t K, int32_t S, int32_t I, int32_t device,
                 int32_t threads, uint8_t* centres, int32_t* assign, int32_t* d1, int32_t* d2, int32_t* sizes, int64_t info[4], char* errbuf,
                 size_t errlen);
/* All monomers of a job in one call, host only, on the buffers of --msa (rows, row_at [n_rows], status) and fmono (int32
 * [n_rows]: the forward monomer a row is an instance of, -1 for none).  Members of monomer m: status 1 and fmono = m;
 * mono_len[m] its length, radius[m] its R.  Per row: sub (the subfamily, -1 for a non-member), d1, d2 (-1 for a
 * non-member).  centres: the centres of monomer 0, 1, ... back to back, k_m x mono_len[m] bytes from cen_off[m]
 * (cen_off: n_mono + 1; centres_cap: the bytes allocated -- K x the sum of the lengths always suffices).  sizes:
 * n_mono x K, info: n_mono x 4 = {member rows, k, rounds, iterations}. */
int sd_split_final_host(const uint8_t* rows, const int64_t* row_at, const uint8_t* status, const int32_t* fmono, int64_t n_rows,
                        const int32_t* mono_len, const int32_t* radius, int32_t n_mono, int32_t K, int32_t S, int32_t I, int32_t threads,
                        int32_t* sub, int32_t* d1, int32_t* d2, uint8_t* centres, int64_t centres_cap, int64_t* cen_off, int32_t* sizes,
                        int64_t* info, char* errbuf, size_t errlen);
/* info = {SD_SPLIT_KMAX, SD_SPLIT_LMAX, SD_SPLIT_NMAX, launches of the assign kernel in this process so far}. */
void sd_split_info(int64_t info[4]);
/* Developer entry (tools/split_bench.py): the arguments of sd_split_dev; the whole split once, then warmup + reps times
 * each, between two HIP events, on its final centres: ms_prep = the plane kernel, ms_assign = one assign pass, ms_modes =
 * one pass of the modes (scan, group, count, centres).  info = k, rounds, iterations, assign launches. */
int sd_split_kernel_bench(const uint8_t* sym, int64_t n, int64_t pitch, int32_t L, int32_t R, int32_t K, int32_t S, int32_t I,
                          int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_assign, float* ms_modes, int64_t info[4]);

/* ---- higher-order repeat units of the final rows (--hor; csrc/sd_hor.hpp holds the rule) ------------------------------
 * Input: the rows of the final TSV in file order.  key = 2 m + s: monomer m of the monomer file, s = 1 its reverse
 * complement (the order of sd_stream_keys for a set without a repeated name), -1 = none.  A row is usable when usable != 0
 * (sd_final_row: reliable == 1) and key >= 0.  Rows x, x + 1 are adjacent when they share read and strand, both are
 * usable and 0 <= start[x+1] - end[x] - 1 <= G.
 *   T [n_mono x n_mono]: an adjacent pair adds 1 to T[m_x][m_x+1] on the forward strand, to T[m_x+1][m_x] on the reverse
 *   strand; rows[m] = the usable rows of m.
 *   succ(a) = the b of largest T[a][b], pred(b) = the a of largest T[a][b], ties to the smallest index, each defined from
 *   a count of C on.  The edge a -> b is kept when succ(a) = b and pred(b) = a; the components with an edge are simple
 *   cycles (kind 0, rotated to the smallest monomer) and simple paths (kind 1, from the head): the orders, sorted by their
 *   smallest monomer.  hor[m] = the order of m (0-based; H1 is order 0) or -1, pos[m] = its position, 1-based, or 0;
 *   order_kind / order_len [n_mono allocated].  An order of more than SD_HOR_PMAX monomers is not numbered: its monomers
 *   are on no order, long_first / long_len [n_mono allocated] name its first monomer and its length.
 *   A unit is a maximal run of rows whose consecutive pairs are adjacent, on one order, with positions rising (forward
 *   strand) or falling (reverse strand); a usable row alone on an order is a unit.  row_unit[x] = the unit of row x (units
 *   are numbered by their first row) or -1; units [cap_units allocated].
 *   info = {orders, units, long orders, 0}.
 * cap_units smaller than the units: SD_ERR_PARAM, info[1] and errbuf give the exact count, T / rows / the orders and
 * row_unit are complete, no unit is written.  n_rows always suffices.
 * Refused before any other work, errbuf naming the value: n_mono < 1 (SD_ERR_PARAM), n_mono > SD_HOR_MMAX
 * (SD_ERR_UNSUPPORTED), G < 0, C < 1, n_rows < 0 or >= 2^31, a key outside -1 .. 2 n_mono - 1 (SD_ERR_PARAM).
 *
 * sd_hor_rows: host threads (csrc/sd_hor.hip).  sd_hor_final_host: the same call on sd_final_row records (key = best, usable =
 * reliable == 1).  The rule is written for host and device (csrc/sd_hor.hpp); the library has no device form of it yet. */
#define SD_HOR_MMAX 2048
#define SD_HOR_PMAX 64
#define SD_HOR_NAME_MAX 192
typedef struct sd_hor_unit {
    int64_t first_row;               /* its first row                                                         */
    int64_t start, end;              /* start of its first row, end of its last                               */
    uint64_t mask;                   /* bit pos - 1 per row                                                   */
    int32_t read, n_rows, order;     /* order: 0-based                                                        */
    int32_t strand;                  /* 0: '+', 1: '-'                                                        */
} sd_hor_unit;
int sd_hor_rows(const int32_t* read, const int64_t* start, const int64_t* end, const int32_t* key, const uint8_t* usable, int64_t n_rows,
                int32_t n_mono, int64_t G, int64_t C, int32_t threads, int64_t* T, int64_t* rows, int32_t* hor, int32_t* pos,
                int32_t* order_kind, int32_t* order_len, int32_t* long_first, int32_t* long_len, int32_t* row_unit, sd_hor_unit* units,
                int64_t cap_units, int64_t info[4], char* errbuf, size_t errlen);
int sd_hor_final_host(const sd_final_row* rows_in, int64_t n_rows, int32_t n_mono, int64_t G, int64_t C, int32_t threads, int64_t* T,
                      int64_t* rows, int32_t* hor, int32_t* pos, int32_t* order_kind, int32_t* order_len, int32_t* long_first,
                      int32_t* long_len, int32_t* row_unit, sd_hor_unit* units, int64_t cap_units, int64_t info[4], char* errbuf,
                      size_t errlen);
/* The name of a mask: the positions present, ascending, as ranges joined by '_' ("1-12", "1-4_7-12", "3"); buf holds
 * SD_HOR_NAME_MAX bytes; returns the length. */
int sd_hor_name(uint64_t mask, char* buf);
/* info = {SD_HOR_MMAX, SD_HOR_PMAX, SD_HOR_NAME_MAX, 0}. */
void sd_hor_info(int64_t info[4]);

/* ---- IUPAC motif hits on both strands of every read (--motif; csrc/sd_motif.hpp holds the rule) -----------------------
 * A motif is a pattern of L codes from ACGTRYSWKMBDHVN, 1 <= L <= SD_MOTIF_LMAX, lower case folded.  N matches every text
 * byte; every other code is a set of bases and matches a text byte only when the byte is an upper-case A C G T of the set.
 * With E mismatches allowed (0 <= E <= SD_MOTIF_EMAX, one value for the request), position i of a read of n bases is a hit
 * on strand + when i + L <= n and at most E constrained positions j have T[i + j] outside the set of P[j]; on strand - by
 * the same rule against the reverse complement of P.  A pattern equal to its reverse complement is reported on + only.
 * Every hit is reported, overlapping ones included: Hamming matches, no indels.
 * Reads as the sd_autocorr_* calls take them: read r is text[read_off[r] .. + read_lens[r]), gaps and any order allowed.
 * hits: sd_motif_hit records in canonical order -- read, then motif in request order, then + before -, then start;
 * per[(r * n_motifs + m) * 2 + strand] (int64) = the hits of read r and motif m on that strand.
 * Limits, each refused (SD_ERR_PARAM) with its numbers in errbuf: at most SD_MOTIF_MAX motifs; every motif needs more than
 * E constrained positions; at most SD_MOTIF_ITEMS_MAX (tile of SD_MOTIF_TILE_WORDS words of a read, pattern-strand) items
 * per call, refused before any device work; at most SD_MOTIF_HITS_MAX hits per call, refused when the size pass has
 * counted them and before a record is written.
 * sd_motif_compile: host only.  Checks names ([A-Za-z0-9_.-]+, unique), patterns and E; *n_strands = the pattern-strands
 *   of the request (two per motif, one for a palindrome) and, where table is not NULL (5 x 2 x n_motifs int32), per
 *   pattern-strand {motif, strand, L, constrained positions, palindrome}.
 * sd_motif_host: text in host memory, `threads` host threads.  *hits is malloc'ed (sd_free), *n_hits its records; per is
 *   the caller's (n_reads x n_motifs x 2).
 * sd_motif_dev: the same from the kernels of csrc/sd_motif.hip on `device`: the reads are uploaded, the call owns its
 *   stream and returns hits and per in host memory.  The same arrays as sd_motif_host.
 * sd_motif_reads_size_dev / sd_motif_reads_write_dev: d_text in the memory of `device`, complete on hip_stream, as
 *   sd_autocorr_reads_dev takes it.  The size call builds the planes, counts every item, scans the counts and fills d_per
 *   (device memory, n_reads x n_motifs x 2 int64) on hip_stream; *n_hits comes to the host: 8 bytes, the only wait.  The
 *   write call -- the next motif call on that device, with the same reads and request -- writes the records into d_hits
 *   (device memory, cap records) on hip_stream and returns with its kernels in flight.  cap < *n_hits: SD_ERR_PARAM with
 *   the exact size in the message, nothing written.  A buffer that is not in device memory: SD_ERR_PARAM ("not in device
 *   memory"); another device's: SD_ERR_UNSUPPORTED.
 * sd_motif_info: info = {SD_MOTIF_TILE_WORDS, pattern-strands a workgroup takes, the most start x pattern-strand products
 *   of one launch, launches of the size and write kernels in this process so far}.
 * sd_motif_kernel_bench: the stages of sd_motif_dev between events, warmup + reps rounds each: ms_prep (the planes),
 *   ms_size (counts, scan, per), ms_write (the records), `reps` floats each; info = {launches of a write round, items,
 *   hits, plane words}. */
#define SD_MOTIF_LMAX 64
#define SD_MOTIF_EMAX 7
#define SD_MOTIF_MAX 1024
#define SD_MOTIF_ITEMS_MAX (1 << 24)
#define SD_MOTIF_HITS_MAX (1 << 28)
#define SD_MOTIF_TILE_WORDS 256
typedef struct {
    int64_t start;        /* leftmost base, 0-based; the hit ends at start + L - 1 (inclusive) */
    int32_t read;
    uint16_t motif;       /* index in the request */
    uint8_t strand;       /* 0: '+', 1: '-' */
    uint8_t mismatches;
} sd_motif_hit;
int sd_motif_compile(const char* const* names, const char* const* patterns, int32_t n_motifs, int32_t E, int32_t* n_strands, int32_t* table,
                     char* errbuf, size_t errlen);
int sd_motif_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                  int32_t n_motifs, int32_t E, int32_t threads, sd_motif_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
                  size_t errlen);
int sd_motif_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                 int32_t n_motifs, int32_t E, int32_t device, sd_motif_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf, size_t errlen);
int sd_motif_reads_size_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                            int32_t n_motifs, int32_t E, int32_t device, void* hip_stream, int64_t* d_per, int64_t* n_hits, char* errbuf,
                            size_t errlen);
int sd_motif_reads_write_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                             int32_t n_motifs, int32_t E, int32_t device, void* hip_stream, sd_motif_hit* d_hits, int64_t cap, char* errbuf,
                             size_t errlen);
void sd_motif_info(int64_t info[4]);
int sd_motif_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                          int32_t n_motifs, int32_t E, int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_size,
                          float* ms_write, int64_t info[4]);

/* ---- IUPAC motif hits with insertions and deletions (--motif-edits; csrc/sd_motif_edit.hpp holds the rule) ------------
 * Patterns, strands, the byte rule, the reads, per and the buffer rules are those of sd_motif_* above.  With K edits allowed
 * (0 <= K <= SD_MOTIF_KMAX): a text byte the code does not match costs 1, an inserted text byte costs 1, a deleted
 * pattern code costs 1 (an N too).  d(j), 1 <= j <= n, is the smallest edit distance of the pattern to any substring of
 * the read that ends just before position j; d(0) = L, d(n + 1) is infinite.  End j is a hit when d(j) <= K and
 * d(j) <= d(j + 1) and (d(j) < d(j - 1) or d(j) = 0): the first end of every valley and every exact occurrence.  The start
 * of a hit is the largest s with ed(pattern, read[s .. j)) = d(j); its length is L - d .. L + d.
 * hits: sd_motif_edit_hit records in canonical order -- read, then motif in request order, then + before -, then end.
 * Limits, each refused (SD_ERR_PARAM) with its numbers in errbuf: at most SD_MOTIF_MAX motifs; every motif needs more than
 * K constrained positions; at most SD_MOTIF_ITEMS_MAX (tile of SD_MOTIF_EDIT_TILE_WORDS words of a read, pattern-strand)
 * items per call, refused before any device work; at most SD_MOTIF_HITS_MAX hits per call, refused when the size pass has
 * counted them and before a record is written.
 * sd_motif_edit_host / sd_motif_edit_dev: as sd_motif_host / sd_motif_dev; both give the same arrays byte for byte.
 * sd_motif_edit_reads_size_dev / sd_motif_edit_reads_write_dev: as sd_motif_reads_size_dev / sd_motif_reads_write_dev,
 *   with a work area of their own: the write call follows the last edit size call on that device.
 * sd_motif_edit_info: info = {bases of a lane's stretch, SD_MOTIF_EDIT_TILE_WORDS, pattern-strands a workgroup takes, the
 *   most end x pattern-strand products of one launch, launches of the size and write kernels in this process so far,
 *   workgroups of one launch at most}.
 * sd_motif_edit_kernel_bench: as sd_motif_kernel_bench. */
#define SD_MOTIF_KMAX 7
#define SD_MOTIF_EDIT_TILE_WORDS 256
typedef struct {
    int64_t start;        /* leftmost base, 0-based; the hit ends at start + length - 1 (inclusive) */
    int32_t read;
    uint16_t motif;       /* index in the request */
    uint8_t length;       /* matched bases: L - edits .. L + edits */
    uint8_t strand_edits; /* strand << 7 | edits; strand 0: '+', 1: '-' */
} sd_motif_edit_hit;
int sd_motif_edit_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                       int32_t n_motifs, int32_t K, int32_t threads, sd_motif_edit_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
                       size_t errlen);
int sd_motif_edit_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                      int32_t n_motifs, int32_t K, int32_t device, sd_motif_edit_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
                      size_t errlen);
int sd_motif_edit_reads_size_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                                 const char* const* patterns, int32_t n_motifs, int32_t K, int32_t device, void* hip_stream, int64_t* d_per,
                                 int64_t* n_hits, char* errbuf, size_t errlen);
int sd_motif_edit_reads_write_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                                  const char* const* patterns, int32_t n_motifs, int32_t K, int32_t device, void* hip_stream,
                                  sd_motif_edit_hit* d_hits, int64_t cap, char* errbuf, size_t errlen);
void sd_motif_edit_info(int64_t info[6]);
int sd_motif_edit_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                               int32_t n_motifs, int32_t K, int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_size,
                               float* ms_write, int64_t info[4]);

/* ---- cyclic pairs and the merge of seed monomers (--autocorr-merge, bin/sd-merge; csrc/sd_cyclic.hpp holds the rule) --
 * n sequences, sequence i = text[off[i] .. off[i] + lens[i]): upper-case A C G T only, length >= 1; anything else is
 * SD_ERR_PARAM with the sequence's index, before any device work.
 * The pair of a query q and a target t: on strand s (0 = +: t, 1 = -: its reverse complement) the text is U = t^s t^s
 * without its last base; D(j) = the smallest unit-cost edit distance of q to a substring of U that ends at j inclusive
 * (the empty substring allowed); dist_s = min D, end_s = the smallest j that attains it; the result is that of +, unless
 * dist_- is strictly smaller.  phase = (end + 1) mod |t|.
 * sd_cyclic_pairs_host / sd_cyclic_pairs_dev: queries qi[m] x targets ti[k] (indices of sequences, repeats allowed),
 * m * k <= 2^24 -> dist / end / strand [m * k], pair (a, b) at a * k + b.  Both give the same arrays byte for byte.  The
 * device form runs queries of <= SD_CYCLIC_QMAX_LONG bp against targets of <= SD_CYCLIC_TMAX bp on the device -- those of
 * <= SD_CYCLIC_QMAX bp one pair to a lane (sd_cyclic_pairs), the longer ones one query across a team of 16, 32 or 64 lanes
 * with 1 to 4 words in each (sd_cyclic_pairs_long) -- and every other pair of the call on `threads` host threads.
 * sd_cyclic_merge_host / sd_cyclic_merge_dev: n <= 2^20 sequences, weight[n], 1 <= P <= 100.  R(q) = (100 - P) |q| / 100
 * rounded down; q is close to a centre c when abs(|q| - |c|) <= R(q) and dist(q in c) <= R(q).  The sequences are visited
 * by weight descending, then index ascending: one close to no centre so far becomes the next centre, any other joins the
 * close centre of smallest dist, the earliest of equals.  block: sequences per step, 0 = the default; the result does not
 * depend on it.  -> per sequence cluster (0-based, in order of creation), centre (the index of the cluster's centre),
 * dist / end / strand of the sequence in its centre (a centre: 0, |c| - 1, 0), and *n_clusters.
 * sd_cyclic_canon: out[len] = the lexicographically smallest among all rotations of seq and of its reverse complement,
 * = s[*rotation ..] s[.. *rotation) with s = seq (*strand 0) or its reverse complement (*strand 1); the smallest such
 * rotation, strand 0 where both give the same record.
 * sd_cyclic_info: info = {SD_CYCLIC_QMAX, SD_CYCLIC_TMAX, the step bound of a launch, launches of the pair kernel in this
 * process so far, pairs of a call at most, the default block (128)}.  The bound of a launch is compound: it takes at most
 * info[2] = 2^31 word steps (columns x words x pairs) or SD_CYCLIC_LAUNCH_WG_MIN workgroups, whichever is more -- a
 * workgroup of 32-word queries is 3e7 steps and more, and the step bound alone would leave most of the device idle.  So
 * info[2] is the most only while workgroups are small; the most there can be is SD_CYCLIC_LAUNCH_WG_MIN times the largest
 * workgroup (64 queries x 32 words x the 2 (2 x 65 535 - 1) columns of one target at the limit): 5.5e11 steps, seconds of
 * kernel, with one of the workgroup's four waves at work on its one target.  That shape was not measured.
 * sd_cyclic_kernel_bench: the launches of sd_cyclic_pairs_dev between two events, warmup untimed rounds, then reps timed
 * ones into ms_pairs[reps]; info = {launches per round, pairs on the device, word steps, workgroups}.  variant: 0 = the
 * kernels the library chooses, 1 = the column in 64-bit words for every class, 2 = in 32-bit halves for the classes of up
 * to four words (the two give the same arrays).  dist / end / strand (all three, or NULL): the arrays of the timed call;
 * a pair beyond the device's limits is not computed here and its three entries are unspecified (where any pair of the
 * call ran on the device, the whole device arrays are copied back, those entries with what the work area held).  It
 * times and runs the lane kernel only: a query of more than SD_CYCLIC_QMAX bp counts as beyond the limit here.
 * The team kernel.  SD_CYCLIC_QMAX stays the lane kernel's limit, and sd_cyclic_info's launches stay those of the lane
 * kernel.  A class of the team kernel is (K, L): K = 1 .. 4 words in each of L = 16, 32 or 64 lanes, 64 K L rows; a
 * query's class is the one of smallest K L that holds it, the larger K where two are equal.
 * sd_cyclic_pairs_team_host: the pairs as sd_cyclic_pairs_host gives them, computed by the team kernel's schedule of class
 * (K, L) on the host -- L lanes in lock step, the carry and the column's symbol handed down one lane per step.  Needs no
 * device.  SD_ERR_PARAM with one line where (K, L) is no class or a query has more than 64 K L bases.
 * sd_cyclic_long_info: info = {SD_CYCLIC_QMAX_LONG, launches of the team kernel in this process so far, the number of
 * instantiated classes (12), teams per wave at L = 16 (4)}.
 * sd_cyclic_long_kernel_bench: as sd_cyclic_kernel_bench for the team kernel; info = {launches per round, pairs on the
 * device, word steps with pad words and ramp steps counted, workgroups}.  K = L = 0: the queries of SD_CYCLIC_QMAX + 1 ..
 * SD_CYCLIC_QMAX_LONG bp in the library's classes; else every query of the call runs in class (K, L), short ones
 * included, and SD_ERR_PARAM where (K, L) is no class or a query has more than 64 K L bases.  Pairs of other queries, and
 * of targets beyond SD_CYCLIC_TMAX, are not computed here. */
#define SD_CYCLIC_QMAX 2048
#define SD_CYCLIC_QMAX_LONG 16384
#define SD_CYCLIC_TMAX 65535
#define SD_CYCLIC_LAUNCH_WG_MIN 1024
int sd_cyclic_pairs_host(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti,
                         int32_t m, int32_t k, int32_t threads, int32_t* dist, int32_t* end, uint8_t* strand, char* errbuf, size_t errlen);
int sd_cyclic_pairs_dev(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti,
                        int32_t m, int32_t k, int32_t device, int32_t threads, int32_t* dist, int32_t* end, uint8_t* strand, char* errbuf,
                        size_t errlen);
int sd_cyclic_merge_host(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int64_t* weight, int32_t P,
                         int32_t block, int32_t threads, int32_t* cluster, int32_t* centre, int32_t* dist, int32_t* end, uint8_t* strand,
                         int32_t* n_clusters, char* errbuf, size_t errlen);
int sd_cyclic_merge_dev(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int64_t* weight, int32_t P,
                        int32_t block, int32_t device, int32_t threads, int32_t* cluster, int32_t* centre, int32_t* dist, int32_t* end,
                        uint8_t* strand, int32_t* n_clusters, char* errbuf, size_t errlen);
int sd_cyclic_canon(const char* seq, int64_t len, char* out, int64_t* rotation, int32_t* strand);
void sd_cyclic_info(int64_t info[6]);
int sd_cyclic_kernel_bench(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti,
                           int32_t m, int32_t k, int32_t device, int32_t variant, int32_t warmup, int32_t reps, float* ms_pairs,
                           int64_t info[4], int32_t* dist, int32_t* end, uint8_t* strand);
int sd_cyclic_pairs_team_host(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti,
                              int32_t m, int32_t k, int32_t K, int32_t L, int32_t threads, int32_t* dist, int32_t* end, uint8_t* strand,
                              char* errbuf, size_t errlen);
void sd_cyclic_long_info(int64_t info[4]);
int sd_cyclic_long_kernel_bench(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti,
                                int32_t m, int32_t k, int32_t device, int32_t K, int32_t L, int32_t warmup, int32_t reps, float* ms_pairs,
                                int64_t info[4], int32_t* dist, int32_t* end, uint8_t* strand);

/* ---- the screen: which chunks of a read can hold a monomer at all (csrc/sd_screen.hip) ------------------------------
 * key[c] = (min over templates j of dist(j, c)) << 16 | the smallest j that attains the minimum, for every chunk c of the
 * reads' standard chunk plan (part_size, overlap; chunks numbered read by read).  dist is the distance of --ed_thr: the
 * infix unit-cost edit distance of template j against the chunk; templates are the monomers in the given order, then
 * their reverse complements.  A chunk passes a threshold thr >= 0 when key >> 16 <= thr.  The distances come from the
 * prefilter's kernels with a sink that reduces in LDS and issues one atomic minimum per (workgroup, chunk): no
 * [chunk][template] matrix is written, 4 bytes per chunk come back.  At most 32 767 monomers of at most 2 048 bp.
 * A handle holds templates, match masks and scratch on one device; calls on one handle serialise. */
typedef struct sd_screen sd_screen;
typedef struct sd_screen_region {
    int32_t read;        /* index of the read                                                       */
    int64_t start;       /* first byte of the region in the read                                    */
    int64_t end_incl;    /* last byte of the region                                                 */
    int32_t n_chunks;    /* passing chunks the region was made of                                   */
    uint32_t best_key;   /* the smallest key among them                                             */
} sd_screen_region;
int sd_screen_create(const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, int32_t device, sd_screen** out,
                     char* errbuf, size_t errlen);
void sd_screen_destroy(sd_screen* h);
/* on != 0: the general distance kernel where the uniform one would run (A/B and tests; the keys are the same) */
int sd_screen_set_general(sd_screen* h, int32_t on);
/* the kernel the next call launches: 0 = sd_hw_dist<W>, 1 = sd_hw_dist_u<W, lo>, 2 = sd_hw_dist_u<W, hi>; *words = W */
int sd_screen_kernel(sd_screen* h, int32_t* words);
/* device time (ms) of the kernels of the calls so far whose keys came back to the host; reset != 0 zeroes the sum */
double sd_screen_kernel_ms(sd_screen* h, int32_t reset);
/* For tools/screen_bench.py: the screen's launch (key fill + distance kernel with the key sink) beside the distance
 * kernel of --ed_thr alone (the same instantiation, writing its [chunk][template] matrix) on the batch of the last
 * sd_screen_chunks call, alternating in one process, each between two HIP events; warmup untimed rounds, then reps
 * timed ones into screen_ms[reps] / dist_ms[reps]. */
int sd_screen_kernel_bench(sd_screen* h, int32_t warmup, int32_t reps, float* screen_ms, float* dist_ms, char* errbuf,
                           size_t errlen);
/* Reads in host memory: packed on host threads, one launch, the keys copied back.  key_out: room for cap keys;
 * *n_chunks (may be NULL) is set even when cap is too small (SD_ERR_PARAM).  SD_ERR_EMPTY for a read of length <= 0,
 * SD_ERR_SYMBOL for a byte outside A C G T N. */
int sd_screen_chunks(sd_screen* h, const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads, int32_t part_size,
                     int32_t overlap, uint32_t* key_out, int64_t cap, int64_t* n_chunks, char* errbuf, size_t errlen);
/* Reads in device memory, the arguments of sd_stream_submit_dev: read r = d_bases[read_off[r] .. read_off[r] + read_lens[r]),
 * read_off and read_lens HOST arrays.  The handle's stream waits for an event recorded on hip_stream, packs the bases
 * with the device packer and screens them; hip_stream is made to wait for the last kernel, so the text may be
 * overwritten or freed on it right after the call.  key_out is device memory of the handle's device -- then the keys are
 * written there, in order with hip_stream, and there is no host-side wait -- or host memory, then the call returns
 * when they have arrived.  The alphabet is not checked here (a byte outside A C G T N is packed under the masked
 * formula of the packer; the decomposition of the same bytes reports it). */
int sd_screen_chunks_dev(sd_screen* h, const void* d_bases, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                         int32_t part_size, int32_t overlap, void* hip_stream, uint32_t* key_out, int64_t cap,
                         int64_t* n_chunks, char* errbuf, size_t errlen);
/* Host only: the same keys by a plain dynamic program (exact, not fast; for tests). */
int sd_screen_chunks_host(const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, const char* const* read_seqs,
                          const int64_t* read_lens, int32_t n_reads, int32_t part_size, int32_t overlap, uint32_t* key_out,
                          int64_t cap, int64_t* n_chunks, char* errbuf, size_t errlen);
/* Host only: the regions of a threshold.  chunk_read[c] = the read of chunk c (ascending: a chunk table); a region is a
 * maximal run a..b of consecutive passing chunks of one read and covers its bytes [a * part_size, min(len, (b + 1) *
 * part_size + overlap)); regions come in read order, then position order.  SD_ERR_PARAM for thr < 0 and for overlap >=
 * part_size (the regions of a read must not overlap).  *n_regions is set even when cap is too small (SD_ERR_PARAM). */
int sd_screen_regions(const uint32_t* keys, const int32_t* chunk_read, int64_t n_chunks, const int64_t* read_lens,
                      int32_t n_reads, int32_t part_size, int32_t overlap, int32_t thr, sd_screen_region* regions_out,
                      int64_t cap, int64_t* n_regions, char* errbuf, size_t errlen);

/* sd_run_files behind the screen: the job runs in two phases inside the one call.  Phase 1 packs and screens every
 * chunk of the reads file in batches dealt over the device entries (devices / n_devices as sd_run_files_devices takes
 * them; NULL / 0: p->device).  Phase 2 is the job of sd_run_files over a read list in which every region of screen_thr
 * replaces its read: for every region, in read order and then position order, exactly the rows of the plain job on the
 * region's substring as a read of its own, with the parent's name and every start and end increased by the region's
 * start; a read without a region contributes no row; nothing is merged across regions.  An input whose chunks all pass
 * gives the files of sd_run_files byte for byte.  p->ed_thr and the scoring keep their meaning inside the regions; the
 * screen's distances depend on neither.  screen_tsv_out (may be NULL): one line per region -- read, start, end (0-based,
 * inclusive), chunks, best distance, best template (' = reverse complement).  SD_FLAG_PROFILE works as in sd_run_files.
 * counts (may be NULL): [0] reads, [1] reads with a region, [2] bases read, [3] bases decomposed; sd_last_run_stats
 * [20..23]: the screen's wall ms, the device ms of its kernels, bases read, bases decomposed.
 * SD_ERR_PARAM, before any device is touched: screen_thr < 0, overlap >= part_size, records_out != NULL ("the record
 * stream holds whole reads"). */
int sd_run_files_screen(const char* reads_fa, const char* monomers_fa, const sd_params* p, const int32_t* devices,
                        int32_t n_devices, const char* raw_tsv_out, const char* final_tsv_out, const char* alt_tsv_out,
                        int32_t min_identity, int32_t second_best, const double* lr_coef, int32_t screen_thr,
                        const char* screen_tsv_out, const char* records_out, int64_t* counts, char* errbuf, size_t errlen);

/* The profile of the last successful sd_run_files* call of this process made with SD_FLAG_PROFILE (summed over its
 * device entries).  Every output may be NULL: *n_monomers, *n_counts and *text_bytes size the buffers of a second
 * call.  text: "name\tsequence\n" per monomer in FASTA order, NUL-terminated (text_bytes counts the NUL); counts as
 * above.  SD_ERR_PARAM when the last call did not profile. */
int sd_last_run_profile(int32_t* n_monomers, int64_t* n_counts, int64_t* text_bytes, char* text, uint64_t* counts);

/* Text of `_alt.tsv` rows (main.py:161-165): for each of n_rows kept blocks one line per monomer name
 * (key): read, name, start, end, "%.2f" of vals[row * n_keys + key], '*' if key == own_key[row] else
 * '-'.  The read of a row is read_names[row_read[row]] (row_read == NULL: read_names[0] for all rows).
 * *txt is malloc'ed (sd_free).  Host only, multi-threaded. */
int sd_format_alt_rows(const char* const* read_names, int32_t n_reads, const int32_t* row_read,
                       const char* const* key_names, int32_t n_keys, const int64_t* starts,
                       const int64_t* ends, const int32_t* own_key, const double* vals, int64_t n_rows,
                       int32_t threads, char** txt, size_t* txt_len);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_H */
