// sd_rows_dev.hip -- per-read row assembly on the device: chunk offsets (main.cpp:109-111) and the seam merge
// (PostProcessing, main.cpp:287-302) on records that never leave HBM.  The merge runs in pieces (sd_seam_dev.hpp, the
// same text the host self-test runs): one lane per piece builds the piece's exit table, one wave per read chains the
// tables into every piece's true entry (a shuffle scan over map composition, 64 pieces per round), one lane per piece
// flags the records its scan keeps, and the flags are counted per tile, scanned and scattered.  A read of one piece
// and a read of a million records take the same path; nothing is sequential over records.
//   sd_rows_append   a batch's chunk-local records -> the job's store, chunk offsets added, scores scaled
//   sd_seam_exits, sd_seam_chain, sd_seam_keep      the piece algebra
//   sd_rows_count, scan_bases (sd_scan_dev.hpp)     kept records per tile, rows before each tile, the row count
//   sd_rows_scatter                                 kept records -> rows, row offsets per read
// No look-back and no spinning: a launch per stage, seven for a job (~5 MB of records in the benchmark's step).
#include "sd_job_dev.hpp"
#include "sd_rows_flags_dev.hpp"
#include "sd_seam_dev.hpp"

namespace sd {


__global__ __launch_bounds__(ROWS_T) void sd_rows_append(const DevRec* __restrict__ dense, const int64_t* __restrict__ roff,
                                                         int n_chunks, const int32_t* __restrict__ add, DevRec* __restrict__ out,
                                                         int64_t base, int64_t cap, int scale) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = ((int64_t)gridDim.x * ROWS_T) >> 6;
    for (int64_t c = ((int64_t)blockIdx.x * ROWS_T + threadIdx.x) >> 6; c < n_chunks; c += nw) {
        const int64_t a = roff[c], b = roff[c + 1];
        const int32_t ad = add[c];
        for (int64_t x = a + lane; x < b; x += 64) {
            DevRec r = dense[x];
            r.start += ad;
            r.end += ad;
            r.score *= scale;
            if (base + x < cap) out[base + x] = r;
        }
    }
}

// the read that owns piece p: the last r < n_reads with piece_start[r] <= p (reads without records own no piece)
__device__ inline int rows_read_of(const int64_t* __restrict__ piece_start, int n_reads, int64_t p) {
    int lo = 0, hi = n_reads;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (piece_start[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(ROWS_T) void sd_seam_exits(const DevRec* __restrict__ recs, const int64_t* __restrict__ read_off,
                                                        const int64_t* __restrict__ piece_start, int n_reads, int64_t n_pieces,
                                                        int S, uint32_t* __restrict__ exits) {
    const int64_t p = (int64_t)blockIdx.x * ROWS_T + threadIdx.x;
    if (p >= n_pieces) return;
    const int r = rows_read_of(piece_start, n_reads, p);
    const int64_t lo = read_off[r];
    exits[p] = seam_piece_exits(recs + lo, read_off[r + 1] - lo, S, p - piece_start[r]);
}

// One wave per read: the true entry of every piece of the read.  64 tables per round: an inclusive scan over
// composition gives lane l the map "pieces base .. base + l", the lane before it the map up to its own piece.
__global__ __launch_bounds__(ROWS_T) void sd_seam_chain(const int64_t* __restrict__ piece_start, int n_reads,
                                                        const uint32_t* __restrict__ exits, uint8_t* __restrict__ entry) {
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * ROWS_T + threadIdx.x) >> 6;   // (the same in every lane of a wave)
    if (r >= n_reads) return;
    const int64_t p0 = piece_start[r], p1 = piece_start[r + 1];
    int carry = 0;
    for (int64_t base = p0; base < p1; base += 64) {
        const int64_t p = base + lane;
        uint32_t f = p < p1 ? exits[p] : SEAM_IDENTITY;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t before = __shfl_up(f, off);
            if (lane >= off) f = seam_compose(before, f);
        }
        uint32_t prev = __shfl_up(f, 1);
        if (lane == 0) prev = SEAM_IDENTITY;
        if (p < p1) entry[p] = (uint8_t)seam_exit(prev, carry);
        carry = seam_exit(__shfl(f, 63), carry);
    }
}

__global__ __launch_bounds__(ROWS_T) void sd_seam_keep(const DevRec* __restrict__ recs, const int64_t* __restrict__ read_off,
                                                       const int64_t* __restrict__ piece_start, int n_reads, int64_t n_pieces,
                                                       int S, const uint8_t* __restrict__ entry, uint8_t* __restrict__ keep) {
    const int64_t p = (int64_t)blockIdx.x * ROWS_T + threadIdx.x;
    if (p >= n_pieces) return;
    const int r = rows_read_of(piece_start, n_reads, p);
    const int64_t lo = read_off[r];
    seam_piece_keep(recs + lo, read_off[r + 1] - lo, S, p - piece_start[r], (int)entry[p], keep + lo);
}

// workgroups [0, n_tiles): the kept records of a tile to their rows; the workgroups behind them: row_off of the reads
__global__ __launch_bounds__(ROWS_T) void sd_rows_scatter(const DevRec* __restrict__ recs, const uint8_t* __restrict__ keep,
                                                          int64_t n, int64_t n_tiles, const int64_t* __restrict__ bbase,
                                                          const int64_t* __restrict__ read_off, int n_reads,
                                                          DevRec* __restrict__ rows, int64_t cap, int64_t* __restrict__ row_off) {
    if ((int64_t)blockIdx.x < n_tiles) {
        const int64_t i0 = (int64_t)blockIdx.x * ROWS_TILE + threadIdx.x * 4;
        const uint32_t f = rows_flags(keep, n, i0);
        int total;
        int64_t at = bbase[blockIdx.x] + block_scan<int>(rows_flag_count(f), &total);
        for (int k = 0; k < 4; ++k)
            if ((f >> (8 * k)) & 1u) {
                if (at < cap) rows[at] = recs[i0 + k];
                ++at;
            }
        return;
    }
    const int64_t r = ((int64_t)blockIdx.x - n_tiles) * ROWS_T + threadIdx.x;
    if (r > n_reads) return;
    row_off[r] = rows_flags_before(keep, bbase, read_off[r]);
}

}  // namespace sd

namespace sdi {

static inline unsigned rows_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + sd::ROWS_T - 1) / sd::ROWS_T); }

void rows_append(RowsWS& ws, hipStream_t st, const sd::DevRec* dense, const int64_t* d_roff, int n_chunks,
                 const int32_t* d_add, int64_t base, int scale) {
    if (n_chunks <= 0) return;
    const unsigned nb = (unsigned)std::min<int64_t>(2048, ((int64_t)n_chunks + 3) / 4);   // a wave per chunk, strided
    hipLaunchKernelGGL(sd::sd_rows_append, dim3(nb), dim3(sd::ROWS_T), 0, st, dense, d_roff, n_chunks, d_add, ws.recs.p,
                       base, (int64_t)ws.recs.cap, scale);
    SD_HIP(hipGetLastError());
}

void rows_assemble(RowsWS& ws, hipStream_t st, const sd::DevRec* recs, const int64_t* read_off, int32_t n_reads, int piece) {
    const size_t nr = (size_t)n_reads + 1;
    ws.n_reads = n_reads;
    ws.piece = piece;
    ws.n_recs = read_off[n_reads];
    ws.h_off.alloc(2 * nr);
    ws.h_total.alloc(1);
    int64_t* pst = ws.h_off.p + nr;
    pst[0] = 0;
    for (size_t r = 0; r < nr; ++r) {
        ws.h_off.p[r] = read_off[r];
        if (r + 1 < nr) pst[r + 1] = pst[r] + sd::seam_piece_count(read_off[r + 1] - read_off[r], piece);
    }
    ws.n_pieces = pst[n_reads];
    ws.n_tiles = (ws.n_recs + sd::ROWS_TILE - 1) / sd::ROWS_TILE;
    const size_t keep_bytes = ((size_t)ws.n_recs + 3) / 4 * 4;
    ws.off.alloc(2 * nr);
    ws.exits.alloc((size_t)ws.n_pieces);
    ws.entry.alloc((size_t)ws.n_pieces);
    ws.keep.alloc(keep_bytes);
    ws.bsum.alloc((size_t)ws.n_tiles);
    ws.bbase.alloc((size_t)ws.n_tiles + 1);
    if (!ws.ev_asm) SD_HIP(hipEventCreateWithFlags(&ws.ev_asm, hipEventDisableTiming));
    ws.settled = false;
    SD_HIP(hipMemcpyAsync(ws.off.p, ws.h_off.p, 2 * nr * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (keep_bytes) SD_HIP(hipMemsetAsync(ws.keep.p, 0, keep_bytes, st));
    const int64_t* d_read_off = ws.off.p;
    const int64_t* d_piece = ws.off.p + nr;
    if (ws.n_pieces > 0) {
        hipLaunchKernelGGL(sd::sd_seam_exits, dim3(rows_grid(ws.n_pieces)), dim3(sd::ROWS_T), 0, st, recs, d_read_off, d_piece,
                           (int)n_reads, ws.n_pieces, piece, ws.exits.p);
        hipLaunchKernelGGL(sd::sd_seam_chain, dim3(rows_grid((int64_t)n_reads * 64)), dim3(sd::ROWS_T), 0, st, d_piece,
                           (int)n_reads, ws.exits.p, ws.entry.p);
        hipLaunchKernelGGL(sd::sd_seam_keep, dim3(rows_grid(ws.n_pieces)), dim3(sd::ROWS_T), 0, st, recs, d_read_off, d_piece,
                           (int)n_reads, ws.n_pieces, piece, ws.entry.p, ws.keep.p);
    }
    if (ws.n_tiles > 0)
        hipLaunchKernelGGL(sd::sd_rows_count, dim3((unsigned)ws.n_tiles), dim3(sd::ROWS_T), 0, st, ws.keep.p, ws.n_recs, ws.bsum.p);
    hipLaunchKernelGGL(sd::scan_bases<int32_t>, dim3(1), dim3(sd::SCAN_T), 0, st, ws.bsum.p, ws.n_tiles, ws.bbase.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipMemcpyAsync(ws.h_total.p, ws.bbase.p + ws.n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SD_HIP(hipEventRecord(ws.ev_asm, st));
}

void rows_scatter(RowsWS& ws, hipStream_t st, const sd::DevRec* recs, sd::DevRec* rows, int64_t cap, int64_t* row_off) {
    const int64_t nb = ws.n_tiles + ((int64_t)ws.n_reads + 1 + sd::ROWS_T - 1) / sd::ROWS_T;
    hipLaunchKernelGGL(sd::sd_rows_scatter, dim3((unsigned)nb), dim3(sd::ROWS_T), 0, st, recs, ws.keep.p, ws.n_recs, ws.n_tiles,
                       ws.bbase.p, ws.off.p, (int)ws.n_reads, rows, cap, row_off);
    SD_HIP(hipGetLastError());
    if (!ws.ev_free) SD_HIP(hipEventCreateWithFlags(&ws.ev_free, hipEventDisableTiming));
    SD_HIP(hipEventRecord(ws.ev_free, st));
    ws.free_recorded = true;
}

// read_off of a caller: n_reads + 1 ascending record indices from 0, fewer than 2^40 records (the tile grid, 2^30
// workgroups, and the piece grid, at most 2^29, then fit a launch's 32-bit grid)
static bool rows_offsets_ok(const int64_t* read_off, int32_t n_reads) {
    if (read_off[0] != 0) return false;
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_off[r + 1] < read_off[r]) return false;
    return read_off[n_reads] < ((int64_t)1 << 40);
}

// sd_scan_selftest: the scan of sd_scan_dev.hpp over d_values with tile sums of type T, finished when it returns
template <class T>
static void scan_selftest(hipStream_t st, const int64_t* d_values, int64_t n, int64_t* d_out) {
    DevBuf<T> tsum;
    DevBuf<int64_t> tbase;
    tsum.alloc((size_t)sd::scan_tiles_of(n));
    tbase.alloc((size_t)sd::scan_tiles_of(n) + 1);
    sd::exclusive_scan_dev(st, sd::ScanArray<int64_t>{d_values}, n, d_out, tsum.p, tbase.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipStreamSynchronize(st));   // (the buffers go back with nothing in flight on them)
}

}  // namespace sdi

extern "C" {

int sd_seam_pieces_selftest(const sd_rec* recs, const int64_t* read_off, int32_t n_reads, int32_t piece, sd_rec* rows,
                            int64_t* row_off, int64_t* n_rows) try {
    if (n_reads < 0 || !read_off || !row_off || (piece != 0 && piece < sd::SEAM_REACH)) return SD_ERR_PARAM;
    if (!rows_offsets_ok(read_off, n_reads) || (read_off[n_reads] > 0 && (!recs || !rows))) return SD_ERR_PARAM;
    const int32_t S = piece ? piece : ROWS_PIECE;
    int64_t w = 0;
    row_off[0] = 0;
    std::vector<uint8_t> keep;
    std::vector<uint32_t> exits;
    for (int32_t r = 0; r < n_reads; ++r) {
        const sd_rec* b = recs + read_off[r];
        const int64_t N = read_off[r + 1] - read_off[r], P = sd::seam_piece_count(N, S);
        keep.assign((size_t)N, 0);
        exits.resize((size_t)P);
        for (int64_t p = 0; p < P; ++p) exits[(size_t)p] = sd::seam_piece_exits(b, N, S, p);
        // the chain as the device takes it: the entry of piece p from the composed map of the pieces before it
        uint32_t upto = sd::SEAM_IDENTITY;
        for (int64_t p = 0; p < P; ++p) {
            sd::seam_piece_keep(b, N, S, p, sd::seam_exit(upto, 0), keep.data());
            upto = sd::seam_compose(upto, exits[(size_t)p]);
        }
        for (int64_t x = 0; x < N; ++x)
            if (keep[(size_t)x]) rows[w++] = b[x];
        row_off[r + 1] = w;
    }
    if (n_rows) *n_rows = w;
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_scan_selftest(const int64_t* values, int64_t n, int32_t tile_sums_32, int32_t device, int64_t* out) try {
    if (n < 0 || n >= ((int64_t)1 << 31) || !out || (n > 0 && !values)) return SD_ERR_PARAM;
    if (const int rc = device_check(device, nullptr, 0)) return rc;
    try {
        DeviceScope on(device);
        OwnedStream st;
        DevBuf<int64_t> d_values, d_out;
        d_values.alloc((size_t)n);
        d_out.alloc((size_t)n + 1);
        if (n > 0) SD_HIP(hipMemcpyAsync(d_values.p, values, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (tile_sums_32) scan_selftest<int32_t>(st, d_values.p, n, d_out.p);
        else scan_selftest<int64_t>(st, d_values.p, n, d_out.p);
        SD_HIP(hipMemcpy(out, d_out.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    } catch (const HipFail&) {
        return SD_ERR_HIP;
    }
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_seam_merge_dev(const sd_rec* d_recs, const int64_t* d_read_off, int32_t n_reads, int32_t piece, int32_t device,
                      void* hip_stream, sd_rec* d_rows, int64_t* d_row_off, int64_t* n_rows) {
    static_assert(sizeof(sd_rec) == sizeof(sd::DevRec), "record layout");
    if (n_reads < 0 || !d_read_off || !d_row_off || device < 0 || (piece != 0 && piece < sd::SEAM_REACH)) return SD_ERR_PARAM;
    if (const int rc = device_check(device, nullptr, 0)) return rc;   // (device < 0: refused above)
    try {
        SD_HIP(hipSetDevice(device));
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        std::vector<int64_t> off((size_t)n_reads + 1);
        SD_HIP(hipMemcpyAsync(off.data(), d_read_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));
        if (!rows_offsets_ok(off.data(), n_reads) || (off[(size_t)n_reads] > 0 && (!d_recs || !d_rows))) return SD_ERR_PARAM;
        RowsWS ws;
        const sd::DevRec* recs = reinterpret_cast<const sd::DevRec*>(d_recs);
        rows_assemble(ws, st, recs, off.data(), n_reads, piece ? piece : ROWS_PIECE);
        rows_scatter(ws, st, recs, reinterpret_cast<sd::DevRec*>(d_rows), off[(size_t)n_reads], d_row_off);
        SD_HIP(hipStreamSynchronize(st));   // (the workspace goes back with nothing in flight on it)
        if (n_rows) *n_rows = ws.h_total.p[0];
    } catch (const HipFail&) {
        return SD_ERR_HIP;
    }
    return SD_OK;
}

int sd_engine_rows_dev(sd_engine* e, sd_rec* d_rows, int64_t cap_rows, int64_t* d_row_off, void* hip_stream, int64_t* n_rows,
                       char* errbuf, size_t errlen) {
    if (!e || !d_row_off || cap_rows < 0 || (cap_rows > 0 && !d_rows)) return SD_ERR_PARAM;
    if (n_rows) *n_rows = 0;
    int64_t total = 0;
    int rc = fetch_begin(e, total, errbuf, errlen);   // (the run is through, a guard trip's repeat included)
    if (rc) return rc;
    if (e->sliced_run && hipEventSynchronize(e->ev_run1) != hipSuccess) { set_err(errbuf, errlen, "device run failed"); return SD_ERR_HIP; }
    try {
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        if (!e->rows_ws) e->rows_ws.reset(new RowsWS);
        RowsWS& ws = *e->rows_ws;
        // (an earlier call's scatter may still read the workspace, on another stream of the caller's)
        ws.wait_idle();
        // The assembly of this run, once: a call that only learned the row count (cap_rows too small) is followed by
        // one that only scatters.  The host has waited for it, so the scatter may go on any stream.
        if (!e->rows_done) {
            const size_t C = e->chunks.size();
            std::vector<int64_t> read_off((size_t)e->n_reads + 1, 0);
            size_t c = 0;
            for (int32_t r = 0; r < e->n_reads; ++r) {
                c += (size_t)e->read_nchunks[(size_t)r];
                read_off[(size_t)r + 1] = e->h_roff.p[std::min(c, C)];
            }
            if (C > 0) {
                ws.h_add.alloc(C);
                for (size_t k = 0; k < C; ++k) ws.h_add.p[k] = (int32_t)e->chunk_off[k];
                ws.add.alloc(C);
                ws.recs.alloc((size_t)std::max<int64_t>(total, 1));
                SD_HIP(hipMemcpyAsync(ws.add.p, ws.h_add.p, C * sizeof(int32_t), hipMemcpyHostToDevice, st));
                rows_append(ws, st, e->d_dense.p, e->d_roff.p, (int)C, ws.add.p, 0, e->score_scale);
            }
            rows_assemble(ws, st, ws.recs.p, read_off.data(), e->n_reads, ROWS_PIECE);
            SD_HIP(hipEventSynchronize(ws.ev_asm));
            ws.settled = true;
            e->rows_done = true;
        }
        const int64_t n = ws.h_total.p[0];
        if (n_rows) *n_rows = n;
        if (cap_rows < n) {
            set_err(errbuf, errlen, "sd_engine_rows_dev: " + std::to_string(n) + " rows, room for " + std::to_string(cap_rows));
            return SD_ERR_PARAM;
        }
        rows_scatter(ws, st, ws.recs.p, reinterpret_cast<sd::DevRec*>(d_rows), cap_rows, d_row_off);
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

}  // extern "C"
