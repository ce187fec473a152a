// sd_final_dev.hip -- the final selection (main.py:107-165; PostProcessor::select) on the device, on identity words
// that never left HBM (sd_final_ws.hpp).  The identity arithmetic, the split test and the end of
// the rule (threshold, logit, the row's bytes) are sd_final_dev.hpp, one text with the host; the maximum searches, a
// left-to-right scan on the host, are (value, index) reductions over lanes here.
//   sd_final_sources   keep flags of the seam merge -> the store index of every merged row, merged row offsets per read
//   sd_final_light     light mode: one lane per row, the word of the row's own monomer
//   sd_final_best      second_best: a group of 8 .. 64 lanes per row strides the T plain and T homopolymer words, each
//                      word read ONCE;
//                      (value, index) reductions that prefer the smaller index on equal values
//   sd_rows_count (sd_rows_flags_dev.hpp), scan_bases (sd_scan_dev.hpp)   kept rows per tile, before each tile, their count
//   sd_final_scatter, sd_final_alt           kept rows -> the caller's rows, row offsets, key identities
// A row the words do not decide (a missing word, a segment edlib aligns by Hirschberg's split) is counted, not guessed.
#include "sd_convert.hpp"
#include "sd_final_ws.hpp"
#include "sd_job_dev.hpp"
#include "sd_rows_flags_dev.hpp"

namespace sd {

// workgroups [0, n_tiles): the kept records of a tile of the STORE -> src of their merged rows; the workgroups behind
// them: the merged row offsets of the reads.  (sd_rows_scatter, writing indices instead of records; the store's tiles are
// the ROWS_TILE of sd_rows_flags_dev.hpp, which both units include.)
__global__ __launch_bounds__(ROWS_T) void sd_final_sources(const uint8_t* __restrict__ keep, int64_t n, int64_t n_tiles,
                                                          const int64_t* __restrict__ bbase, const int64_t* __restrict__ read_off,
                                                          int n_reads, int64_t* __restrict__ src, int64_t cap,
                                                          int64_t* __restrict__ moff) {
    if ((int64_t)blockIdx.x < n_tiles) {
        const int64_t i0 = (int64_t)blockIdx.x * ROWS_TILE + threadIdx.x * 4;
        const uint32_t f = rows_flags(keep, n, i0);
        int total;
        int64_t at = bbase[blockIdx.x] + block_scan<int>(rows_flag_count(f), &total);
        for (int k = 0; k < 4; ++k)
            if ((f >> (8 * k)) & 1u) {
                if (at < cap) src[at] = i0 + k;
                ++at;
            }
        return;
    }
    const int64_t r = ((int64_t)blockIdx.x - n_tiles) * ROWS_T + threadIdx.x;
    if (r > n_reads) return;
    moff[r] = rows_flags_before(keep, bbase, read_off[r]);
}

// the read that owns merged row m: the first r with moff[r + 1] > m (reads without rows own none)
__device__ inline int fin_read_of(const int64_t* __restrict__ moff, int n_reads, int64_t m) {
    int lo = 0, hi = n_reads - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (moff[mid + 1] > m) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the whole 80 bytes of a row, padding included (a struct assignment need not copy padding)
__device__ inline void fin_copy_row(sd_final_row* dst, const sd_final_row* src) {
    static_assert(sizeof(sd_final_row) == 80 && alignof(sd_final_row) == 8, "sd_final_row layout");
    const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
    uint64_t* d = reinterpret_cast<uint64_t*>(dst);
    for (int i = 0; i < 10; ++i) d[i] = s[i];
}

struct FinArgs {
    FinalTables tb;
    const DevRec* recs;
    const int64_t* ridx;       // null: row m is recs[m]
    const int64_t* widx;
    const uint32_t* words;
    const uint32_t* hwords;
    const int64_t* moff;
    const int64_t* rlen;       // null: segments are not clamped
    int n_reads;
    const int64_t* n_ptr;      // the number of rows
    int64_t cap;               // rows the outputs have room for
    sd_final_row* rows;
    double* alt;
    uint8_t* keep;
    unsigned long long* und;
};

// lane 0 of a row's group, with the row's identities: the undecided count or the row and its flag
__device__ inline void fin_finish(const FinArgs& a, int64_t m, const DevRec& x, bool missing, int ko, double score, int sb, double sbs,
                                  int h0, double h0s, int h1, double h1s) {
    const int r = fin_read_of(a.moff, a.n_reads, m);
    if (missing || final_seg_splits(final_seg_len(x.start, x.end, a.rlen ? a.rlen[r] : -1), a.tb.tmax)) {
        atomicAdd(a.und, 1ull);
        return;   // (the flag stays 0)
    }
    sd_rec xr;
    xr.tmpl = x.tmpl; xr.start = x.start; xr.end = x.end; xr.score = x.score;
    sd_final_row f;
    if (final_fill_row(a.tb, r, xr, ko, score, sb, sbs, h0, h0s, h1, h1s, &f)) {
        fin_copy_row(a.rows + m, &f);
        a.keep[m] = 1;
    }
}

__global__ __launch_bounds__(ROWS_T) void sd_final_light(FinArgs a) {
    const int64_t m = (int64_t)blockIdx.x * ROWS_T + threadIdx.x;
    if (m >= *a.n_ptr || m >= a.cap) return;
    const DevRec x = a.recs[a.ridx ? a.ridx[m] : m];
    const bool bad_t = x.tmpl < 0 || x.tmpl >= a.tb.n_tmpl;
    const uint32_t w = a.words[a.widx[m]];
    fin_finish(a, m, x, bad_t || final_word_missing(w), bad_t ? 0 : a.tb.key_of_t[x.tmpl], final_ident_percent(w), -1, -1.0, -1, -1.0, -1, -1.0);
}

// L lanes per row (a power of two, 8 .. 64: the smallest that holds T, so that small sets do not idle a wave)
template <int L>
__global__ __launch_bounds__(ROWS_T) void sd_final_best(FinArgs a) {
    const int l = threadIdx.x % L;
    const int64_t m = (int64_t)blockIdx.x * (ROWS_T / L) + threadIdx.x / L;   // (the same in every lane of a group)
    if (m >= *a.n_ptr || m >= a.cap) return;
    const int T = a.tb.n_tmpl, nK = a.tb.n_keys;
    const DevRec x = a.recs[a.ridx ? a.ridx[m] : m];
    const bool bad_t = x.tmpl < 0 || x.tmpl >= T;
    const uint32_t* __restrict__ v = a.words + (size_t)a.widx[m] * (size_t)T;
    const uint32_t* __restrict__ hw = a.hwords + (size_t)a.widx[m] * (size_t)T;
    // ONE pass over the row's words, each read once.  Homopolymer words (main.py:130-135: all monomers, the own one
    // included, stable sort by -score): ranks 0 and 1 = the two best under final_better.  Plain words (main.py:118-128):
    // template j speaks for its key k only if it is the LAST template of that name (kcol[k] == j) -- then its identity
    // is the key's, goes to alt, is the row's own score (k == ko) or a candidate for the first maximum among the other
    // keys.  And: is every word there?
    const int ko = bad_t ? 0 : a.tb.key_of_t[x.tmpl];
    int missing = bad_t ? 1 : 0;
    double v1 = 0, v2 = 0, sbs = 0, score = 0;
    int i1 = -1, i2 = -1, sb = -1, own = 0;
    for (int j = l; j < T; j += L) {
        const uint32_t w = v[j], h = hw[j];
        missing |= (final_word_missing(w) || final_word_missing(h)) ? 1 : 0;
        const double hv = final_ident_percent(h);
        if (final_better(hv, j, v1, i1)) { v2 = v1; i2 = i1; v1 = hv; i1 = j; }
        else if (final_better(hv, j, v2, i2)) { v2 = hv; i2 = j; }
        const int k = a.tb.key_of_il[j];
        if (a.tb.kcol[k] != j) continue;
        const double kv = final_ident_percent(w);
        a.alt[(size_t)m * (size_t)nK + (size_t)k] = kv;
        if (k == ko) { score = kv; own = 1; }
        else if (final_better(kv, k, sbs, sb)) { sbs = kv; sb = k; }
    }
    for (int off = L / 2; off > 0; off >>= 1) {
        missing |= __shfl_xor(missing, off, L);
        const double o1 = __shfl_xor(v1, off, L), o2 = __shfl_xor(v2, off, L);
        const int j1 = __shfl_xor(i1, off, L), j2 = __shfl_xor(i2, off, L);
        if (final_better(o1, j1, v1, i1)) {          // the other half's best wins: the second is mine or its second
            if (final_better(v1, i1, o2, j2)) { v2 = v1; i2 = i1; } else { v2 = o2; i2 = j2; }
            v1 = o1; i1 = j1;
        } else if (final_better(o1, j1, v2, i2)) { v2 = o1; i2 = j1; }
        const double os = __shfl_xor(sbs, off, L);
        const int js = __shfl_xor(sb, off, L);
        if (final_better(os, js, sbs, sb)) { sbs = os; sb = js; }
        const double oc = __shfl_xor(score, off, L);   // (exactly one lane met the own key's template)
        const int oo = __shfl_xor(own, off, L);
        if (oo) { score = oc; own = 1; }
    }
    if (l != 0) return;
    fin_finish(a, m, x, missing != 0, ko, score, sb, sb < 0 ? -1.0 : sbs, i1 < 0 ? -1 : a.tb.key_of_il[i1], i1 < 0 ? -1.0 : v1,
               i2 < 0 ? -1 : a.tb.key_of_il[i2], i2 < 0 ? -1.0 : v2);
}

// workgroups [0, n_tiles): the kept rows of a tile to the caller's rows, and where each went; behind them: row_off
__global__ __launch_bounds__(ROWS_T) void sd_final_scatter(const sd_final_row* __restrict__ sel, const uint8_t* __restrict__ keep,
                                                          int64_t n, int64_t n_tiles, const int64_t* __restrict__ bbase,
                                                          const int64_t* __restrict__ moff, int n_reads,
                                                          sd_final_row* __restrict__ out, int64_t cap, int64_t* __restrict__ dst,
                                                          int64_t* __restrict__ row_off) {
    if ((int64_t)blockIdx.x < n_tiles) {
        const int64_t i0 = (int64_t)blockIdx.x * ROWS_TILE + threadIdx.x * 4;
        const uint32_t f = rows_flags(keep, n, i0);
        int total;
        int64_t at = bbase[blockIdx.x] + block_scan<int>(rows_flag_count(f), &total);
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= n) break;
            if ((f >> (8 * k)) & 1u) {
                if (at < cap) fin_copy_row(out + at, sel + i0 + k);
                dst[i0 + k] = at < cap ? at : -1;
                ++at;
            } else {
                dst[i0 + k] = -1;
            }
        }
        return;
    }
    const int64_t r = ((int64_t)blockIdx.x - n_tiles) * ROWS_T + threadIdx.x;
    if (r > n_reads) return;
    row_off[r] = rows_flags_before(keep, bbase, moff[r]);
}

// a wave per row (strided): the key identities of the kept rows to their places
__global__ __launch_bounds__(ROWS_T) void sd_final_alt(const double* __restrict__ sel, const int64_t* __restrict__ dst,
                                                      const int64_t* __restrict__ n_ptr, int64_t cap, int n_keys,
                                                      double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = ((int64_t)gridDim.x * ROWS_T) >> 6;
    const int64_t n = *n_ptr < cap ? *n_ptr : cap;
    for (int64_t m = ((int64_t)blockIdx.x * ROWS_T + threadIdx.x) >> 6; m < n; m += nw) {
        const int64_t at = dst[m];
        if (at < 0) continue;
        for (int k = lane; k < n_keys; k += 64) out[(size_t)at * (size_t)n_keys + (size_t)k] = sel[(size_t)m * (size_t)n_keys + (size_t)k];
    }
}

}  // namespace sd

namespace sdi {

static inline unsigned fin_grid(int64_t items, int per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }

void final_sources(FinalWS& f, RowsWS& ws, hipStream_t st) {
    const int64_t cap = std::max<int64_t>(ws.n_recs, 1);
    f.src.alloc((size_t)cap);
    f.moff.alloc((size_t)ws.n_reads + 1);
    f.settled = false;
    const int64_t nb = ws.n_tiles + ((int64_t)ws.n_reads + 1 + sd::ROWS_T - 1) / sd::ROWS_T;
    hipLaunchKernelGGL(sd::sd_final_sources, dim3((unsigned)nb), dim3(sd::ROWS_T), 0, st, ws.keep.p, ws.n_recs, ws.n_tiles,
                       ws.bbase.p, ws.off.p, (int)ws.n_reads, f.src.p, cap, f.moff.p);
    SD_HIP(hipGetLastError());
}

void final_select(FinalWS& f, hipStream_t st, const sd::FinalTables& dtb, const sd::DevRec* recs, const int64_t* ridx,
                  const int64_t* widx, const uint32_t* words, const uint32_t* hwords, const int64_t* moff,
                  const int64_t* d_rlen, int32_t n_reads, int64_t cap_rows, const int64_t* n_ptr) {
    const int64_t cap = std::max<int64_t>(cap_rows, 0);
    f.cap_rows = cap;
    f.n_reads = n_reads;
    f.n_keys = dtb.second_best ? dtb.n_keys : 0;
    f.n_ptr = n_ptr;
    f.d_moff = moff;
    f.n_tiles = (cap + sd::ROWS_TILE - 1) / sd::ROWS_TILE;
    const size_t keep_bytes = ((size_t)cap + 3) / 4 * 4;
    f.rows.alloc((size_t)cap);
    if (dtb.second_best) f.alt.alloc((size_t)cap * (size_t)dtb.n_keys);
    f.keep.alloc(keep_bytes);
    f.dst.alloc((size_t)cap);
    f.bsum.alloc((size_t)f.n_tiles);
    f.bbase.alloc((size_t)f.n_tiles + 1);
    f.und.alloc(1);
    f.h_counts.alloc(2);
    if (!f.ev_sel) SD_HIP(hipEventCreateWithFlags(&f.ev_sel, hipEventDisableTiming));
    f.settled = false;
    if (keep_bytes) SD_HIP(hipMemsetAsync(f.keep.p, 0, keep_bytes, st));
    SD_HIP(hipMemsetAsync(f.und.p, 0, sizeof(unsigned long long), st));
    sd::FinArgs a{dtb, recs, ridx, widx, words, hwords, moff, d_rlen, (int)n_reads, n_ptr, cap, f.rows.p, f.alt.p, f.keep.p, f.und.p};
    if (cap > 0 && n_reads > 0) {
        if (!dtb.second_best) {
            hipLaunchKernelGGL(sd::sd_final_light, dim3(fin_grid(cap, sd::ROWS_T)), dim3(sd::ROWS_T), 0, st, a);
        } else {
            const int T = dtb.n_tmpl;
            if (T <= 8) hipLaunchKernelGGL(sd::sd_final_best<8>, dim3(fin_grid(cap, sd::ROWS_T / 8)), dim3(sd::ROWS_T), 0, st, a);
            else if (T <= 16) hipLaunchKernelGGL(sd::sd_final_best<16>, dim3(fin_grid(cap, sd::ROWS_T / 16)), dim3(sd::ROWS_T), 0, st, a);
            else if (T <= 32) hipLaunchKernelGGL(sd::sd_final_best<32>, dim3(fin_grid(cap, sd::ROWS_T / 32)), dim3(sd::ROWS_T), 0, st, a);
            else hipLaunchKernelGGL(sd::sd_final_best<64>, dim3(fin_grid(cap, sd::ROWS_T / 64)), dim3(sd::ROWS_T), 0, st, a);
        }
    }
    if (f.n_tiles > 0)
        hipLaunchKernelGGL(sd::sd_rows_count, dim3((unsigned)f.n_tiles), dim3(sd::ROWS_T), 0, st, f.keep.p, cap, f.bsum.p);
    hipLaunchKernelGGL(sd::scan_bases<int32_t>, dim3(1), dim3(sd::SCAN_T), 0, st, f.bsum.p, f.n_tiles, f.bbase.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipMemcpyAsync(f.h_counts.p, f.bbase.p + f.n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SD_HIP(hipMemcpyAsync(f.h_counts.p + 1, f.und.p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SD_HIP(hipEventRecord(f.ev_sel, st));
}

void final_scatter(FinalWS& f, hipStream_t st, sd_final_row* out, int64_t cap, int64_t* row_off, double* alt) {
    const int64_t nb = f.n_tiles + ((int64_t)f.n_reads + 1 + sd::ROWS_T - 1) / sd::ROWS_T;
    // (rows behind *n_ptr carry no flag: the tiles run over the whole capacity)
    hipLaunchKernelGGL(sd::sd_final_scatter, dim3((unsigned)nb), dim3(sd::ROWS_T), 0, st, f.rows.p, f.keep.p, f.cap_rows, f.n_tiles,
                       f.bbase.p, f.d_moff, (int)f.n_reads, out, cap, f.dst.p, row_off);
    if (alt && f.n_keys > 0 && f.cap_rows > 0) {
        const unsigned g = (unsigned)std::min<int64_t>(4096, (f.cap_rows + 3) / 4);
        hipLaunchKernelGGL(sd::sd_final_alt, dim3(g), dim3(sd::ROWS_T), 0, st, f.alt.p, f.dst.p, f.n_ptr, f.cap_rows, f.n_keys, alt);
    }
    SD_HIP(hipGetLastError());
    if (!f.ev_free) SD_HIP(hipEventCreateWithFlags(&f.ev_free, hipEventDisableTiming));
    SD_HIP(hipEventRecord(f.ev_free, st));
    f.free_recorded = true;
}

// the PostProcessor of the two test entries
static int final_entry_pp(sd::PostProcessor& pp, const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens,
                          int32_t n_mono, int32_t min_identity, int32_t second_best, const double* lr_coef, int32_t per) {
    if (n_mono <= 0 || !mono_names || !mono_seqs || !mono_lens || !lr_coef) return SD_ERR_PARAM;
    std::vector<sd::Seq> monos;
    for (int32_t m = 0; m < n_mono; ++m) {
        if (!mono_names[m] || !mono_seqs[m] || mono_lens[m] <= 0) return SD_ERR_PARAM;
        monos.push_back(sd::Seq{mono_names[m], std::string(mono_seqs[m], (size_t)mono_lens[m])});
    }
    std::string err;
    const int rc = pp.init(monos, min_identity, second_best != 0, lr_coef, -1, 1, err);
    if (rc) return rc;
    return per == (second_best ? 2 * n_mono : 1) ? SD_OK : SD_ERR_PARAM;
}

// row_off: n_reads + 1 ascending offsets from 0; every word index inside the word arrays
static bool final_entry_ok(const int64_t* row_off, int32_t n_reads, const int64_t* widx, int64_t n_word_rows) {
    if (row_off[0] != 0) return false;
    for (int32_t r = 0; r < n_reads; ++r)
        if (row_off[r + 1] < row_off[r]) return false;
    if (row_off[n_reads] >= ((int64_t)1 << 31)) return false;
    for (int64_t b = 0; b < row_off[n_reads]; ++b)
        if (widx[b] < 0 || widx[b] >= n_word_rows) return false;
    return true;
}

}  // namespace sdi

extern "C" {

int sd_final_select_host(const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                         int32_t min_identity, int32_t second_best, const double* lr_coef, const sd_rec* rows,
                         const int64_t* row_off, int32_t n_reads, const int64_t* widx, const uint32_t* words,
                         const uint32_t* hwords, int64_t n_word_rows, int32_t per, const int64_t* read_len,
                         sd_final_row* out, int64_t* out_off, double* alt, int64_t* n_rows, int64_t* n_undecided) try {
    if (n_reads < 0 || !row_off || !out_off || n_word_rows < 0) return SD_ERR_PARAM;
    sd::PostProcessor pp;
    int rc = final_entry_pp(pp, mono_names, mono_seqs, mono_lens, n_mono, min_identity, second_best, lr_coef, per);
    if (rc) return rc;
    const int64_t nB = row_off[n_reads];
    if (nB > 0 && (!rows || !widx || !words || !out || (second_best && (!hwords || !alt)))) return SD_ERR_PARAM;
    if (!final_entry_ok(row_off, n_reads, widx, n_word_rows)) return SD_ERR_PARAM;
    for (int64_t b = 0; b < nB; ++b)
        if (rows[b].tmpl < 0 || rows[b].tmpl >= 2 * n_mono) return SD_ERR_PARAM;
    return pp.select_words(rows, row_off, n_reads, widx, words, hwords, read_len, out, out_off, alt, n_rows, n_undecided);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_final_select_dev(const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                        int32_t min_identity, int32_t second_best, const double* lr_coef, const sd_rec* d_rows,
                        const int64_t* d_row_off, int32_t n_reads, const int64_t* d_widx, const uint32_t* d_words,
                        const uint32_t* d_hwords, int64_t n_word_rows, int32_t per, const int64_t* d_read_len, int32_t device,
                        void* hip_stream, sd_final_row* d_out, int64_t* d_out_off, double* d_alt, int64_t* n_rows,
                        int64_t* n_undecided) try {
    static_assert(sizeof(sd_rec) == sizeof(sd::DevRec), "record layout");
    if (n_reads < 0 || !d_row_off || !d_out_off || n_word_rows < 0 || device < 0) return SD_ERR_PARAM;
    sd::PostProcessor pp;
    int rc = final_entry_pp(pp, mono_names, mono_seqs, mono_lens, n_mono, min_identity, second_best, lr_coef, per);
    if (rc) return rc;
    if ((rc = device_check(device, nullptr, 0))) return rc;   // (device < 0: refused above)
    try {
        SD_HIP(hipSetDevice(device));
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        std::vector<int64_t> off((size_t)n_reads + 1);
        SD_HIP(hipMemcpyAsync(off.data(), d_row_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));
        if (off[0] != 0 || off[(size_t)n_reads] < 0 || off[(size_t)n_reads] >= ((int64_t)1 << 31)) return SD_ERR_PARAM;
        const int64_t nB = off[(size_t)n_reads];
        if (nB > 0 && (!d_rows || !d_widx || !d_words || !d_out || (second_best && (!d_hwords || !d_alt)))) return SD_ERR_PARAM;
        std::vector<int64_t> widx((size_t)nB);
        std::vector<sd_rec> rows((size_t)nB);
        if (nB > 0) {
            SD_HIP(hipMemcpyAsync(widx.data(), d_widx, (size_t)nB * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(rows.data(), d_rows, (size_t)nB * sizeof(sd_rec), hipMemcpyDeviceToHost, st));
            SD_HIP(hipStreamSynchronize(st));
        }
        if (!final_entry_ok(off.data(), n_reads, widx.data(), n_word_rows)) return SD_ERR_PARAM;
        for (int64_t b = 0; b < nB; ++b)
            if (rows[(size_t)b].tmpl < 0 || rows[(size_t)b].tmpl >= 2 * n_mono) return SD_ERR_PARAM;
        FinalDevTables dt;
        dt.upload(pp.final_tables());
        FinalWS f;
        final_select(f, st, dt.tb, reinterpret_cast<const sd::DevRec*>(d_rows), nullptr, d_widx, d_words, d_hwords, d_row_off,
                     d_read_len, n_reads, nB, d_row_off + n_reads);
        SD_HIP(hipEventSynchronize(f.ev_sel));
        final_scatter(f, st, d_out, f.h_counts.p[0], d_out_off, second_best ? d_alt : nullptr);
        SD_HIP(hipStreamSynchronize(st));   // (the workspace goes back with nothing in flight on it)
        if (n_rows) *n_rows = f.h_counts.p[0];
        if (n_undecided) *n_undecided = f.h_counts.p[1];
    } catch (const HipFail&) {
        return SD_ERR_HIP;
    }
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
