// sd_text_dev.hip -- the text of device rows, formatted on the device: the last link of the chain DeviceReads -> device
// rows -> device final rows.  The bytes of a row are sd_text_dev.hpp, one text with the host twin at the end of this file.
//   sd_text_raw_len / sd_text_final_len   one lane per row: the row is checked against its tables (a bad index is counted,
//                      never followed), the bytes of the tile's rows before it go to row_pos[row] and the tile's sum (256
//                      rows) to tsum; the raw
//                      kernel also finds the row's read (row_read).  With alt, the lanes of the final kernel then stride
//                      the tile's n_keys identities per row, coalesced, and add each line's digits into the row's LDS slot.
//   scan_bases         (sd_scan_dev.hpp) one workgroup: the tile sums -> the bytes before each tile (int64)
//   scan_place         (sd_scan_dev.hpp) row_pos[row] = bytes before the row; row_pos[n_rows] = the total
//   sd_text_read_pos   the row offsets are checked; read_pos[r] = row_pos[row_off[r]]; totals and counts -> 32 bytes
//   sd_text_write      a workgroup takes 256 consecutive rows (_alt: whole final rows of about 256 lines together, their
//                      line positions from a scan inside the workgroup), whose text is one byte range.  The range is cut
//                      into tiles of 32 KB that begin on a 16-byte line of the text buffer; for every tile each lane
//                      writes its row through a window (TextWindow) into LDS, and the workgroup streams the tile out, one
//                      16-byte store per lane and line.  Only the first and the last line of a range can be shared with
//                      a neighbouring workgroup: those are written byte by byte, the range's own bytes only.  A row
//                      longer than a tile (a long read name) is simply in more than one tile's window.
// Nothing is allocated per call: scratch that scales with the job is the caller's, tile sums and counters are grow-only
// buffers of the sd_text_tables object.
#include "sd_pipeline.hpp"
#include "sd_scan_dev.hpp"
#include "sd_text_dev.hpp"

namespace sd {

constexpr int TEXT_T = SCAN_T;          // lanes per workgroup = rows per tile
constexpr int TEXT_TILE = 32768;        // bytes of text staged in LDS at a time
enum { TEXT_RAW = 0, TEXT_FINAL = 1, TEXT_ALT = 2 };
enum { CNT_BYTES = 0, CNT_ALT_BYTES = 1, CNT_ODD = 2, CNT_BAD = 3 };
typedef unsigned long long text_u64;

// the read r with row_off[r] <= i < row_off[r + 1] where the offsets rise; in [0, n_reads) whatever they hold
__device__ inline int32_t text_read_of(const int64_t* __restrict__ row_off, int32_t n_reads, int64_t i) {
    int32_t lo = 0, hi = n_reads;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (row_off[mid] > i) hi = mid; else lo = mid + 1;
    }
    return lo > 0 ? lo - 1 : 0;
}

__global__ __launch_bounds__(TEXT_T) void sd_text_raw_len(TextNames R, TextNames T, const sd_rec* __restrict__ rows, int64_t n,
                                                         const int64_t* __restrict__ row_off, int32_t* __restrict__ row_read,
                                                         int64_t* __restrict__ row_pos, int64_t* __restrict__ tsum,
                                                         text_u64* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * TEXT_T + threadIdx.x;
    int64_t len = 0;
    if (i < n) {
        int32_t rd = 0;
        bool ok = R.n > 0;
        if (ok) {
            rd = text_read_of(row_off, R.n, i);
            ok = row_off[rd] <= i && i < row_off[rd + 1];
        }
        const sd_rec r = rows[i];
        ok = ok && text_raw_ok(T, r);
        if (ok) len = text_raw_len(R, T, rd, r, i > row_off[rd] ? rows[i - 1].end : 0);
        else atomicAdd(cnt + CNT_BAD, 1ull);
        row_read[i] = rd;
    }
    int64_t total;
    const int64_t ex = block_scan<int64_t>(len, &total);
    if (i < n) row_pos[i] = ex;
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(TEXT_T) void sd_text_final_len(TextNames R, TextNames K, const sd_final_row* __restrict__ rows, int64_t n,
                                                           const int64_t* __restrict__ row_off, const double* __restrict__ alt,
                                                           int32_t n_keys, int64_t* __restrict__ row_pos, int64_t* __restrict__ alt_pos,
                                                           int64_t* __restrict__ tsum, int64_t* __restrict__ atsum,
                                                           text_u64* __restrict__ cnt) {
    __shared__ int acc[TEXT_T];
    const int64_t i0 = (int64_t)blockIdx.x * TEXT_T, i = i0 + threadIdx.x;
    acc[threadIdx.x] = 0;
    int64_t len = 0, common = 0;
    bool ok = false;
    int odd = 0;
    if (i < n) {
        const sd_final_row f = rows[i];
        ok = text_final_ok(R, K, f) && row_off[f.read] <= i && i < row_off[f.read + 1];
        if (ok) {
            len = text_final_len(R, K, f, &odd);
            common = text_alt_common(R, f);
        } else {
            atomicAdd(cnt + CNT_BAD, 1ull);
        }
    }
    int64_t total;
    const int64_t ex = block_scan<int64_t>(len, &total);
    if (i < n) row_pos[i] = ex;
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
    if (!alt) {
        if (odd) atomicAdd(cnt + CNT_ODD, (text_u64)odd);
        return;
    }
    __syncthreads();
    const int64_t left = n - i0;
    const uint32_t nl = (uint32_t)(left < TEXT_T ? (left > 0 ? left : 0) : TEXT_T) * (uint32_t)n_keys;
    const double* __restrict__ a = alt + i0 * n_keys;
    for (uint32_t j = threadIdx.x; j < nl; j += TEXT_T) atomicAdd(&acc[j / (uint32_t)n_keys], text_fixed2_len(a[j], &odd));
    __syncthreads();
    const int64_t alen = ok ? (int64_t)n_keys * common + (K.off[n_keys] - K.off[0]) + acc[threadIdx.x] : 0;
    if (odd) atomicAdd(cnt + CNT_ODD, (text_u64)odd);
    const int64_t aex = block_scan<int64_t>(alen, &total);
    if (i < n) alt_pos[i] = aex;
    if (threadIdx.x == 0) atsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(TEXT_T) void sd_text_read_pos(const int64_t* __restrict__ row_off, int32_t n_reads, int64_t n,
                                                          const int64_t* __restrict__ row_pos, const int64_t* __restrict__ alt_pos,
                                                          int64_t* __restrict__ read_pos, int64_t* __restrict__ alt_read_pos,
                                                          text_u64* __restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * TEXT_T + threadIdx.x;
    if (r > n_reads) return;
    const int64_t o = row_off[r];
    const bool bad = o < 0 || o > n || (r == 0 && o != 0) || (r == n_reads && o != n) || (r < n_reads && row_off[r + 1] < o);
    if (bad) atomicAdd(cnt + CNT_BAD, 1ull);
    const int64_t oc = o < 0 ? 0 : (o > n ? n : o);
    read_pos[r] = row_pos[oc];
    if (alt_pos) alt_read_pos[r] = alt_pos[oc];
    if (r == 0) {
        cnt[CNT_BYTES] = (text_u64)row_pos[n];
        cnt[CNT_ALT_BYTES] = alt_pos ? (text_u64)alt_pos[n] : 0ull;
    }
}

struct TextWriteArgs {
    TextNames R, K;                  // read names; template names (raw) or key names + "None"
    const void* rows;                // sd_rec (raw) or sd_final_row
    int64_t n_rows;
    const int64_t* row_off;          // raw: for prev_end
    const int32_t* row_read;         // raw: the read of a row
    const double* alt;
    int32_t n_keys;
    int32_t rows_per_wg;             // alt: final rows per workgroup
    const int64_t* pos;              // row_pos (raw, final) or alt_pos
    char* text;
    int64_t cap;                     // bytes of text: nothing is written at or behind it
};

template <int KIND>
__global__ __launch_bounds__(TEXT_T) void sd_text_write(TextWriteArgs a) {
    __shared__ uint4 tile4[TEXT_TILE / 16];
    char* tile = reinterpret_cast<char*>(tile4);
    const int tid = threadIdx.x;
    // the items of this workgroup: rows, or the lines of whole final rows
    int64_t first, n_items, base = 0;
    if (KIND == TEXT_ALT) {
        first = (int64_t)blockIdx.x * a.rows_per_wg;
        const int64_t r1 = first + a.rows_per_wg < a.n_rows ? first + a.rows_per_wg : a.n_rows;
        n_items = (r1 - first) * a.n_keys;
        base = a.pos[first];
    } else {
        first = (int64_t)blockIdx.x * TEXT_T;
        n_items = a.n_rows - first < TEXT_T ? a.n_rows - first : TEXT_T;
    }
    const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(a.text) & 15);
    for (int64_t b0 = 0; b0 < n_items; b0 += TEXT_T) {
        const int64_t j = b0 + tid;
        bool have = j < n_items;
        int64_t pos = 0, end = 0, lo, hi;
        int64_t row = 0;
        int32_t k = 0, rd = 0, prev = 0;
        sd_rec rr{};
        sd_final_row f{};
        double v = 0;
        if (KIND == TEXT_ALT) {
            int64_t len = 0;
            if (have) {
                const uint32_t rw = (uint32_t)j / (uint32_t)a.n_keys;   // (a workgroup holds max(256, n_keys) lines)
                row = first + rw;
                k = (int32_t)((uint32_t)j - rw * (uint32_t)a.n_keys);
                f = static_cast<const sd_final_row*>(a.rows)[row];
                v = a.alt[row * a.n_keys + k];
                have = text_final_ok(a.R, a.K, f);
                int odd = 0;
                if (have) len = text_alt_line_len(text_alt_common(a.R, f), a.K, k, v, &odd);
            }
            int64_t total;
            pos = base + block_scan<int64_t>(len, &total);
            end = pos + len;
            lo = base;
            hi = base + total;
            base = hi;
        } else {
            const int64_t e = b0 + TEXT_T < n_items ? b0 + TEXT_T : n_items;
            lo = a.pos[first + b0];
            hi = a.pos[first + e];
            if (have) {
                row = first + j;
                pos = a.pos[row];
                end = a.pos[row + 1];
                if (KIND == TEXT_RAW) {
                    rr = static_cast<const sd_rec*>(a.rows)[row];
                    rd = a.row_read[row];
                    have = rd >= 0 && rd < a.R.n && text_raw_ok(a.K, rr);
                    if (have) prev = row > a.row_off[rd] ? static_cast<const sd_rec*>(a.rows)[row - 1].end : 0;
                } else {
                    f = static_cast<const sd_final_row*>(a.rows)[row];
                    have = text_final_ok(a.R, a.K, f);
                }
            }
        }
        if (hi > a.cap) hi = a.cap;   // (positions the size call did not make: still nothing outside the text)
        if (lo < 0) lo = 0;
        // tiles of the range [lo, hi): each begins on a 16-byte line of the text buffer
        for (int64_t org = ((lo + mis) & ~(int64_t)15) - mis; org < hi; org += TEXT_TILE) {
            const int64_t w_lo = org > lo ? org : lo, w_hi = org + TEXT_TILE < hi ? org + TEXT_TILE : hi;
            const TextWindow w{tile, org, w_lo, w_hi};
            if (have && pos < w_hi && end > w_lo) {
                if (KIND == TEXT_RAW) (void)text_raw_put(w, pos, a.R, a.K, rd, rr, prev);
                else if (KIND == TEXT_FINAL) (void)text_final_put(w, pos, a.R, a.K, f);
                else (void)text_alt_put(w, pos, a.R, a.K, f, k, v);
            }
            __syncthreads();
            const int nch = (int)((w_hi - org + 15) >> 4);
            for (int c = tid; c < nch; c += TEXT_T) {
                const int64_t g = org + 16 * (int64_t)c;
                if (g >= w_lo && g + 16 <= w_hi) {
                    *reinterpret_cast<uint4*>(a.text + g) = tile4[c];
                } else {   // a line shared with the neighbouring range: this range's bytes only
                    const int64_t x1 = g + 16 < w_hi ? g + 16 : w_hi;
                    for (int64_t x = g > w_lo ? g : w_lo; x < x1; ++x) a.text[x] = tile[x - org];
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace sd

// ---- the name tables and the C-ABI ----------------------------------------------------------------------------------
struct sd_text_tables {
    std::vector<char> rbytes, cbytes;        // read names; column names with "None" behind them
    std::vector<int64_t> roff, coff;         // n_reads + 1; n_cols + 2
    int32_t n_reads = 0, n_cols = 0;
    std::mutex m;                            // one size call at a time: tile sums and counters are the object's
    int device = -1;                         // where the tables were uploaded (-1: not yet)
    DevBuf<char> d_rb, d_cb;
    DevBuf<int64_t> d_ro, d_co, tsum, tbase;
    DevBuf<sd::text_u64> cnt;
    PinBuf<sd::text_u64> h_cnt;
    hipEvent_t ev_size = nullptr, ev_use = nullptr;
    hipStream_t use_stream = nullptr;
    bool used = false;                       // ev_use has been recorded: a kernel may still read the tables
    sd::TextNames R(bool dev) const { return sd::TextNames{dev ? d_rb.p : rbytes.data(), dev ? d_ro.p : roff.data(), n_reads}; }
    // cols: n_cols names (raw: the templates), or with_none: the keys and "None"
    sd::TextNames K(bool dev, bool with_none) const {
        return sd::TextNames{dev ? d_cb.p : cbytes.data(), dev ? d_co.p : coff.data(), n_cols + (with_none ? 1 : 0)};
    }
};

namespace sdi {

static void text_names(const char* const* names, int32_t n, bool none, std::vector<char>& bytes, std::vector<int64_t>& off) {
    off.assign(1, 0);
    for (int32_t i = 0; i < n + (none ? 1 : 0); ++i) {
        const char* s = i < n ? names[i] : "None";
        bytes.insert(bytes.end(), s, s + std::strlen(s));
        off.push_back((int64_t)bytes.size());
    }
}

// device present, ordinal valid, tables on it (uploaded at the first call); the caller holds t->m and a DeviceScope
static int text_dev_check(int32_t device, char* eb, size_t el) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_err(eb, el, "no usable HIP device");
        return SD_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_err(eb, el, "device " + std::to_string(device) + " does not exist");
        return SD_ERR_PARAM;
    }
    return SD_OK;
}
static int text_upload(sd_text_tables* t, int32_t device, char* eb, size_t el) {
    if (t->device == device) return SD_OK;
    if (t->device >= 0) {
        set_err(eb, el, "the name tables lie on device " + std::to_string(t->device) + ", the call names device " + std::to_string(device));
        return SD_ERR_PARAM;
    }
    t->d_rb.upload(t->rbytes);
    t->d_cb.upload(t->cbytes);
    t->d_ro.upload(t->roff);
    t->d_co.upload(t->coff);
    ensure_event(t->ev_size, hipEventDisableTiming);
    ensure_event(t->ev_use, hipEventDisableTiming);
    t->device = device;
    return SD_OK;
}
// the write kernels read the tables whenever their stream gets to them: destroy waits for the last of them
static void text_used(sd_text_tables* t, hipStream_t st) {
    if (t->used && t->use_stream != st) SD_HIP(hipEventSynchronize(t->ev_use));   // (an event remembers one stream)
    SD_HIP(hipEventRecord(t->ev_use, st));
    t->use_stream = st;
    t->used = true;
}

static inline unsigned text_grid(int64_t items, int per) { return (unsigned)std::max<int64_t>(1, (items + per - 1) / per); }

// the tile bases of one position array and their place in it, then (last) the read positions and the counts; waits for
// the 32 bytes
static void text_scan_place(sd_text_tables* t, hipStream_t st, int64_t* pos, int64_t n, int64_t n_tiles, int which) {
    int64_t* tsum = t->tsum.p + which * std::max<int64_t>(1, n_tiles);
    int64_t* tbase = t->tbase.p + which * (n_tiles + 1);
    hipLaunchKernelGGL(sd::scan_bases<int64_t>, dim3(1), dim3(sd::TEXT_T), 0, st, tsum, n_tiles, tbase);
    hipLaunchKernelGGL(sd::scan_place<int64_t>, dim3(text_grid(n, sd::TEXT_T)), dim3(sd::TEXT_T), 0, st, pos, n, tbase, n_tiles);
}
static int text_size_end(sd_text_tables* t, hipStream_t st, const int64_t* row_off, int64_t n, const int64_t* row_pos,
                         const int64_t* alt_pos, int64_t* read_pos, int64_t* alt_read_pos, int64_t* bytes, int64_t* alt_bytes,
                         const char* who, char* eb, size_t el) {
    hipLaunchKernelGGL(sd::sd_text_read_pos, dim3(text_grid((int64_t)t->n_reads + 1, sd::TEXT_T)), dim3(sd::TEXT_T), 0, st, row_off,
                       t->n_reads, n, row_pos, alt_pos, read_pos, alt_read_pos, t->cnt.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipMemcpyAsync(t->h_cnt.p, t->cnt.p, 4 * sizeof(sd::text_u64), hipMemcpyDeviceToHost, st));
    SD_HIP(hipEventRecord(t->ev_size, st));
    SD_HIP(hipEventSynchronize(t->ev_size));   // the only wait: totals and counts
    if (bytes) *bytes = (int64_t)t->h_cnt.p[sd::CNT_BYTES];
    if (alt_bytes) *alt_bytes = alt_pos ? (int64_t)t->h_cnt.p[sd::CNT_ALT_BYTES] : 0;
    if (t->h_cnt.p[sd::CNT_BAD]) {
        set_err(eb, el, std::string(who) + ": a read, key or template index outside its table, or row offsets that do not rise from 0 to n_rows");
        return SD_ERR_PARAM;
    }
    if (t->h_cnt.p[sd::CNT_ODD]) {
        set_err(eb, el, std::string(who) + ": " + std::to_string(t->h_cnt.p[sd::CNT_ODD]) +
                            " identities are infinite, NaN or 2^40 and more: the device does not print them (the host call does)");
        return SD_ERR_UNSUPPORTED;
    }
    return SD_OK;
}

static void text_size_scratch(sd_text_tables* t, hipStream_t st, int64_t n_tiles) {
    t->tsum.alloc(2 * (size_t)std::max<int64_t>(1, n_tiles));
    t->tbase.alloc(2 * (size_t)(n_tiles + 1));
    t->cnt.alloc(4);
    t->h_cnt.alloc(4);
    SD_HIP(hipMemsetAsync(t->cnt.p, 0, 4 * sizeof(sd::text_u64), st));
}

// ---- the host twin ----
constexpr int64_t TEXT_HOST_BLOCK = 2048;   // rows per unit of the host's parallel loops

static bool text_offsets_ok(const int64_t* row_off, int32_t n_reads, int64_t n) {
    if (row_off[0] != 0 || row_off[n_reads] != n) return false;
    for (int32_t r = 0; r < n_reads; ++r)
        if (row_off[r + 1] < row_off[r]) return false;
    return true;
}
// exclusive scan in place: pos[i] = bytes before row i, pos[n] = all
static int64_t text_host_scan(int64_t* pos, int64_t n) {
    int64_t run = 0;
    for (int64_t i = 0; i < n; ++i) { const int64_t l = pos[i]; pos[i] = run; run += l; }
    pos[n] = run;
    return run;
}
template <class F>
static void text_host_blocks(int64_t n, int threads, F&& body) {
    sd::parallel_for((n + TEXT_HOST_BLOCK - 1) / TEXT_HOST_BLOCK, std::max(1, threads), 1, [&](int64_t b) {
        const int64_t e = std::min(n, (b + 1) * TEXT_HOST_BLOCK);
        for (int64_t i = b * TEXT_HOST_BLOCK; i < e; ++i) body(i);
    });
}

}  // namespace sdi

extern "C" {

int sd_text_tables_create(sd_text_tables** out, const char* const* read_names, int32_t n_reads, const char* const* col_names,
                          int32_t n_cols, char* errbuf, size_t errlen) try {
    if (!out || n_reads < 0 || n_cols < 0 || (n_reads > 0 && !read_names) || (n_cols > 0 && !col_names)) {
        set_err(errbuf, errlen, "sd_text_tables_create: missing name table");
        return SD_ERR_PARAM;
    }
    for (int32_t i = 0; i < n_reads; ++i)
        if (!read_names[i]) { set_err(errbuf, errlen, "sd_text_tables_create: missing read name"); return SD_ERR_PARAM; }
    for (int32_t i = 0; i < n_cols; ++i)
        if (!col_names[i]) { set_err(errbuf, errlen, "sd_text_tables_create: missing column name"); return SD_ERR_PARAM; }
    std::unique_ptr<sd_text_tables> t(new sd_text_tables);
    t->n_reads = n_reads;
    t->n_cols = n_cols;
    text_names(read_names, n_reads, false, t->rbytes, t->roff);
    text_names(col_names, n_cols, true, t->cbytes, t->coff);
    *out = t.release();
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_text_tables_destroy(sd_text_tables* t) {
    if (!t) return;
    if (t->used && hipEventSynchronize(t->ev_use) != hipSuccess) (void)hipGetLastError();   // (the buffers go to a pool below)
    if (t->ev_size) (void)hipEventDestroy(t->ev_size);
    if (t->ev_use) (void)hipEventDestroy(t->ev_use);
    delete t;
}

int sd_text_final_size_dev(sd_text_tables* t, const sd_final_row* d_rows, int64_t n_rows, const int64_t* d_row_off, const double* d_alt,
                           int32_t n_keys, int32_t device, void* hip_stream, int64_t* d_row_pos, int64_t* d_alt_pos,
                           int64_t* d_read_pos, int64_t* d_alt_read_pos, int64_t* final_bytes, int64_t* alt_bytes, char* errbuf,
                           size_t errlen) try {
    static const char* who = "sd_text_final_size_dev";
    if (!t || n_rows < 0 || !d_row_off || !d_row_pos || !d_read_pos || (n_rows > 0 && !d_rows) || (d_alt && (!d_alt_pos || !d_alt_read_pos))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    if (n_keys != t->n_cols) {
        set_err(errbuf, errlen, std::string(who) + ": n_keys = " + std::to_string(n_keys) + ", the table holds " + std::to_string(t->n_cols) + " keys");
        return SD_ERR_PARAM;
    }
    int rc = text_dev_check(device, errbuf, errlen);
    if (rc) return rc;
    try {
        std::lock_guard<std::mutex> g(t->m);
        DeviceScope on(device);
        if ((rc = text_upload(t, device, errbuf, errlen))) return rc;
        if ((rc = buffer_on_device(d_row_off, device, who, "row offset", errbuf, errlen))) return rc;
        if ((rc = buffer_on_device(d_row_pos, device, who, "row position", errbuf, errlen))) return rc;
        if ((rc = buffer_on_device(d_read_pos, device, who, "read position", errbuf, errlen))) return rc;
        if (n_rows > 0 && (rc = buffer_on_device(d_rows, device, who, "row", errbuf, errlen))) return rc;
        if (d_alt && (rc = buffer_on_device(d_alt_pos, device, who, "alt position", errbuf, errlen))) return rc;
        if (d_alt && n_rows > 0 && (rc = buffer_on_device(d_alt, device, who, "alt", errbuf, errlen))) return rc;
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        const int64_t n_tiles = (n_rows + sd::TEXT_T - 1) / sd::TEXT_T;
        text_size_scratch(t, st, n_tiles);
        hipLaunchKernelGGL(sd::sd_text_final_len, dim3(text_grid(n_rows, sd::TEXT_T)), dim3(sd::TEXT_T), 0, st, t->R(true), t->K(true, true),
                           d_rows, n_rows, d_row_off, d_alt, n_keys, d_row_pos, d_alt_pos, t->tsum.p,
                           t->tsum.p + std::max<int64_t>(1, n_tiles), t->cnt.p);
        text_scan_place(t, st, d_row_pos, n_rows, n_tiles, 0);
        if (d_alt) text_scan_place(t, st, d_alt_pos, n_rows, n_tiles, 1);
        return text_size_end(t, st, d_row_off, n_rows, d_row_pos, d_alt ? d_alt_pos : nullptr, d_read_pos, d_alt_read_pos, final_bytes,
                             alt_bytes, who, errbuf, errlen);
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_text_final_write_dev(sd_text_tables* t, const sd_final_row* d_rows, int64_t n_rows, const double* d_alt, int32_t n_keys,
                            int32_t device, void* hip_stream, const int64_t* d_row_pos, const int64_t* d_alt_pos, char* d_final_text,
                            int64_t final_bytes, char* d_alt_text, int64_t alt_bytes, char* errbuf, size_t errlen) try {
    static const char* who = "sd_text_final_write_dev";
    if (!t || n_rows < 0 || final_bytes < 0 || alt_bytes < 0 || !d_row_pos || (n_rows > 0 && !d_rows) || (final_bytes > 0 && !d_final_text) ||
        (d_alt && (!d_alt_pos || (alt_bytes > 0 && !d_alt_text)))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    if (n_keys != t->n_cols) {
        set_err(errbuf, errlen, std::string(who) + ": n_keys = " + std::to_string(n_keys) + ", the table holds " + std::to_string(t->n_cols) + " keys");
        return SD_ERR_PARAM;
    }
    int rc = text_dev_check(device, errbuf, errlen);
    if (rc) return rc;
    try {
        std::lock_guard<std::mutex> g(t->m);
        DeviceScope on(device);
        if ((rc = text_upload(t, device, errbuf, errlen))) return rc;
        if (final_bytes > 0 && (rc = buffer_on_device(d_final_text, device, who, "text", errbuf, errlen))) return rc;
        if (d_alt && alt_bytes > 0 && (rc = buffer_on_device(d_alt_text, device, who, "alt text", errbuf, errlen))) return rc;
        if (n_rows == 0) return SD_OK;
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        sd::TextWriteArgs a{t->R(true), t->K(true, true), d_rows, n_rows, nullptr, nullptr, d_alt, n_keys, 1, d_row_pos, d_final_text, final_bytes};
        if (final_bytes > 0)
            hipLaunchKernelGGL(sd::sd_text_write<sd::TEXT_FINAL>, dim3(text_grid(n_rows, sd::TEXT_T)), dim3(sd::TEXT_T), 0, st, a);
        if (d_alt && alt_bytes > 0 && n_keys > 0) {
            a.rows_per_wg = std::max(1, sd::TEXT_T / n_keys);
            a.pos = d_alt_pos;
            a.text = d_alt_text;
            a.cap = alt_bytes;
            hipLaunchKernelGGL(sd::sd_text_write<sd::TEXT_ALT>, dim3(text_grid(n_rows, a.rows_per_wg)), dim3(sd::TEXT_T), 0, st, a);
        }
        SD_HIP(hipGetLastError());
        text_used(t, st);
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_text_raw_size_dev(sd_text_tables* t, const sd_rec* d_rows, int64_t n_rows, const int64_t* d_row_off, int32_t device,
                         void* hip_stream, int32_t* d_row_read, int64_t* d_row_pos, int64_t* d_read_pos, int64_t* text_bytes,
                         char* errbuf, size_t errlen) try {
    static const char* who = "sd_text_raw_size_dev";
    if (!t || n_rows < 0 || !d_row_off || !d_row_pos || !d_read_pos || (n_rows > 0 && (!d_rows || !d_row_read))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    int rc = text_dev_check(device, errbuf, errlen);
    if (rc) return rc;
    try {
        std::lock_guard<std::mutex> g(t->m);
        DeviceScope on(device);
        if ((rc = text_upload(t, device, errbuf, errlen))) return rc;
        if ((rc = buffer_on_device(d_row_off, device, who, "row offset", errbuf, errlen))) return rc;
        if ((rc = buffer_on_device(d_row_pos, device, who, "row position", errbuf, errlen))) return rc;
        if ((rc = buffer_on_device(d_read_pos, device, who, "read position", errbuf, errlen))) return rc;
        if (n_rows > 0 && (rc = buffer_on_device(d_rows, device, who, "row", errbuf, errlen))) return rc;
        if (n_rows > 0 && (rc = buffer_on_device(d_row_read, device, who, "row read", errbuf, errlen))) return rc;
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        const int64_t n_tiles = (n_rows + sd::TEXT_T - 1) / sd::TEXT_T;
        text_size_scratch(t, st, n_tiles);
        hipLaunchKernelGGL(sd::sd_text_raw_len, dim3(text_grid(n_rows, sd::TEXT_T)), dim3(sd::TEXT_T), 0, st, t->R(true), t->K(true, false),
                           d_rows, n_rows, d_row_off, d_row_read, d_row_pos, t->tsum.p, t->cnt.p);
        text_scan_place(t, st, d_row_pos, n_rows, n_tiles, 0);
        return text_size_end(t, st, d_row_off, n_rows, d_row_pos, nullptr, d_read_pos, nullptr, text_bytes, nullptr, who, errbuf, errlen);
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_text_raw_write_dev(sd_text_tables* t, const sd_rec* d_rows, int64_t n_rows, const int64_t* d_row_off, int32_t device,
                          void* hip_stream, const int32_t* d_row_read, const int64_t* d_row_pos, char* d_text, int64_t text_bytes,
                          char* errbuf, size_t errlen) try {
    static const char* who = "sd_text_raw_write_dev";
    if (!t || n_rows < 0 || text_bytes < 0 || !d_row_off || !d_row_pos || (n_rows > 0 && (!d_rows || !d_row_read)) ||
        (text_bytes > 0 && !d_text)) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    int rc = text_dev_check(device, errbuf, errlen);
    if (rc) return rc;
    try {
        std::lock_guard<std::mutex> g(t->m);
        DeviceScope on(device);
        if ((rc = text_upload(t, device, errbuf, errlen))) return rc;
        if (text_bytes > 0 && (rc = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return rc;
        if (n_rows == 0 || text_bytes == 0) return SD_OK;
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        sd::TextWriteArgs a{t->R(true), t->K(true, false), d_rows, n_rows, d_row_off, d_row_read, nullptr, 0, 1, d_row_pos, d_text, text_bytes};
        hipLaunchKernelGGL(sd::sd_text_write<sd::TEXT_RAW>, dim3(text_grid(n_rows, sd::TEXT_T)), dim3(sd::TEXT_T), 0, st, a);
        SD_HIP(hipGetLastError());
        text_used(t, st);
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_text_final_host(sd_text_tables* t, const sd_final_row* rows, int64_t n_rows, const int64_t* row_off, const double* alt,
                       int32_t n_keys, int32_t threads, char** final_text, int64_t* final_bytes, char** alt_text, int64_t* alt_bytes,
                       int64_t* row_pos, int64_t* alt_pos, int64_t* read_pos, int64_t* alt_read_pos, char* errbuf, size_t errlen) try {
    static const char* who = "sd_text_final_host";
    if (final_text) *final_text = nullptr;
    if (alt_text) *alt_text = nullptr;
    if (!t || n_rows < 0 || !row_off || !final_text || !final_bytes || (n_rows > 0 && !rows) || (alt && (!alt_text || !alt_bytes))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    if (n_keys != t->n_cols) {
        set_err(errbuf, errlen, std::string(who) + ": n_keys = " + std::to_string(n_keys) + ", the table holds " + std::to_string(t->n_cols) + " keys");
        return SD_ERR_PARAM;
    }
    const sd::TextNames R = t->R(false), K = t->K(false, true);
    bool ok = text_offsets_ok(row_off, t->n_reads, n_rows);
    for (int64_t i = 0; ok && i < n_rows; ++i)
        ok = sd::text_final_ok(R, K, rows[i]) && row_off[rows[i].read] <= i && i < row_off[rows[i].read + 1];
    if (!ok) {
        set_err(errbuf, errlen, std::string(who) + ": a read or key index outside its table, or row offsets that do not rise from 0 to n_rows");
        return SD_ERR_PARAM;
    }
    std::vector<int64_t> own_pos, own_apos;
    if (!row_pos) { own_pos.resize((size_t)n_rows + 1); row_pos = own_pos.data(); }
    if (alt && !alt_pos) { own_apos.resize((size_t)n_rows + 1); alt_pos = own_apos.data(); }
    text_host_blocks(n_rows, threads, [&](int64_t i) {
        int odd = 0;
        row_pos[i] = sd::text_final_len(R, K, rows[i], &odd);
        if (alt) {
            const int64_t common = sd::text_alt_common(R, rows[i]);
            int64_t s = 0;
            for (int32_t k = 0; k < n_keys; ++k) s += sd::text_alt_line_len(common, K, k, alt[i * n_keys + k], &odd);
            alt_pos[i] = s;
        }
    });
    const int64_t fb = text_host_scan(row_pos, n_rows), ab = alt ? text_host_scan(alt_pos, n_rows) : 0;
    char* ft = static_cast<char*>(std::malloc((size_t)std::max<int64_t>(fb, 1)));
    char* at = alt ? static_cast<char*>(std::malloc((size_t)std::max<int64_t>(ab, 1))) : nullptr;
    if (!ft || (alt && !at)) { std::free(ft); std::free(at); return SD_ERR_INTERNAL; }
    const sd::TextWindow wf{ft, 0, 0, fb}, wa{at, 0, 0, ab};
    text_host_blocks(n_rows, threads, [&](int64_t i) {
        (void)sd::text_final_put(wf, row_pos[i], R, K, rows[i]);
        if (alt) {
            int64_t p = alt_pos[i];
            for (int32_t k = 0; k < n_keys; ++k) p = sd::text_alt_put(wa, p, R, K, rows[i], k, alt[i * n_keys + k]);
        }
    });
    for (int32_t r = 0; r <= t->n_reads; ++r) {
        if (read_pos) read_pos[r] = row_pos[row_off[r]];
        if (alt && alt_read_pos) alt_read_pos[r] = alt_pos[row_off[r]];
    }
    *final_text = ft;
    *final_bytes = fb;
    if (alt) { *alt_text = at; *alt_bytes = ab; }
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_text_raw_host(sd_text_tables* t, const sd_rec* rows, int64_t n_rows, const int64_t* row_off, int32_t threads, char** text,
                     int64_t* text_bytes, int64_t* row_pos, int64_t* read_pos, char* errbuf, size_t errlen) try {
    static const char* who = "sd_text_raw_host";
    if (text) *text = nullptr;
    if (!t || n_rows < 0 || !row_off || !text || !text_bytes || (n_rows > 0 && !rows)) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    const sd::TextNames R = t->R(false), T = t->K(false, false);
    bool ok = text_offsets_ok(row_off, t->n_reads, n_rows);
    for (int64_t i = 0; ok && i < n_rows; ++i) ok = sd::text_raw_ok(T, rows[i]);
    if (!ok) {
        set_err(errbuf, errlen, std::string(who) + ": a template index outside its table, or row offsets that do not rise from 0 to n_rows");
        return SD_ERR_PARAM;
    }
    std::vector<int64_t> own_pos;
    if (!row_pos) { own_pos.resize((size_t)n_rows + 1); row_pos = own_pos.data(); }
    std::vector<int32_t> row_read((size_t)n_rows);
    sd::parallel_for(t->n_reads, std::max(1, (int)threads), 16, [&](int64_t r) {
        for (int64_t i = row_off[r]; i < row_off[r + 1]; ++i) row_read[(size_t)i] = (int32_t)r;
    });
    auto prev_end = [&](int64_t i) { return i > row_off[row_read[(size_t)i]] ? rows[i - 1].end : 0; };
    text_host_blocks(n_rows, threads, [&](int64_t i) { row_pos[i] = sd::text_raw_len(R, T, row_read[(size_t)i], rows[i], prev_end(i)); });
    const int64_t nb = text_host_scan(row_pos, n_rows);
    char* out = static_cast<char*>(std::malloc((size_t)std::max<int64_t>(nb, 1)));
    if (!out) return SD_ERR_INTERNAL;
    const sd::TextWindow w{out, 0, 0, nb};
    text_host_blocks(n_rows, threads, [&](int64_t i) { (void)sd::text_raw_put(w, row_pos[i], R, T, row_read[(size_t)i], rows[i], prev_end(i)); });
    if (read_pos)
        for (int32_t r = 0; r <= t->n_reads; ++r) read_pos[r] = row_pos[row_off[r]];
    *text = out;
    *text_bytes = nb;
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
