// sd_autocorr.hip -- k-mer autocorrelation of every read against itself (--autocorr): where the tandem arrays are and what
// their period is in bases, without a monomer file.  sd_autocorr.hpp holds the definition and everything host and device
// compute alike; this file holds the kernels, the host form and the C-ABI (include/sd_hip.h: sd_autocorr_*).
//   sd_autocorr_prep   a wave per 64 bases: three ballots turn the byte text into the bit planes lo | hi | valid of
//                      sd_autocorr.hpp (zeros behind every read, one word of zeros after each)
//   sd_autocorr_pairs  a workgroup (256 lanes) per (tile of a window, block of 256 lags).  The partner stretch -- the tile's
//                      words shifted by the block's first lag, 72 words per plane -- goes to LDS; the tile's own words are
//                      the same for every lane and come through the scalar cache.  A lane owns one lag d: per tile word it
//                      reads two new 32-bit words of each partner plane (adjacent lanes hold adjacent lags, so a wave reads
//                      2 or 3 addresses: broadcasts), aligns them by d & 31 (v_alignbit), forms the equality word
//                      (autocorr_eq), finds the starts of k-runs in the 96 bits {this word, the next} by shift-and doubling
//                      (autocorr_runs, at most 5 steps), masks to the tile and adds a population count.  The end condition
//                      i <= n - d - k is the partner's valid plane: no bounds test in the loop.  One 64-bit vector atomic
//                      add per (window, lag) and workgroup ends it, skipped for a zero.
// Launches: the work items are (tile, lag block) pairs; a launch takes at most AUTOCORR_LAUNCH_WG of them (sd_autocorr.hpp:
// 2^33 base-lag products), so a 250-Mb read with D = 2^20 is about 30 000 launches of the order of 100 microseconds each and
// never one long kernel.  Workgroups whose lags all exceed n - k, or whose tile has no position left for them, return at once.
#include <algorithm>
#include <atomic>
#include <cstring>

#include "sd_autocorr.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"

namespace sd {

constexpr int AC_T = 256;                                                    // threads per workgroup (= AUTOCORR_LAGS)
constexpr int AC_PW = AUTOCORR_TILE_WORDS + 1 + AUTOCORR_LAGS / 64 + 3;      // partner words per plane in LDS
// the last 32-bit word a lane reads: word t + 1 = tile words (an unaligned tile spans one more), two words on, and the
// lane's own offset (lag - first lag rounded down to a word) >> 5
static_assert(2 * (AUTOCORR_TILE_WORDS + 1) + 2 + ((63 + AUTOCORR_LAGS - 1) >> 5) < 2 * AC_PW, "the partner stretch leaves LDS");
static_assert(3 * AC_PW <= AC_T, "one partner word per thread");
static_assert(AC_T == AUTOCORR_LAGS, "one lag per lane");

__global__ __launch_bounds__(AC_T) void sd_autocorr_prep(const uint8_t* __restrict__ text, const int64_t* __restrict__ roff,
                                                         const int64_t* __restrict__ rlen, const int64_t* __restrict__ pw, int n_reads,
                                                         int64_t words, uint64_t* __restrict__ lo, uint64_t* __restrict__ hi,
                                                         uint64_t* __restrict__ v) {
    const int lane = threadIdx.x & 63;
    const int64_t nwave = (int64_t)gridDim.x * (AC_T / 64);
    for (int64_t j = (int64_t)blockIdx.x * (AC_T / 64) + (threadIdx.x >> 6); j < words; j += nwave) {
        int a = 0, b = n_reads;   // the read of word j: the last one whose planes start at or before it
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (pw[m] <= j) a = m; else b = m;
        }
        const int64_t i = (j - pw[a]) * 64 + lane;
        const int c = i < rlen[a] ? autocorr_code(text[roff[a] + i]) : -1;
        const uint64_t bv = __ballot(c >= 0), bl = __ballot(c >= 0 && (c & 1)), bh = __ballot(c >= 0 && (c & 2));
        if (lane == 0) {
            lo[j] = bl;
            hi[j] = bh;
            v[j] = bv;
        }
    }
}

void launch_autocorr_prep(hipStream_t st, unsigned grid, const uint8_t* text, const int64_t* roff, const int64_t* rlen, const int64_t* pw,
                          int n_reads, int64_t words, uint64_t* lo, uint64_t* hi, uint64_t* v) {
    hipLaunchKernelGGL(sd_autocorr_prep, dim3(grid), dim3(AC_T), 0, st, text, roff, rlen, pw, n_reads, words, lo, hi, v);
}

struct AcArgs {
    const uint64_t *lo, *hi, *v;                      // the planes of the job
    const int64_t *rlen, *pw, *win_off, *tile_off;    // per read (tile_off, pw, win_off: n_reads + 1)
    int n_reads, k;
    int sh[5];                                        // autocorr_steps(k)
    int64_t W, D;
    int64_t tile0, n_tiles, lb0;                      // the launch: its first tile and first lag block
    unsigned long long* counts;
};

template <int NS>
__global__ __launch_bounds__(AC_T) void sd_autocorr_pairs(AcArgs a) {
    __shared__ uint64_t part[3][AC_PW];
    const int64_t tile = a.tile0 + blockIdx.y;
    const int64_t dl = 1 + (a.lb0 + blockIdx.x) * AUTOCORR_LAGS;   // the block's first lag
    if (tile >= a.n_tiles || dl > a.D) return;
    int r = 0, rb = a.n_reads;   // the read of the tile: the last one whose tiles start at or before it
    while (rb - r > 1) {
        const int m = (r + rb) >> 1;
        if (a.tile_off[m] <= tile) r = m; else rb = m;
    }
    const int64_t n = a.rlen[r];
    if (dl + a.k > n) return;   // every lag of the block exceeds n - k: all zeros
    const int64_t j = tile - a.tile_off[r], tpw = autocorr_tiles_per_window(n, a.W), w = j / tpw;
    const int64_t ws = autocorr_win_start(w, a.W), we = autocorr_win_end(n, w, a.W);
    const int64_t ta = ws + (j - w * tpw) * AUTOCORR_TILE, tb = ta + AUTOCORR_TILE < we ? ta + AUTOCORR_TILE : we;
    if (ta + dl + a.k > n) return;   // no position of the tile has i <= n - d - k
    const int64_t tw0 = ta >> 6, rw = autocorr_words(n), base = a.pw[r];
    const int nwt = (int)(((tb - 1) >> 6) - tw0) + 1;   // <= AUTOCORR_TILE_WORDS + 1
    const int64_t pb = tw0 + (dl >> 6);                 // the first partner word
    if (threadIdx.x < 3 * AC_PW) {
        const int p = threadIdx.x / AC_PW, x = threadIdx.x - p * AC_PW;
        const uint64_t* src = p == 0 ? a.lo : p == 1 ? a.hi : a.v;
        part[p][x] = pb + x < rw ? src[base + pb + x] : 0;   // (behind the read: invalid)
    }
    __syncthreads();
    const int64_t d = dl + threadIdx.x;
    const int dr = (int)(d - ((dl >> 6) << 6)), s = dr & 31;
    const uint32_t* L = reinterpret_cast<const uint32_t*>(part[0]) + (dr >> 5);
    const uint32_t* H = reinterpret_cast<const uint32_t*>(part[1]) + (dr >> 5);
    const uint32_t* V = reinterpret_cast<const uint32_t*>(part[2]) + (dr >> 5);
    const uint64_t *gl = a.lo + base + tw0, *gh = a.hi + base + tw0, *gv = a.v + base + tw0;   // (the same in every lane)
    uint32_t l0 = L[0], h0 = H[0], v0 = V[0];
    auto eq = [&](int t) -> uint64_t {   // the equality word of tile word t; t ascending
        const uint32_t l1 = L[2 * t + 1], l2 = L[2 * t + 2], h1 = H[2 * t + 1], h2 = H[2 * t + 2], v1 = V[2 * t + 1], v2 = V[2 * t + 2];
        const uint64_t pl = __builtin_amdgcn_alignbit(l1, l0, s) | (uint64_t)__builtin_amdgcn_alignbit(l2, l1, s) << 32;
        const uint64_t ph = __builtin_amdgcn_alignbit(h1, h0, s) | (uint64_t)__builtin_amdgcn_alignbit(h2, h1, s) << 32;
        const uint64_t pv = __builtin_amdgcn_alignbit(v1, v0, s) | (uint64_t)__builtin_amdgcn_alignbit(v2, v1, s) << 32;
        l0 = l2; h0 = h2; v0 = v2;
        return autocorr_eq(gl[t], gh[t], gv[t], pl, ph, pv);
    };
    uint64_t cur = eq(0);
    uint32_t acc = 0;
    for (int t = 0; t < nwt; ++t) {   // (not unrolled: four words per scalar load and wait measured slower at k >= 8)
        const uint64_t next = eq(t + 1);   // (word t + 1 exists: the zero word behind the read at the latest)
        const uint64_t x = autocorr_runs<NS>(cur, next, a.sh) & autocorr_word_mask(tw0 + t, ta, tb);
        acc += (uint32_t)__popcll(x);
        cur = next;
    }
    if (d <= a.D && acc) atomicAdd(a.counts + ((a.win_off[r] + w) * a.D + (d - 1)), (unsigned long long)acc);
}

}  // namespace sd

namespace sdi {
namespace {

std::atomic<int64_t> g_ac_launches{0};   // launches of sd_autocorr_pairs in this process (sd_autocorr_info)

// Per device, kept between calls (sd_job_dev.hpp: DevWork): the planes and the per-read tables
// [roff | rlen | pw | win_off | tile_off].
struct AcCtx : DevWork, ReadTable {
    DevBuf<uint64_t> planes;
    DevBuf<uint8_t> text;       // sd_autocorr_dev: the reads, back to back
};

// win_off (n_reads + 1, may be null) and the windows of the reads; SD_ERR_UNSUPPORTED when the count leaves 62 bits
int ac_layout(const int64_t* read_lens, int32_t n_reads, int64_t W, int64_t* win_off, int64_t& windows) {
    unsigned __int128 c = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] < 0) return SD_ERR_PARAM;
        if (win_off) win_off[r] = (int64_t)c;
        c += (unsigned __int128)sd::autocorr_windows(read_lens[r], W);
        if (c >> 62) return SD_ERR_UNSUPPORTED;
    }
    if (win_off) win_off[n_reads] = (int64_t)c;
    windows = (int64_t)c;
    return SD_OK;
}

// k, D, W and the cap on cells, with the numbers in errbuf
int ac_limits(const char* who, const int64_t* read_lens, int32_t n_reads, int64_t k, int64_t D, int64_t W, int64_t* win_off, int64_t& windows,
              char* errbuf, size_t errlen) {
    if (!sd::autocorr_k_ok(k)) {
        set_err(errbuf, errlen, std::string(who) + ": k = " + std::to_string(k) + ", must be 1 .. " + std::to_string(sd::AUTOCORR_KMAX));
        return SD_ERR_PARAM;
    }
    if (!sd::autocorr_d_ok(D)) {
        set_err(errbuf, errlen, std::string(who) + ": D = " + std::to_string(D) + ", must be 1 .. " + std::to_string(sd::AUTOCORR_DMAX));
        return SD_ERR_PARAM;
    }
    if (!sd::autocorr_w_ok(W)) { set_err(errbuf, errlen, std::string(who) + ": W = " + std::to_string(W) + ", must be 0 (one window) or more"); return SD_ERR_PARAM; }
    if (n_reads < 0 || (n_reads > 0 && !read_lens)) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    const int rc = ac_layout(read_lens, n_reads, W, win_off, windows);
    if (rc) { set_err(errbuf, errlen, std::string(who) + (rc == SD_ERR_PARAM ? ": a negative read length" : ": 2^62 windows or more")); return rc; }
    if (windows > sd::AUTOCORR_CELLS_MAX / D) {
        set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(windows) + " windows x " + std::to_string(D) + " lags, the cap is " +
                                    std::to_string(sd::AUTOCORR_CELLS_MAX) + " cells (AUTOCORR_CELLS_MAX): use longer windows, fewer lags or fewer reads per call");
        return SD_ERR_PARAM;
    }
    return SD_OK;
}

// ---- the host form ------------------------------------------------------------------------------------------------------
struct AcPlanes : sd::AutocorrPlanes {
    static uint64_t at(const std::vector<uint64_t>& p, int64_t rw, int64_t idx) { return idx < rw ? p[(size_t)idx] : 0; }
    // the equality word of word t at lag d
    uint64_t eq(int64_t t, int64_t d) const {
        if (t >= rw) return 0;
        const int64_t q = t + (d >> 6);
        const int s = (int)(d & 63);
        auto sh = [&](const std::vector<uint64_t>& p) {
            const uint64_t a = at(p, rw, q);
            return s ? (a >> s) | (at(p, rw, q + 1) << (64 - s)) : a;
        };
        return sd::autocorr_eq(lo[(size_t)t], hi[(size_t)t], v[(size_t)t], sh(lo), sh(hi), sh(v));
    }
};

// the hits of one read at lag d, by window, added to out[w * D + d - 1]
void ac_host_lag(const AcPlanes& p, int64_t n, int k, int64_t d, int64_t D, int64_t W, int ns, const int* shifts, int64_t* out) {
    if (n - d - k < 0) return;
    const int64_t tl = (n - d - k) >> 6;   // the word of the last position that can be a hit
    uint64_t cur = p.eq(0, d);
    for (int64_t t = 0; t <= tl; ++t) {
        const uint64_t next = p.eq(t + 1, d);
        const uint64_t x = sd::autocorr_runs_n(ns, cur, next, shifts);
        cur = next;
        if (!x) continue;
        if (W <= 0) { out[d - 1] += __builtin_popcountll(x); continue; }
        const int64_t last = std::min(n - 1, 64 * t + 63);
        for (int64_t w = 64 * t / W; w <= last / W; ++w) {
            const uint64_t m = x & sd::autocorr_word_mask(t, sd::autocorr_win_start(w, W), sd::autocorr_win_end(n, w, W));
            if (m) out[w * D + d - 1] += __builtin_popcountll(m);
        }
    }
}

void ac_host(const uint8_t* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int k, int64_t D, int64_t W,
             const int64_t* win_off, int threads, int64_t* counts) {
    int shifts[5] = {0, 0, 0, 0, 0};
    const int ns = sd::autocorr_steps(k, shifts);
    std::vector<AcPlanes> planes((size_t)n_reads);
    sd::parallel_for(n_reads, threads, 1, [&](int64_t r) { planes[(size_t)r].build(text + read_off[r], read_lens[r]); });
    std::vector<int64_t> item_off((size_t)n_reads + 1, 0);   // items: (read, lag) with lag <= n - k
    for (int32_t r = 0; r < n_reads; ++r)
        item_off[(size_t)r + 1] = item_off[(size_t)r] + std::max<int64_t>(0, std::min<int64_t>(D, read_lens[r] - k));
    sd::parallel_for(item_off[(size_t)n_reads], threads, 8, [&](int64_t it) {
        const int32_t r = (int32_t)(std::upper_bound(item_off.begin(), item_off.end(), it) - item_off.begin()) - 1;
        ac_host_lag(planes[(size_t)r], read_lens[r], k, it - item_off[(size_t)r] + 1, D, W, ns, shifts, counts + win_off[r] * D);
    });
}

// ---- the device passes --------------------------------------------------------------------------------------------------
struct AcBench {
    int warmup, reps;
    float *ms_prep, *ms_pairs;
    int64_t* info;
};

// The job on `st`: tables up, counters zeroed, planes built, every (tile, lag block) launched.  d_text + roff[r] = read r.
// Nothing waits (bench: the timed repetitions do).  Throws HipFail.
void ac_enqueue(AcCtx& c, hipStream_t st, const uint8_t* d_text, const int64_t* roff, const int64_t* read_lens, int32_t n_reads, int k,
                int64_t D, int64_t W, const int64_t* win_off, int64_t windows, int64_t* d_counts, const AcBench* bench) {
    c.shape(5, n_reads);
    int64_t *h_off = c.h(0), *h_len = c.h(1), *h_pw = c.h(2), *h_win = c.h(3), *h_tile = c.h(4);
    int64_t words = 0, tiles = 0, maxn = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        h_off[r] = roff[r];
        h_len[r] = read_lens[r];
        h_pw[r] = words;
        h_win[r] = win_off[r];
        h_tile[r] = tiles;
        words += sd::autocorr_plane_words(read_lens[r]);
        tiles += sd::autocorr_tiles(read_lens[r], W);
        maxn = std::max(maxn, read_lens[r]);
    }
    h_off[n_reads] = 0; h_len[n_reads] = 0; h_pw[n_reads] = words; h_win[n_reads] = windows; h_tile[n_reads] = tiles;
    c.planes.alloc(3 * (size_t)words);
    c.upload(5, st);
    const size_t cells = (size_t)windows * (size_t)D;
    if (cells) SD_HIP(hipMemsetAsync(d_counts, 0, cells * sizeof(int64_t), st));
    if (n_reads == 0 || words == 0) return;
    uint64_t *lo = c.planes.p, *hi = lo + words, *v = hi + words;
    const int64_t *d_off = c.d(0), *d_len = c.d(1), *d_pw = c.d(2), *d_win = c.d(3), *d_tile = c.d(4);
    const unsigned prep_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((words + 3) / 4, (int64_t)c.n_cu * 32));
    auto prep = [&]() {
        hipLaunchKernelGGL(sd::sd_autocorr_prep, dim3(prep_grid), dim3(sd::AC_T), 0, st, d_text, d_off, d_len, d_pw, (int)n_reads, words, lo, hi, v);
        SD_HIP(hipGetLastError());
    };
    sd::AcArgs a{lo, hi, v, d_len, d_pw, d_win, d_tile, (int)n_reads, k, {0, 0, 0, 0, 0}, W, D, 0, tiles, 0,
                 reinterpret_cast<unsigned long long*>(d_counts)};
    const int ns = sd::autocorr_steps(k, a.sh);
    // lags above the longest read's n - k count nothing anywhere: their blocks are not launched
    const int64_t d_eff = std::min<int64_t>(D, maxn - k);
    const int64_t nlb = d_eff > 0 ? (d_eff + sd::AUTOCORR_LAGS - 1) / sd::AUTOCORR_LAGS : 0;
    const int64_t ly = std::min<int64_t>(nlb, sd::AUTOCORR_LAUNCH_WG), tx = ly > 0 ? std::max<int64_t>(1, sd::AUTOCORR_LAUNCH_WG / ly) : 0;
    int64_t launches = 0, wgs = 0;
    auto pairs = [&]() {
        launches = 0;
        wgs = 0;
        for (int64_t lb0 = 0; lb0 < nlb; lb0 += ly)
            for (int64_t t0 = 0; t0 < tiles; t0 += tx) {
                a.lb0 = lb0;
                a.tile0 = t0;
                const dim3 grid((unsigned)std::min<int64_t>(ly, nlb - lb0), (unsigned)std::min<int64_t>(tx, tiles - t0));   // <= AUTOCORR_LAUNCH_WG
#define SD_AC(NS) hipLaunchKernelGGL(sd::sd_autocorr_pairs<NS>, grid, dim3(sd::AC_T), 0, st, a)
                switch (ns) {
                    case 0: SD_AC(0); break;
                    case 1: SD_AC(1); break;
                    case 2: SD_AC(2); break;
                    case 3: SD_AC(3); break;
                    case 4: SD_AC(4); break;
                    default: SD_AC(5); break;
                }
#undef SD_AC
                SD_HIP(hipGetLastError());
                launches += 1;
                wgs += (int64_t)grid.x * grid.y;
            }
        g_ac_launches.fetch_add(launches);
    };
    if (!bench) {
        prep();
        pairs();
        return;
    }
    StageClock clock;   // the planes, then the pairs on them
    clock.time(st, bench->warmup, bench->reps, bench->ms_prep, prep);
    clock.time(st, bench->warmup, bench->reps, bench->ms_pairs, pairs, [&]() {
        if (cells) SD_HIP(hipMemsetAsync(d_counts, 0, cells * sizeof(int64_t), st));
    });
    bench->info[0] = launches;
    bench->info[1] = wgs;
    bench->info[2] = (int64_t)cells;
    bench->info[3] = words;
}

int ac_dev(const char* who, const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D,
           int64_t W, int32_t device, int64_t* counts, char* errbuf, size_t errlen, const AcBench* bench) {
    std::vector<int64_t> win_off((size_t)std::max(n_reads, 0) + 1, 0);
    int64_t windows = 0;
    int rc = ac_limits(who, read_lens, n_reads, k, D, W, win_off.data(), windows, errbuf, errlen);
    if (rc) return rc;
    const int64_t cells = windows * D;
    if ((rc = reads_text_args(who, text, read_off, read_lens, n_reads, cells > 0 && !counts, errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    try {
        DeviceScope on(device);
        AcCtx& c = device_ctx<AcCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        OwnedStream st;
        DevBuf<int64_t> d_counts;
        d_counts.alloc((size_t)cells);
        const std::vector<int64_t> off = reads_upload(c.text, st, text, read_off, read_lens, n_reads);
        ac_enqueue(c, st, c.text.p, off.data(), read_lens, n_reads, k, D, W, win_off.data(), windows, d_counts.p, bench);
        c.in_flight(st);
        if (cells) SD_HIP(hipMemcpyAsync(counts, d_counts.p, sizeof(int64_t) * (size_t)cells, hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));
        c.waited();
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
}

}  // namespace
}  // namespace sdi

extern "C" {

int sd_autocorr_layout(const int64_t* read_lens, int32_t n_reads, int64_t W, int64_t* win_off, int64_t* windows_total) try {
    if (n_reads < 0 || (n_reads > 0 && !read_lens) || !windows_total || !sd::autocorr_w_ok(W)) return SD_ERR_PARAM;
    return ac_layout(read_lens, n_reads, W, win_off, *windows_total);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_autocorr_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D, int64_t W,
                     int32_t threads, int64_t* counts, char* errbuf, size_t errlen) try {
    static const char* who = "sd_autocorr_host";
    std::vector<int64_t> win_off((size_t)std::max(n_reads, 0) + 1, 0);
    int64_t windows = 0;
    int rc = ac_limits(who, read_lens, n_reads, k, D, W, win_off.data(), windows, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, text, read_off, read_lens, n_reads, windows * D > 0 && !counts, errbuf, errlen))) return rc;
    std::memset(counts, 0, sizeof(int64_t) * (size_t)(windows * D));
    ac_host(reinterpret_cast<const uint8_t*>(text), read_off, read_lens, n_reads, k, D, W, win_off.data(), std::max(1, threads), counts);
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_autocorr_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D, int64_t W,
                    int32_t device, int32_t threads, int64_t* counts, char* errbuf, size_t errlen) try {
    (void)threads;   // (every cell is the kernel's: the host has nothing to add)
    return ac_dev("sd_autocorr_dev", text, read_off, read_lens, n_reads, k, D, W, device, counts, errbuf, errlen, nullptr);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_autocorr_reads_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D,
                          int64_t W, int32_t device, void* hip_stream, int64_t* d_counts, char* errbuf, size_t errlen) try {
    static const char* who = "sd_autocorr_reads_dev";
    std::vector<int64_t> win_off((size_t)std::max(n_reads, 0) + 1, 0);
    int64_t windows = 0, bases = 0;
    int rc = ac_limits(who, read_lens, n_reads, k, D, W, win_off.data(), windows, errbuf, errlen);
    if (rc) return rc;
    const int64_t cells = windows * D;
    if ((rc = reads_text_args(who, d_text, read_off, read_lens, n_reads, cells > 0 && !d_counts, errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    for (int32_t r = 0; r < n_reads; ++r) bases += read_lens[r];
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        if (cells > 0 && (rc = buffer_on_device(d_counts, device, who, "count", errbuf, errlen))) return rc;
        if (bases > 0 && (rc = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return rc;
        AcCtx& c = device_ctx<AcCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();   // the previous call's kernels read the buffers this one overwrites
        ac_enqueue(c, st, static_cast<const uint8_t*>(d_text), read_off, read_lens, n_reads, k, D, W, win_off.data(), windows, d_counts, nullptr);
        c.in_flight(st);
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_autocorr_positions(const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D, int64_t W, int64_t* positions) try {
    std::vector<int64_t> win_off((size_t)std::max(n_reads, 0) + 1, 0);
    int64_t windows = 0;
    const int rc = ac_limits("sd_autocorr_positions", read_lens, n_reads, k, D, W, win_off.data(), windows, nullptr, 0);
    if (rc) return rc;
    if (windows > 0 && !positions) return SD_ERR_PARAM;
    for (int32_t r = 0; r < n_reads; ++r) {
        const int64_t n = read_lens[r], nw = sd::autocorr_windows(n, W);
        for (int64_t w = 0; w < nw; ++w) {
            int64_t* o = positions + (win_off[(size_t)r] + w) * D;
            const int64_t ws = sd::autocorr_win_start(w, W), we = sd::autocorr_win_end(n, w, W);
            for (int64_t d = 1; d <= D; ++d) o[d - 1] = sd::autocorr_positions(n, k, d, ws, we);
        }
    }
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_autocorr_peaks(const int64_t* counts, int64_t n_windows, int64_t D, int64_t LO, int64_t R, int64_t P, int64_t* lag, int64_t* count) try {
    if (n_windows < 0 || !sd::autocorr_d_ok(D) || LO < 1 || R < 0 || P < 0 || (n_windows > 0 && !counts) || (n_windows > 0 && P > 0 && (!lag || !count)))
        return SD_ERR_PARAM;
    std::vector<int64_t> found;
    for (int64_t w = 0; w < n_windows; ++w) {
        const int64_t* a = counts + w * D;
        found.clear();
        for (int64_t d = LO; d <= D; ++d)
            if (sd::autocorr_is_peak(a, D, LO, R, d)) found.push_back(d);
        std::sort(found.begin(), found.end(), [&](int64_t x, int64_t y) { return sd::autocorr_peak_before(a[x - 1], x, a[y - 1], y); });
        for (int64_t i = 0; i < P; ++i) {
            const bool have = i < (int64_t)found.size();
            lag[w * P + i] = have ? found[(size_t)i] : 0;
            count[w * P + i] = have ? a[found[(size_t)i] - 1] : 0;
        }
    }
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_autocorr_seed(const char* text, int64_t n, int32_t k, int64_t p, int64_t* start, int64_t* run) try {
    if (!start || !run || n < 0 || (n > 0 && !text) || !sd::autocorr_k_ok(k) || p < 1) return SD_ERR_PARAM;
    *start = -1;
    *run = 0;
    // match[i]: T[i] matches T[i + p]; i is a hit when k matches follow from i on.  From the right, so that a run of
    // hits is complete at its first position; >= lets the earlier of two equal runs win.
    int64_t matches = 0, hits = 0;
    for (int64_t i = n - p - 1; i >= 0; --i) {
        const uint8_t c = (uint8_t)text[i];
        matches = (sd::autocorr_code(c) >= 0 && c == (uint8_t)text[i + p]) ? matches + 1 : 0;
        hits = matches >= k ? hits + 1 : 0;
        if (hits > 0 && hits >= *run) { *run = hits; *start = i; }
    }
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_autocorr_info(int64_t info[4]) {
    info[0] = sd::AUTOCORR_TILE;
    info[1] = sd::AUTOCORR_LAGS;
    info[2] = sd::AUTOCORR_LAUNCH_WORK;
    info[3] = g_ac_launches.load();
}

int sd_autocorr_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t D,
                             int64_t W, int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_pairs, int64_t info[4]) try {
    if (warmup < 0 || reps < 1 || !ms_prep || !ms_pairs || !info || n_reads <= 0) return SD_ERR_PARAM;
    int64_t windows = 0;
    const int rc = ac_limits("sd_autocorr_kernel_bench", read_lens, n_reads, k, D, W, nullptr, windows, nullptr, 0);
    if (rc) return rc;
    std::vector<int64_t> counts((size_t)std::max<int64_t>(windows * D, 1));
    for (int i = 0; i < 4; ++i) info[i] = 0;
    const AcBench b{warmup, reps, ms_prep, ms_pairs, info};
    return ac_dev("sd_autocorr_kernel_bench", text, read_off, read_lens, n_reads, k, D, W, device, counts.data(), nullptr, 0, &b);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
