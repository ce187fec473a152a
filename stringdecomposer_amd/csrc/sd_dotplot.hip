// sd_dotplot.hip -- windowed k-mer identity of every read against itself (--dotplot): the read cut into windows of W bases,
// every window scored against every earlier window by the selected k-mers they share, both strands on request, without a
// monomer file.  sd_dotplot.hpp holds the definition and everything host and device compute alike; this file holds the
// kernels, the host form and the C-ABI (include/sd_hip.h: sd_dotplot_*).  No kernel uses an atomic: every tile count, every
// element of a set and every cell has exactly one writer.
//   sd_dotplot_tiles<false>  the count pass: a workgroup (256 lanes) per tile -- up to DOTPLOT_TILE positions of ONE window.
//                            The tile's bases and the k - 1 behind it go to LDS as codes (dotplot_base); a lane takes four
//                            positions, builds both codes from k LDS bytes (dotplot_kmer) and tests h(code) % M; ballots
//                            and population counts give the tile's selected positions per strand.
//   exclusive_scan_dev       (sd_scan_dev.hpp) the exclusive scan of the tile counts (the forward tiles of the call, then
//                            the reverse ones) = where every tile's codes go
//   sd_dotplot_windows       one workgroup: per (window, strand) the offset and the count of its set, and the summary the
//                            host reads: total, largest count, the first set over DOTPLOT_SET_MAX.
//   sd_dotplot_tiles<true>   the gather: the same arithmetic, the selected codes written at the tile's offset in position
//                            order (ballot prefix), so the codes of a window and strand lie together.
//   sd_dotplot_sets          a workgroup per (window, strand): its codes to LDS, a sorting network whose comparators all
//                            put the smaller key at the lower index (the first step of every merge compares mirrored
//                            elements), so "padding" is the count: a comparator whose upper index is behind the last
//                            element does nothing, and no key value is reserved (k = 32 uses them all).  Duplicates are
//                            dropped by a ballot prefix; the distinct list goes back to the front of the set's stretch and
//                            its length to kmers / kmers_rc.
//   sd_dotplot_pairs<RC>     the hot path: a workgroup per (window i, stretch of DOTPLOT_JSEG cells of its row).  S_i sorted
//                            in LDS; a wave takes every fourth j of the stretch, a lane DP_ILP keys of S_j (then of R_j)
//                            per step from global memory, 64 apart, each a branch-free binary search in LDS
//                            (ds_read_b64): independent chains, since one chain alone waits for the LDS's latency.  Hits
//                            are counted by ballot and population count, one store per cell by lane 0.
// Launches: a launch of the pair kernel takes whole rows while rows' cells x the call's largest set x strands stay within
// DOTPLOT_LAUNCH_WORK (at least one row), so a 5-Mb array at W = 2 000 is 24 launches of at most 0.6 ms each.
#include <algorithm>
#include <atomic>
#include <cstring>

#include "sd_dotplot.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"
#include "sd_scan_dev.hpp"

namespace sd {

constexpr int DP_T = 256;        // threads of a workgroup of the tile, set and pair kernels
constexpr int DP_WIN_T = 1024;   // ... of the window kernel
#ifndef SD_DOTPLOT_ILP
#define SD_DOTPLOT_ILP 8
#endif
constexpr int DP_ILP = SD_DOTPLOT_ILP;   // elements of S_j a lane looks up per step of the pair kernel: 1, 2, 4 or 8
static_assert(DP_ILP == 1 || DP_ILP == 2 || DP_ILP == 4 || DP_ILP == 8, "the rest of a set is taken in halving steps");
static_assert(DOTPLOT_TILE == 4 * DP_T, "four positions per lane");
static_assert((DOTPLOT_SET_MAX & (DOTPLOT_SET_MAX - 1)) == 0 && DOTPLOT_SET_MAX * sizeof(uint64_t) <= 32768, "a set is 32 KB of LDS");

struct DpArgs {
    const uint8_t* text;
    const int64_t *roff, *rlen, *win_off, *tile_off, *cell_off;   // per read; the three offsets: n_reads + 1
    int n_reads, k, rc;
    uint32_t M;
    int64_t W, B, windows, tiles;
    int32_t* tcnt;       // [strand][tile]: selected positions
    int64_t* toff;       // [strand][tile] + 1: the exclusive scan
    int64_t* woff;       // [strand][window]: where the set starts
    int32_t* wraw;       // [strand][window]: its selected positions
    int64_t* summary;    // total, largest wraw, 2 w + strand of the first wraw over the cap (-1: none), that wraw
    uint64_t* sets;
    int32_t *kmers, *kmers_rc, *shared, *shared_rc;
};

template <bool GATHER>
__global__ __launch_bounds__(DP_T) void sd_dotplot_tiles(DpArgs a, int64_t tile0) {
    __shared__ uint8_t code[DOTPLOT_TILE + DOTPLOT_KMAX];
    __shared__ int wt[2][4][DP_T / 64];
    const int64_t t = tile0 + blockIdx.x;
    if (t >= a.tiles) return;
    const int r = dotplot_find(a.tile_off, a.n_reads, t);
    const int64_t n = a.rlen[r], tl = t - a.tile_off[r], tpw = dotplot_tiles_per_window(a.W), wl = tl / tpw;
    const int64_t ws = wl * a.W, we = ws + a.W < n ? ws + a.W : n;
    const int64_t ta = ws + (tl - wl * tpw) * DOTPLOT_TILE, tb = ta + DOTPLOT_TILE < we ? ta + DOTPLOT_TILE : we;
    const uint8_t* text = a.text + a.roff[r];
    for (int x = threadIdx.x; x < DOTPLOT_TILE + a.k - 1; x += DP_T) code[x] = ta + x < n ? dotplot_base(text[ta + x]) : 4;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    uint64_t f[4], rv[4];
    bool sf[4], sr[4];
    int pf[4], pr[4];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
        const int x = sub * DP_T + threadIdx.x;
        sf[sub] = sr[sub] = false;
        f[sub] = rv[sub] = 0;
        if (ta + x < tb && dotplot_kmer(code + x, a.k, f[sub], rv[sub])) {
            sf[sub] = dotplot_selected(f[sub], a.M);
            sr[sub] = a.rc && dotplot_selected(rv[sub], a.M);
        }
        const uint64_t bf = __ballot(sf[sub]), br = __ballot(sr[sub]);
        pf[sub] = __popcll(bf & below);
        pr[sub] = __popcll(br & below);
        if (lane == 0) {
            wt[0][sub][wave] = __popcll(bf);
            wt[1][sub][wave] = __popcll(br);
        }
    }
    __syncthreads();
    const int* flat0 = &wt[0][0][0];
    const int* flat1 = &wt[1][0][0];
    if (!GATHER) {
        if (threadIdx.x < (a.rc ? 2 : 1)) {
            const int* w = threadIdx.x ? flat1 : flat0;
            int s = 0;
            for (int i = 0; i < 4 * (DP_T / 64); ++i) s += w[i];
            a.tcnt[threadIdx.x * a.tiles + t] = s;
        }
        return;
    }
    const int64_t of = a.toff[t], orc = a.rc ? a.toff[a.tiles + t] : 0;
    int bf = 0, br = 0;   // selected positions of the tile in the subs before
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
        int wf = 0, wr = 0, tf = 0, tr = 0;   // ... in the waves before this one, and in all waves, of this sub
        for (int i = 0; i < DP_T / 64; ++i) {
            if (i < wave) { wf += wt[0][sub][i]; wr += wt[1][sub][i]; }
            tf += wt[0][sub][i];
            tr += wt[1][sub][i];
        }
        if (sf[sub]) a.sets[of + bf + wf + pf[sub]] = f[sub];
        if (sr[sub]) a.sets[orc + br + wr + pr[sub]] = rv[sub];
        bf += tf;
        br += tr;
    }
}

__global__ __launch_bounds__(DP_WIN_T) void sd_dotplot_windows(DpArgs a) {
    __shared__ int64_t red[3][DP_WIN_T];
    const int tid = threadIdx.x, strands = a.rc ? 2 : 1;
    const int64_t tpw = dotplot_tiles_per_window(a.W);
    int64_t best = 0, bad = -1, badn = 0;
    for (int64_t x = tid; x < strands * a.windows; x += DP_WIN_T) {
        const int64_t st = x / a.windows, w = x - st * a.windows;
        const int r = dotplot_find(a.win_off, a.n_reads, w);
        const int64_t wl = w - a.win_off[r], last = a.win_off[r + 1] - a.win_off[r] - 1;
        const int64_t t0 = a.tile_off[r] + wl * tpw, t1 = wl < last ? t0 + tpw : a.tile_off[r + 1];
        const int64_t b = a.toff[st * a.tiles + t0], e = a.toff[st * a.tiles + t1];
        a.woff[x] = b;
        a.wraw[x] = (int32_t)(e - b);   // (a window is at most 2^30 positions)
        if (e - b > best) best = e - b;
        if (e - b > DOTPLOT_SET_MAX && (bad < 0 || 2 * w + st < bad)) { bad = 2 * w + st; badn = e - b; }
    }
    red[0][tid] = best;
    red[1][tid] = bad;
    red[2][tid] = badn;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < DP_WIN_T; ++i) {
            if (red[0][i] > best) best = red[0][i];
            if (red[1][i] >= 0 && (bad < 0 || red[1][i] < bad)) { bad = red[1][i]; badn = red[2][i]; }
        }
        a.summary[0] = a.toff[strands * a.tiles];
        a.summary[1] = best;
        a.summary[2] = bad;
        a.summary[3] = badn;
    }
}

__global__ __launch_bounds__(DP_T) void sd_dotplot_sets(DpArgs a, int64_t set0) {
    __shared__ uint64_t key[DOTPLOT_SET_MAX];
    __shared__ int wt[DP_T / 64];
    const int64_t x = set0 + blockIdx.x;   // [strand][window]
    if (x >= (a.rc ? 2 : 1) * a.windows) return;
    const int n = a.wraw[x];
    int32_t* out = x < a.windows ? a.kmers + x : a.kmers_rc + (x - a.windows);
    if (n <= 0 || n > DOTPLOT_SET_MAX) {   // (over the cap: refused before this launch)
        if (threadIdx.x == 0) *out = 0;
        return;
    }
    uint64_t* g = a.sets + a.woff[x];
    for (int i = threadIdx.x; i < n; i += DP_T) key[i] = g[i];
    int P = 1;
    while (P < n) P <<= 1;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        const int half = size >> 1;
        for (int t = threadIdx.x; t < P / 2; t += DP_T) {   // the mirrored step
            const int blk = t / half, o = t - blk * half, l = blk * size + o, h = blk * size + size - 1 - o;
            if (h < n) {
                const uint64_t u = key[l], v = key[h];
                if (u > v) { key[l] = v; key[h] = u; }
            }
        }
        __syncthreads();
        for (int stride = half >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < P / 2; t += DP_T) {
                const int l = 2 * stride * (t / stride) + (t % stride), h = l + stride;
                if (h < n) {
                    const uint64_t u = key[l], v = key[h];
                    if (u > v) { key[l] = v; key[h] = u; }
                }
            }
            __syncthreads();
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += DP_T) {   // (uniform trip count)
        const int i = i0 + threadIdx.x;
        const bool first = i < n && (i == 0 || key[i] != key[i - 1]);
        const uint64_t b = __ballot(first);
        if (lane == 0) wt[wave] = __popcll(b);
        __syncthreads();
        int at = base + __popcll(b & (((uint64_t)1 << lane) - 1)), all = 0;
        for (int w = 0; w < DP_T / 64; ++w) {
            if (w < wave) at += wt[w];
            all += wt[w];
        }
        if (first) g[at] = key[i];
        base += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = base;
}

// hits of the keys sj[e0 + 64 c + lane], c < C, in the ni > 0 sorted keys of LDS; the same in every lane of the wave.  The C
// searches of a lane are independent chains of LDS reads, so one wait covers C of them: the kernel waits for the LDS's
// latency, not for its bandwidth (profiles/dotplot_timing.md).
template <int C>
__device__ inline int dp_step(const uint64_t* S, int ni, const uint64_t* __restrict__ sj, int nj, int e0, int lane) {
    uint64_t q[C];
    bool live[C];
    unsigned lo[C];   // in bytes: a probe is one add, the read, the compare and a select
    const char* Sb = reinterpret_cast<const char*>(S);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int e = e0 + 64 * c + lane;
        live[c] = e < nj;
        q[c] = live[c] ? sj[e] : 0;
        lo[c] = 0;
    }
    for (int len = ni; len > 1;) {   // (ni is the wave's: no divergence)
        const int half = len >> 1;
        const unsigned step = (unsigned)half * sizeof(uint64_t);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const unsigned at = lo[c] + step;
            if (*reinterpret_cast<const uint64_t*>(Sb + at) <= q[c]) lo[c] = at;
        }
        len -= half;
    }
    int acc = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) acc += __popcll(__ballot(live[c] && *reinterpret_cast<const uint64_t*>(Sb + lo[c]) == q[c]));
    return acc;
}

// hits of the nj sorted keys at sj in the ni sorted keys of LDS: steps of DP_ILP x 64 keys, the rest in halving steps
__device__ inline int dp_hits(const uint64_t* S, int ni, const uint64_t* __restrict__ sj, int nj, int lane) {
    int acc = 0, e0 = 0;
    if (ni <= 0) return 0;
    for (; e0 + 64 * (DP_ILP - 1) < nj; e0 += 64 * DP_ILP) acc += dp_step<DP_ILP>(S, ni, sj, nj, e0, lane);
    if (DP_ILP > 4 && e0 + 64 * 3 < nj) { acc += dp_step<4>(S, ni, sj, nj, e0, lane); e0 += 64 * 4; }
    if (DP_ILP > 2 && e0 + 64 < nj) { acc += dp_step<2>(S, ni, sj, nj, e0, lane); e0 += 64 * 2; }
    if (DP_ILP > 1 && e0 < nj) acc += dp_step<1>(S, ni, sj, nj, e0, lane);
    return acc;
}

template <bool RC>
__global__ __launch_bounds__(DP_T) void sd_dotplot_pairs(DpArgs a, int64_t row0, int64_t rows) {
    __shared__ uint64_t S[DOTPLOT_SET_MAX];
    const int64_t i = row0 + blockIdx.x;
    if (blockIdx.x >= rows || i >= a.windows) return;
    const int r = dotplot_find(a.win_off, a.n_reads, i);
    const int64_t w0 = a.win_off[r], il = i - w0, rcells = dotplot_row_cells(il, a.B), jlo = il - rcells + 1;
    const int64_t seg = blockIdx.y;
    if (seg * DOTPLOT_JSEG >= rcells) return;
    int ni = a.kmers[i];
    if (ni > DOTPLOT_SET_MAX) ni = DOTPLOT_SET_MAX;   // (cannot be: the sets kernel wrote it)
    const uint64_t* si = a.sets + a.woff[i];
    for (int x = threadIdx.x; x < ni; x += DP_T) S[x] = si[x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t jhi = il - seg * DOTPLOT_JSEG, jend = jhi - DOTPLOT_JSEG + 1 > jlo ? jhi - DOTPLOT_JSEG + 1 : jlo;
    const int64_t row = a.cell_off[r] + dotplot_row_off(il, a.B);
    for (int64_t jl = jhi - wave; jl >= jend; jl -= DP_T / 64) {
        const int64_t j = w0 + jl;
        const int hits = dp_hits(S, ni, a.sets + a.woff[j], a.kmers[j], lane);
        if (lane == 0) a.shared[row + (jl - jlo)] = hits;
        if (RC) {
            const int hr = dp_hits(S, ni, a.sets + a.woff[a.windows + j], a.kmers_rc[j], lane);
            if (lane == 0) a.shared_rc[row + (jl - jlo)] = hr;
        }
    }
}

}  // namespace sd

namespace sdi {
namespace {

std::atomic<int64_t> g_dp_launches{0};   // launches of sd_dotplot_pairs in this process (sd_dotplot_info)

// Per device, kept between calls (sd_job_dev.hpp: DevWork); the per-read tables are
// [roff | rlen | win_off | tile_off | cell_off].
struct DpCtx : DevWork, ReadTable {
    DevBuf<int32_t> tcnt, wraw;
    DevBuf<int64_t> toff, woff, summary, tsum, tbase;   // tsum, tbase: the tiles of the scan of tcnt
    DevBuf<uint64_t> sets;
    DevBuf<uint8_t> text;       // sd_dotplot_dev: the reads, back to back
    DevBuf<int32_t> out;        // sd_dotplot_dev: kmers | kmers_rc | shared | shared_rc
    PinBuf<int64_t> h_summary;
    hipEvent_t ev_sum = nullptr;
};

// win_off, cell_off (n_reads + 1 each, may be null) and the totals; SD_ERR_UNSUPPORTED when a count leaves 62 bits
int dp_layout(const int64_t* read_lens, int32_t n_reads, int64_t W, int64_t B, int64_t* win_off, int64_t* cell_off, int64_t& windows,
              int64_t& cells) {
    unsigned __int128 nwin = 0, ncell = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] < 0) return SD_ERR_PARAM;
        if (win_off) win_off[r] = (int64_t)nwin;
        if (cell_off) cell_off[r] = (int64_t)ncell;
        const unsigned __int128 nw = (unsigned __int128)sd::dotplot_windows(read_lens[r], W), b = (unsigned __int128)B;
        nwin += nw;
        ncell += B <= 0 || nw <= b + 1 ? nw * (nw + 1) / 2 : (b + 1) * (b + 2) / 2 + (nw - b - 1) * (b + 1);
        if ((nwin >> 62) || (ncell >> 62)) return SD_ERR_UNSUPPORTED;
    }
    if (win_off) win_off[n_reads] = (int64_t)nwin;
    if (cell_off) cell_off[n_reads] = (int64_t)ncell;
    windows = (int64_t)nwin;
    cells = (int64_t)ncell;
    return SD_OK;
}

// k, W, M, B and the cap on cells, with the numbers in errbuf
int dp_limits(const char* who, const int64_t* read_lens, int32_t n_reads, int64_t k, int64_t W, int64_t B, int64_t M, int64_t* win_off,
              int64_t* cell_off, int64_t& windows, int64_t& cells, char* errbuf, size_t errlen) {
    const std::string me(who);
    if (!sd::dotplot_k_ok(k)) { set_err(errbuf, errlen, me + ": k = " + std::to_string(k) + ", must be 1 .. " + std::to_string(sd::DOTPLOT_KMAX)); return SD_ERR_PARAM; }
    if (!sd::dotplot_w_ok(W)) { set_err(errbuf, errlen, me + ": W = " + std::to_string(W) + ", must be 1 .. " + std::to_string(sd::DOTPLOT_WMAX)); return SD_ERR_PARAM; }
    if (!sd::dotplot_m_ok(M)) { set_err(errbuf, errlen, me + ": M = " + std::to_string(M) + ", must be 1 .. " + std::to_string(sd::DOTPLOT_MMAX)); return SD_ERR_PARAM; }
    if (!sd::dotplot_b_ok(B)) { set_err(errbuf, errlen, me + ": B = " + std::to_string(B) + ", must be 0 (all) .. " + std::to_string(sd::DOTPLOT_BMAX)); return SD_ERR_PARAM; }
    if (n_reads < 0 || (n_reads > 0 && !read_lens)) { set_err(errbuf, errlen, me + ": missing argument"); return SD_ERR_PARAM; }
    const int rc = dp_layout(read_lens, n_reads, W, B, win_off, cell_off, windows, cells);
    if (rc) { set_err(errbuf, errlen, me + (rc == SD_ERR_PARAM ? ": a negative read length" : ": 2^62 windows or cells, or more")); return rc; }
    if (cells > sd::DOTPLOT_CELLS_MAX) {
        set_err(errbuf, errlen, me + ": " + std::to_string(windows) + " windows make " + std::to_string(cells) + " cells, the cap is " +
                                    std::to_string(sd::DOTPLOT_CELLS_MAX) + " (SD_DOTPLOT_CELLS_MAX): use longer windows, a band or fewer reads per call");
        return SD_ERR_PARAM;
    }
    return SD_OK;
}

// the refusal of a window over the cap: key = 2 x (window of the call) + strand
int dp_refuse_set(const char* who, const int64_t* win_off, int32_t n_reads, int64_t key, int64_t count, char* errbuf, size_t errlen) {
    const int64_t w = key >> 1;
    const int r = sd::dotplot_find(win_off, n_reads, w);
    set_err(errbuf, errlen, std::string(who) + ": read " + std::to_string(r) + " window " + std::to_string(w - win_off[r]) + " has " +
                                std::to_string(count) + " selected " + ((key & 1) ? "reverse" : "forward") + " k-mers, the cap is " +
                                std::to_string(sd::DOTPLOT_SET_MAX) + " (SD_DOTPLOT_SET_MAX): use a larger M");
    return SD_ERR_PARAM;
}

// the text of the reads and, where there are windows or cells, a place for every result
int dp_text_args(const char* who, const void* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int rc, int64_t windows,
                 int64_t cells, const void* kmers, const void* kmers_rc, const void* shared, const void* shared_rc, char* errbuf, size_t errlen) {
    const bool no_output = (windows > 0 && (!kmers || (rc && !kmers_rc))) || (cells > 0 && (!shared || (rc && !shared_rc)));
    return reads_text_args(who, text, read_off, read_lens, n_reads, no_output, errbuf, errlen);
}

// ---- the host form ------------------------------------------------------------------------------------------------------
int dp_host(const char* who, const uint8_t* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int k, int64_t W, int64_t B,
            uint32_t M, int rc, const int64_t* win_off, const int64_t* cell_off, int64_t windows, int threads, int32_t* kmers, int32_t* kmers_rc,
            int32_t* shared, int32_t* shared_rc, char* errbuf, size_t errlen) {
    std::vector<std::vector<uint8_t>> codes((size_t)n_reads);
    sd::parallel_for(n_reads, threads, 1, [&](int64_t r) {
        const int64_t n = read_lens[r];
        auto& c = codes[(size_t)r];
        c.assign((size_t)n + sd::DOTPLOT_KMAX, 4);
        for (int64_t i = 0; i < n; ++i) c[(size_t)i] = sd::dotplot_base(text[read_off[r] + i]);
    });
    std::vector<std::vector<uint64_t>> sets(2 * (size_t)windows);   // [2 w + strand]
    std::vector<int64_t> raw(2 * (size_t)windows, 0);
    auto each = [&](int64_t w, bool keep) {
        const int r = sd::dotplot_find(win_off, n_reads, w);
        const int64_t n = read_lens[r], ws = (w - win_off[r]) * W, we = std::min(n, ws + W);
        const uint8_t* c = codes[(size_t)r].data();
        auto &F = sets[2 * (size_t)w], &R = sets[2 * (size_t)w + 1];
        int64_t nf = 0, nr = 0;
        for (int64_t i = ws; i < we; ++i) {
            uint64_t f, rv;
            if (!sd::dotplot_kmer(c + i, k, f, rv)) continue;
            if (sd::dotplot_selected(f, M)) { ++nf; if (keep) F.push_back(f); }
            if (rc && sd::dotplot_selected(rv, M)) { ++nr; if (keep) R.push_back(rv); }
        }
        raw[2 * (size_t)w] = nf;
        raw[2 * (size_t)w + 1] = nr;
        if (!keep) return;
        for (auto* s : {&F, &R}) {
            std::sort(s->begin(), s->end());
            s->erase(std::unique(s->begin(), s->end()), s->end());
        }
        kmers[w] = (int32_t)F.size();
        if (rc) kmers_rc[w] = (int32_t)R.size();
    };
    sd::parallel_for(windows, threads, 4, [&](int64_t w) { each(w, false); });   // the counting pass: nothing is kept
    for (int64_t x = 0; x < 2 * windows; ++x)
        if (raw[(size_t)x] > sd::DOTPLOT_SET_MAX) return dp_refuse_set(who, win_off, n_reads, x, raw[(size_t)x], errbuf, errlen);
    sd::parallel_for(windows, threads, 4, [&](int64_t w) { each(w, true); });
    auto common = [](const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
        size_t i = 0, j = 0;
        int32_t c = 0;
        while (i < a.size() && j < b.size()) {
            if (a[i] < b[j]) ++i;
            else if (b[j] < a[i]) ++j;
            else { ++c; ++i; ++j; }
        }
        return c;
    };
    sd::parallel_for(windows, threads, 1, [&](int64_t i) {
        const int r = sd::dotplot_find(win_off, n_reads, i);
        const int64_t w0 = win_off[r], il = i - w0, rcells = sd::dotplot_row_cells(il, B), jlo = il - rcells + 1;
        const int64_t row = cell_off[r] + sd::dotplot_row_off(il, B);
        for (int64_t jl = jlo; jl <= il; ++jl) {
            shared[row + jl - jlo] = common(sets[2 * (size_t)i], sets[2 * (size_t)(w0 + jl)]);
            if (rc) shared_rc[row + jl - jlo] = common(sets[2 * (size_t)i], sets[2 * (size_t)(w0 + jl) + 1]);
        }
    });
    return SD_OK;
}

// ---- the device passes --------------------------------------------------------------------------------------------------
struct DpBench {
    int warmup, reps;
    float *ms_count, *ms_sets, *ms_pairs;
    int64_t* info;
};

struct DpJob {
    sd::DpArgs a;
    std::vector<int64_t> win_off, cell_off;
    int64_t *tsum = nullptr, *tbase = nullptr;   // the tiles of the scan of tcnt
    int64_t cells = 0, selected = 0, largest = 0, launches = 0, workgroups = 0;
};

// tables up; `a` filled but for the sets and the results
void dp_tables(DpCtx& c, hipStream_t st, DpJob& j, const uint8_t* d_text, const int64_t* roff, const int64_t* read_lens, int32_t n_reads, int k,
               int64_t W, int64_t B, uint32_t M, int rc, int64_t windows) {
    c.shape(5, n_reads);
    int64_t *h_off = c.h(0), *h_len = c.h(1), *h_win = c.h(2), *h_tile = c.h(3), *h_cell = c.h(4);
    int64_t tiles = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        h_off[r] = roff[r];
        h_len[r] = read_lens[r];
        h_win[r] = j.win_off[(size_t)r];
        h_cell[r] = j.cell_off[(size_t)r];
        h_tile[r] = tiles;
        tiles += sd::dotplot_tiles(read_lens[r], W);
    }
    h_off[n_reads] = 0; h_len[n_reads] = 0; h_win[n_reads] = windows; h_cell[n_reads] = j.cells; h_tile[n_reads] = tiles;
    c.upload(5, st);
    const size_t strands = rc ? 2 : 1;
    c.tcnt.alloc(strands * (size_t)tiles);
    c.toff.alloc(strands * (size_t)tiles + 1);
    c.tsum.alloc((size_t)sd::scan_tiles_of((int64_t)strands * tiles));
    c.tbase.alloc((size_t)sd::scan_tiles_of((int64_t)strands * tiles) + 1);
    c.woff.alloc(strands * (size_t)windows);
    c.wraw.alloc(strands * (size_t)windows);
    c.summary.alloc(4);
    c.h_summary.alloc(4);
    j.a = sd::DpArgs{d_text, c.d(0), c.d(1), c.d(2), c.d(3), c.d(4), (int)n_reads, k, rc, M, W, B, windows, tiles,
                     c.tcnt.p, c.toff.p, c.woff.p, c.wraw.p, c.summary.p, nullptr, nullptr, nullptr, nullptr, nullptr};
    j.tsum = c.tsum.p;
    j.tbase = c.tbase.p;
}

template <bool GATHER>
void dp_tiles(const DpJob& j, hipStream_t st) {
    for (int64_t t0 = 0; t0 < j.a.tiles; t0 += sd::DOTPLOT_LAUNCH_TILES) {
        const unsigned grid = (unsigned)std::min<int64_t>(sd::DOTPLOT_LAUNCH_TILES, j.a.tiles - t0);
        hipLaunchKernelGGL(sd::sd_dotplot_tiles<GATHER>, dim3(grid), dim3(sd::DP_T), 0, st, j.a, t0);
        SD_HIP(hipGetLastError());
    }
}

void dp_count(const DpJob& j, hipStream_t st) {
    dp_tiles<false>(j, st);
    sd::exclusive_scan_dev(st, sd::ScanArray<int32_t>{j.a.tcnt}, (j.a.rc ? 2 : 1) * j.a.tiles, j.a.toff, j.tsum, j.tbase);
    hipLaunchKernelGGL(sd::sd_dotplot_windows, dim3(1), dim3(sd::DP_WIN_T), 0, st, j.a);
    SD_HIP(hipGetLastError());
}

void dp_sets(const DpJob& j, hipStream_t st) {
    dp_tiles<true>(j, st);
    const int64_t n = (j.a.rc ? 2 : 1) * j.a.windows;
    for (int64_t s0 = 0; s0 < n; s0 += sd::DOTPLOT_LAUNCH_TILES) {
        const unsigned grid = (unsigned)std::min<int64_t>(sd::DOTPLOT_LAUNCH_TILES, n - s0);
        hipLaunchKernelGGL(sd::sd_dotplot_sets, dim3(grid), dim3(sd::DP_T), 0, st, j.a, s0);
        SD_HIP(hipGetLastError());
    }
}

// whole rows per launch while their cells x the largest set x strands stay within DOTPLOT_LAUNCH_WORK; at least one row
void dp_pairs(DpJob& j, hipStream_t st, int32_t n_reads) {
    const int64_t per_cell = std::max<int64_t>(1, j.largest) * (j.a.rc ? 2 : 1);
    int64_t row0 = 0, rows = 0, work = 0, widest = 0, launches = 0, wgs = 0;
    auto flush = [&]() {
        if (!rows) return;
        const dim3 grid((unsigned)rows, (unsigned)((widest + sd::DOTPLOT_JSEG - 1) / sd::DOTPLOT_JSEG));
        if (j.a.rc) hipLaunchKernelGGL(sd::sd_dotplot_pairs<true>, grid, dim3(sd::DP_T), 0, st, j.a, row0, rows);
        else hipLaunchKernelGGL(sd::sd_dotplot_pairs<false>, grid, dim3(sd::DP_T), 0, st, j.a, row0, rows);
        SD_HIP(hipGetLastError());
        launches += 1;
        wgs += (int64_t)grid.x * grid.y;
        row0 += rows;
        rows = work = widest = 0;
    };
    for (int32_t r = 0; r < n_reads; ++r)
        for (int64_t il = 0, nw = j.win_off[(size_t)r + 1] - j.win_off[(size_t)r]; il < nw; ++il) {
            const int64_t cells = sd::dotplot_row_cells(il, j.a.B);   // <= 16 384: the rows' cells stay within the cap of a call
            if (rows && (work + cells * per_cell > sd::DOTPLOT_LAUNCH_WORK || rows >= ((int64_t)1 << 20))) flush();
            rows += 1;
            work += cells * per_cell;
            widest = std::max(widest, cells);
        }
    flush();
    j.launches = launches;
    j.workgroups = wgs;
    g_dp_launches.fetch_add(launches);
}

// The job on `st` up to the summary, which the host waits for: the counting pass is the only device work before a refusal.
int dp_begin(const char* who, DpCtx& c, hipStream_t st, DpJob& j, int32_t n_reads, char* errbuf, size_t errlen) {
    if (j.a.windows == 0) return SD_OK;
    dp_count(j, st);
    SD_HIP(hipMemcpyAsync(c.h_summary.p, c.summary.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ensure_event(c.ev_sum, hipEventDisableTiming);
    SD_HIP(hipEventRecord(c.ev_sum, st));
    SD_HIP(hipEventSynchronize(c.ev_sum));
    j.selected = c.h_summary.p[0];
    j.largest = c.h_summary.p[1];
    if (c.h_summary.p[2] >= 0) return dp_refuse_set(who, j.win_off.data(), n_reads, c.h_summary.p[2], c.h_summary.p[3], errbuf, errlen);
    c.sets.alloc((size_t)j.selected);
    j.a.sets = c.sets.p;
    return SD_OK;
}

// the timed repetitions of the three passes, each on the results of the one before
void dp_bench(DpJob& j, hipStream_t st, int32_t n_reads, const DpBench& b) {
    StageClock clock;
    clock.time(st, b.warmup, b.reps, b.ms_count, [&]() { dp_count(j, st); });
    clock.time(st, b.warmup, b.reps, b.ms_sets, [&]() { dp_sets(j, st); });
    clock.time(st, b.warmup, b.reps, b.ms_pairs, [&]() { dp_pairs(j, st, n_reads); });
    b.info[0] = j.launches;
    b.info[1] = j.workgroups;
    b.info[2] = j.cells;
    b.info[3] = j.a.windows;
    b.info[4] = j.selected;
    b.info[5] = j.largest;
}

int dp_dev(const char* who, const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t W, int64_t B,
           int64_t M, int32_t rc, int32_t device, int32_t* kmers, int32_t* kmers_rc, int32_t* shared, int32_t* shared_rc, char* errbuf,
           size_t errlen, const DpBench* bench) {
    DpJob j;
    j.win_off.assign((size_t)std::max(n_reads, 0) + 1, 0);
    j.cell_off.assign((size_t)std::max(n_reads, 0) + 1, 0);
    int64_t windows = 0;
    int e = dp_limits(who, read_lens, n_reads, k, W, B, M, j.win_off.data(), j.cell_off.data(), windows, j.cells, errbuf, errlen);
    if (e) return e;
    rc = rc ? 1 : 0;
    if ((e = dp_text_args(who, text, read_off, read_lens, n_reads, rc, windows, j.cells, kmers, kmers_rc, shared, shared_rc, errbuf, errlen))) return e;
    if ((e = device_check(device, errbuf, errlen))) return e;
    try {
        DeviceScope on(device);
        DpCtx& c = device_ctx<DpCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        OwnedStream st;
        const std::vector<int64_t> off = reads_upload(c.text, st, text, read_off, read_lens, n_reads);
        dp_tables(c, st, j, c.text.p, off.data(), read_lens, n_reads, k, W, B, (uint32_t)M, rc, windows);
        const size_t nw = (size_t)windows, nc = (size_t)j.cells;
        c.out.alloc(2 * nw + 2 * nc);
        j.a.kmers = c.out.p;
        j.a.kmers_rc = c.out.p + nw;
        j.a.shared = c.out.p + 2 * nw;
        j.a.shared_rc = c.out.p + 2 * nw + nc;
        e = dp_begin(who, c, st, j, n_reads, errbuf, errlen);
        if (e == SD_OK && windows > 0) {
            if (bench) {
                dp_bench(j, st, n_reads, *bench);
            } else {
                dp_sets(j, st);
                dp_pairs(j, st, n_reads);
            }
            SD_HIP(hipMemcpyAsync(kmers, j.a.kmers, nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(shared, j.a.shared, nc * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            if (rc) {
                SD_HIP(hipMemcpyAsync(kmers_rc, j.a.kmers_rc, nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                SD_HIP(hipMemcpyAsync(shared_rc, j.a.shared_rc, nc * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            }
        }
        SD_HIP(hipStreamSynchronize(st));
        return e;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
}

}  // namespace
}  // namespace sdi

extern "C" {

int sd_dotplot_layout(const int64_t* read_lens, int32_t n_reads, int64_t W, int64_t B, int64_t* win_off, int64_t* cell_off,
                      int64_t* windows_total, int64_t* cells_total) try {
    if (n_reads < 0 || (n_reads > 0 && !read_lens) || !windows_total || !cells_total || !sd::dotplot_w_ok(W) || !sd::dotplot_b_ok(B)) return SD_ERR_PARAM;
    return dp_layout(read_lens, n_reads, W, B, win_off, cell_off, *windows_total, *cells_total);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_dotplot_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t W, int64_t B,
                    int64_t M, int32_t rc, int32_t threads, int32_t* kmers, int32_t* kmers_rc, int32_t* shared, int32_t* shared_rc,
                    char* errbuf, size_t errlen) try {
    static const char* who = "sd_dotplot_host";
    std::vector<int64_t> win_off((size_t)std::max(n_reads, 0) + 1, 0), cell_off((size_t)std::max(n_reads, 0) + 1, 0);
    int64_t windows = 0, cells = 0;
    int e = dp_limits(who, read_lens, n_reads, k, W, B, M, win_off.data(), cell_off.data(), windows, cells, errbuf, errlen);
    if (e) return e;
    rc = rc ? 1 : 0;
    if ((e = dp_text_args(who, text, read_off, read_lens, n_reads, rc, windows, cells, kmers, kmers_rc, shared, shared_rc, errbuf, errlen))) return e;
    return dp_host(who, reinterpret_cast<const uint8_t*>(text), read_off, read_lens, n_reads, k, W, B, (uint32_t)M, rc, win_off.data(),
                   cell_off.data(), windows, std::max(1, threads), kmers, kmers_rc, shared, shared_rc, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_dotplot_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t W, int64_t B,
                   int64_t M, int32_t rc, int32_t device, int32_t* kmers, int32_t* kmers_rc, int32_t* shared, int32_t* shared_rc, char* errbuf,
                   size_t errlen) try {
    return dp_dev("sd_dotplot_dev", text, read_off, read_lens, n_reads, k, W, B, M, rc, device, kmers, kmers_rc, shared, shared_rc, errbuf, errlen,
                  nullptr);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_dotplot_reads_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t W, int64_t B,
                         int64_t M, int32_t rc, int32_t device, void* hip_stream, int32_t* d_kmers, int32_t* d_kmers_rc, int32_t* d_shared,
                         int32_t* d_shared_rc, char* errbuf, size_t errlen) try {
    static const char* who = "sd_dotplot_reads_dev";
    DpJob j;
    j.win_off.assign((size_t)std::max(n_reads, 0) + 1, 0);
    j.cell_off.assign((size_t)std::max(n_reads, 0) + 1, 0);
    int64_t windows = 0, bases = 0;
    int e = dp_limits(who, read_lens, n_reads, k, W, B, M, j.win_off.data(), j.cell_off.data(), windows, j.cells, errbuf, errlen);
    if (e) return e;
    rc = rc ? 1 : 0;
    if ((e = dp_text_args(who, d_text, read_off, read_lens, n_reads, rc, windows, j.cells, d_kmers, d_kmers_rc, d_shared, d_shared_rc, errbuf, errlen)))
        return e;
    if ((e = device_check(device, errbuf, errlen))) return e;
    for (int32_t r = 0; r < n_reads; ++r) bases += read_lens[r];
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        if (bases > 0 && (e = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return e;
        if (windows > 0 && (e = buffer_on_device(d_kmers, device, who, "kmers", errbuf, errlen))) return e;
        if (windows > 0 && rc && (e = buffer_on_device(d_kmers_rc, device, who, "kmers_rc", errbuf, errlen))) return e;
        if (j.cells > 0 && (e = buffer_on_device(d_shared, device, who, "shared", errbuf, errlen))) return e;
        if (j.cells > 0 && rc && (e = buffer_on_device(d_shared_rc, device, who, "shared_rc", errbuf, errlen))) return e;
        DpCtx& c = device_ctx<DpCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();   // the previous call's kernels read the buffers this one overwrites
        dp_tables(c, st, j, static_cast<const uint8_t*>(d_text), read_off, read_lens, n_reads, k, W, B, (uint32_t)M, rc, windows);
        j.a.kmers = d_kmers;
        j.a.kmers_rc = d_kmers_rc;
        j.a.shared = d_shared;
        j.a.shared_rc = d_shared_rc;
        e = dp_begin(who, c, st, j, n_reads, errbuf, errlen);
        if (e == SD_OK && windows > 0) {
            dp_sets(j, st);
            dp_pairs(j, st, n_reads);
        }
        c.in_flight(st);
        return e;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

uint64_t sd_dotplot_hash(uint64_t x) { return sd::dotplot_hash(x); }

void sd_dotplot_info(int64_t info[6]) {
    info[0] = sd::DOTPLOT_TILE;
    info[1] = sd::DOTPLOT_JSEG;
    info[2] = sd::DOTPLOT_SET_MAX;
    info[3] = sd::DOTPLOT_LAUNCH_WORK;
    info[4] = sd::DOTPLOT_CELLS_MAX;
    info[5] = g_dp_launches.load();
}

int sd_dotplot_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int32_t k, int64_t W, int64_t B,
                            int64_t M, int32_t rc, int32_t device, int32_t warmup, int32_t reps, float* ms_count, float* ms_sets,
                            float* ms_pairs, int64_t info[6]) try {
    if (warmup < 0 || reps < 1 || !ms_count || !ms_sets || !ms_pairs || !info || n_reads <= 0) return SD_ERR_PARAM;
    int64_t windows = 0, cells = 0;
    const int e = dp_limits("sd_dotplot_kernel_bench", read_lens, n_reads, k, W, B, M, nullptr, nullptr, windows, cells, nullptr, 0);
    if (e) return e;
    std::vector<int32_t> out(2 * (size_t)windows + 2 * (size_t)cells + 4);
    for (int i = 0; i < 6; ++i) info[i] = 0;
    const DpBench b{warmup, reps, ms_count, ms_sets, ms_pairs, info};
    return dp_dev("sd_dotplot_kernel_bench", text, read_off, read_lens, n_reads, k, W, B, M, rc, device, out.data(), out.data() + windows,
                  out.data() + 2 * windows, out.data() + 2 * windows + cells, nullptr, 0, &b);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
