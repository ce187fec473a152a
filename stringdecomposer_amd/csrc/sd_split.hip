// sd_split.hip -- subfamilies of every monomer's instances (--split): a clustering of the rows of --msa per forward
// monomer, integer work on bit planes.  sd_split.hpp holds the rule and everything host and device compute alike; this
// file holds the kernels, the host form and the C-ABI (include/sd_hip.h: sd_split_*).
//   sd_split_plan / sd_split_members   the member rows of every monomer of the job (status 1, a forward-monomer index),
//                      counted and grouped by monomer with group_scatter (sd_group_dev.hpp).  A member's slot in its
//                      monomer depends on the atomics; nothing computed does: ties between rows go by the row's index in
//                      the job, which every slot carries.
//   sd_split_prep      a wave per member row: three ballots per 64 columns turn its symbol bytes into three bit planes,
//                      W = ceil(L / 64) words each, slot-minor (a lane of the assign kernel reads a coalesced word)
//   sd_split_assign<W> a lane per row, the centres' planes in LDS (at most 64 x 3 x 8 words = 12 KB; every lane reads the
//                      same word: a broadcast).  Distances are popcounts of (a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2); the lane
//                      keeps the best and the second best.  Per workgroup: the rows that changed, the rows per centre and
//                      the 64-bit maximum of split_key over the candidates, from LDS with one atomic each.
//   the modes          sd_split_scan (cluster offsets from the sizes of the last assign) -> sd_split_group (group_scatter
//                      by cluster: a wave holds rows of one cluster) -> sd_split_count (a workgroup per 1 024 rows of one
//                      cluster: per column three ballots give the six symbol masks by bit logic, their popcounts go to
//                      LDS counters, flushed once per workgroup and (column, symbol)) -> sd_split_centres (counts ->
//                      planes, ties to the smallest code, an empty cluster keeps its centre)
//   sd_split_trial     the trial's centres: the current ones and the seed row's planes
//   sd_split_retire    a rejected seed stops being a candidate; the key over those that are
// Per pass the host reads 16 bytes (key, changed, last cluster's size); rows, planes and counts stay in HBM, and every
// kernel and copy is ordered on one stream.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <numeric>

#include "sd_group_dev.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"
#include "sd_split.hpp"

namespace sd {

constexpr int SP_T = 256;            // threads per workgroup (= GROUP_T)
constexpr int SP_CHUNK = 1024;       // rows of one cluster per workgroup of sd_split_count
static_assert(SP_T == GROUP_T, "group_scatter is called by workgroups of GROUP_T threads");
static_assert(SPLIT_KMAX * 3 * SPLIT_WMAX * 8 <= 16 * 1024, "the centres' planes fit a corner of LDS");

struct SpMember {
    const uint8_t* status;
    const int32_t* fmono;
    int M;
    __device__ bool in(int64_t m) const { return status[m] == 1 && fmono[m] >= 0 && fmono[m] < M; }
    __device__ int kind(int64_t m) const { return in(m) ? (int)GROUP_IN : (int)GROUP_OUT; }
    __device__ int group(int64_t m) const { return fmono[m]; }
    __device__ void aside(int64_t, int64_t) const {}
};

__global__ __launch_bounds__(SP_T) void sd_split_plan(SpMember src, int64_t n_rows, int32_t* __restrict__ mcount) {
    __shared__ int hist[GROUP_HIST];
    const int nb = src.M < GROUP_HIST ? src.M : GROUP_HIST;
    for (int i = threadIdx.x; i < nb; i += SP_T) hist[i] = 0;
    __syncthreads();
    const int64_t m = (int64_t)blockIdx.x * SP_T + threadIdx.x;
    if (m < n_rows && src.in(m)) {
        const int g = src.group(m);
        if (g < GROUP_HIST) atomicAdd(&hist[g], 1); else atomicAdd(&mcount[g], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += SP_T)
        if (hist[i]) atomicAdd(&mcount[i], hist[i]);
}

__global__ __launch_bounds__(SP_T) void sd_split_members(SpMember src, int64_t n_rows, int32_t* __restrict__ cursor, int32_t* __restrict__ order) {
    group_scatter(src, n_rows, n_rows, src.M, cursor, order);
}

// slot j of the monomer = row order[j] of the job
__global__ __launch_bounds__(SP_T) void sd_split_prep(const uint8_t* __restrict__ rows, const int64_t* __restrict__ row_at,
                                                      const int32_t* __restrict__ order, int64_t n, int L, int W,
                                                      uint64_t* __restrict__ planes, int32_t* __restrict__ rowid, uint8_t* __restrict__ cand) {
    const int lane = threadIdx.x & 63;
    const int64_t nwave = (int64_t)gridDim.x * (SP_T / 64);
    for (int64_t j = (int64_t)blockIdx.x * (SP_T / 64) + (threadIdx.x >> 6); j < n; j += nwave) {
        const int32_t r = order[j];
        const uint8_t* x = rows + row_at[r];
        for (int w = 0; w < W; ++w) {
            const int g = 64 * w + lane;
            const int s = g < L ? split_sym(x[g]) : 0;
            const uint64_t b0 = __ballot(s & 1), b1 = __ballot(s & 2), b2 = __ballot(s & 4);
            if (lane == 0) {
                planes[(int64_t)(0 * W + w) * n + j] = b0;
                planes[(int64_t)(1 * W + w) * n + j] = b1;
                planes[(int64_t)(2 * W + w) * n + j] = b2;
            }
        }
        if (lane == 0) { rowid[j] = r; cand[j] = 1; }
    }
}

template <int W>
__global__ __launch_bounds__(SP_T) void sd_split_assign(const uint64_t* __restrict__ planes, int64_t n, const uint64_t* __restrict__ cen, int k,
                                                        const int32_t* prev, int32_t* asg, int32_t* __restrict__ d1o, int32_t* __restrict__ d2o,
                                                        const uint8_t* __restrict__ cand, const int32_t* __restrict__ rowid, SplitStat* stat) {
    __shared__ uint64_t c[SPLIT_KMAX * 3 * W];
    __shared__ unsigned long long wkey;
    __shared__ uint32_t wch, hist[SPLIT_KMAX];
    for (int i = threadIdx.x; i < k * 3 * W; i += SP_T) {
        const int cc = i / (3 * W), r = i - cc * 3 * W, p = r / W;
        c[i] = cen[(cc * 3 + p) * SPLIT_WMAX + (r - p * W)];
    }
    if (threadIdx.x < SPLIT_KMAX) hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) { wkey = 0; wch = 0; }
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * SP_T + threadIdx.x;
    if (j < n) {
        uint64_t a[3][W];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int w = 0; w < W; ++w) a[p][w] = planes[(int64_t)(p * W + w) * n + j];
        SplitBest b;
        for (int cc = 0; cc < k; ++cc) {
            const uint64_t* q = c + cc * 3 * W;
            int d = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) d += split_word_dist(a[0][w], a[1][w], a[2][w], q[w], q[W + w], q[2 * W + w]);
            b.take(d, cc);
        }
        if (!prev || prev[j] != b.at) atomicAdd(&wch, 1u);
        asg[j] = b.at;
        d1o[j] = b.d1;
        d2o[j] = b.second();
        atomicAdd(&hist[b.at], 1u);
        if (cand[j]) atomicMax(&wkey, (unsigned long long)split_key(b.d1, (uint32_t)rowid[j]));
    }
    __syncthreads();
    if ((int)threadIdx.x < k && hist[threadIdx.x]) {
        atomicAdd(&stat->sizes[threadIdx.x], hist[threadIdx.x]);
        if ((int)threadIdx.x == k - 1) atomicAdd(&stat->last, hist[threadIdx.x]);
    }
    if (threadIdx.x == 0) {
        if (wch) atomicAdd(&stat->changed, wch);
        if (wkey) atomicMax(&stat->key, wkey);
    }
}

// tabs = coff[65] | woff[65] | cursor[66]: where a cluster's rows begin in the grouped order, where its workgroups of
// sd_split_count begin, and group_scatter's cursors
constexpr int SP_COFF = 0, SP_WOFF = SPLIT_KMAX + 1, SP_CURSOR = 2 * (SPLIT_KMAX + 1), SP_TABS = 3 * (SPLIT_KMAX + 1) + 1;

__global__ void sd_split_scan(const SplitStat* __restrict__ stat, int k, int32_t* __restrict__ tabs) {
    if (threadIdx.x || blockIdx.x) return;
    int32_t at = 0, wg = 0;
    for (int c = 0; c < k; ++c) {
        tabs[SP_COFF + c] = at;
        tabs[SP_WOFF + c] = wg;
        tabs[SP_CURSOR + c] = at;
        at += (int32_t)stat->sizes[c];
        wg += ((int32_t)stat->sizes[c] + SP_CHUNK - 1) / SP_CHUNK;
    }
    tabs[SP_COFF + k] = at;
    tabs[SP_WOFF + k] = wg;
    tabs[SP_CURSOR + k] = 0;
}

struct SpCluster {
    const int32_t* asg;
    __device__ int kind(int64_t) const { return (int)GROUP_IN; }
    __device__ int group(int64_t m) const { return asg[m]; }
    __device__ void aside(int64_t, int64_t) const {}
};

__global__ __launch_bounds__(SP_T) void sd_split_group(SpCluster src, int64_t n, int k, int32_t* __restrict__ tabs, int32_t* __restrict__ order2) {
    group_scatter(src, n, n, k, tabs + SP_CURSOR, order2);
}

__global__ __launch_bounds__(SP_T) void sd_split_count(const uint64_t* __restrict__ planes, int64_t n, int L, int W, int k,
                                                       const int32_t* __restrict__ tabs, const int32_t* __restrict__ order2,
                                                       int32_t* __restrict__ counts) {
    __shared__ int cnt[SPLIT_LMAX * SPLIT_SYMS];
    const int b = blockIdx.x;
    if (b >= tabs[SP_WOFF + k]) return;
    int c = 0;   // the last cluster whose workgroups begin at or before b: it has one there
    for (int x = 1; x < k; ++x)
        if (tabs[SP_WOFF + x] <= b) c = x;
    for (int i = threadIdx.x; i < L * SPLIT_SYMS; i += SP_T) cnt[i] = 0;
    __syncthreads();
    const int64_t first = (int64_t)tabs[SP_COFF + c] + (int64_t)(b - tabs[SP_WOFF + c]) * SP_CHUNK;
    const int64_t end = first + SP_CHUNK < tabs[SP_COFF + c + 1] ? first + SP_CHUNK : tabs[SP_COFF + c + 1];
    const int lane = threadIdx.x & 63;
    for (int64_t base = first + (threadIdx.x >> 6) * 64; base < end; base += SP_T) {   // (uniform in a wave)
        const bool valid = base + lane < end;
        const int64_t j = valid ? order2[base + lane] : 0;
        const uint64_t mv = __ballot(valid);
        for (int w = 0; w < W; ++w) {
            const uint64_t a0 = valid ? planes[(int64_t)(0 * W + w) * n + j] : 0;
            const uint64_t a1 = valid ? planes[(int64_t)(1 * W + w) * n + j] : 0;
            const uint64_t a2 = valid ? planes[(int64_t)(2 * W + w) * n + j] : 0;
            const int nb = L - 64 * w < 64 ? L - 64 * w : 64;
            for (int bit = 0; bit < nb; ++bit) {
                const uint64_t m0 = __ballot((a0 >> bit) & 1), m1 = __ballot((a1 >> bit) & 1), m2 = __ballot((a2 >> bit) & 1);
                if (lane < SPLIT_SYMS) {   // lane s counts symbol s
                    const uint64_t m = ((lane & 1) ? m0 : ~m0) & ((lane & 2) ? m1 : ~m1) & ((lane & 4) ? m2 : ~m2) & mv;
                    if (m) atomicAdd(&cnt[(64 * w + bit) * SPLIT_SYMS + lane], __popcll(m));
                }
            }
        }
    }
    __syncthreads();
    int32_t* out = counts + (int64_t)c * L * SPLIT_SYMS;
    for (int i = threadIdx.x; i < L * SPLIT_SYMS; i += SP_T)
        if (cnt[i]) atomicAdd(&out[i], cnt[i]);
}

// a thread per (cluster, word)
__global__ __launch_bounds__(SP_T) void sd_split_centres(const int32_t* __restrict__ counts, const SplitStat* __restrict__ stat, int L, int W, int k,
                                                         uint64_t* __restrict__ cen) {
    const int i = blockIdx.x * SP_T + threadIdx.x;
    if (i >= k * W) return;
    const int c = i / W, w = i - c * W;
    if (stat->sizes[c] == 0) return;   // an empty cluster keeps its centre
    uint64_t p0 = 0, p1 = 0, p2 = 0;
    for (int bit = 0; bit < 64 && 64 * w + bit < L; ++bit) {
        const uint64_t s = (uint64_t)split_mode(counts + ((int64_t)c * L + 64 * w + bit) * SPLIT_SYMS);
        p0 |= (s & 1) << bit;
        p1 |= ((s >> 1) & 1) << bit;
        p2 |= ((s >> 2) & 1) << bit;
    }
    cen[(c * 3 + 0) * SPLIT_WMAX + w] = p0;
    cen[(c * 3 + 1) * SPLIT_WMAX + w] = p1;
    cen[(c * 3 + 2) * SPLIT_WMAX + w] = p2;
}

// dst = the k centres of src, then row `row` of the job as centre k
__global__ __launch_bounds__(SP_T) void sd_split_trial(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, int k,
                                                       const uint8_t* __restrict__ rows, const int64_t* __restrict__ row_at, uint32_t row, int L, int W) {
    for (int i = threadIdx.x; i < k * 3 * SPLIT_WMAX; i += SP_T) dst[i] = src[i];
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const uint8_t* x = rows + row_at[row];
    for (int w = 0; w < W; ++w) {
        const int g = 64 * w + lane;
        const int s = g < L ? split_sym(x[g]) : 0;
        const uint64_t b0 = __ballot(s & 1), b1 = __ballot(s & 2), b2 = __ballot(s & 4);
        if (lane == 0) {
            dst[(k * 3 + 0) * SPLIT_WMAX + w] = b0;
            dst[(k * 3 + 1) * SPLIT_WMAX + w] = b1;
            dst[(k * 3 + 2) * SPLIT_WMAX + w] = b2;
        }
    }
}

__global__ __launch_bounds__(SP_T) void sd_split_retire(const int32_t* __restrict__ rowid, const int32_t* __restrict__ d1, uint8_t* __restrict__ cand,
                                                        int64_t n, uint32_t row, SplitStat* stat) {
    __shared__ unsigned long long wkey;
    if (threadIdx.x == 0) wkey = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * SP_T + threadIdx.x;
    if (j < n) {
        if ((uint32_t)rowid[j] == row) cand[j] = 0;
        else if (cand[j]) atomicMax(&wkey, (unsigned long long)split_key(d1[j], (uint32_t)rowid[j]));
    }
    __syncthreads();
    if (threadIdx.x == 0 && wkey) atomicMax(&stat->key, wkey);
}

// the slots' results to the rows of the job
__global__ __launch_bounds__(SP_T) void sd_split_out(const int32_t* __restrict__ rowid, const int32_t* __restrict__ asg, const int32_t* __restrict__ d1,
                                                     const int32_t* __restrict__ d2, int64_t n, int32_t* __restrict__ sub, int32_t* __restrict__ o1,
                                                     int32_t* __restrict__ o2) {
    const int64_t j = (int64_t)blockIdx.x * SP_T + threadIdx.x;
    if (j >= n) return;
    const int32_t r = rowid[j];
    sub[r] = asg[j];
    o1[r] = d1[j];
    o2[r] = d2[j];
}

// the centres as symbol bytes, k rows of L
__global__ __launch_bounds__(SP_T) void sd_split_cen_out(const uint64_t* __restrict__ cen, int k, int L, uint8_t* __restrict__ out) {
    const int i = blockIdx.x * SP_T + threadIdx.x;
    if (i >= k * L) return;
    const int c = i / L, g = i - c * L, w = g >> 6, bit = g & 63;
    const uint64_t* q = cen + c * 3 * SPLIT_WMAX;
    out[i] = (uint8_t)(((q[w] >> bit) & 1) | (((q[SPLIT_WMAX + w] >> bit) & 1) << 1) | (((q[2 * SPLIT_WMAX + w] >> bit) & 1) << 2));
}

}  // namespace sd

namespace sdi {
namespace {

std::atomic<int64_t> g_sp_launches{0};   // launches of sd_split_assign in this process (sd_split_info)

// ---- the host form ------------------------------------------------------------------------------------------------------
// rows: n x pitch symbol bytes, row i = member i
struct SpHost {
    const uint8_t* sym;
    int64_t n, pitch;
    int L, W, threads;
    std::vector<uint64_t> planes;   // [n][3][W]
    std::vector<uint8_t> cand;
    struct State {
        std::vector<int32_t> asg, d1, d2;
        std::vector<uint64_t> cen;   // [SPLIT_KMAX][3][W]
        sd::SplitStat stat;
    } A, B;
    State *cur = &A, *tr = &B;

    SpHost(const uint8_t* s, int64_t n_, int64_t pitch_, int L_, int threads_)
        : sym(s), n(n_), pitch(pitch_), L(L_), W(sd::split_words(L_)), threads(std::max(1, threads_)) {
        planes.assign((size_t)n * 3 * W, 0);
        cand.assign((size_t)n, 1);
        for (State* s2 : {&A, &B}) {
            s2->asg.assign((size_t)n, 0);
            s2->d1.assign((size_t)n, 0);
            s2->d2.assign((size_t)n, 0);
            s2->cen.assign((size_t)sd::SPLIT_KMAX * 3 * W, 0);
            std::memset(&s2->stat, 0, sizeof(sd::SplitStat));
        }
        sd::parallel_for(n, threads, 256, [&](int64_t i) { to_planes(sym + i * pitch, &planes[(size_t)i * 3 * W]); });
    }
    void to_planes(const uint8_t* x, uint64_t* p) const {
        for (int w = 0; w < 3 * W; ++w) p[w] = 0;
        for (int g = 0; g < L; ++g) {
            const uint64_t s = (uint64_t)sd::split_sym(x[g]);
            p[g >> 6] |= (s & 1) << (g & 63);
            p[W + (g >> 6)] |= ((s >> 1) & 1) << (g & 63);
            p[2 * W + (g >> 6)] |= ((s >> 2) & 1) << (g & 63);
        }
    }
    void start() {
        std::fill(tr->asg.begin(), tr->asg.end(), 0);
        std::memset(&tr->stat, 0, sizeof(sd::SplitStat));
        tr->stat.sizes[0] = (uint32_t)n;
    }
    void modes(int k) {
        const int64_t slab = 4096, ns = (n + slab - 1) / slab;
        const size_t cells = (size_t)k * L * sd::SPLIT_SYMS;
        const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads, ns));
        std::vector<std::vector<int32_t>> part((size_t)nt, std::vector<int32_t>(cells, 0));
        sd::parallel_for(nt, nt, 1, [&](int64_t t) {   // thread t: slabs t, t + nt, ...
            int32_t* cnt = part[(size_t)t].data();
            for (int64_t s = t; s < ns; s += nt)
                for (int64_t i = s * slab; i < std::min(n, (s + 1) * slab); ++i) {
                    const uint8_t* x = sym + i * pitch;
                    int32_t* c = cnt + (size_t)tr->asg[(size_t)i] * L * sd::SPLIT_SYMS;
                    for (int g = 0; g < L; ++g) c[g * sd::SPLIT_SYMS + sd::split_sym(x[g])] += 1;
                }
        });
        for (int c = 0; c < k; ++c) {
            if (tr->stat.sizes[c] == 0) continue;   // an empty cluster keeps its centre
            uint64_t* q = &tr->cen[(size_t)c * 3 * W];
            for (int w = 0; w < 3 * W; ++w) q[w] = 0;
            for (int g = 0; g < L; ++g) {
                int64_t v[sd::SPLIT_SYMS] = {0, 0, 0, 0, 0, 0};
                for (int t = 0; t < nt; ++t)
                    for (int s = 0; s < sd::SPLIT_SYMS; ++s) v[s] += part[(size_t)t][((size_t)c * L + g) * sd::SPLIT_SYMS + s];
                const uint64_t s = (uint64_t)sd::split_mode(v);
                q[g >> 6] |= (s & 1) << (g & 63);
                q[W + (g >> 6)] |= ((s >> 1) & 1) << (g & 63);
                q[2 * W + (g >> 6)] |= ((s >> 2) & 1) << (g & 63);
            }
        }
    }
    sd::SplitStat assign(int k, bool first) {
        const std::vector<int32_t>& prev = first ? cur->asg : tr->asg;
        const int64_t slab = 1024, ns = (n + slab - 1) / slab;
        std::vector<sd::SplitStat> part((size_t)ns);
        sd::parallel_for(ns, threads, 1, [&](int64_t s) {
            sd::SplitStat& st = part[(size_t)s];
            std::memset(&st, 0, sizeof st);
            for (int64_t i = s * slab; i < std::min(n, (s + 1) * slab); ++i) {
                const uint64_t* a = &planes[(size_t)i * 3 * W];
                sd::SplitBest b;
                for (int c = 0; c < k; ++c) {
                    const uint64_t* q = &tr->cen[(size_t)c * 3 * W];
                    int d = 0;
                    for (int w = 0; w < W; ++w) d += sd::split_word_dist(a[w], a[W + w], a[2 * W + w], q[w], q[W + w], q[2 * W + w]);
                    b.take(d, c);
                }
                if (prev[(size_t)i] != b.at) st.changed += 1;   // (first: not used)
                tr->asg[(size_t)i] = b.at;
                tr->d1[(size_t)i] = b.d1;
                tr->d2[(size_t)i] = b.second();
                st.sizes[b.at] += 1;
                if (cand[(size_t)i]) st.key = std::max<unsigned long long>(st.key, sd::split_key(b.d1, (uint32_t)i));
            }
        });
        sd::SplitStat& out = tr->stat;
        std::memset(&out, 0, sizeof out);
        for (const sd::SplitStat& st : part) {
            out.key = std::max(out.key, st.key);
            out.changed += st.changed;
            for (int c = 0; c < k; ++c) out.sizes[c] += st.sizes[c];
        }
        out.last = out.sizes[k - 1];
        return out;
    }
    void accept() { std::swap(cur, tr); }
    void begin(int k, uint32_t row) {
        std::copy(cur->cen.begin(), cur->cen.begin() + (size_t)k * 3 * W, tr->cen.begin());
        to_planes(sym + (int64_t)row * pitch, &tr->cen[(size_t)k * 3 * W]);
    }
    unsigned long long reject(uint32_t row) {
        cand[row] = 0;
        unsigned long long key = 0;
        for (int64_t i = 0; i < n; ++i)
            if (cand[(size_t)i]) key = std::max<unsigned long long>(key, sd::split_key(cur->d1[(size_t)i], (uint32_t)i));
        return key;
    }
    void centres_out(int k, uint8_t* out) const {
        for (int c = 0; c < k; ++c)
            for (int g = 0; g < L; ++g) {
                const uint64_t* q = &cur->cen[(size_t)c * 3 * W];
                out[(size_t)c * L + g] = (uint8_t)(((q[g >> 6] >> (g & 63)) & 1) | (((q[W + (g >> 6)] >> (g & 63)) & 1) << 1) |
                                                   (((q[2 * W + (g >> 6)] >> (g & 63)) & 1) << 2));
            }
    }
};

int sp_params(const char* who, int64_t n, int64_t pitch, int32_t L, int32_t R, int32_t K, int32_t S, int32_t I, char* errbuf, size_t errlen) {
    std::string bad;
    if (n < 0 || L < 1 || pitch < L) bad = "n = " + std::to_string(n) + " rows of pitch " + std::to_string(pitch) + " for L = " + std::to_string(L) + " columns";
    else if (R < 1) bad = "R = " + std::to_string(R) + ", the radius is 1 or more";
    else if (K < 1 || K > sd::SPLIT_KMAX) bad = "K = " + std::to_string(K) + ", must be 1 .. " + std::to_string(sd::SPLIT_KMAX);
    else if (S < 1) bad = "min_size = " + std::to_string(S) + ", must be 1 or more";
    else if (I < 1) bad = "max_iter = " + std::to_string(I) + ", must be 1 or more";
    else if (n > sd::SPLIT_NMAX)
        bad = std::to_string(n) + " member rows, the cap is " + std::to_string(sd::SPLIT_NMAX) + " (SPLIT_NMAX)";
    if (bad.empty()) return SD_OK;
    set_err(errbuf, errlen, std::string(who) + ": " + bad);
    return SD_ERR_PARAM;
}

// the host form on a matrix; centres: K x L bytes (k rows written), sizes: K, info: {k, rounds, iterations, 0}
void sp_host_core(const uint8_t* sym, int64_t n, int64_t pitch, int L, int R, int K, int S, int I, int threads, uint8_t* centres, int32_t* asg,
                  int32_t* d1, int32_t* d2, int32_t* sizes, int64_t* info) {
    for (int c = 0; c < K; ++c) sizes[c] = 0;
    info[3] = 0;
    SpHost h(sym, n, pitch, L, threads);
    sd::split_drive(h, n, R, K, S, I, info);
    if (n <= 0) return;
    const int k = (int)info[0];
    h.centres_out(k, centres);
    std::copy(h.cur->asg.begin(), h.cur->asg.end(), asg);
    std::copy(h.cur->d1.begin(), h.cur->d1.end(), d1);
    std::copy(h.cur->d2.begin(), h.cur->d2.end(), d2);
    for (int c = 0; c < k; ++c) sizes[c] = (int32_t)h.cur->stat.sizes[c];
}

// ---- the device passes --------------------------------------------------------------------------------------------------
struct SpBench {
    int warmup, reps;
    float *ms_prep, *ms_assign, *ms_modes;
};

// Per device, kept between calls (sd_job_dev.hpp: DevWork).  Every call is done with it when it returns: nothing is left
// in flight, so no call settles.
struct SpCtx : DevWork {
    DevBuf<uint64_t> planes, cen;
    DevBuf<int32_t> slots, counts, tabs, order, mcount;
    DevBuf<uint8_t> cand, up_rows, up_status, cen_sym;
    DevBuf<int64_t> up_at;
    DevBuf<int32_t> up_fmono, o_sub, o_d1, o_d2;
    DevBuf<sd::SplitStat> stat;   // two states and the key of a rejected round
    PinBuf<sd::SplitStat> h_stat;
    PinBuf<int32_t> h_counts;
};

inline unsigned sp_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + sd::SP_T - 1) / sd::SP_T); }

// one monomer's rows on the device: the backend of split_drive
struct SpDev {
    SpCtx& c;
    hipStream_t st;
    const uint8_t* rows;
    const int64_t* row_at;
    const int32_t* order;   // the monomer's members: slot -> row of the job
    int64_t n;
    int L, W;
    struct State {
        int32_t *asg, *d1, *d2;
        uint64_t* cen;
        sd::SplitStat* stat;
    } A, B;
    State *cur = &A, *tr = &B;
    int32_t *rowid, *order2;
    sd::SplitStat* kstat;

    SpDev(SpCtx& c_, hipStream_t st_, const uint8_t* rows_, const int64_t* row_at_, const int32_t* order_, int64_t n_, int L_)
        : c(c_), st(st_), rows(rows_), row_at(row_at_), order(order_), n(n_), L(L_), W(sd::split_words(L_)) {
        c.planes.alloc((size_t)3 * W * n);
        c.slots.alloc((size_t)8 * n);
        c.cand.alloc((size_t)n);
        c.cen.alloc((size_t)2 * sd::SPLIT_KMAX * 3 * sd::SPLIT_WMAX);
        c.counts.alloc((size_t)sd::SPLIT_KMAX * sd::SPLIT_LMAX * sd::SPLIT_SYMS);
        c.tabs.alloc(sd::SP_TABS);
        c.stat.alloc(3);
        c.h_stat.alloc(1);
        int32_t* s = c.slots.p;
        rowid = s;
        order2 = s + n;
        A = State{s + 2 * n, s + 3 * n, s + 4 * n, c.cen.p, c.stat.p};
        B = State{s + 5 * n, s + 6 * n, s + 7 * n, c.cen.p + sd::SPLIT_KMAX * 3 * sd::SPLIT_WMAX, c.stat.p + 1};
        kstat = c.stat.p + 2;
    }
    void prep() {
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, (int64_t)c.n_cu * 32));
        hipLaunchKernelGGL(sd::sd_split_prep, dim3(grid), dim3(sd::SP_T), 0, st, rows, row_at, order, n, L, W, c.planes.p, rowid, c.cand.p);
        SD_HIP(hipGetLastError());
    }
    void start() {
        SD_HIP(hipMemsetAsync(tr->asg, 0, sizeof(int32_t) * (size_t)n, st));
        std::memset(c.h_stat.p, 0, sizeof(sd::SplitStat));
        c.h_stat.p->sizes[0] = (uint32_t)n;
        SD_HIP(hipMemcpyAsync(tr->stat, c.h_stat.p, sizeof(sd::SplitStat), hipMemcpyHostToDevice, st));
        SD_HIP(hipStreamSynchronize(st));   // (h_stat is read into again)
    }
    void modes(int k) {
        SD_HIP(hipMemsetAsync(c.counts.p, 0, sizeof(int32_t) * (size_t)k * L * sd::SPLIT_SYMS, st));
        hipLaunchKernelGGL(sd::sd_split_scan, dim3(1), dim3(64), 0, st, tr->stat, k, c.tabs.p);
        hipLaunchKernelGGL(sd::sd_split_group, dim3(sp_grid(n)), dim3(sd::SP_T), 0, st, sd::SpCluster{tr->asg}, n, k, c.tabs.p, order2);
        const unsigned wgs = (unsigned)((n + sd::SP_CHUNK - 1) / sd::SP_CHUNK + k);   // sum of ceil(size / SP_CHUNK) at most
        hipLaunchKernelGGL(sd::sd_split_count, dim3(wgs), dim3(sd::SP_T), 0, st, c.planes.p, n, L, W, k, c.tabs.p, order2, c.counts.p);
        hipLaunchKernelGGL(sd::sd_split_centres, dim3(sp_grid((int64_t)k * W)), dim3(sd::SP_T), 0, st, c.counts.p, tr->stat, L, W, k, tr->cen);
        SD_HIP(hipGetLastError());
    }
    void assign_launch(int k, bool first) {
        SD_HIP(hipMemsetAsync(tr->stat, 0, sizeof(sd::SplitStat), st));
        const int32_t* prev = first ? cur->asg : tr->asg;
#define SD_SP(WW) hipLaunchKernelGGL(sd::sd_split_assign<WW>, dim3(sp_grid(n)), dim3(sd::SP_T), 0, st, c.planes.p, n, tr->cen, k, prev, tr->asg, tr->d1, tr->d2, c.cand.p, rowid, tr->stat)
        switch (W) {
            case 1: SD_SP(1); break;
            case 2: SD_SP(2); break;
            case 3: SD_SP(3); break;
            case 4: SD_SP(4); break;
            case 5: SD_SP(5); break;
            case 6: SD_SP(6); break;
            case 7: SD_SP(7); break;
            default: SD_SP(8); break;
        }
#undef SD_SP
        SD_HIP(hipGetLastError());
        g_sp_launches.fetch_add(1);
    }
    sd::SplitStat fetch(const sd::SplitStat* from) {   // key, changed, last: 16 bytes
        SD_HIP(hipMemcpyAsync(c.h_stat.p, from, 16, hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));
        return *c.h_stat.p;
    }
    sd::SplitStat assign(int k, bool first) {
        assign_launch(k, first);
        return fetch(tr->stat);
    }
    void accept() { std::swap(cur, tr); }
    void begin(int k, uint32_t row) {
        hipLaunchKernelGGL(sd::sd_split_trial, dim3(1), dim3(sd::SP_T), 0, st, cur->cen, tr->cen, k, rows, row_at, row, L, W);
        SD_HIP(hipGetLastError());
    }
    unsigned long long reject(uint32_t row) {
        SD_HIP(hipMemsetAsync(kstat, 0, sizeof(sd::SplitStat), st));
        hipLaunchKernelGGL(sd::sd_split_retire, dim3(sp_grid(n)), dim3(sd::SP_T), 0, st, rowid, cur->d1, c.cand.p, n, row, kstat);
        SD_HIP(hipGetLastError());
        return fetch(kstat).key;
    }
};

static_assert(offsetof(sd::SplitStat, sizes) == 16, "the host reads the first 16 bytes of a SplitStat");

// the timed repetitions of the three stages on the trial state of a finished monomer (its results are out already)
void sp_bench(SpDev& d, int k, const SpBench& b) {
    SD_HIP(hipMemcpyAsync(d.tr->cen, d.cur->cen, sizeof(uint64_t) * sd::SPLIT_KMAX * 3 * sd::SPLIT_WMAX, hipMemcpyDeviceToDevice, d.st));
    d.assign_launch(k, true);
    StageClock clock;
    clock.time(d.st, b.warmup, b.reps, b.ms_prep, [&]() { d.prep(); });
    clock.time(d.st, b.warmup, b.reps, b.ms_assign, [&]() { d.assign_launch(k, false); });
    clock.time(d.st, b.warmup, b.reps, b.ms_modes, [&]() { d.modes(k); });
}

struct SpJob {
    const uint8_t* rows;        // device: rows in the layout of --msa (sd_split_dev: the matrix's)
    const int64_t* row_at;
    const uint8_t* status;
    const int32_t* fmono;
    int64_t n_rows;
    const int32_t *mono_len, *radius;
    const char* const* names;
    int32_t n_mono, K, S, I;
    int32_t *sub, *d1, *d2;     // device, n_rows
    uint8_t* centres;           // device
    int64_t centres_cap;
    int64_t* cen_off;           // host, n_mono + 1
    int32_t* sizes;             // host, n_mono x K
    int64_t* info;              // host, n_mono x 4: members, k, rounds, iterations
};

std::string sp_name(const SpJob& j, int m) {
    return j.names && j.names[m] ? std::string("monomer ") + j.names[m] : "monomer " + std::to_string(m);
}

// Every monomer of the job on `st`.  Waits for the stream many times (16 bytes per pass); the last copies may be in
// flight when it returns.  Throws HipFail; other refusals come back as a code with errbuf set.
int sp_run(const char* who, SpCtx& c, hipStream_t st, const SpJob& j, const SpBench* bench, char* errbuf, size_t errlen) {
    const int M = j.n_mono;
    for (int m = 0; m <= M; ++m) j.cen_off[m] = 0;
    for (int64_t i = 0; i < (int64_t)M * j.K; ++i) j.sizes[i] = 0;
    for (int64_t i = 0; i < (int64_t)M * 4; ++i) j.info[i] = 0;
    if (j.n_rows > 0) {
        SD_HIP(hipMemsetAsync(j.sub, 0xFF, sizeof(int32_t) * (size_t)j.n_rows, st));   // -1: no member
        SD_HIP(hipMemsetAsync(j.d1, 0xFF, sizeof(int32_t) * (size_t)j.n_rows, st));
        SD_HIP(hipMemsetAsync(j.d2, 0xFF, sizeof(int32_t) * (size_t)j.n_rows, st));
    }
    if (M == 0 || j.n_rows == 0) return SD_OK;
    // the members of every monomer, grouped
    c.mcount.alloc((size_t)M + 1);
    c.h_counts.alloc((size_t)M + 1);
    c.order.alloc((size_t)j.n_rows);
    const sd::SpMember src{j.status, j.fmono, M};
    SD_HIP(hipMemsetAsync(c.mcount.p, 0, sizeof(int32_t) * ((size_t)M + 1), st));
    hipLaunchKernelGGL(sd::sd_split_plan, dim3(sp_grid(j.n_rows)), dim3(sd::SP_T), 0, st, src, j.n_rows, c.mcount.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipMemcpyAsync(c.h_counts.p, c.mcount.p, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, st));
    SD_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> base((size_t)M + 1, 0);
    for (int m = 0; m < M; ++m) {
        const int64_t n = c.h_counts.p[m];
        if (n > sd::SPLIT_NMAX) {
            set_err(errbuf, errlen, std::string(who) + ": " + sp_name(j, m) + " has " + std::to_string(n) + " member rows, the cap is " +
                                        std::to_string(sd::SPLIT_NMAX) + " (SPLIT_NMAX)");
            return SD_ERR_PARAM;
        }
        j.info[4 * m] = n;
        base[(size_t)m + 1] = base[(size_t)m] + n;
    }
    for (int m = 0; m < M; ++m) c.h_counts.p[m] = (int32_t)base[(size_t)m];   // the cursors of group_scatter: where a group begins
    c.h_counts.p[M] = 0;
    SD_HIP(hipMemcpyAsync(c.mcount.p, c.h_counts.p, sizeof(int32_t) * ((size_t)M + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sd::sd_split_members, dim3(sp_grid(j.n_rows)), dim3(sd::SP_T), 0, st, src, j.n_rows, c.mcount.p, c.order.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipStreamSynchronize(st));   // (h_counts was read)
    int64_t at = 0;
    for (int m = 0; m < M; ++m) {
        const int64_t n = base[(size_t)m + 1] - base[(size_t)m];
        const int L = j.mono_len[m], K = j.K;
        j.cen_off[m] = at;
        if (n == 0) continue;
        int64_t* info = j.info + 4 * m;
        if ((int64_t)K * L > j.centres_cap - at) {
            set_err(errbuf, errlen, std::string(who) + ": the centre buffer of " + std::to_string(j.centres_cap) + " bytes is too small for " + sp_name(j, m));
            return SD_ERR_PARAM;
        }
        const int32_t* order = c.order.p + base[(size_t)m];
        SpDev d(c, st, j.rows, j.row_at, order, n, L);
        d.prep();
        int64_t inf[3];
        sd::split_drive(d, n, j.radius[m], K, j.S, j.I, inf);
        const int k = (int)inf[0];
        info[1] = inf[0]; info[2] = inf[1]; info[3] = inf[2];
        hipLaunchKernelGGL(sd::sd_split_out, dim3(sp_grid(n)), dim3(sd::SP_T), 0, st, d.rowid, d.cur->asg, d.cur->d1, d.cur->d2, n, j.sub, j.d1, j.d2);
        hipLaunchKernelGGL(sd::sd_split_cen_out, dim3(sp_grid((int64_t)k * L)), dim3(sd::SP_T), 0, st, d.cur->cen, k, L, j.centres + at);
        SD_HIP(hipGetLastError());
        SD_HIP(hipMemcpyAsync(c.h_stat.p, d.cur->stat, sizeof(sd::SplitStat), hipMemcpyDeviceToHost, st));   // once per monomer: the sizes
        SD_HIP(hipStreamSynchronize(st));
        for (int x = 0; x < k; ++x) j.sizes[(size_t)m * K + x] = (int32_t)c.h_stat.p->sizes[x];
        at += (int64_t)k * L;
        if (bench) sp_bench(d, k, *bench);
    }
    j.cen_off[M] = at;
    for (int m = M - 1; m >= 0; --m)
        if (base[(size_t)m + 1] == base[(size_t)m]) j.cen_off[m] = j.cen_off[m + 1];   // (a monomer without members: an empty stretch)
    return SD_OK;
}

// a symbol matrix as the one monomer of a job on `device`: uploaded, split by the kernels, the results back
int sp_matrix_dev(const char* who, const uint8_t* sym, int64_t n, int64_t pitch, int32_t L, int32_t R, int32_t K, int32_t S, int32_t I, int32_t device,
                  int32_t threads, uint8_t* centres, int32_t* asg, int32_t* d1, int32_t* d2, int32_t* sizes, int64_t* info, char* errbuf, size_t errlen,
                  const SpBench* bench) {
    int rc = sp_params(who, n, pitch, L, R, K, S, I, errbuf, errlen);
    if (rc) return rc;
    if (!sizes || !info || (n > 0 && (!sym || !centres || !asg || !d1 || !d2))) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    if (L > sd::SPLIT_LMAX || n == 0) {   // a monomer the kernels do not take: the host form, the same results
        sp_host_core(sym, n, pitch, L, R, K, S, I, std::max(1, threads), centres, asg, d1, d2, sizes, info);
        return SD_OK;
    }
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    try {
        DeviceScope on(device);
        SpCtx& c = device_ctx<SpCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        OwnedStream st;
        std::vector<int64_t> at((size_t)n);
        for (int64_t i = 0; i < n; ++i) at[(size_t)i] = i * pitch;
        c.up_rows.alloc((size_t)n * pitch);
        c.up_at.alloc((size_t)n);
        c.up_status.alloc((size_t)n);
        c.up_fmono.alloc((size_t)n);
        c.o_sub.alloc((size_t)n);
        c.o_d1.alloc((size_t)n);
        c.o_d2.alloc((size_t)n);
        c.cen_sym.alloc((size_t)K * L);
        SD_HIP(hipMemcpyAsync(c.up_rows.p, sym, (size_t)n * pitch, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.up_at.p, at.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemsetAsync(c.up_status.p, 1, (size_t)n, st));
        SD_HIP(hipMemsetAsync(c.up_fmono.p, 0, sizeof(int32_t) * (size_t)n, st));
        int64_t cen_off[2], inf[4];
        const SpJob j{c.up_rows.p, c.up_at.p, c.up_status.p, c.up_fmono.p, n, &L, &R, nullptr, 1, K, S, I,
                      c.o_sub.p, c.o_d1.p, c.o_d2.p, c.cen_sym.p, (int64_t)K * L, cen_off, sizes, inf};
        rc = sp_run(who, c, st, j, bench, errbuf, errlen);
        if (rc == SD_OK) {
            SD_HIP(hipMemcpyAsync(asg, c.o_sub.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(d1, c.o_d1.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(d2, c.o_d2.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(centres, c.cen_sym.p, (size_t)inf[1] * L, hipMemcpyDeviceToHost, st));
        }
        SD_HIP(hipStreamSynchronize(st));
        info[0] = inf[1]; info[1] = inf[2]; info[2] = inf[3]; info[3] = 1;
        return rc;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
}

int sp_job_params(const char* who, int64_t n_rows, const int32_t* mono_len, const int32_t* radius, int32_t n_mono, int32_t K, int32_t S, int32_t I,
                  char* errbuf, size_t errlen) {
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 31) || n_mono < 0 || (n_mono > 0 && (!mono_len || !radius))) {
        set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(n_rows) + " rows (fewer than 2^31), " + std::to_string(n_mono) + " monomers");
        return SD_ERR_PARAM;
    }
    for (int m = 0; m < n_mono; ++m) {
        const int rc = sp_params(who, 0, mono_len[m], mono_len[m], radius[m], K, S, I, errbuf, errlen);
        if (rc) return rc;
    }
    if (n_mono == 0) return sp_params(who, 0, 1, 1, 1, K, S, I, errbuf, errlen);
    return SD_OK;
}

}  // namespace
}  // namespace sdi

extern "C" {

int sd_split_host(const uint8_t* sym, int64_t n, int64_t pitch, int32_t L, int32_t R, int32_t K, int32_t S, int32_t I, int32_t threads,
                  uint8_t* centres, int32_t* assign, int32_t* d1, int32_t* d2, int32_t* sizes, int64_t info[4], char* errbuf, size_t errlen) try {
    static const char* who = "sd_split_host";
    const int rc = sp_params(who, n, pitch, L, R, K, S, I, errbuf, errlen);
    if (rc) return rc;
    if (!sizes || !info || (n > 0 && (!sym || !centres || !assign || !d1 || !d2))) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    sp_host_core(sym, n, pitch, L, R, K, S, I, std::max(1, threads), centres, assign, d1, d2, sizes, info);
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_split_dev(const uint8_t* sym, int64_t n, int64_t pitch, int32_t L, int32_t R, int32_t K, int32_t S, int32_t I, int32_t device,
                 int32_t threads, uint8_t* centres, int32_t* assign, int32_t* d1, int32_t* d2, int32_t* sizes, int64_t info[4], char* errbuf,
                 size_t errlen) try {
    return sp_matrix_dev("sd_split_dev", sym, n, pitch, L, R, K, S, I, device, threads, centres, assign, d1, d2, sizes, info, errbuf, errlen, nullptr);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_split_final_host(const uint8_t* rows, const int64_t* row_at, const uint8_t* status, const int32_t* fmono, int64_t n_rows,
                        const int32_t* mono_len, const int32_t* radius, int32_t n_mono, int32_t K, int32_t S, int32_t I, int32_t threads,
                        int32_t* sub, int32_t* d1, int32_t* d2, uint8_t* centres, int64_t centres_cap, int64_t* cen_off, int32_t* sizes,
                        int64_t* info, char* errbuf, size_t errlen) try {
    static const char* who = "sd_split_final_host";
    const int rc = sp_job_params(who, n_rows, mono_len, radius, n_mono, K, S, I, errbuf, errlen);
    if (rc) return rc;
    if (!cen_off || (n_mono > 0 && (!sizes || !info)) || (n_rows > 0 && (!rows || !row_at || !status || !fmono || !sub || !d1 || !d2))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    for (int64_t i = 0; i < n_rows; ++i) sub[i] = d1[i] = d2[i] = -1;
    std::vector<std::vector<int32_t>> mem((size_t)n_mono);
    for (int64_t i = 0; i < n_rows; ++i)
        if (status[i] == 1 && fmono[i] >= 0 && fmono[i] < n_mono) mem[(size_t)fmono[i]].push_back((int32_t)i);
    int64_t at = 0;
    for (int m = 0; m < n_mono; ++m) {
        const std::vector<int32_t>& r = mem[(size_t)m];
        const int64_t n = (int64_t)r.size();
        const int L = mono_len[m];
        cen_off[m] = at;
        int64_t* inf = info + 4 * m;
        inf[0] = n; inf[1] = inf[2] = inf[3] = 0;
        for (int c = 0; c < K; ++c) sizes[(size_t)m * K + c] = 0;
        if (n == 0) continue;
        if (n > sd::SPLIT_NMAX) {
            set_err(errbuf, errlen, std::string(who) + ": monomer " + std::to_string(m) + " has " + std::to_string(n) + " member rows, the cap is " +
                                        std::to_string(sd::SPLIT_NMAX) + " (SPLIT_NMAX)");
            return SD_ERR_PARAM;
        }
        if ((int64_t)K * L > centres_cap - at || !centres) {
            set_err(errbuf, errlen, std::string(who) + ": the centre buffer of " + std::to_string(centres_cap) + " bytes is too small for monomer " + std::to_string(m));
            return SD_ERR_PARAM;
        }
        std::vector<uint8_t> sym((size_t)n * L), cen((size_t)K * L, 0);
        for (int64_t i = 0; i < n; ++i) std::memcpy(&sym[(size_t)i * L], rows + row_at[r[(size_t)i]], (size_t)L);
        std::vector<int32_t> a((size_t)n), x1((size_t)n), x2((size_t)n);
        int64_t got[4];
        sp_host_core(sym.data(), n, L, L, radius[m], K, S, I, std::max(1, threads), cen.data(), a.data(), x1.data(), x2.data(), sizes + (size_t)m * K, got);
        inf[1] = got[0]; inf[2] = got[1]; inf[3] = got[2];
        for (int64_t i = 0; i < n; ++i) {
            sub[r[(size_t)i]] = a[(size_t)i];
            d1[r[(size_t)i]] = x1[(size_t)i];
            d2[r[(size_t)i]] = x2[(size_t)i];
        }
        std::memcpy(centres + at, cen.data(), (size_t)got[0] * L);
        at += got[0] * L;
    }
    cen_off[n_mono] = at;
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_split_info(int64_t info[4]) {
    info[0] = sd::SPLIT_KMAX;
    info[1] = sd::SPLIT_LMAX;
    info[2] = sd::SPLIT_NMAX;
    info[3] = g_sp_launches.load();
}

int sd_split_kernel_bench(const uint8_t* sym, int64_t n, int64_t pitch, int32_t L, int32_t R, int32_t K, int32_t S, int32_t I, int32_t device,
                          int32_t warmup, int32_t reps, float* ms_prep, float* ms_assign, float* ms_modes, int64_t info[4]) try {
    if (warmup < 0 || reps < 1 || !ms_prep || !ms_assign || !ms_modes || !info || n < 1 || L > sd::SPLIT_LMAX) return SD_ERR_PARAM;
    std::vector<uint8_t> cen((size_t)std::max(K, 1) * (size_t)std::max(L, 1));
    std::vector<int32_t> a((size_t)n), x1((size_t)n), x2((size_t)n), sizes((size_t)std::max(K, 1));
    const SpBench b{warmup, reps, ms_prep, ms_assign, ms_modes};
    const int64_t before = g_sp_launches.load();
    const int rc = sp_matrix_dev("sd_split_kernel_bench", sym, n, pitch, L, R, K, S, I, device, 1, cen.data(), a.data(), x1.data(), x2.data(), sizes.data(),
                                 info, nullptr, 0, &b);
    info[3] = g_sp_launches.load() - before;
    return rc;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
