// sd_lags.hip -- identity of every row of the final TSV to its next D neighbours in the same read (--lags): block against
// block, on the device.  sd_lags.hpp says which pairs exist and who aligns them; this file holds the kernels, the host
// form and the C-ABI (include/sd_hip.h: sd_lag_*).
//
// Every other alignment of this library is a block against a MONOMER: the monomer's match masks are built once on the host
// (nw_build_masks) and shared by all lanes.  Here both sides differ per pair, so a lane builds the masks of its own target
// from the read text in HBM -- 5 symbols x K 64-bit words, top-aligned exactly as nw_build_masks lays them out, so that
// nw_pair's invariants hold (carry at bit 63, padding rows below) -- keeps them in LDS, lane-interleaved (word index major,
// lane minor: a wave's read of "word b of symbol s" is 64 consecutive 8-byte slots, no bank conflict), and runs the
// existing walk nw_pair<K, NwQueryAscii, NwNoSink, LS = T> on them.
//   sd_lag_rows      (device-resident form) one lane per final row: its segment (final_seg_first / final_seg_len) and read
//   sd_lag_plan      one lane per (row, lag): partner or not, who aligns the pair, the word class of its target; per class
//                    the number of pairs and the longest query (workgroup histogram in LDS, then global adds)
//   group_scan / sd_lag_scatter   the lane kernel's pairs -> order[], grouped by word class (sd_group_dev.hpp: the
//                    grouping of the device profiles); the pairs it does not take -> a compact list of pair ids
//   sd_lag_pairs<K>  one lane per pair of class K; 40 K bytes of LDS per lane.  The sums n, M, C per (read, lag) are reduced
//                    in a small table in LDS per workgroup and flushed with 64-bit global atomics (integers: any order)
// Workgroup: 256 lanes for K <= 4 (40 KB of masks at K = 4: three workgroups per CU, the register budget of the identity
// kernel), 128 lanes for K = 6 and 8 (30 / 40 KB: four / three workgroups per CU, where 256 lanes -- 60 / 80 KB -- would
// leave two / one).
#include <algorithm>
#include <cstring>
#include <memory>

#include "sd_final_ws.hpp"
#include "sd_group_dev.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"
#include "sd_lags.hpp"
#include "sd_nw_kernel.hpp"

namespace sd {

constexpr int LAG_T = 256;           // threads per workgroup of the row / plan / scatter kernels
constexpr int LAG_SLOTS = 128;       // (read, lag) entries of a workgroup's table of sums
constexpr uint8_t LAG_CLS_HOST = 7;  // cls[]: 0 none, 1 + word class, 7 = a pair the lane kernel does not take
// sum[]: [0, 6) pairs per word class, [6] (the scan's end), then
enum { LAG_SUM_HOST = 7, LAG_SUM_NONE = 8, LAG_SUM_QMAX = 9, LAG_SUM_BAD = 15, LAG_SUM_FAIL = 16, LAG_SUM_N = 17 };

template <int K>
__host__ __device__ constexpr int lag_threads() { return K <= 4 ? 256 : 128; }

struct LagRowsArgs {
    const sd_final_row* rows;
    int64_t n;
    const int64_t* rlen;
    const int64_t* toff;
    int n_reads;
    int64_t* seg_start;
    int32_t* seg_len;
    int32_t* seg_read;
    int32_t* sum;
};

__global__ __launch_bounds__(LAG_T) void sd_lag_rows(LagRowsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * LAG_T + threadIdx.x;
    if (i >= a.n) return;
    const sd_final_row x = a.rows[i];
    if (x.read < 0 || x.read >= a.n_reads) {   // (a row of no read: no pair, counted)
        atomicAdd(&a.sum[LAG_SUM_BAD], 1);
        a.seg_start[i] = 0;
        a.seg_len[i] = 0;
        a.seg_read[i] = -1 - (int32_t)(i & 1);   // never equal to a neighbour's
        return;
    }
    const int64_t rl = a.rlen[x.read];
    a.seg_start[i] = a.toff[x.read] + final_seg_first(x.start, rl);
    a.seg_len[i] = (int32_t)final_seg_len(x.start, x.end, rl);
    a.seg_read[i] = x.read;
}

__global__ __launch_bounds__(LAG_T) void sd_lag_plan(const int32_t* __restrict__ seg_len, const int32_t* __restrict__ seg_read,
                                                     int64_t n_seg, int D, uint8_t* __restrict__ cls, int32_t* __restrict__ dist,
                                                     int32_t* __restrict__ matches, int32_t* __restrict__ sum) {
    __shared__ int hist[LAG_SUM_N];
    if (threadIdx.x < LAG_SUM_N) hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * LAG_T + threadIdx.x;
    if (p < n_seg * D) {
        const int64_t s = p / D, t = s + (p - s * D) + 1;
        uint8_t c = 0;
        int32_t d = -1;
        uint8_t who = LAG_NONE;
        if (t < n_seg && seg_read[t] == seg_read[s] && seg_read[s] >= 0) who = lag_pair_class(seg_len[s], seg_len[t]);
        if (who == LAG_DEV) {
            const int k = lag_class_of_words(lag_words(seg_len[t]));
            c = (uint8_t)(1 + k);
            atomicAdd(&hist[k], 1);
            atomicMax(&hist[LAG_SUM_QMAX + k], seg_len[s]);
        } else if (who == LAG_HOST) {
            c = LAG_CLS_HOST;
            d = -2;
            atomicAdd(&hist[LAG_SUM_HOST], 1);
        } else {
            atomicAdd(&hist[LAG_SUM_NONE], 1);
        }
        cls[p] = c;
        dist[p] = d;      // (a lane-kernel pair: overwritten by its walk)
        matches[p] = 0;
    }
    __syncthreads();
    if (threadIdx.x < LAG_SUM_N && hist[threadIdx.x]) {
        if (threadIdx.x >= LAG_SUM_QMAX && threadIdx.x < LAG_SUM_QMAX + LAG_CLASSES) atomicMax(&sum[threadIdx.x], hist[threadIdx.x]);
        else atomicAdd(&sum[threadIdx.x], hist[threadIdx.x]);
    }
}

// the pairs of a plan as group_scatter reads them: the lane kernel's by word class, the others aside as pair ids
struct LagSrc {
    const uint8_t* cls;
    int32_t* hlist;
    __device__ int kind(int64_t p) const { return cls[p] == 0 ? GROUP_OUT : cls[p] == LAG_CLS_HOST ? GROUP_ASIDE : GROUP_IN; }
    __device__ int group(int64_t p) const { return cls[p] - 1; }
    __device__ void aside(int64_t p, int64_t pos) const { hlist[pos] = (int32_t)p; }
};

__global__ __launch_bounds__(GROUP_T) void sd_lag_scatter(const uint8_t* __restrict__ cls, int64_t n_pairs, int32_t* __restrict__ cursor,
                                                          int32_t* __restrict__ order, int32_t* __restrict__ hlist) {
    group_scatter(LagSrc{cls, hlist}, n_pairs, n_pairs, LAG_CLASSES, cursor, order);
}

// {n, M, C} of one pair into the workgroup's table; a key that finds no slot within 8 probes goes to HBM directly
__device__ __forceinline__ void lag_sum_add(unsigned long long* skey, unsigned long long* sval, unsigned long long key, int m, int c,
                                            unsigned long long* __restrict__ gsums) {
    const unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 40);
    for (int probe = 0; probe < 8; ++probe) {
        const unsigned slot = (h + probe) & (LAG_SLOTS - 1);
        const unsigned long long prev = atomicCAS(&skey[slot], ~0ull, key);
        if (prev == ~0ull || prev == key) {
            atomicAdd(&sval[slot * 3], 1ull);
            atomicAdd(&sval[slot * 3 + 1], (unsigned long long)m);
            atomicAdd(&sval[slot * 3 + 2], (unsigned long long)c);
            return;
        }
    }
    atomicAdd(gsums + key * 3, 1ull);
    atomicAdd(gsums + key * 3 + 1, (unsigned long long)m);
    atomicAdd(gsums + key * 3 + 2, (unsigned long long)c);
}

// order[0 .. count): pair ids p = s * D + (d - 1) whose target (row s + d) has K words.  ck: gridDim.x * T lanes x cap
// checkpoint slots x K x 16 B, planar as nw_pair wants them.  gsums may be null (bench: the walk without its reduction).
template <int K>
__global__ __launch_bounds__(lag_threads<K>(), K <= 4 ? 3 : 1) void sd_lag_pairs(
    const uint8_t* __restrict__ text, const int64_t* __restrict__ seg_start, const int32_t* __restrict__ seg_len,
    const int32_t* __restrict__ seg_read, const int32_t* __restrict__ order, int count, int D, int cap, uint32_t* __restrict__ ck,
    int32_t* __restrict__ dist, int32_t* __restrict__ matches, unsigned long long* __restrict__ gsums, int* __restrict__ fails) {
    constexpr int T = lag_threads<K>();
    __shared__ uint2 masks[5 * K * T];
    __shared__ unsigned long long skey[LAG_SLOTS], sval[LAG_SLOTS * 3];
    for (int i = threadIdx.x; i < LAG_SLOTS; i += T) { skey[i] = ~0ull; sval[3 * i] = 0; sval[3 * i + 1] = 0; sval[3 * i + 2] = 0; }
    __syncthreads();
    uint2* mine = masks + threadIdx.x;   // word (sym * K + b) of this lane at mine[(sym * K + b) * T]
    uint32_t* ckl = ck + (size_t)blockIdx.x * (size_t)cap * K * 4 * T + threadIdx.x;
    for (int i = blockIdx.x * T + threadIdx.x; i < count; i += gridDim.x * T) {
        const int p = order[i];
        const int s = p / D, d1 = p - s * D, t = s + d1 + 1;
        const int ql = seg_len[s], tl = seg_len[t];
        // the target's match masks: template symbol k at bit 64 K - tl + k (nw_build_masks), a 32-bit half at a time
        const int pad = 64 * K - tl;
        NwQueryAscii tq{text, seg_start[t]};
#pragma unroll 1
        for (int h = 0; h < 2 * K; ++h) {
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
            const int k0 = 32 * h - pad;   // the template symbol of the half's bit 0
            for (int j = k0 < 0 ? -k0 : 0; j < 32; ++j) {
                const int c = tq.code(k0 + j);
                const uint32_t bit = 1u << j;
                a0 |= c == 0 ? bit : 0u;
                a1 |= c == 1 ? bit : 0u;
                a2 |= c == 2 ? bit : 0u;
                a3 |= c == 3 ? bit : 0u;
                a4 |= c == 4 ? bit : 0u;
            }
            uint32_t* w = reinterpret_cast<uint32_t*>(mine + (h >> 1) * T) + (h & 1);
            w[0] = a0;
            w[2 * K * T] = a1;       // (a symbol's K words: K * T slots of two dwords)
            w[4 * K * T] = a2;
            w[6 * K * T] = a3;
            w[8 * K * T] = a4;
        }
        NwQueryAscii q{text, seg_start[s]};
        int dd = -2, mm = 0;
        const bool ok = nw_pair<K, NwQueryAscii, NwNoSink, T>(q, ql, mine, tl, false, ckl, nullptr, (size_t)T, cap, dd, mm);
        if (!ok) { atomicAdd(fails, 1); dd = -2; mm = 0; }   // (cannot happen: the slots are sized by the longest query)
        dist[p] = dd;
        matches[p] = mm;
        if (ok && gsums) lag_sum_add(skey, sval, (unsigned long long)((int64_t)seg_read[s] * D + d1), mm, dd + mm, gsums);
    }
    __syncthreads();
    if (gsums)
        for (int i = threadIdx.x; i < LAG_SLOTS; i += T) {
            const unsigned long long key = skey[i];
            if (key == ~0ull) continue;
            atomicAdd(gsums + key * 3, sval[3 * i]);
            atomicAdd(gsums + key * 3 + 1, sval[3 * i + 1]);
            atomicAdd(gsums + key * 3 + 2, sval[3 * i + 2]);
        }
}

}  // namespace sd

namespace sdi {
namespace {

// Per device, kept between calls (sd_job_dev.hpp: DevWork): the text, the plan, the grouping and the checkpoints.
struct LagCtx : DevWork, FinalText {
    DevBuf<uint8_t> cls, ck;
    DevBuf<int64_t> seg_start;
    DevBuf<int32_t> seg_len, seg_read, order, hlist, sum, base, cursor;
    PinBuf<int32_t> h_sum;
    hipEvent_t ev_plan = nullptr;
};

inline unsigned lag_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + sd::LAG_T - 1) / sd::LAG_T); }

// plan + grouping on st over the segments in c (seg_len, seg_read); the summary on its way to c.h_sum, ev_plan recorded
void lag_plan(LagCtx& c, hipStream_t st, int64_t n_seg, int D, int32_t* d_dist, int32_t* d_matches, bool clear_sum) {
    const int64_t n_pairs = n_seg * D;
    c.cls.alloc((size_t)n_pairs);
    c.order.alloc((size_t)n_pairs);
    c.hlist.alloc((size_t)n_pairs);
    c.base.alloc(sd::LAG_CLASSES + 1);
    c.cursor.alloc(sd::LAG_CLASSES + 1);
    c.h_sum.alloc(sd::LAG_SUM_N);
    if (clear_sum) SD_HIP(hipMemsetAsync(c.sum.p, 0, sd::LAG_SUM_N * sizeof(int32_t), st));
    if (n_pairs > 0)
        hipLaunchKernelGGL(sd::sd_lag_plan, dim3(lag_grid(n_pairs)), dim3(sd::LAG_T), 0, st, c.seg_len.p, c.seg_read.p, n_seg, D, c.cls.p,
                           d_dist, d_matches, c.sum.p);
    group_scan(st, c.sum.p, sd::LAG_CLASSES, c.base.p, c.cursor.p);
    if (n_pairs > 0)
        hipLaunchKernelGGL(sd::sd_lag_scatter, dim3(lag_grid(n_pairs)), dim3(sd::GROUP_T), 0, st, c.cls.p, n_pairs, c.cursor.p, c.order.p,
                           c.hlist.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipMemcpyAsync(c.h_sum.p, c.sum.p, sd::LAG_SUM_N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ensure_event(c.ev_plan, hipEventDisableTiming);
    SD_HIP(hipEventRecord(c.ev_plan, st));
}

struct LagLaunch { int K, grid, cap, first, count; };

// the launches of the lane kernel from the summary the host has seen; grows c.ck (no walk is in flight: settle())
std::vector<LagLaunch> lag_launches(LagCtx& c) {
    std::vector<LagLaunch> out;
    const int32_t* hs = c.h_sum.p;
    size_t need = 0;
    int first = 0;
    for (int k = 0; k < sd::LAG_CLASSES; ++k) {
        const int count = hs[k];
        if (count > 0) {
            const int K = sd::lag_words_of_class(k), S = sd::nw_block_cols(K), T = K <= 4 ? 256 : 128;
            const int cap = std::max(1, (std::max(1, (int)hs[sd::LAG_SUM_QMAX + k]) + S - 1) / S);
            const size_t lane_bytes = (size_t)cap * K * 16;
            const int per_cu = K <= 4 ? 3 : K == 6 ? 4 : 3;
            int64_t grid = std::min<int64_t>((int64_t)c.n_cu * per_cu, ((int64_t)count + T - 1) / T);
            grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(((size_t)1 << 30) / (lane_bytes * T))));
            out.push_back(LagLaunch{K, (int)grid, cap, first, count});
            need = std::max(need, lane_bytes * T * (size_t)grid);
        }
        first += count;
    }
    c.ck.alloc(need);
    return out;
}

void lag_walk(LagCtx& c, hipStream_t st, const LagLaunch& L, int D, int32_t* d_dist, int32_t* d_matches, int64_t* d_sums) {
    with_words(L.K, [&](auto words) {
        constexpr int K = decltype(words)::value;
        hipLaunchKernelGGL(sd::sd_lag_pairs<K>, dim3(L.grid), dim3(sd::lag_threads<K>()), 0, st, c.text.p, c.seg_start.p, c.seg_len.p,
                           c.seg_read.p, c.order.p + L.first, L.count, D, L.cap, reinterpret_cast<uint32_t*>(c.ck.p), d_dist, d_matches,
                           reinterpret_cast<unsigned long long*>(d_sums), c.sum.p + sd::LAG_SUM_FAIL);
    });
    SD_HIP(hipGetLastError());
}

// ---- the host form --------------------------------------------------------------------------------------------------
// pairs `ids` (null: every pair) of the segments (start, len, group) of `text`; dist / matches of the others untouched
int lag_host_pairs(const char* text, const int64_t* seg_start, const int32_t* seg_len, const int32_t* seg_read, int64_t n_seg, int D,
                   const int32_t* ids, int64_t n_ids, int threads, int32_t* dist, int32_t* matches) {
    std::vector<int64_t> at;
    std::vector<const char*> q, t;
    std::vector<int32_t> ql, tl;
    auto take = [&](int64_t p) {
        const int64_t s = p / D, x = s + (p - s * D) + 1;
        if (x >= n_seg || seg_read[x] != seg_read[s] || seg_read[s] < 0) { dist[p] = -1; matches[p] = 0; return; }
        at.push_back(p);
        q.push_back(text + seg_start[s]);
        ql.push_back(seg_len[s]);
        t.push_back(text + seg_start[x]);
        tl.push_back(seg_len[x]);
    };
    if (ids) for (int64_t i = 0; i < n_ids; ++i) take(ids[i]);
    else for (int64_t p = 0; p < n_seg * D; ++p) take(p);
    const int64_t n = (int64_t)at.size();
    if (n == 0) return SD_OK;
    std::vector<int32_t> hd((size_t)n), hm((size_t)n), hc((size_t)n);
    const int rc = sd_nw_identity_batch(q.data(), ql.data(), t.data(), tl.data(), n, std::max(1, threads), hd.data(), hm.data(), hc.data());
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i) { dist[at[(size_t)i]] = hd[(size_t)i]; matches[at[(size_t)i]] = hm[(size_t)i]; }
    return SD_OK;
}

void lag_host_sums(const int32_t* seg_read, int64_t n_seg, int D, const int32_t* ids, int64_t n_ids, const int32_t* dist,
                   const int32_t* matches, int64_t* sums) {
    auto add = [&](int64_t p) {
        if (dist[p] < 0) return;
        const int64_t s = p / D;
        int64_t* o = sums + ((int64_t)seg_read[s] * D + (p - s * D)) * 3;
        o[0] += 1;
        o[1] += matches[p];
        o[2] += (int64_t)dist[p] + matches[p];
    };
    if (ids) for (int64_t i = 0; i < n_ids; ++i) add(ids[i]);
    else for (int64_t p = 0; p < n_seg * D; ++p) add(p);
}

// the checked segments of the two segment calls: start (in seq + lo) / len / group per segment, sums zeroed
int lag_segment_args(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg, const int64_t* group_off,
                     int32_t n_groups, int32_t D, int32_t* dist, int32_t* matches, int64_t* sums,
                     std::vector<int64_t>& st, std::vector<int32_t>& ln, std::vector<int32_t>& rd, int64_t& lo, int64_t& hi) {
    if (!sd::lag_d_ok(D) || (n_seg > 0 && (!dist || !matches))) return SD_ERR_PARAM;
    if (group_off && n_groups >= 0)
        for (int32_t g = 0; g < n_groups; ++g)
            if (group_off[g + 1] < group_off[g]) return SD_ERR_PARAM;
    // (no errbuf in the C-ABI of these calls: the codes alone)
    const int64_t limit = (((int64_t)1 << 31) + D - 1) / D;
    const int rc = segment_args("sd_lag_segments", seq, seqlen, starts, ends, n_seg, group_off, n_groups, sums, limit,
                                "segments x D must stay below 2^31", st, ln, &rd, lo, hi, nullptr, 0);
    if (rc) return rc;
    std::memset(sums, 0, sizeof(int64_t) * 3 * (size_t)n_groups * (size_t)D);
    return SD_OK;
}

}  // namespace
}  // namespace sdi

extern "C" {

int sd_lag_segments(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg, const int64_t* group_off,
                    int32_t n_groups, int32_t D, int32_t threads, int32_t* dist, int32_t* matches, int64_t* sums) try {
    std::vector<int64_t> st;
    std::vector<int32_t> ln, rd;
    int64_t lo = 0, hi = 0;
    int rc = lag_segment_args(seq, seqlen, starts, ends, n_seg, group_off, n_groups, D, dist, matches, sums, st, ln, rd, lo, hi);
    if (rc || n_seg == 0) return rc;
    rc = lag_host_pairs(seq + lo, st.data(), ln.data(), rd.data(), n_seg, D, nullptr, 0, threads, dist, matches);
    if (rc) return rc;
    lag_host_sums(rd.data(), n_seg, D, nullptr, 0, dist, matches, sums);
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

// bench != null: sd_lag_kernel_bench's timing of the stages instead of one plain pass
struct sd_lag_bench {
    int warmup, reps;
    float *ms_group, *ms_pairs, *ms_walk, *ms_ident;
    int64_t* info;
};

static int lag_segments_dev(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                            const int64_t* group_off, int32_t n_groups, int32_t D, int32_t device, int32_t threads, int32_t* dist,
                            int32_t* matches, int64_t* sums, const sd_lag_bench* bench) {
    std::vector<int64_t> sst;
    std::vector<int32_t> ln, rd;
    int64_t lo = 0, hi = 0;
    int rc = lag_segment_args(seq, seqlen, starts, ends, n_seg, group_off, n_groups, D, dist, matches, sums, sst, ln, rd, lo, hi);
    if (rc) return rc;
    if ((rc = device_check(device, nullptr, 0))) return rc;
    if (n_seg == 0) return SD_OK;
    const int64_t n_pairs = n_seg * D, text = hi - lo;
    const char* tx = seq + lo;
    if (!text_is_acgtn(tx, text)) {   // a byte the lane kernel does not read: every pair is the host's
        if (bench) return SD_ERR_UNSUPPORTED;
        rc = lag_host_pairs(tx, sst.data(), ln.data(), rd.data(), n_seg, D, nullptr, 0, threads, dist, matches);
        if (rc == SD_OK) lag_host_sums(rd.data(), n_seg, D, nullptr, 0, dist, matches, sums);
        return rc;
    }
    try {
        DeviceScope on(device);
        LagCtx& c = device_ctx<LagCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        OwnedStream st;
        DevBuf<int32_t> d_dist, d_matches;
        DevBuf<int64_t> d_sums;
        const size_t n_sums = (size_t)n_groups * D * 3;
        c.text.alloc((size_t)text + 8);
        c.seg_start.alloc((size_t)n_seg);
        c.seg_len.alloc((size_t)n_seg);
        c.seg_read.alloc((size_t)n_seg);
        c.sum.alloc(sd::LAG_SUM_N);
        d_dist.alloc((size_t)n_pairs);
        d_matches.alloc((size_t)n_pairs);
        d_sums.alloc(n_sums);
        SD_HIP(hipMemsetAsync(c.text.p + text, 0, 8, st));
        if (text) SD_HIP(hipMemcpyAsync(c.text.p, tx, (size_t)text, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.seg_start.p, sst.data(), sizeof(int64_t) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.seg_len.p, ln.data(), sizeof(int32_t) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.seg_read.p, rd.data(), sizeof(int32_t) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        StageClock clock;
        const auto clear_sums = [&]() { SD_HIP(hipMemsetAsync(d_sums.p, 0, sizeof(int64_t) * std::max<size_t>(n_sums, 1), st)); };
        clear_sums();
        const auto plan = [&]() { lag_plan(c, st, n_seg, D, d_dist.p, d_matches.p, true); };   // plan, scan and scatter
        if (bench) clock.time(st, bench->warmup, bench->reps, bench->ms_group, plan);
        else plan();
        SD_HIP(hipEventSynchronize(c.ev_plan));
        const std::vector<LagLaunch> launches = lag_launches(c);
        const int64_t nh = c.h_sum.p[sd::LAG_SUM_HOST];
        std::vector<int32_t> hl((size_t)nh);
        if (nh > 0) SD_HIP(hipMemcpy(hl.data(), c.hlist.p, sizeof(int32_t) * (size_t)nh, hipMemcpyDeviceToHost));   // (the stream is idle)
        if (bench) {
            int64_t nd = 0, Kmost = 0, cmost = -1;
            for (const LagLaunch& L : launches) { nd += L.count; if (L.count > cmost) { cmost = L.count; Kmost = L.K; } }
            if (nd == 0) return SD_ERR_UNSUPPORTED;
            for (int pass = 0; pass < 2; ++pass)   // with the reduction, then the walk alone
                clock.time(st, bench->warmup, bench->reps, pass == 0 ? bench->ms_pairs : bench->ms_walk, [&]() {
                    for (const LagLaunch& L : launches) lag_walk(c, st, L, D, d_dist.p, d_matches.p, pass == 0 ? d_sums.p : nullptr);
                }, clear_sums);
            // the yardstick: the light identity kernel (sd_nw_pairs: one template per segment) on as many pairs -- every
            // pair's query against the first target of the most frequent class as the one template, its masks in LDS
            int32_t first_p = 0, first_at = 0;
            for (const LagLaunch& L : launches) if (L.K == Kmost) first_at = L.first;
            SD_HIP(hipMemcpy(&first_p, c.order.p + first_at, sizeof(int32_t), hipMemcpyDeviceToHost));
            const int64_t ts = first_p / D + (first_p % D) + 1;
            std::vector<std::string> tmpl(1, std::string(tx + sst[(size_t)ts], (size_t)ln[(size_t)ts]));
            std::vector<unsigned long long> peq;
            std::vector<int32_t> tl;
            const int K = (int)Kmost, S = sd::nw_block_cols(K);
            sd::nw_build_masks(tmpl, K, peq, tl);
            std::vector<int32_t> qidx;   // the queries of that class's pairs, then of the others up to nd
            {
                std::vector<int32_t> ord((size_t)nd);
                SD_HIP(hipMemcpy(ord.data(), c.order.p, sizeof(int32_t) * (size_t)nd, hipMemcpyDeviceToHost));
                int qmax = 1;
                for (int32_t p : ord) { qidx.push_back(p / D); qmax = std::max(qmax, (int)ln[(size_t)(p / D)]); }
                const int cap = std::max(1, (qmax + S - 1) / S);
                int64_t lanes = std::min<int64_t>((int64_t)c.n_cu * 3 * 256, (nd + 255) / 256 * 256);
                lanes = std::max<int64_t>(256, std::min<int64_t>(lanes, (int64_t)(((size_t)1 << 30) / ((size_t)cap * K * 16)) / 256 * 256));
                DevBuf<int32_t> d_idx, d_pt, d_tl, d_d, d_m;
                DevBuf<unsigned long long> d_peq;
                DevBuf<uint8_t> d_ck;
                DevBuf<int> d_ckpos;
                d_idx.upload(qidx);
                d_pt.upload(std::vector<int32_t>((size_t)n_seg, 0));
                d_tl.upload(tl);
                d_peq.upload(peq);
                d_d.alloc((size_t)n_seg);
                d_m.alloc((size_t)n_seg);
                d_ck.alloc((size_t)lanes * cap * K * 16);
                d_ckpos.alloc((size_t)lanes * cap);
                clock.time(st, bench->warmup, bench->reps, bench->ms_ident, [&]() {
                    sd::launch_nw_pairs(K, st, (int)(lanes / 256), c.text.p, c.seg_start.p, c.seg_len.p, d_idx.p, nd, 1, d_pt.p, d_peq.p, d_tl.p,
                                        0, cap, d_ck.p, d_ckpos.p, d_d.p, d_m.p);
                    SD_HIP(hipGetLastError());
                });
                SD_HIP(hipStreamSynchronize(st));
                bench->info[4] = cap;
                bench->info[5] = lanes / 256;
            }
            bench->info[0] = nd;
            bench->info[1] = nh;
            bench->info[2] = Kmost;
            bench->info[3] = cmost;
            for (const LagLaunch& L : launches) if (L.K == Kmost) { bench->info[6] = L.grid; bench->info[7] = L.cap; }
            clear_sums();
        }
        for (const LagLaunch& L : launches) lag_walk(c, st, L, D, d_dist.p, d_matches.p, d_sums.p);
        c.in_flight(st);
        // the host's pairs, under the kernel
        int hrc = SD_OK;
        if (nh > 0) {
            std::vector<int32_t> hd((size_t)n_pairs), hm((size_t)n_pairs);
            hrc = lag_host_pairs(tx, sst.data(), ln.data(), rd.data(), n_seg, D, hl.data(), nh, threads, hd.data(), hm.data());
            SD_HIP(hipMemcpyAsync(dist, d_dist.p, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(matches, d_matches.p, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(sums, d_sums.p, sizeof(int64_t) * n_sums, hipMemcpyDeviceToHost, st));
            SD_HIP(hipStreamSynchronize(st));
            if (hrc == SD_OK) {
                for (int64_t i = 0; i < nh; ++i) { dist[hl[(size_t)i]] = hd[(size_t)hl[(size_t)i]]; matches[hl[(size_t)i]] = hm[(size_t)hl[(size_t)i]]; }
                lag_host_sums(rd.data(), n_seg, D, hl.data(), nh, dist, matches, sums);
            }
        } else {
            SD_HIP(hipMemcpyAsync(dist, d_dist.p, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(matches, d_matches.p, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
            SD_HIP(hipMemcpyAsync(sums, d_sums.p, sizeof(int64_t) * n_sums, hipMemcpyDeviceToHost, st));
            SD_HIP(hipStreamSynchronize(st));
        }
        int32_t fails = 0;
        SD_HIP(hipMemcpy(&fails, c.sum.p + sd::LAG_SUM_FAIL, sizeof fails, hipMemcpyDeviceToHost));
        c.waited();
        if (hrc) return hrc;
        return fails ? SD_ERR_INTERNAL : SD_OK;
    } catch (const HipFail&) {
        return SD_ERR_HIP;
    }
}

int sd_lag_segments_dev(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                        const int64_t* group_off, int32_t n_groups, int32_t D, int32_t device, int32_t threads, int32_t* dist,
                        int32_t* matches, int64_t* sums) try {
    return lag_segments_dev(seq, seqlen, starts, ends, n_seg, group_off, n_groups, D, device, threads, dist, matches, sums, nullptr);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_lag_kernel_bench(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                        const int64_t* group_off, int32_t n_groups, int32_t D, int32_t device, int32_t warmup, int32_t reps,
                        float* ms_group, float* ms_pairs, float* ms_walk, float* ms_ident, int64_t info[8]) try {
    if (warmup < 0 || reps < 1 || !ms_group || !ms_pairs || !ms_walk || !ms_ident || !info) return SD_ERR_PARAM;
    if (n_seg <= 0 || !sd::lag_d_ok(D)) return SD_ERR_PARAM;
    std::vector<int32_t> dist((size_t)n_seg * D), matches((size_t)n_seg * D);
    std::vector<int64_t> sums((size_t)std::max(n_groups, 1) * D * 3);
    for (int i = 0; i < 8; ++i) info[i] = 0;
    const sd_lag_bench b{warmup, reps, ms_group, ms_pairs, ms_walk, ms_ident, info};
    return lag_segments_dev(seq, seqlen, starts, ends, n_seg, group_off, n_groups, D, device, 1, dist.data(), matches.data(), sums.data(), &b);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_lag_final_host(const sd_final_row* rows, int64_t n_rows, const char* text, const int64_t* read_off, const int64_t* read_lens,
                      int32_t n_reads, int32_t D, int32_t threads, int32_t* dist, int32_t* matches, int64_t* sums) try {
    if (!sd::lag_d_ok(D)) return SD_ERR_PARAM;
    if (n_rows < 0 || n_reads < 0 || !sums || (n_rows > 0 && (!rows || !dist || !matches)) || (n_reads > 0 && (!read_off || !read_lens)))
        return SD_ERR_PARAM;
    if (n_rows * (int64_t)D >= ((int64_t)1 << 31)) return SD_ERR_UNSUPPORTED;
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_off[r] < 0 || read_lens[r] < 0 || (read_lens[r] > 0 && !text)) return SD_ERR_PARAM;
    std::vector<int64_t> st((size_t)n_rows);
    std::vector<int32_t> ln((size_t)n_rows), rd((size_t)n_rows);
    for (int64_t i = 0; i < n_rows; ++i) {
        const int32_t r = rows[i].read;
        if (r < 0 || r >= n_reads) return SD_ERR_PARAM;
        st[(size_t)i] = read_off[r] + sd::final_seg_first(rows[i].start, read_lens[r]);
        ln[(size_t)i] = (int32_t)sd::final_seg_len(rows[i].start, rows[i].end, read_lens[r]);
        if (ln[(size_t)i] >= (1 << 27)) return SD_ERR_UNSUPPORTED;
        rd[(size_t)i] = r;
    }
    std::memset(sums, 0, sizeof(int64_t) * 3 * (size_t)n_reads * (size_t)D);
    if (n_rows == 0) return SD_OK;
    const int rc = lag_host_pairs(text, st.data(), ln.data(), rd.data(), n_rows, D, nullptr, 0, threads, dist, matches);
    if (rc) return rc;
    lag_host_sums(rd.data(), n_rows, D, nullptr, 0, dist, matches, sums);
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_lag_final_dev(const sd_final_row* d_rows, int64_t n_rows, const void* d_text, const int64_t* read_off, const int64_t* read_lens,
                     int32_t n_reads, int32_t D, int32_t device, void* hip_stream, int32_t* d_dist, int32_t* d_matches, int64_t* d_sums,
                     int64_t classes[3], char* errbuf, size_t errlen) try {
    static const char* who = "sd_lag_final_dev";
    if (!sd::lag_d_ok(D)) {
        set_err(errbuf, errlen, std::string(who) + ": D = " + std::to_string(D) + ", must be 1 .. " + std::to_string(sd::LAG_DMAX));
        return SD_ERR_PARAM;
    }
    if (n_rows < 0 || n_reads < 0 || (n_rows > 0 && (!d_rows || !d_dist || !d_matches)) || (n_reads > 0 && (!read_off || !read_lens || !d_sums))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    if (n_rows * (int64_t)D >= ((int64_t)1 << 31)) {
        set_err(errbuf, errlen, std::string(who) + ": rows x D must stay below 2^31");
        return SD_ERR_UNSUPPORTED;
    }
    int64_t text = 0;
    int rc = final_reads_args(who, d_text, read_off, read_lens, n_reads, text, errbuf, errlen);
    if (rc) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        if (n_rows > 0 && (rc = buffer_on_device(d_rows, device, who, "row", errbuf, errlen))) return rc;
        if (n_rows > 0 && (rc = buffer_on_device(d_dist, device, who, "distance", errbuf, errlen))) return rc;
        if (n_rows > 0 && (rc = buffer_on_device(d_matches, device, who, "match", errbuf, errlen))) return rc;
        if (n_reads > 0 && (rc = buffer_on_device(d_sums, device, who, "sum", errbuf, errlen))) return rc;
        if (text > 0 && (rc = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return rc;
        if (classes) { classes[0] = 0; classes[1] = 0; classes[2] = 0; }
        const size_t n_sums = (size_t)n_reads * D * 3;
        if (n_sums) SD_HIP(hipMemsetAsync(d_sums, 0, sizeof(int64_t) * n_sums, st));
        if (n_rows == 0) return SD_OK;
        LagCtx& c = device_ctx<LagCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();   // the previous call's kernels read the buffers this one overwrites
        c.seg_start.alloc((size_t)n_rows);
        c.seg_len.alloc((size_t)n_rows);
        c.seg_read.alloc((size_t)n_rows);
        c.sum.alloc(sd::LAG_SUM_N);
        final_text_gather(c, st, d_text, read_off, read_lens, n_reads, text);
        SD_HIP(hipMemsetAsync(c.sum.p, 0, sd::LAG_SUM_N * sizeof(int32_t), st));
        sd::LagRowsArgs a{d_rows, n_rows, c.rlen(), c.toff(), (int)n_reads, c.seg_start.p, c.seg_len.p, c.seg_read.p, c.sum.p};
        hipLaunchKernelGGL(sd::sd_lag_rows, dim3(lag_grid(n_rows)), dim3(sd::LAG_T), 0, st, a);
        SD_HIP(hipGetLastError());
        lag_plan(c, st, n_rows, D, d_dist, d_matches, false);
        c.in_flight(st);
        SD_HIP(hipEventSynchronize(c.ev_plan));   // the only wait: the class counts, which size the launches
        const int32_t* hs = c.h_sum.p;
        if (hs[sd::LAG_SUM_BAD]) {
            set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(hs[sd::LAG_SUM_BAD]) + " rows with a read index outside the reads");
            return SD_ERR_PARAM;
        }
        int64_t nd = 0;
        for (int k = 0; k < sd::LAG_CLASSES; ++k) nd += hs[k];
        if (classes) { classes[0] = hs[sd::LAG_SUM_NONE]; classes[1] = nd; classes[2] = hs[sd::LAG_SUM_HOST]; }
        c.settle();   // (nothing behind the plan yet: the checkpoints may grow)
        for (const LagLaunch& L : lag_launches(c)) lag_walk(c, st, L, D, d_dist, d_matches, d_sums);
        c.in_flight(st);
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_lag_identities(const int32_t* dist, const int32_t* matches, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = sd::lag_identity(dist[i], matches[i]);
}

void sd_lag_periods(const int64_t* sums, int64_t n_groups, int32_t D, int32_t* period, double* pooled) {
    for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t* s = sums + g * D * 3;
        period[g] = sd::lag_period(s, D);
        for (int32_t d = 0; d < D; ++d) pooled[g * D + d] = sd::lag_pooled(s + 3 * d);
    }
}

}  // extern "C"
