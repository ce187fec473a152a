// sd_heat.hip -- all-against-all identity of the rows of a read, kept as sums per bin (--heatmap): block against block
// on the device, one target against many queries.  sd_heat.hpp says which pairs exist, where a pair's sums go and who
// aligns it; this file holds the kernels, the host form and the C-ABI (include/sd_hip.h: sd_heat_*).
//
// sd_lag_pairs (sd_lags.hip) lets every lane build the masks of its own target: 40 K bytes of LDS per lane and a serial
// loop over the target's bases in every lane.  All-against-all means every target meets hundreds of queries, so here
// a WAVE takes one target and up to 64 consecutive queries (a strip): the wave builds the target's match masks once --
// lane l holds base 64 b + l of word b, five ballots give the word's five symbol masks -- into LDS in the layout of
// nw_build_masks (top-aligned, 5 symbols x K words, back to back), and every lane then runs the existing walk
// nw_pair<K, NwQueryAscii, NwNoSink> for its own query against them: the mask reads are broadcast reads.
//   sd_heat_rows     (device-resident form) one lane per final row: its segment and read, rows per read, order of the reads
//   sd_heat_plan     one lane per row as a TARGET: its word class and its number of strips (position in the group, W);
//                    targets per class and the longest query of the job (workgroup histogram in LDS, then global adds)
//   group_scan / sd_heat_scatter   the targets the kernel takes -> order[], grouped by word class (sd_group_dev.hpp)
//   exclusive_scan_dev   (sd_scan_dev.hpp) exclusive prefix of the strip counts in that order (64-bit): work item i of a
//                    class is strip i - scan[t] of the target t found by a binary search in the scan
//   sd_heat_pairs<K> one-wave workgroups, grid-stride over the work items of class K.  No per-pair store: in a wave the
//                    target's bin J is fixed and the query's bin I = x / B is monotone over the lanes, so {1, m, d + m}
//                    are summed over the lanes of a cell by a segmented shuffle reduction (6 steps, two packed dwords)
//                    and the first lane of each cell issues one triple of 64-bit atomic adds (integers: any order)
// Working memory: O(rows) for segments, classes, order and scan, O(cells) for the sums, checkpoints per resident wave.
// Nothing has one entry per pair or per work item.
// Workgroup = one wave (64 lanes), so the barrier between the mask build and the walk is the wave's own.  LDS: 40 K bytes
// per wave (320 B at K = 8), no limit on occupancy.  Launch bounds ask for 3 waves per SIMD at every K, the register
// budget of sd_nw_pairs (__launch_bounds__(256, 3)); the compiler's resource remarks give 100 / 134 / 146 / 136 / 140 /
// 144 VGPRs at K = 1 / 2 / 3 / 4 / 6 / 8 (4 / 3 / 3 / 3 / 3 / 3 waves per SIMD), no scratch (profiles/heatmap_timing.md).
// A strip that is not full still costs a wave: groups of 256 rows fill 51 of 64 lanes on average, and there the kernel is
// slower per pair than sd_lag_pairs; on an array of 16 384 rows (63.8 lanes) it is faster (the same file).
#include <algorithm>
#include <cstring>
#include <memory>

#include "sd_final_ws.hpp"
#include "sd_group_dev.hpp"
#include "sd_heat.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"
#include "sd_nw_kernel.hpp"
#include "sd_scan_dev.hpp"

namespace sd {

constexpr int HEAT_T = 256;   // threads per workgroup of the row / plan kernels
// sum[]: [0, 6) targets per word class, [6] (the scan's end), then
enum { HEAT_SUM_QMAX = 7, HEAT_SUM_BAD = 8, HEAT_SUM_ORDER = 9, HEAT_SUM_FAIL = 10, HEAT_SUM_N = 11 };
enum { HEAT_MODE_KEEP_MASKS = 1, HEAT_MODE_NO_SINK = 2 };   // bench: the walk alone

struct HeatRowsArgs {
    const sd_final_row* rows;
    int64_t n;
    const int64_t* rlen;
    const int64_t* toff;
    int n_reads;
    int64_t* seg_start;
    int32_t* seg_len;
    int32_t* seg_grp;
    int32_t* per_read;
    int32_t* sum;
};

__global__ __launch_bounds__(HEAT_T) void sd_heat_rows(HeatRowsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * HEAT_T + threadIdx.x;
    if (i >= a.n) return;
    const sd_final_row x = a.rows[i];
    if (x.read < 0 || x.read >= a.n_reads) {   // (a row of no read: counted, the call is refused)
        atomicAdd(&a.sum[HEAT_SUM_BAD], 1);
        a.seg_start[i] = 0;
        a.seg_len[i] = 0;
        a.seg_grp[i] = 0;
        return;
    }
    if (i > 0 && a.rows[i - 1].read > x.read) atomicAdd(&a.sum[HEAT_SUM_ORDER], 1);   // (the rows of a read are not adjacent)
    const int64_t rl = a.rlen[x.read];
    a.seg_start[i] = a.toff[x.read] + final_seg_first(x.start, rl);
    a.seg_len[i] = (int32_t)final_seg_len(x.start, x.end, rl);
    a.seg_grp[i] = x.read;
    atomicAdd(&a.per_read[x.read], 1);
}

__global__ __launch_bounds__(HEAT_T) void sd_heat_plan(const int32_t* __restrict__ seg_len, const int32_t* __restrict__ seg_grp,
                                                       const int64_t* __restrict__ grp_off, int64_t n_seg, int64_t W,
                                                       uint8_t* __restrict__ cls, int32_t* __restrict__ strips, int32_t* __restrict__ sum) {
    __shared__ int hist[HEAT_SUM_N];
    if (threadIdx.x < HEAT_SUM_N) hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t y = (int64_t)blockIdx.x * HEAT_T + threadIdx.x;
    if (y < n_seg) {
        const int32_t tl = seg_len[y];
        const int64_t s = heat_strips(y - grp_off[seg_grp[y]], W);
        const int k = heat_target_class(tl);
        uint8_t c = 0;
        if (s > 0 && k >= 0) {
            c = (uint8_t)(1 + k);
            atomicAdd(&hist[k], 1);
        }
        if (tl >= 1 && tl <= LAG_QMAX) atomicMax(&hist[HEAT_SUM_QMAX], tl);   // the longest query a lane can walk
        cls[y] = c;
        strips[y] = c ? (int32_t)s : 0;
    }
    __syncthreads();
    if (threadIdx.x < HEAT_SUM_N && hist[threadIdx.x]) {
        if (threadIdx.x == HEAT_SUM_QMAX) atomicMax(&sum[threadIdx.x], hist[threadIdx.x]);
        else atomicAdd(&sum[threadIdx.x], hist[threadIdx.x]);
    }
}

// the targets of a plan as group_scatter reads them: the kernel's by word class, the others out
struct HeatSrc {
    const uint8_t* cls;
    __device__ int kind(int64_t y) const { return cls[y] == 0 ? GROUP_OUT : GROUP_IN; }
    __device__ int group(int64_t y) const { return cls[y] - 1; }
    __device__ void aside(int64_t, int64_t) const {}
};

__global__ __launch_bounds__(GROUP_T) void sd_heat_scatter(const uint8_t* __restrict__ cls, int64_t n_seg, int32_t* __restrict__ cursor,
                                                           int32_t* __restrict__ order) {
    group_scatter(HeatSrc{cls}, n_seg, n_seg, LAG_CLASSES, cursor, order);
}

// the strips of the i-th target in the order of the grouping, 0 behind the targets: what scan[] (n_seg + 1 entries) sums
struct HeatStrips {
    const int32_t *strips, *order, *base;
    __device__ int64_t operator()(int64_t i) const { return i < base[LAG_CLASSES] ? strips[order[i]] : 0; }
};

// bound[k] = the first work item of class k, bound[LAG_CLASSES] = all of them
__global__ void sd_heat_bounds(const int64_t* __restrict__ scan, const int32_t* __restrict__ base, int64_t* __restrict__ bound) {
    if (blockIdx.x == 0 && threadIdx.x <= LAG_CLASSES) bound[threadIdx.x] = scan[base[threadIdx.x]];
}

struct HeatArgs {
    const uint8_t* text;
    const int64_t* seg_start;
    const int32_t* seg_len;
    const int32_t* seg_grp;
    const int64_t* grp_off;      // [n_groups + 1]
    const int64_t* cell_off;     // [n_groups + 1]
    const int32_t* order;        // the class's targets
    const int64_t* scan;         // their first work items (the job's numbering); scan[count] = the class's end
    int count;                   // targets of the class
    int64_t items;               // work items of the class
    int64_t B, W;
    int cap;                     // checkpoint slots per lane
    uint32_t* ck;                // gridDim.x waves x cap slots x K x 16 B x 64 lanes, planar as nw_pair wants them
    unsigned long long* sums;    // [cells][3]
    int* fails;
    int mode;
};

template <int K>
__global__ __launch_bounds__(HEAT_STRIP, 3) void sd_heat_pairs(HeatArgs a) {
    __shared__ uint2 masks[5 * K];
    const int lane = threadIdx.x;
    uint32_t* ckl = a.ck + (size_t)blockIdx.x * (size_t)a.cap * K * 4 * HEAT_STRIP + lane;
    const int64_t item0 = a.scan[0];
    for (int64_t w = blockIdx.x; w < a.items; w += gridDim.x) {
        // the target of work item w: the last one whose first item is not behind it.  A 64-ary search: the lanes probe 64
        // places of the range at once and a ballot picks the part to go on with (16 384 targets: 3 rounds, not 14)
        const int64_t key = item0 + w;
        int lo = 0, n = a.count;   // scan[lo] <= key, the answer in [lo, lo + n)
        while (n > 1) {
            const int step = (n + HEAT_STRIP - 1) / HEAT_STRIP;
            const bool ok = lane * step < n && a.scan[lo + lane * step] <= key;   // (a prefix of the lanes; lane 0 always)
            const int j = __popcll(__ballot(ok)) - 1;
            n = min(step, n - j * step);
            lo += j * step;
        }
        const int y = a.order[lo];
        const int64_t strip = key - a.scan[lo];
        const int tl = a.seg_len[y], g = a.seg_grp[y];
        const int64_t g0 = a.grp_off[g], pos = y - g0;
        const int64_t x = heat_first_query(pos, a.W) + strip * HEAT_STRIP + lane;   // this lane's query, counted in the group
        const bool has = x < pos;
        const int ql = has ? a.seg_len[g0 + x] : 0;
        const bool walk = has && lag_pair_class(ql, tl) == LAG_DEV;
        if (!(a.mode & HEAT_MODE_KEEP_MASKS) || w == (int64_t)blockIdx.x) {
            // the target's match masks: template symbol k at bit 64 K - tl + k (nw_build_masks); lane l holds bit l of word b
            const int pad = 64 * K - tl;
            const int64_t t0 = a.seg_start[y];
#pragma unroll
            for (int b = 0; b < K; ++b) {
                const int k = 64 * b + lane - pad;   // (< tl for every lane)
                int c = -1;
                if (k >= 0) {
                    const uint32_t ch = a.text[t0 + k];
                    c = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
                }
                const unsigned long long m0 = __ballot(c == 0), m1 = __ballot(c == 1), m2 = __ballot(c == 2), m3 = __ballot(c == 3),
                                         m4 = __ballot(c == 4);
                const unsigned long long m = lane == 0 ? m0 : lane == 1 ? m1 : lane == 2 ? m2 : lane == 3 ? m3 : m4;
                if (lane < 5) masks[lane * K + b] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
            }
        }
        __syncthreads();
        int dd = 0, mm = 0;
        bool add = false;
        if (walk) {
            NwQueryAscii q{a.text, a.seg_start[g0 + x]};
            add = nw_pair<K, NwQueryAscii, NwNoSink>(q, ql, masks, tl, false, ckl, nullptr, (size_t)HEAT_STRIP, a.cap, dd, mm);
            if (!add) atomicAdd(a.fails, 1);   // (cannot happen: the slots are sized by the longest query)
        }
        if (!(a.mode & HEAT_MODE_NO_SINK)) {
            // lanes of one cell are consecutive (I is monotone over the lanes): sum {1, m, d + m} down to the cell's first lane
            const uint32_t I = (uint32_t)x / (uint32_t)a.B;
            const uint32_t Iup = __shfl_up(I, 1);
            const bool head = lane == 0 || Iup != I;
            const unsigned long long heads = __ballot(head);
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const int end = above ? lane + __ffsll((long long)above) : 64;   // the first lane of the next cell
            uint32_t nm = add ? (1u << 20) | (uint32_t)mm : 0u;   // pairs << 20 | matches: 64 x 512 matches at the most
            uint32_t cc = add ? (uint32_t)(dd + mm) : 0u;
#pragma unroll
            for (int off = 1; off < HEAT_STRIP; off <<= 1) {
                const uint32_t a1 = __shfl_down(nm, off), a2 = __shfl_down(cc, off);
                if (lane + off < end) { nm += a1; cc += a2; }
            }
            if (head && (nm >> 20)) {
                const int64_t nb = heat_bins(a.grp_off[g + 1] - g0, a.B), J = pos / a.B;
                unsigned long long* o = a.sums + (a.cell_off[g] + heat_cell(nb, (int64_t)I, J)) * 3;
                atomicAdd(o, (unsigned long long)(nm >> 20));
                atomicAdd(o + 1, (unsigned long long)(nm & 0xfffffu));
                atomicAdd(o + 2, (unsigned long long)cc);
            }
        }
        __syncthreads();   // the next item's masks overwrite these
    }
}

}  // namespace sd

namespace sdi {
namespace {

// Per device, kept between calls (sd_job_dev.hpp: DevWork): text, segments, plan, grouping, scan and checkpoints.
struct HeatCtx : DevWork, FinalText {
    DevBuf<uint8_t> cls, ck;
    DevBuf<int64_t> seg_start, grp, scan, tsum, tbase, bound;   // grp: [group_off | cell_off]; tsum, tbase: the scan's tiles
    DevBuf<int32_t> seg_len, seg_grp, strips, order, sum, base, cursor, per_read;
    PinBuf<int64_t> h_grp, h_bound;
    PinBuf<int32_t> h_sum, h_len, h_per_read;
    hipEvent_t ev_plan = nullptr;
};

inline unsigned heat_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + sd::HEAT_T - 1) / sd::HEAT_T); }

// ---- the closed forms ---------------------------------------------------------------------------------------------------
// cell_off (n_groups + 1, may be null), cells and pairs of the groups; SD_ERR_UNSUPPORTED when a count leaves 63 bits
int heat_layout(const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int64_t* cell_off, int64_t& cells, int64_t& pairs) {
    uint64_t p = 0;
    unsigned __int128 c = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t n = group_off[g + 1] - group_off[g];
        if (n < 0 || n >= ((int64_t)1 << 31)) return n < 0 ? SD_ERR_PARAM : SD_ERR_UNSUPPORTED;
        if (cell_off) cell_off[g] = (int64_t)c;
        c += (unsigned __int128)sd::heat_cells(sd::heat_bins(n, B));
        if (c >> 62) return SD_ERR_UNSUPPORTED;
        if (!sd::heat_add_pairs(n, W, p) || p >> 63) return SD_ERR_UNSUPPORTED;
    }
    if (cell_off) cell_off[n_groups] = (int64_t)c;
    cells = (int64_t)c;
    pairs = (int64_t)p;
    return SD_OK;
}

// B, W, max_pairs and the two refusals for size, with the numbers in errbuf
int heat_limits(const char* who, const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int64_t max_pairs, int64_t* cell_off,
                int64_t& cells, int64_t& pairs, char* errbuf, size_t errlen) {
    if (!sd::heat_b_ok(B)) {
        set_err(errbuf, errlen, std::string(who) + ": B = " + std::to_string(B) + ", must be 1 .. " + std::to_string(sd::HEAT_BMAX));
        return SD_ERR_PARAM;
    }
    if (!sd::heat_w_ok(W)) { set_err(errbuf, errlen, std::string(who) + ": W = " + std::to_string(W) + ", must be 0 (no limit) or more"); return SD_ERR_PARAM; }
    if (max_pairs < 0) { set_err(errbuf, errlen, std::string(who) + ": max_pairs = " + std::to_string(max_pairs) + ", must be 0 (no limit) or more"); return SD_ERR_PARAM; }
    const int rc = heat_layout(group_off, n_groups, B, W, cell_off, cells, pairs);
    if (rc) { set_err(errbuf, errlen, std::string(who) + (rc == SD_ERR_PARAM ? ": group offsets that decrease" : ": a group of 2^31 rows or more, or counts beyond 2^62")); return rc; }
    if (cells > sd::HEAT_CELLS_MAX) {
        set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(cells) + " cells, the cap is " + std::to_string(sd::HEAT_CELLS_MAX) +
                                    " (HEAT_CELLS_MAX): use more rows per bin");
        return SD_ERR_PARAM;
    }
    if (max_pairs > 0 && pairs > max_pairs) {
        set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(pairs) + " pairs, max_pairs is " + std::to_string(max_pairs) +
                                    ": use a row distance limit W, or raise max_pairs");
        return SD_ERR_PARAM;
    }
    return SD_OK;
}

// the segments of a job on the host: start (in text) / length per row, the groups' first rows and first cells
struct HeatJob {
    const char* text;
    const int64_t* st;
    const int32_t* ln;
    const int64_t* goff;
    const int64_t* coff;
    int32_t n_groups;
    int64_t B, W;
};

// {kernel pairs, host pairs, pairs with an empty side} by lag_pair_class, from prefix counts per group (sd_heat.hpp: inside
// the kernel's limits the class depends on the query alone)
void heat_classes(const HeatJob& j, bool acgtn, int64_t classes[3]) {
    int64_t dev = 0, host = 0, none = 0;
    std::vector<int64_t> e, l;
    for (int32_t g = 0; g < j.n_groups; ++g) {
        const int64_t g0 = j.goff[g], n = j.goff[g + 1] - g0;
        e.assign((size_t)n + 1, 0);
        l.assign((size_t)n + 1, 0);
        for (int64_t x = 0; x < n; ++x) {
            e[(size_t)x + 1] = e[(size_t)x] + (j.ln[g0 + x] <= 0);
            l[(size_t)x + 1] = l[(size_t)x] + (j.ln[g0 + x] > sd::LAG_QMAX);
        }
        for (int64_t y = 1; y < n; ++y) {
            const int64_t lo = sd::heat_first_query(y, j.W), cnt = y - lo, empty = e[(size_t)y] - e[(size_t)lo];
            const int32_t tl = j.ln[g0 + y];
            if (tl <= 0) { none += cnt; continue; }
            none += empty;
            const int64_t h = tl > sd::LAG_TMAX || !acgtn ? cnt - empty : l[(size_t)y] - l[(size_t)lo];
            host += h;
            dev += cnt - empty - h;
        }
    }
    classes[0] = dev;
    classes[1] = host;
    classes[2] = none;
}

// The host form: the pairs of the job (which = 0: every pair; 1: those lag_pair_class gives to the host), aligned in
// batches by sd_nw_identity_batch and ADDED to sums.  Memory: a batch of pairs, never all of them.
int heat_host(const HeatJob& j, int which, int threads, int64_t* sums) {
    constexpr size_t BATCH = (size_t)1 << 16;
    std::vector<const char*> q, t;
    std::vector<int32_t> ql, tl, hd, hm, hc;
    std::vector<int64_t> cell, longq;
    auto flush = [&]() -> int {
        const int64_t n = (int64_t)q.size();
        if (n == 0) return SD_OK;
        hd.resize((size_t)n); hm.resize((size_t)n); hc.resize((size_t)n);
        const int rc = sd_nw_identity_batch(q.data(), ql.data(), t.data(), tl.data(), n, std::max(1, threads), hd.data(), hm.data(), hc.data());
        if (rc) return rc;
        for (int64_t i = 0; i < n; ++i) {
            if (hd[(size_t)i] < 0) continue;
            int64_t* o = sums + cell[(size_t)i] * 3;
            o[0] += 1;
            o[1] += hm[(size_t)i];
            o[2] += (int64_t)hd[(size_t)i] + hm[(size_t)i];
        }
        q.clear(); t.clear(); ql.clear(); tl.clear(); cell.clear();
        return SD_OK;
    };
    for (int32_t g = 0; g < j.n_groups; ++g) {
        const int64_t g0 = j.goff[g], n = j.goff[g + 1] - g0, nb = sd::heat_bins(n, j.B);
        longq.clear();
        if (which == 1)
            for (int64_t x = 0; x < n; ++x) if (j.ln[g0 + x] > sd::LAG_QMAX) longq.push_back(x);
        auto take = [&](int64_t x, int64_t y) -> int {
            q.push_back(j.text + j.st[g0 + x]);
            ql.push_back(j.ln[g0 + x]);
            t.push_back(j.text + j.st[g0 + y]);
            tl.push_back(j.ln[g0 + y]);
            cell.push_back(j.coff[g] + sd::heat_cell(nb, x / j.B, y / j.B));
            return q.size() >= BATCH ? flush() : SD_OK;
        };
        for (int64_t y = 1; y < n; ++y) {
            const int32_t len = j.ln[g0 + y];
            if (len <= 0) continue;
            const int64_t lo = sd::heat_first_query(y, j.W);
            int rc = SD_OK;
            if (which == 0 || len > sd::LAG_TMAX) {
                for (int64_t x = lo; x < y && rc == SD_OK; ++x)
                    if (j.ln[g0 + x] > 0 && (which == 0 || sd::lag_pair_class(j.ln[g0 + x], len) == sd::LAG_HOST)) rc = take(x, y);
            } else {
                for (auto it = std::lower_bound(longq.begin(), longq.end(), lo); it != longq.end() && *it < y && rc == SD_OK; ++it)
                    if (sd::lag_pair_class(j.ln[g0 + *it], len) == sd::LAG_HOST) rc = take(*it, y);
            }
            if (rc) return rc;
        }
    }
    return flush();
}

// ---- the device passes --------------------------------------------------------------------------------------------------
// plan + grouping + scan on st over the segments in c (seg_len, seg_grp, grp); the summary and the classes' item bounds on
// their way to c.h_sum / c.h_bound, ev_plan recorded
void heat_plan(HeatCtx& c, hipStream_t st, int64_t n_seg, int32_t n_groups, int64_t W, bool clear_sum) {
    const int64_t n_tiles = sd::scan_tiles_of(n_seg);
    c.cls.alloc((size_t)n_seg);
    c.strips.alloc((size_t)n_seg);
    c.order.alloc((size_t)n_seg);
    c.scan.alloc((size_t)n_seg + 1);
    c.tsum.alloc((size_t)n_tiles);
    c.tbase.alloc((size_t)n_tiles + 1);
    c.bound.alloc(sd::LAG_CLASSES + 1);
    c.base.alloc(sd::LAG_CLASSES + 1);
    c.cursor.alloc(sd::LAG_CLASSES + 1);
    c.h_sum.alloc(sd::HEAT_SUM_N);
    c.h_bound.alloc(sd::LAG_CLASSES + 1);
    if (clear_sum) SD_HIP(hipMemsetAsync(c.sum.p, 0, sd::HEAT_SUM_N * sizeof(int32_t), st));
    const unsigned grid = heat_grid(n_seg);
    hipLaunchKernelGGL(sd::sd_heat_plan, dim3(grid), dim3(sd::HEAT_T), 0, st, c.seg_len.p, c.seg_grp.p, c.grp.p, n_seg, W, c.cls.p, c.strips.p,
                       c.sum.p);
    group_scan(st, c.sum.p, sd::LAG_CLASSES, c.base.p, c.cursor.p);
    hipLaunchKernelGGL(sd::sd_heat_scatter, dim3(grid), dim3(sd::GROUP_T), 0, st, c.cls.p, n_seg, c.cursor.p, c.order.p);
    sd::exclusive_scan_dev(st, sd::HeatStrips{c.strips.p, c.order.p, c.base.p}, n_seg, c.scan.p, c.tsum.p, c.tbase.p);
    hipLaunchKernelGGL(sd::sd_heat_bounds, dim3(1), dim3(64), 0, st, c.scan.p, c.base.p, c.bound.p);
    SD_HIP(hipGetLastError());
    SD_HIP(hipMemcpyAsync(c.h_sum.p, c.sum.p, sd::HEAT_SUM_N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SD_HIP(hipMemcpyAsync(c.h_bound.p, c.bound.p, (sd::LAG_CLASSES + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ensure_event(c.ev_plan, hipEventDisableTiming);
    SD_HIP(hipEventRecord(c.ev_plan, st));
}

struct HeatLaunch { int K, grid, cap, first, count; int64_t items; };

// the launches of the pair kernel from the summary the host has seen; grows c.ck (no walk is in flight: settle())
std::vector<HeatLaunch> heat_launches(HeatCtx& c) {
    std::vector<HeatLaunch> out;
    const int32_t* hs = c.h_sum.p;
    const int64_t* hb = c.h_bound.p;
    size_t need = 0;
    int first = 0;
    for (int k = 0; k < sd::LAG_CLASSES; ++k) {
        const int count = hs[k];
        const int64_t items = hb[k + 1] - hb[k];
        if (count > 0 && items > 0) {
            const int K = sd::lag_words_of_class(k), S = sd::nw_block_cols(K);
            const int cap = std::max(1, (std::max(1, (int)hs[sd::HEAT_SUM_QMAX]) + S - 1) / S);   // the longest query of the job
            const size_t wave_bytes = (size_t)cap * K * 16 * sd::HEAT_STRIP;
            int64_t grid = std::min<int64_t>((int64_t)c.n_cu * 12, items);   // 3 waves per SIMD
            grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(((size_t)1 << 30) / wave_bytes)));
            out.push_back(HeatLaunch{K, (int)grid, cap, first, count, items});
            need = std::max(need, wave_bytes * (size_t)grid);
        }
        first += count;
    }
    c.ck.alloc(need);
    return out;
}

void heat_walk(HeatCtx& c, hipStream_t st, const HeatLaunch& L, int32_t n_groups, int64_t B, int64_t W, int64_t* d_sums, int mode) {
    const sd::HeatArgs a{c.text.p, c.seg_start.p, c.seg_len.p, c.seg_grp.p, c.grp.p, c.grp.p + n_groups + 1, c.order.p + L.first,
                         c.scan.p + L.first, L.count, L.items, B, W, L.cap, reinterpret_cast<uint32_t*>(c.ck.p),
                         reinterpret_cast<unsigned long long*>(d_sums), c.sum.p + sd::HEAT_SUM_FAIL, mode};
    with_words(L.K, [&](auto words) {
        hipLaunchKernelGGL(sd::sd_heat_pairs<decltype(words)::value>, dim3(L.grid), dim3(sd::HEAT_STRIP), 0, st, a);
    });
    SD_HIP(hipGetLastError());
}

// group_off | cell_off of the job, pinned, on their way to c.grp
void heat_upload_groups(HeatCtx& c, hipStream_t st, const int64_t* group_off, const int64_t* cell_off, int32_t n_groups) {
    const size_t ng = (size_t)n_groups + 1;
    c.h_grp.alloc(2 * ng);
    c.grp.alloc(2 * ng);
    std::memcpy(c.h_grp.p, group_off, ng * sizeof(int64_t));
    std::memcpy(c.h_grp.p + ng, cell_off, ng * sizeof(int64_t));
    SD_HIP(hipMemcpyAsync(c.grp.p, c.h_grp.p, 2 * ng * sizeof(int64_t), hipMemcpyHostToDevice, st));
}

}  // namespace
}  // namespace sdi

extern "C" {

int sd_heat_layout(const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int64_t* cell_off, int64_t* cells_total,
                   int64_t* pairs) try {
    if (!group_off || n_groups < 0 || !cells_total || !pairs || !sd::heat_b_ok(B) || !sd::heat_w_ok(W)) return SD_ERR_PARAM;
    return heat_layout(group_off, n_groups, B, W, cell_off, *cells_total, *pairs);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_heat_segments(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg, const int64_t* group_off,
                     int32_t n_groups, int64_t B, int64_t W, int64_t max_pairs, int32_t which, int32_t threads, int64_t* sums,
                     char* errbuf, size_t errlen) try {
    static const char* who = "sd_heat_segments";
    if (which != 0 && which != 1) { set_err(errbuf, errlen, std::string(who) + ": which = " + std::to_string(which) + ", must be 0 or 1"); return SD_ERR_PARAM; }
    std::vector<int64_t> st, coff((size_t)std::max(n_groups, 0) + 1);
    std::vector<int32_t> ln;
    int64_t lo = 0, hi = 0, cells = 0, pairs = 0;
    int rc = segment_args(who, seq, seqlen, starts, ends, n_seg, group_off, n_groups, sums, (int64_t)1 << 31, "2^31 segments or more", st, ln,
                          nullptr, lo, hi, errbuf, errlen);
    if (rc) return rc;
    if ((rc = heat_limits(who, group_off, n_groups, B, W, max_pairs, coff.data(), cells, pairs, errbuf, errlen))) return rc;
    std::memset(sums, 0, sizeof(int64_t) * 3 * (size_t)cells);
    const HeatJob j{seq + lo, st.data(), ln.data(), group_off, coff.data(), n_groups, B, W};
    if (which == 1 && !text_is_acgtn(j.text, hi - lo)) which = 0;   // (a text outside ACGTN: every pair is the host's)
    if ((rc = heat_host(j, which, threads, sums))) set_err(errbuf, errlen, std::string(who) + ": the host alignment failed");
    return rc;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

// bench != null: sd_heat_kernel_bench's timing of the stages instead of one plain pass
struct sd_heat_bench {
    int warmup, reps;
    float *ms_group, *ms_pairs, *ms_walk;
    int64_t* info;
};

static int heat_segments_dev(const char* who, const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                             const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int64_t max_pairs, int32_t device,
                             int32_t threads, int64_t* sums, int64_t classes[3], char* errbuf, size_t errlen, const sd_heat_bench* bench) {
    std::vector<int64_t> sst, coff((size_t)std::max(n_groups, 0) + 1);
    std::vector<int32_t> ln, grp;
    int64_t lo = 0, hi = 0, cells = 0, pairs = 0;
    int rc = segment_args(who, seq, seqlen, starts, ends, n_seg, group_off, n_groups, sums, (int64_t)1 << 31, "2^31 segments or more", sst, ln,
                          &grp, lo, hi, errbuf, errlen);
    if (rc) return rc;
    if ((rc = heat_limits(who, group_off, n_groups, B, W, max_pairs, coff.data(), cells, pairs, errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    std::memset(sums, 0, sizeof(int64_t) * 3 * (size_t)cells);
    const int64_t text = hi - lo;
    const char* tx = seq + lo;
    const HeatJob j{tx, sst.data(), ln.data(), group_off, coff.data(), n_groups, B, W};
    const bool acgtn = text_is_acgtn(tx, text);
    int64_t cl[3];
    heat_classes(j, acgtn, cl);
    if (classes) { classes[0] = cl[0]; classes[1] = cl[1]; classes[2] = cl[2]; }
    if (!acgtn || cl[0] == 0) {   // a byte the kernel does not read: every pair is the host's
        if (bench) return SD_ERR_UNSUPPORTED;
        if ((rc = heat_host(j, 0, threads, sums))) set_err(errbuf, errlen, std::string(who) + ": the host alignment failed");
        return rc;
    }
    try {
        DeviceScope on(device);
        HeatCtx& c = device_ctx<HeatCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        OwnedStream st;
        DevBuf<int64_t> d_sums;
        const size_t n_sums = (size_t)cells * 3;
        c.text.alloc((size_t)text + 8);
        c.seg_start.alloc((size_t)n_seg);
        c.seg_len.alloc((size_t)n_seg);
        c.seg_grp.alloc((size_t)n_seg);
        c.sum.alloc(sd::HEAT_SUM_N);
        d_sums.alloc(n_sums);
        SD_HIP(hipMemsetAsync(c.text.p + text, 0, 8, st));
        if (text) SD_HIP(hipMemcpyAsync(c.text.p, tx, (size_t)text, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.seg_start.p, sst.data(), sizeof(int64_t) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.seg_len.p, ln.data(), sizeof(int32_t) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.seg_grp.p, grp.data(), sizeof(int32_t) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        heat_upload_groups(c, st, group_off, coff.data(), n_groups);
        StageClock clock;
        const auto clear_sums = [&]() { SD_HIP(hipMemsetAsync(d_sums.p, 0, sizeof(int64_t) * std::max<size_t>(n_sums, 1), st)); };
        clear_sums();
        const auto plan = [&]() { heat_plan(c, st, n_seg, n_groups, W, true); };   // plan, scatter and scan
        if (bench) clock.time(st, bench->warmup, bench->reps, bench->ms_group, plan);
        else plan();
        SD_HIP(hipEventSynchronize(c.ev_plan));
        const std::vector<HeatLaunch> launches = heat_launches(c);
        if (bench) {
            int64_t items = 0, Kmost = 0, imost = -1;
            for (const HeatLaunch& L : launches) { items += L.items; if (L.items > imost) { imost = L.items; Kmost = L.K; } }
            for (int pass = 0; pass < 2; ++pass)   // the whole kernel, then the walk alone: masks built once per wave, no sink
                clock.time(st, bench->warmup, bench->reps, pass == 0 ? bench->ms_pairs : bench->ms_walk, [&]() {
                    for (const HeatLaunch& L : launches)
                        heat_walk(c, st, L, n_groups, B, W, d_sums.p, pass == 0 ? 0 : sd::HEAT_MODE_KEEP_MASKS | sd::HEAT_MODE_NO_SINK);
                }, clear_sums);
            bench->info[0] = cl[0];
            bench->info[1] = cl[1];
            bench->info[2] = Kmost;
            bench->info[3] = items;
            bench->info[4] = cells;
            for (const HeatLaunch& L : launches) if (L.K == Kmost) { bench->info[5] = L.items; bench->info[6] = L.grid; bench->info[7] = L.cap; }
            clear_sums();
        }
        for (const HeatLaunch& L : launches) heat_walk(c, st, L, n_groups, B, W, d_sums.p, 0);
        c.in_flight(st);
        // the host's pairs, under the kernel
        std::vector<int64_t> hsums;
        int hrc = SD_OK;
        if (cl[1] > 0 && !bench) {
            hsums.assign(n_sums, 0);
            hrc = heat_host(j, 1, threads, hsums.data());
        }
        SD_HIP(hipMemcpyAsync(sums, d_sums.p, sizeof(int64_t) * n_sums, hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));
        int32_t fails = 0;
        SD_HIP(hipMemcpy(&fails, c.sum.p + sd::HEAT_SUM_FAIL, sizeof fails, hipMemcpyDeviceToHost));
        c.waited();
        if (hrc) { set_err(errbuf, errlen, std::string(who) + ": the host alignment failed"); return hrc; }
        for (size_t i = 0; i < hsums.size(); ++i) sums[i] += hsums[i];
        if (fails) { set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(fails) + " pairs ran out of checkpoint slots"); return SD_ERR_INTERNAL; }
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
}

int sd_heat_segments_dev(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                         const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int64_t max_pairs, int32_t device,
                         int32_t threads, int64_t* sums, int64_t classes[3], char* errbuf, size_t errlen) try {
    return heat_segments_dev("sd_heat_segments_dev", seq, seqlen, starts, ends, n_seg, group_off, n_groups, B, W, max_pairs, device, threads,
                             sums, classes, errbuf, errlen, nullptr);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_heat_kernel_bench(const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                         const int64_t* group_off, int32_t n_groups, int64_t B, int64_t W, int32_t device, int32_t warmup, int32_t reps,
                         float* ms_group, float* ms_pairs, float* ms_walk, int64_t info[8]) try {
    if (warmup < 0 || reps < 1 || !ms_group || !ms_pairs || !ms_walk || !info || n_seg <= 0) return SD_ERR_PARAM;
    int64_t cells = 0, pairs = 0;
    if (!group_off || n_groups < 0 || !sd::heat_b_ok(B) || !sd::heat_w_ok(W)) return SD_ERR_PARAM;
    int rc = heat_layout(group_off, n_groups, B, W, nullptr, cells, pairs);
    if (rc) return rc;
    if (cells > sd::HEAT_CELLS_MAX) return SD_ERR_PARAM;
    std::vector<int64_t> sums((size_t)std::max<int64_t>(cells, 1) * 3);
    for (int i = 0; i < 8; ++i) info[i] = 0;
    const sd_heat_bench b{warmup, reps, ms_group, ms_pairs, ms_walk, info};
    return heat_segments_dev("sd_heat_kernel_bench", seq, seqlen, starts, ends, n_seg, group_off, n_groups, B, W, 0, device, 1, sums.data(),
                             nullptr, nullptr, 0, &b);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

// the rows of a device-final job as groups: rows per read from row order (the rows of a read adjacent, reads ascending)
static int heat_final_groups(const char* who, const sd_final_row* rows, int64_t n_rows, int32_t n_reads, std::vector<int64_t>& goff,
                             char* errbuf, size_t errlen) {
    goff.assign((size_t)n_reads + 1, 0);
    for (int64_t i = 0; i < n_rows; ++i) {
        const int32_t r = rows[i].read;
        if (r < 0 || r >= n_reads) { set_err(errbuf, errlen, std::string(who) + ": row " + std::to_string(i) + " has a read index outside the reads"); return SD_ERR_PARAM; }
        if (i > 0 && rows[i - 1].read > r) { set_err(errbuf, errlen, std::string(who) + ": the rows are not in the order of their reads"); return SD_ERR_PARAM; }
        goff[(size_t)r + 1] += 1;
    }
    for (int32_t r = 0; r < n_reads; ++r) goff[(size_t)r + 1] += goff[(size_t)r];
    return SD_OK;
}

int sd_heat_final_host(const sd_final_row* rows, int64_t n_rows, const char* text, const int64_t* read_off, const int64_t* read_lens,
                       int32_t n_reads, int64_t B, int64_t W, int64_t max_pairs, int32_t which, int32_t threads, int64_t* sums,
                       int64_t n_cells, int64_t classes[3], char* errbuf, size_t errlen) try {
    static const char* who = "sd_heat_final_host";
    if (which != 0 && which != 1) { set_err(errbuf, errlen, std::string(who) + ": which = " + std::to_string(which) + ", must be 0 or 1"); return SD_ERR_PARAM; }
    if (n_rows < 0 || n_reads < 0 || n_rows >= ((int64_t)1 << 31) || (n_rows > 0 && !rows) || (n_reads > 0 && (!read_off || !read_lens)) || (n_cells > 0 && !sums)) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_off[r] < 0 || read_lens[r] < 0 || (read_lens[r] > 0 && !text)) { set_err(errbuf, errlen, std::string(who) + ": negative read offset or length, or no text"); return SD_ERR_PARAM; }
    std::vector<int64_t> goff, coff((size_t)n_reads + 1), st((size_t)n_rows);
    std::vector<int32_t> ln((size_t)n_rows);
    int64_t cells = 0, pairs = 0;
    int rc = heat_final_groups(who, rows, n_rows, n_reads, goff, errbuf, errlen);
    if (rc) return rc;
    if ((rc = heat_limits(who, goff.data(), n_reads, B, W, max_pairs, coff.data(), cells, pairs, errbuf, errlen))) return rc;
    if (cells != n_cells) { set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(cells) + " cells, the caller's sums hold " + std::to_string(n_cells)); return SD_ERR_PARAM; }
    for (int64_t i = 0; i < n_rows; ++i) {
        const int32_t r = rows[i].read;
        st[(size_t)i] = read_off[r] + sd::final_seg_first(rows[i].start, read_lens[r]);
        const int64_t l = sd::final_seg_len(rows[i].start, rows[i].end, read_lens[r]);
        if (l >= (1 << 27)) { set_err(errbuf, errlen, std::string(who) + ": a segment of 2^27 bases or more"); return SD_ERR_UNSUPPORTED; }
        ln[(size_t)i] = (int32_t)l;
    }
    bool acgtn = true;
    for (int32_t r = 0; r < n_reads && acgtn; ++r) acgtn = text_is_acgtn(text + read_off[r], read_lens[r]);
    std::memset(sums, 0, sizeof(int64_t) * 3 * (size_t)cells);
    const HeatJob j{text, st.data(), ln.data(), goff.data(), coff.data(), n_reads, B, W};
    if (classes) heat_classes(j, acgtn, classes);
    if ((rc = heat_host(j, acgtn ? which : 0, threads, sums))) set_err(errbuf, errlen, std::string(who) + ": the host alignment failed");
    return rc;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_heat_final_dev(const sd_final_row* d_rows, int64_t n_rows, const void* d_text, const int64_t* read_off, const int64_t* read_lens,
                      int32_t n_reads, int64_t B, int64_t W, int64_t max_pairs, int32_t device, void* hip_stream, int64_t* d_sums,
                      int64_t n_cells, int64_t classes[3], char* errbuf, size_t errlen) try {
    static const char* who = "sd_heat_final_dev";
    if (classes) { classes[0] = 0; classes[1] = 0; classes[2] = 0; }
    if (!sd::heat_b_ok(B) || !sd::heat_w_ok(W) || max_pairs < 0) {   // (the text of the refusal: heat_limits)
        int64_t zero[1] = {0}, a = 0, b = 0;
        return heat_limits(who, zero, 0, B, W, max_pairs, nullptr, a, b, errbuf, errlen);
    }
    if (n_rows < 0 || n_reads < 0 || n_cells < 0 || n_rows >= ((int64_t)1 << 31) || (n_rows > 0 && !d_rows) || (n_reads > 0 && (!read_off || !read_lens)) ||
        (n_cells > 0 && !d_sums)) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    int64_t text = 0;
    int rc = final_reads_args(who, d_text, read_off, read_lens, n_reads, text, errbuf, errlen);
    if (rc) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        if (n_rows > 0 && (rc = buffer_on_device(d_rows, device, who, "row", errbuf, errlen))) return rc;
        if (n_cells > 0 && (rc = buffer_on_device(d_sums, device, who, "sum", errbuf, errlen))) return rc;
        if (text > 0 && (rc = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return rc;
        HeatCtx& c = device_ctx<HeatCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();   // the previous call's kernels read the buffers this one overwrites
        const size_t nr = (size_t)n_reads + 1;
        c.seg_start.alloc((size_t)n_rows);
        c.seg_len.alloc((size_t)n_rows);
        c.seg_grp.alloc((size_t)n_rows);
        c.per_read.alloc(nr);
        c.h_per_read.alloc(nr);
        c.h_len.alloc((size_t)n_rows);
        c.sum.alloc(sd::HEAT_SUM_N);
        c.h_sum.alloc(sd::HEAT_SUM_N);
        final_text_gather(c, st, d_text, read_off, read_lens, n_reads, text);
        SD_HIP(hipMemsetAsync(c.sum.p, 0, sd::HEAT_SUM_N * sizeof(int32_t), st));
        SD_HIP(hipMemsetAsync(c.per_read.p, 0, nr * sizeof(int32_t), st));
        if (n_rows > 0) {
            sd::HeatRowsArgs a{d_rows, n_rows, c.rlen(), c.toff(), (int)n_reads, c.seg_start.p, c.seg_len.p, c.seg_grp.p,
                               c.per_read.p, c.sum.p};
            hipLaunchKernelGGL(sd::sd_heat_rows, dim3(heat_grid(n_rows)), dim3(sd::HEAT_T), 0, st, a);
            SD_HIP(hipGetLastError());
            SD_HIP(hipMemcpyAsync(c.h_len.p, c.seg_len.p, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        SD_HIP(hipMemcpyAsync(c.h_per_read.p, c.per_read.p, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SD_HIP(hipMemcpyAsync(c.h_sum.p, c.sum.p, sd::HEAT_SUM_N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        c.in_flight(st);
        SD_HIP(hipStreamSynchronize(st));   // the first wait: rows per read and the rows' lengths, for the closed forms
        if (c.h_sum.p[sd::HEAT_SUM_BAD] || c.h_sum.p[sd::HEAT_SUM_ORDER]) {
            set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(c.h_sum.p[sd::HEAT_SUM_BAD]) + " rows with a read index outside the reads, " +
                                        std::to_string(c.h_sum.p[sd::HEAT_SUM_ORDER]) + " rows before a row of an earlier read");
            return SD_ERR_PARAM;
        }
        std::vector<int64_t> goff(nr, 0), coff(nr, 0);
        for (int32_t r = 0; r < n_reads; ++r) goff[(size_t)r + 1] = goff[(size_t)r] + c.h_per_read.p[r];
        int64_t cells = 0, pairs = 0;
        if ((rc = heat_limits(who, goff.data(), n_reads, B, W, max_pairs, coff.data(), cells, pairs, errbuf, errlen))) return rc;
        if (cells != n_cells) { set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(cells) + " cells, the caller's sums hold " + std::to_string(n_cells)); return SD_ERR_PARAM; }
        if (cells) SD_HIP(hipMemsetAsync(d_sums, 0, sizeof(int64_t) * 3 * (size_t)cells, st));
        if (n_rows == 0) return SD_OK;
        // (the segments' starts stay on the device: the classes need lengths only; the text is ACGTN, as every DeviceReads is)
        std::vector<int64_t> none;
        const HeatJob j{nullptr, none.data(), c.h_len.p, goff.data(), coff.data(), n_reads, B, W};
        int64_t cl[3];
        heat_classes(j, true, cl);
        if (classes) { classes[0] = cl[0]; classes[1] = cl[1]; classes[2] = cl[2]; }
        heat_upload_groups(c, st, goff.data(), coff.data(), n_reads);
        heat_plan(c, st, n_rows, n_reads, W, false);
        c.in_flight(st);
        SD_HIP(hipEventSynchronize(c.ev_plan));   // the second wait: targets and work items per class, which size the launches
        c.settle();   // (nothing behind the plan yet: the checkpoints may grow)
        for (const HeatLaunch& L : heat_launches(c)) heat_walk(c, st, L, n_reads, B, W, d_sums, 0);
        c.in_flight(st);
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_heat_identities(const int64_t* sums, int64_t n_cells, double* out) {
    for (int64_t i = 0; i < n_cells; ++i) out[i] = sd::heat_pooled(sums + 3 * i);
}

}  // extern "C"
