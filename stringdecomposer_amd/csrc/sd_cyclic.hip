// sd_cyclic.hip -- cyclic pairs and the merge of seed monomers (--autocorr-merge, bin/sd-merge): the infix edit distance of
// a query to a target written twice, on both strands, with the place where the best fit ends.  sd_cyclic.hpp holds the rule
// and everything host and device compute alike; this file holds the kernel, the host form and the C-ABI (include/sd_hip.h:
// sd_cyclic_*).
//   sd_cyclic_pairs<W, U>  (U: the column in 32-bit halves, the classes of up to four words)
//                       one lane per (query, target), a wave's lanes share the target: a workgroup (4 waves) takes a group
//                       of up to 64 queries of one word class W and up to CYCLIC_TB targets; its waves take the targets in
//                       turn, + strand then - strand.  The group's match masks sit in LDS as [symbol][word][lane] -- a
//                       column's W reads are 64 consecutive words each, free of bank conflicts (the [query][symbol][word]
//                       order of sd_hw_dist puts every lane of a read on one bank at W = 32) -- 2 KB x W, 64 KB at 32
//                       words.  The target's bases are 2-bit codes, 16 to a word; the word's index is the same in every
//                       lane, so it comes through a scalar load, once per 16 columns.  The text is not doubled: the column
//                       counter wraps at |t|.  Per column, after the last word: cyclic_take.  The strand is chosen in the
//                       lane; a pair's result is three plain vector stores.  No atomics; nothing depends on the geometry.
// The host builds everything the kernel reads (masks, packed targets, groups, units); the inputs are kilobytes.  Pairs beyond
// the device's limits (query > 2 048 bp, target > 65 535 bp) are computed by the host form inside the same call.
#include <atomic>
#include <cstring>

#include "sd_cyclic.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"

static_assert(SD_CYCLIC_QMAX == sd::CYCLIC_QMAX && SD_CYCLIC_TMAX == sd::CYCLIC_TMAX && SD_CYCLIC_LAUNCH_WG_MIN == sd::CYCLIC_LAUNCH_WG_MIN,
              "include/sd_hip.h states the limits");
static_assert(sd::CYCLIC_LANES * 4 * sd::CYCLIC_WMAX * 8 <= 65536, "a group's masks fit the LDS of a workgroup");

namespace sd {

constexpr int CY_T = CYCLIC_LANES * CYCLIC_WAVES;

struct CyUnit {    // a workgroup: a group of queries and a run of targets
    int32_t group, t0, nt, pad;
};
struct CyGroup {   // up to 64 queries of one class, consecutive in the sorted order
    int32_t peq64, q0, nq, pad;   // peq64: the group's masks start at word 64 * peq64
};
struct CyArgs {
    const uint64_t* peq;
    const CyUnit* units;
    const CyGroup* groups;
    const int32_t *qlen, *qrow, *qrad;   // per sorted query: length, row of the result, radius of the length condition
    const uint32_t* tw;                  // the targets' codes, 16 to a word, every target on a word of its own
    const int64_t* toff;                 // per target: its first word
    const int32_t *tlen, *tcol;          // per target: length, column of the result
    int32_t k;
    int64_t unit0;
    int32_t* dist;
    int32_t* end;
    uint8_t* strand;
};

// cyclic_step in 32-bit halves, as sd_hw_dist_u (sd_filter.hip) has it: the three-input boolean steps are single
// v_bitop3_b32 instructions (truth table over a = 0xF0, b = 0xCC, c = 0xAA), the carries between words are plain 0 / 1
// values.  The same column, bit for bit.
template <int W, class Eq>
__device__ inline int cyclic_step_u(uint32_t* PvL, uint32_t* PvH, uint32_t* MvL, uint32_t* MvH, Eq&& eq) {
    constexpr uint32_t TT_XH = (0xF0 ^ 0xCC) | 0xAA;               // (a ^ b) | c
    constexpr uint32_t TT_ORN = 0xF0 | (~(0xCC | 0xAA) & 0xFF);    // a | ~(b | c)
    uint32_t cP = 0, cM = 0;
#pragma unroll
    for (int b = 0; b < W; ++b) {
        const uint64_t E = eq(b);
        uint32_t EqL = (uint32_t)E;
        const uint32_t EqH = (uint32_t)(E >> 32);
        const uint32_t pvL = PvL[b], pvH = PvH[b], mvL = MvL[b], mvH = MvH[b];
        const uint32_t XvL = EqL | mvL, XvH = EqH | mvH;
        EqL |= cM;
        const uint64_t sum = (((uint64_t)(EqH & pvH) << 32) | (EqL & pvL)) + (((uint64_t)pvH << 32) | pvL);
        const uint32_t XhL = __builtin_amdgcn_bitop3_b32((uint32_t)sum, pvL, EqL, TT_XH);
        const uint32_t XhH = __builtin_amdgcn_bitop3_b32((uint32_t)(sum >> 32), pvH, EqH, TT_XH);
        uint32_t PhL = __builtin_amdgcn_bitop3_b32(mvL, XhL, pvL, TT_ORN);
        uint32_t PhH = __builtin_amdgcn_bitop3_b32(mvH, XhH, pvH, TT_ORN);
        uint32_t MhL = pvL & XhL, MhH = pvH & XhH;
        const uint32_t oP = PhH >> 31, oM = MhH >> 31;
        PhH = __builtin_amdgcn_alignbit(PhH, PhL, 31);
        MhH = __builtin_amdgcn_alignbit(MhH, MhL, 31);
        PhL = (PhL << 1) | cP;
        MhL = (MhL << 1) | cM;
        PvL[b] = __builtin_amdgcn_bitop3_b32(MhL, XvL, PhL, TT_ORN);
        PvH[b] = __builtin_amdgcn_bitop3_b32(MhH, XvH, PhH, TT_ORN);
        MvL[b] = PhL & XvL;
        MvH[b] = PhH & XvH;
        cP = oP;
        cM = oM;
    }
    return (int)cP - (int)cM;
}

// The columns of one strand of a target of n bases (tw: its codes) for the lane's query of m bases, masks at e[(c * W + b) *
// 64].  U: the column in 32-bit halves (cyclic_step_u) instead of 64-bit words (cyclic_step).
template <int W, bool U>
__device__ inline CyclicBest cy_strand(const uint64_t* e, int m, const uint32_t* tw, int n, int st) {
    const int pad = cyclic_pad(m, W);
    uint64_t Pv[U ? 1 : W], Mv[U ? 1 : W];
    uint32_t PvL[U ? W : 1], PvH[U ? W : 1], MvL[U ? W : 1], MvH[U ? W : 1];
#pragma unroll
    for (int b = 0; b < W; ++b) {
        const uint64_t pv = cyclic_fresh_pv(pad, b);
        if constexpr (U) { PvL[b] = (uint32_t)pv; PvH[b] = (uint32_t)(pv >> 32); MvL[b] = MvH[b] = 0u; }
        else { Pv[b] = pv; Mv[b] = 0ull; }
    }
    CyclicBest best = cyclic_fresh(m);
    int p = 0, cur = -1;
    uint32_t word = 0;
#pragma unroll 1
    for (int j = 0; j < 2 * n - 1; ++j) {
        const int x = cyclic_index(p, n, st);
        if ((x >> 4) != cur) { cur = x >> 4; word = tw[cur]; }   // (the same in every lane)
        int c = (word >> (2 * (x & 15))) & 3;
        if (st) c = 3 - c;
        const uint64_t* ec = e + (size_t)c * W * CYCLIC_LANES;
        auto eq = [&](int b) { return ec[b * CYCLIC_LANES]; };
        int hout;
        if constexpr (U) hout = cyclic_step_u<W>(PvL, PvH, MvL, MvH, eq);
        else hout = cyclic_step<W>(Pv, Mv, W, eq);
        cyclic_take(best, hout, j);
        if (++p == n) p = 0;
    }
    return best;
}

template <int W, bool U>
__global__ __launch_bounds__(CY_T) void sd_cyclic_pairs(CyArgs a) {
    extern __shared__ uint64_t speq[];   // [4][W][64]
    const CyUnit u = a.units[a.unit0 + blockIdx.x];
    const CyGroup g = a.groups[u.group];
    const uint64_t* src = a.peq + (int64_t)g.peq64 * 64;
    for (int i = threadIdx.x; i < 4 * W * CYCLIC_LANES; i += CY_T) speq[i] = src[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (lane >= g.nq) return;   // (no barrier behind this line)
    const int qs = g.q0 + lane;
    const int m = a.qlen[qs], rad = a.qrad[qs];
    const int64_t row = (int64_t)a.qrow[qs] * a.k;
    for (int t = u.t0 + wave; t < u.t0 + u.nt; t += CYCLIC_WAVES) {
        const int n = a.tlen[t];
        const int64_t at = row + a.tcol[t];
        const bool close = abs(m - n) <= rad;
        if (__ballot(close) == 0) {   // the length condition fails in every lane
            a.dist[at] = -1; a.end[at] = -1; a.strand[at] = 0;
            continue;
        }
        const uint32_t* tw = a.tw + a.toff[t];
        CyclicBest plus = cyclic_fresh(m), minus = plus;
#pragma unroll 1
        for (int st = 0; st < 2; ++st) {
            const CyclicBest best = cy_strand<W, U>(speq + lane, m, tw, n, st);
            if (st) minus = best; else plus = best;   // (two values, not an array: no scratch memory)
        }
        const int st = cyclic_strand(plus.best, minus.best);
        a.dist[at] = close ? (st ? minus.best : plus.best) : -1;
        a.end[at] = close ? (st ? minus.end : plus.end) : -1;
        a.strand[at] = close ? (uint8_t)st : (uint8_t)0;
    }
}

}  // namespace sd

namespace sdi {
namespace {

std::atomic<int64_t> g_cy_launches{0};   // launches of the pair kernel in this process (sd_cyclic_info)

// the sequences of a call, checked: codes 0 .. 3 back to back
struct CySeqs {
    std::vector<uint8_t> codes;
    std::vector<int64_t> at;     // n + 1
    std::vector<int32_t> len;
    int32_t n = 0;
    const uint8_t* seq(int32_t i) const { return codes.data() + at[(size_t)i]; }
};
int cy_seqs(const char* who, const char* text, const int64_t* off, const int64_t* lens, int32_t n, int64_t n_max, CySeqs& S, char* errbuf, size_t errlen) {
    if (n < 0 || (n > 0 && (!text || !off || !lens))) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    if (n > n_max) { set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(n) + " sequences, the cap is " + std::to_string(n_max)); return SD_ERR_PARAM; }
    S.n = n;
    S.at.assign((size_t)n + 1, 0);
    S.len.resize((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        if (off[i] < 0) { set_err(errbuf, errlen, std::string(who) + ": sequence " + std::to_string(i) + " has a negative offset"); return SD_ERR_PARAM; }
        if (lens[i] < 1) { set_err(errbuf, errlen, std::string(who) + ": sequence " + std::to_string(i) + " is empty"); return SD_ERR_PARAM; }
        if (lens[i] >= ((int64_t)1 << 30)) { set_err(errbuf, errlen, std::string(who) + ": sequence " + std::to_string(i) + " has 2^30 bases or more"); return SD_ERR_PARAM; }
        S.len[(size_t)i] = (int32_t)lens[i];
        S.at[(size_t)i + 1] = S.at[(size_t)i] + lens[i];
    }
    S.codes.resize((size_t)S.at[(size_t)n]);
    for (int32_t i = 0; i < n; ++i) {
        const uint8_t* s = reinterpret_cast<const uint8_t*>(text) + off[i];
        uint8_t* d = S.codes.data() + S.at[(size_t)i];
        for (int64_t x = 0; x < lens[i]; ++x) {
            const int c = sd::cyclic_code(s[x]);
            if (c < 0) {
                set_err(errbuf, errlen, std::string(who) + ": sequence " + std::to_string(i) + " holds a byte outside ACGT at position " + std::to_string(x));
                return SD_ERR_PARAM;
            }
            d[x] = (uint8_t)c;
        }
    }
    return SD_OK;
}
int cy_pair_args(const char* who, const CySeqs& S, const int32_t* qi, const int32_t* ti, int32_t m, int32_t k, bool no_output, char* errbuf, size_t errlen) {
    if (m < 0 || k < 0 || (m > 0 && !qi) || (k > 0 && !ti) || ((int64_t)m * k > 0 && no_output)) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    if ((int64_t)m * k > sd::CYCLIC_PAIRS_MAX) {
        set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(m) + " x " + std::to_string(k) + " pairs, the cap is " + std::to_string(sd::CYCLIC_PAIRS_MAX) + " per call");
        return SD_ERR_PARAM;
    }
    for (int32_t a = 0; a < m; ++a)
        if (qi[a] < 0 || qi[a] >= S.n) { set_err(errbuf, errlen, std::string(who) + ": query " + std::to_string(a) + " is not a sequence"); return SD_ERR_PARAM; }
    for (int32_t b = 0; b < k; ++b)
        if (ti[b] < 0 || ti[b] >= S.n) { set_err(errbuf, errlen, std::string(who) + ": target " + std::to_string(b) + " is not a sequence"); return SD_ERR_PARAM; }
    return SD_OK;
}

// ---- the host form ------------------------------------------------------------------------------------------------------
// the pairs (a, b) with want(a, b); radius (may be null): the length condition per query, a pair that fails it gets dist -1
template <class Want>
void cy_host(const CySeqs& S, const int32_t* qi, const int32_t* ti, int32_t m, int32_t k, const int32_t* radius, int threads, Want&& want,
             int32_t* dist, int32_t* end, uint8_t* strand) {
    sd::parallel_for((int64_t)m * k, threads, 1, [&](int64_t x) {
        const int32_t a = (int32_t)(x / k), b = (int32_t)(x - (int64_t)a * k);
        if (!want(a, b)) return;
        const int32_t q = qi[a], t = ti[b];
        if (radius && std::abs(S.len[(size_t)q] - S.len[(size_t)t]) > radius[a]) { dist[x] = -1; end[x] = -1; strand[x] = 0; return; }
        thread_local sd::CyclicScratch sc;
        sd::cyclic_pair(S.seq(q), S.len[(size_t)q], S.seq(t), S.len[(size_t)t], sc, dist + x, end + x, strand + x);
    });
}

// ---- the device form ----------------------------------------------------------------------------------------------------
struct CyCtx : DevWork {
    DevBuf<uint64_t> peq;
    DevBuf<sd::CyUnit> units;
    DevBuf<sd::CyGroup> groups;
    DevBuf<int32_t> q3, t2, dist, end;   // q3: qlen | qrow | qrad, t2: tlen | tcol
    DevBuf<uint32_t> tw;
    DevBuf<int64_t> toff;
    DevBuf<uint8_t> strand;
};

struct CyLaunch {
    int W;
    int64_t unit0;
    unsigned n_units;
};
struct CyBench {
    int warmup, reps, variant;
    float* ms;
    int64_t* info;
};

// The classes of up to this many words run the column in 32-bit halves (sd_cyclic_pairs<W, true>), the others in 64-bit
// words.  Both are instantiated up to four words, where they were measured against each other
// (profiles/cyclic_timing.md); sd_cyclic_kernel_bench can force either.
constexpr int CY_HALVES_UP_TO = 4;   // (the halves are 15 to 30 % ahead in every class of one to four words)
enum { CY_DEFAULT = 0, CY_WORDS = 1, CY_HALVES = 2 };

template <int W>
void cy_launch_w(hipStream_t st, unsigned grid, const sd::CyArgs& a, int variant) {
    const size_t lds = (size_t)W * 4 * sd::CYCLIC_LANES * sizeof(uint64_t);
    if constexpr (W <= 4) {
        if (variant == CY_HALVES || (variant == CY_DEFAULT && W <= CY_HALVES_UP_TO)) {
            hipLaunchKernelGGL((sd::sd_cyclic_pairs<W, true>), dim3(grid), dim3(sd::CY_T), lds, st, a);
            return;
        }
    }
    hipLaunchKernelGGL((sd::sd_cyclic_pairs<W, false>), dim3(grid), dim3(sd::CY_T), lds, st, a);
}
void cy_launch(hipStream_t st, const CyLaunch& l, sd::CyArgs a, int variant) {
    a.unit0 = l.unit0;
    switch (l.W) {
        case 1: cy_launch_w<1>(st, l.n_units, a, variant); break;
        case 2: cy_launch_w<2>(st, l.n_units, a, variant); break;
        case 3: cy_launch_w<3>(st, l.n_units, a, variant); break;
        case 4: cy_launch_w<4>(st, l.n_units, a, variant); break;
        case 6: cy_launch_w<6>(st, l.n_units, a, variant); break;
        case 8: cy_launch_w<8>(st, l.n_units, a, variant); break;
        case 12: cy_launch_w<12>(st, l.n_units, a, variant); break;
        case 16: cy_launch_w<16>(st, l.n_units, a, variant); break;
        case 24: cy_launch_w<24>(st, l.n_units, a, variant); break;
        default: cy_launch_w<32>(st, l.n_units, a, variant); break;
    }
    SD_HIP(hipGetLastError());
}

// The pairs of a checked call on `device`: the in-limit rows x in-limit columns through the kernel, the rest on host
// threads.  Throws HipFail.
void cy_dev(CyCtx& c, hipStream_t st, const CySeqs& S, const int32_t* qi, const int32_t* ti, int32_t m, int32_t k, const int32_t* radius,
            int threads, int32_t* dist, int32_t* end, uint8_t* strand, const CyBench* bench) {
    const int64_t pairs = (int64_t)m * k;
    if (pairs == 0) return;
    std::vector<uint8_t> row_in((size_t)m), col_in((size_t)k);
    std::vector<int32_t> rows, cols;
    for (int32_t a = 0; a < m; ++a)
        if ((row_in[(size_t)a] = S.len[(size_t)qi[a]] <= sd::CYCLIC_QMAX)) rows.push_back(a);
    for (int32_t b = 0; b < k; ++b)
        if ((col_in[(size_t)b] = S.len[(size_t)ti[b]] <= sd::CYCLIC_TMAX)) cols.push_back(b);
    const bool on_device = !rows.empty() && !cols.empty();
    if (on_device) {
        // the queries by class, groups of 64, their masks as [symbol][word][lane]
        std::stable_sort(rows.begin(), rows.end(), [&](int32_t x, int32_t y) { return sd::cyclic_class(S.len[(size_t)qi[x]]) < sd::cyclic_class(S.len[(size_t)qi[y]]); });
        const size_t nq = rows.size(), nt = cols.size();
        std::vector<int32_t> q3(3 * nq), t2(2 * nt);
        std::vector<sd::CyGroup> groups;
        std::vector<int> group_w;
        int64_t peq64 = 0;
        for (size_t x = 0; x < nq;) {
            const int W = sd::cyclic_class(S.len[(size_t)qi[rows[x]]]);
            size_t e = x;
            while (e < nq && e - x < (size_t)sd::CYCLIC_LANES && sd::cyclic_class(S.len[(size_t)qi[rows[e]]]) == W) ++e;
            groups.push_back(sd::CyGroup{(int32_t)peq64, (int32_t)x, (int32_t)(e - x), 0});
            group_w.push_back(W);
            peq64 += 4 * W;
            x = e;
        }
        std::vector<uint64_t> peq((size_t)peq64 * 64, 0);
        sd::parallel_for((int64_t)groups.size(), threads, 1, [&](int64_t gi) {
            const sd::CyGroup& g = groups[(size_t)gi];
            const int W = group_w[(size_t)gi];
            uint64_t* base = peq.data() + (size_t)g.peq64 * 64;
            for (int l = 0; l < g.nq; ++l) {
                const int32_t s = qi[rows[(size_t)(g.q0 + l)]];
                sd::cyclic_masks(S.seq(s), S.len[(size_t)s], W, base + l, sd::CYCLIC_LANES);
            }
        });
        for (size_t x = 0; x < nq; ++x) {
            q3[x] = S.len[(size_t)qi[rows[x]]];
            q3[nq + x] = rows[x];
            q3[2 * nq + x] = radius ? radius[rows[x]] : INT32_MAX;
        }
        // the targets packed, and their runs: up to CYCLIC_TB targets, closed at CYCLIC_TB_COLS columns
        std::vector<int64_t> toff(nt + 1, 0);
        for (size_t y = 0; y < nt; ++y) {
            const int32_t n = S.len[(size_t)ti[cols[y]]];
            t2[y] = n;
            t2[nt + y] = cols[y];
            toff[y + 1] = toff[y] + (n + 15) / 16;
        }
        std::vector<uint32_t> tw((size_t)toff[nt], 0);
        sd::parallel_for((int64_t)nt, threads, 16, [&](int64_t y) {
            const int32_t s = ti[cols[(size_t)y]];
            const uint8_t* t = S.seq(s);
            uint32_t* w = tw.data() + toff[(size_t)y];
            for (int i = 0; i < S.len[(size_t)s]; ++i) w[i >> 4] |= (uint32_t)t[i] << (2 * (i & 15));
        });
        struct Run { int32_t t0, nt; int64_t cols; };
        std::vector<Run> runs;
        for (size_t y = 0; y < nt;) {
            Run r{(int32_t)y, 0, 0};
            while (y < nt && r.nt < sd::CYCLIC_TB && (r.nt == 0 || r.cols < sd::CYCLIC_TB_COLS)) {
                r.cols += 2 * (2 * (int64_t)t2[y] - 1);
                ++r.nt;
                ++y;
            }
            runs.push_back(r);
        }
        // units by class (the groups are in class order), launches closed at CYCLIC_LAUNCH_WORK word steps
        std::vector<sd::CyUnit> units;
        std::vector<CyLaunch> launches;
        int64_t work = 0, steps = 0;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            const int W = group_w[gi];
            for (const Run& r : runs) {
                const int64_t w = r.cols * W * groups[gi].nq;
                if (launches.empty() || launches.back().W != W ||
                    (work + w > sd::CYCLIC_LAUNCH_WORK && launches.back().n_units >= (unsigned)sd::CYCLIC_LAUNCH_WG_MIN)) {
                    launches.push_back(CyLaunch{W, (int64_t)units.size(), 0});
                    work = 0;
                }
                units.push_back(sd::CyUnit{(int32_t)gi, r.t0, r.nt, 0});
                ++launches.back().n_units;
                work += w;
                steps += w;
            }
        }
        c.peq.alloc(peq.size());
        c.units.alloc(units.size());
        c.groups.alloc(groups.size());
        c.q3.alloc(q3.size());
        c.t2.alloc(t2.size());
        c.tw.alloc(tw.size());
        c.toff.alloc(toff.size());
        c.dist.alloc((size_t)pairs);
        c.end.alloc((size_t)pairs);
        c.strand.alloc((size_t)pairs);
        SD_HIP(hipMemcpyAsync(c.peq.p, peq.data(), sizeof(uint64_t) * peq.size(), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.units.p, units.data(), sizeof(sd::CyUnit) * units.size(), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.groups.p, groups.data(), sizeof(sd::CyGroup) * groups.size(), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.q3.p, q3.data(), sizeof(int32_t) * q3.size(), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.t2.p, t2.data(), sizeof(int32_t) * t2.size(), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.tw.p, tw.data(), sizeof(uint32_t) * tw.size(), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(c.toff.p, toff.data(), sizeof(int64_t) * toff.size(), hipMemcpyHostToDevice, st));
        sd::CyArgs a{};
        a.peq = c.peq.p; a.units = c.units.p; a.groups = c.groups.p;
        a.qlen = c.q3.p; a.qrow = c.q3.p + nq; a.qrad = c.q3.p + 2 * nq;
        a.tw = c.tw.p; a.toff = c.toff.p; a.tlen = c.t2.p; a.tcol = c.t2.p + nt;
        a.k = k;
        a.dist = c.dist.p; a.end = c.end.p; a.strand = c.strand.p;
        auto run = [&]() {
            for (const CyLaunch& l : launches) cy_launch(st, l, a, bench ? bench->variant : CY_DEFAULT);
            g_cy_launches.fetch_add((int64_t)launches.size());
        };
        if (bench) {
            StageClock clock;
            clock.time(st, bench->warmup, bench->reps, bench->ms, run);
            bench->info[0] = (int64_t)launches.size();
            bench->info[1] = (int64_t)nq * (int64_t)nt;
            bench->info[2] = steps;
            bench->info[3] = (int64_t)units.size();
        } else {
            run();
        }
        c.in_flight(st);
        SD_HIP(hipMemcpyAsync(dist, c.dist.p, sizeof(int32_t) * (size_t)pairs, hipMemcpyDeviceToHost, st));
        SD_HIP(hipMemcpyAsync(end, c.end.p, sizeof(int32_t) * (size_t)pairs, hipMemcpyDeviceToHost, st));
        SD_HIP(hipMemcpyAsync(strand, c.strand.p, (size_t)pairs, hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));   // (the host arrays of this scope were read by the copies above)
        c.waited();
    }
    if (bench) return;   // (the bench entry times the kernel: the pairs beyond the device's limits are not computed)
    if (!on_device || rows.size() < (size_t)m || cols.size() < (size_t)k)
        cy_host(S, qi, ti, m, k, radius, threads, [&](int32_t a, int32_t b) { return !on_device || !row_in[(size_t)a] || !col_in[(size_t)b]; }, dist, end, strand);
}

int cy_pairs_dev(const char* who, const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti, int32_t m,
                 int32_t k, int32_t device, int32_t threads, int32_t* dist, int32_t* end, uint8_t* strand, char* errbuf, size_t errlen, const CyBench* bench) {
    CySeqs S;
    int rc = cy_seqs(who, text, off, lens, n, INT32_MAX, S, errbuf, errlen);
    if (rc) return rc;
    if ((rc = cy_pair_args(who, S, qi, ti, m, k, !dist || !end || !strand, errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    try {
        DeviceScope on(device);
        CyCtx& c = device_ctx<CyCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        OwnedStream st;
        cy_dev(c, st, S, qi, ti, m, k, nullptr, std::max(1, threads), dist, end, strand, bench);
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
}

int cy_merge_args(const char* who, int32_t n, const int64_t* weight, int32_t P, int32_t& block, bool no_output, char* errbuf, size_t errlen) {
    if ((n > 0 && !weight) || no_output) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    if (P < 1 || P > 100) { set_err(errbuf, errlen, std::string(who) + ": P = " + std::to_string(P) + ", the identity of a cluster is 1 .. 100 percent"); return SD_ERR_PARAM; }
    if (block < 0) { set_err(errbuf, errlen, std::string(who) + ": block = " + std::to_string(block) + ", the block is 0 (the default) or a number of sequences"); return SD_ERR_PARAM; }
    block = block == 0 ? sd::CYCLIC_BLOCK : std::min(block, sd::CYCLIC_BLOCK_MAX);
    return SD_OK;
}

}  // namespace
}  // namespace sdi

extern "C" {

int sd_cyclic_pairs_host(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti, int32_t m, int32_t k,
                         int32_t threads, int32_t* dist, int32_t* end, uint8_t* strand, char* errbuf, size_t errlen) try {
    static const char* who = "sd_cyclic_pairs_host";
    CySeqs S;
    int rc = cy_seqs(who, text, off, lens, n, INT32_MAX, S, errbuf, errlen);
    if (rc) return rc;
    if ((rc = cy_pair_args(who, S, qi, ti, m, k, !dist || !end || !strand, errbuf, errlen))) return rc;
    cy_host(S, qi, ti, m, k, nullptr, std::max(1, threads), [](int32_t, int32_t) { return true; }, dist, end, strand);
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_cyclic_pairs_dev(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti, int32_t m, int32_t k,
                        int32_t device, int32_t threads, int32_t* dist, int32_t* end, uint8_t* strand, char* errbuf, size_t errlen) try {
    return cy_pairs_dev("sd_cyclic_pairs_dev", text, off, lens, n, qi, ti, m, k, device, threads, dist, end, strand, errbuf, errlen, nullptr);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_cyclic_merge_host(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int64_t* weight, int32_t P, int32_t block,
                         int32_t threads, int32_t* cluster, int32_t* centre, int32_t* dist, int32_t* end, uint8_t* strand, int32_t* n_clusters,
                         char* errbuf, size_t errlen) try {
    static const char* who = "sd_cyclic_merge_host";
    int rc = cy_merge_args(who, n, weight, P, block, !n_clusters || (n > 0 && (!cluster || !centre || !dist || !end || !strand)), errbuf, errlen);
    if (rc) return rc;
    CySeqs S;
    if ((rc = cy_seqs(who, text, off, lens, n, sd::CYCLIC_N_MAX, S, errbuf, errlen))) return rc;
    const int th = std::max(1, threads);
    sd::CyclicMergeOut o{cluster, centre, dist, end, strand};
    sd::cyclic_merge(lens, n, weight, P, block, [&](const std::vector<int32_t>& q, const std::vector<int32_t>& t, const std::vector<int32_t>& rad,
                                                    std::vector<int32_t>& d, std::vector<int32_t>& e, std::vector<uint8_t>& s) {
        const size_t pairs = q.size() * t.size();
        d.resize(pairs); e.resize(pairs); s.resize(pairs);
        cy_host(S, q.data(), t.data(), (int32_t)q.size(), (int32_t)t.size(), rad.data(), th, [](int32_t, int32_t) { return true; }, d.data(), e.data(), s.data());
    }, o);
    *n_clusters = o.n_clusters;
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_cyclic_merge_dev(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int64_t* weight, int32_t P, int32_t block,
                        int32_t device, int32_t threads, int32_t* cluster, int32_t* centre, int32_t* dist, int32_t* end, uint8_t* strand,
                        int32_t* n_clusters, char* errbuf, size_t errlen) try {
    static const char* who = "sd_cyclic_merge_dev";
    int rc = cy_merge_args(who, n, weight, P, block, !n_clusters || (n > 0 && (!cluster || !centre || !dist || !end || !strand)), errbuf, errlen);
    if (rc) return rc;
    CySeqs S;
    if ((rc = cy_seqs(who, text, off, lens, n, sd::CYCLIC_N_MAX, S, errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    const int th = std::max(1, threads);
    try {
        DeviceScope on(device);
        CyCtx& c = device_ctx<CyCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        OwnedStream st;
        sd::CyclicMergeOut o{cluster, centre, dist, end, strand};
        sd::cyclic_merge(lens, n, weight, P, block, [&](const std::vector<int32_t>& q, const std::vector<int32_t>& t, const std::vector<int32_t>& rad,
                                                        std::vector<int32_t>& d, std::vector<int32_t>& e, std::vector<uint8_t>& s) {
            const size_t pairs = q.size() * t.size();
            d.resize(pairs); e.resize(pairs); s.resize(pairs);
            cy_dev(c, st, S, q.data(), t.data(), (int32_t)q.size(), (int32_t)t.size(), rad.data(), th, d.data(), e.data(), s.data(), nullptr);
        }, o);
        *n_clusters = o.n_clusters;
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_cyclic_canon(const char* seq, int64_t len, char* out, int64_t* rotation, int32_t* strand) try {
    if (!seq || !out || !rotation || !strand || len < 1 || len >= ((int64_t)1 << 30)) return SD_ERR_PARAM;
    for (int64_t i = 0; i < len; ++i)
        if (sd::cyclic_code((uint8_t)seq[i]) < 0) return SD_ERR_PARAM;
    const std::string c = sd::cyclic_canon(std::string(seq, (size_t)len), rotation, strand);
    std::memcpy(out, c.data(), (size_t)len);
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_cyclic_info(int64_t info[6]) {
    info[0] = sd::CYCLIC_QMAX;
    info[1] = sd::CYCLIC_TMAX;
    info[2] = sd::CYCLIC_LAUNCH_WORK;
    info[3] = g_cy_launches.load();
    info[4] = sd::CYCLIC_PAIRS_MAX;
    info[5] = sd::CYCLIC_BLOCK;
}

int sd_cyclic_kernel_bench(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti, int32_t m, int32_t k,
                           int32_t device, int32_t variant, int32_t warmup, int32_t reps, float* ms_pairs, int64_t info[4], int32_t* dist,
                           int32_t* end, uint8_t* strand) try {
    if (warmup < 0 || reps < 1 || !ms_pairs || !info || m <= 0 || k <= 0 || variant < CY_DEFAULT || variant > CY_HALVES) return SD_ERR_PARAM;
    for (int i = 0; i < 4; ++i) info[i] = 0;
    for (int i = 0; i < reps; ++i) ms_pairs[i] = 0;
    const CyBench b{warmup, reps, variant, ms_pairs, info};
    std::vector<int32_t> d, e;
    std::vector<uint8_t> s;
    if (!dist || !end || !strand) {   // (the arrays of the timed variant, for a caller that wants to compare them)
        d.resize((size_t)m * (size_t)k);
        e.resize(d.size());
        s.resize(d.size());
        dist = d.data(); end = e.data(); strand = s.data();
    }
    return cy_pairs_dev("sd_cyclic_kernel_bench", text, off, lens, n, qi, ti, m, k, device, 16, dist, end, strand, nullptr, 0, &b);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
