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
//   sd_cyclic_pairs_long<K, L>  queries of 2 049 .. 16 384 bp: a query lies over a team of L lanes, K words of Pv / Mv per
//                       lane in 32-bit halves; the columns run down the team as a systolic pipeline (sd_cyclic.hpp, "the team
//                       form"), lane l at step s on column s - l.  What a lane hands down -- the carry's two bits and the
//                       column's symbol -- is one register, moved by one DPP wave_shr:1; a team's lane 0 ignores what it
//                       gets from the team before it and decodes the target through the scalar path of the lane kernel.  A
//                       wave holds 64 / L teams, different queries against the same target, so the steps are uniform; a
//                       workgroup's four waves take the targets of a run in turn.  The group's masks sit in LDS as
//                       [word of the lane][symbol][lane of the wave], 2 KB x K: the symbol moves a lane's address by 512 B,
//                       twice round the 64 banks, so a read's bank is (2 x lane) mod 64 whatever symbols the lanes
//                       hold, and each half wave of a ds_read_b64 covers the banks once.  The team's last lane applies the
//                       end rule and writes the pair with three vector stores.
// The host builds everything the kernels read (masks, packed targets, groups, units); the inputs are kilobytes.  Pairs beyond
// the device's limits (query > 16 384 bp, target > 65 535 bp) are computed by the host form inside the same call.
#include <atomic>
#include <cstring>

#include "sd_cyclic.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"

static_assert(SD_CYCLIC_QMAX == sd::CYCLIC_QMAX && SD_CYCLIC_TMAX == sd::CYCLIC_TMAX && SD_CYCLIC_LAUNCH_WG_MIN == sd::CYCLIC_LAUNCH_WG_MIN,
              "include/sd_hip.h states the limits");
static_assert(sd::CYCLIC_LANES * 4 * sd::CYCLIC_WMAX * 8 <= 65536, "a group's masks fit the LDS of a workgroup");
static_assert(SD_CYCLIC_QMAX_LONG == sd::CYCLIC_QMAX_LONG && sd::CYCLIC_QMAX_LONG == 64 * sd::CYCLIC_TEAM_KMAX * sd::CYCLIC_LANES,
              "include/sd_hip.h states the team kernel's limit: four words in each of a wave's lanes");

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

// The team form.  One strand of a target of n bases for the team this lane belongs to: l = the lane's place in its team,
// e = the masks at this lane ([b][symbol][64]), m = the team's query.  Every lane of the wave runs every step (the DPP move
// needs them all); a lane whose column is outside the strand leaves its words and what it hands down as they are.  The
// result is the last lane's.
template <int K, int L>
__device__ inline CyclicBest cy_team_strand(const uint64_t* e, int m, int l, const uint32_t* tw, int n, int st) {
    const int pad = cyclic_pad(m, K * L);
    uint32_t PvL[K], PvH[K], MvL[K], MvH[K];
#pragma unroll
    for (int b = 0; b < K; ++b) {
        const uint64_t pv = cyclic_fresh_pv(pad, l * K + b);
        PvL[b] = (uint32_t)pv; PvH[b] = (uint32_t)(pv >> 32); MvL[b] = MvH[b] = 0u;
    }
    CyclicBest best = cyclic_fresh(m);
    const int cols = 2 * n - 1, steps = cyclic_team_steps(cols, L);
    uint32_t hand = 0u;
    int p = 0, cur = -1, c0 = 0;
    uint32_t word = 0;
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        // what the lane above handed down at its previous step: one DPP move (wave lane 0 gets 0)
        uint32_t in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hand, 0x138 /*wave_shr:1*/, 0xf, 0xf, true);
        if (s < cols) {   // column s enters at lane 0 (s, p, the word: the same in every lane)
            const int x = cyclic_index(p, n, st);
            if ((x >> 4) != cur) { cur = x >> 4; word = tw[cur]; }
            c0 = (word >> (2 * (x & 15))) & 3;
            if (st) c0 = 3 - c0;
            if (++p == n) p = 0;
        }
        if (l == 0) in = cyclic_team_pack(0u, 0u, c0);   // (a team's first lane: not the last lane of the team before)
        const int j = cyclic_team_column(s, l);
        if ((unsigned)j < (unsigned)cols) {
            hand = cyclic_team_lane<K>(PvL, PvH, MvL, MvH, in, [&](int c, int b) { return e[(b * 4 + c) * CYCLIC_LANES]; });
            cyclic_take(best, cyclic_team_delta(hand), j);   // (means something in the last lane only, where j = s - (L - 1))
        }
    }
    return best;
}

template <int K, int L>
__global__ __launch_bounds__(CY_T) void sd_cyclic_pairs_long(CyArgs a) {
    extern __shared__ uint64_t speq[];   // [K][4][64]
    const CyUnit u = a.units[a.unit0 + blockIdx.x];
    const CyGroup g = a.groups[u.group];   // nq <= 64 / L teams
    const uint64_t* src = a.peq + (int64_t)g.peq64 * 64;
    for (int i = threadIdx.x; i < 4 * K * CYCLIC_LANES; i += CY_T) speq[i] = src[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int team = lane / L, l = lane % L;
    const bool live = team < g.nq;          // (the lanes of a missing team run along on masks of 0 and write nothing)
    const bool writes = live && l == L - 1;
    const int qs = g.q0 + (live ? team : 0);
    const int m = a.qlen[qs], rad = a.qrad[qs];
    const int64_t row = (int64_t)a.qrow[qs] * a.k;
    for (int t = u.t0 + wave; t < u.t0 + u.nt; t += CYCLIC_WAVES) {
        const int n = a.tlen[t];
        const int64_t at = row + a.tcol[t];
        const bool close = abs(m - n) <= rad;
        if (__ballot(close && live) == 0) {   // the length condition fails in every team
            if (writes) { a.dist[at] = -1; a.end[at] = -1; a.strand[at] = 0; }
            continue;
        }
        const uint32_t* tw = a.tw + a.toff[t];
        CyclicBest plus = cyclic_fresh(m), minus = plus;
#pragma unroll 1
        for (int st = 0; st < 2; ++st) {
            const CyclicBest best = cy_team_strand<K, L>(speq + lane, m, l, tw, n, st);
            if (st) minus = best; else plus = best;
        }
        if (writes) {
            const int st = cyclic_strand(plus.best, minus.best);
            a.dist[at] = close ? (st ? minus.best : plus.best) : -1;
            a.end[at] = close ? (st ? minus.end : plus.end) : -1;
            a.strand[at] = close ? (uint8_t)st : (uint8_t)0;
        }
    }
}

}  // namespace sd

namespace sdi {
namespace {

std::atomic<int64_t> g_cy_launches{0};        // launches of the lane kernel sd_cyclic_pairs in this process (sd_cyclic_info)
std::atomic<int64_t> g_cy_long_launches{0};   // ... of the team kernel sd_cyclic_pairs_long (sd_cyclic_long_info)

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

// a forced class of the team kernel: one of the twelve, and no query of the call longer than it holds
int cy_team_args(const char* who, const CySeqs& S, const int32_t* qi, int32_t m, int32_t K, int32_t L, char* errbuf, size_t errlen) {
    if (!sd::cyclic_team_is_class(K, L)) {
        set_err(errbuf, errlen, std::string(who) + ": K = " + std::to_string(K) + ", L = " + std::to_string(L) + " is no class of the team kernel (K 1 .. 4 words, L 16, 32 or 64 lanes)");
        return SD_ERR_PARAM;
    }
    for (int32_t a = 0; a < m; ++a)
        if (S.len[(size_t)qi[a]] > 64 * K * L) {
            set_err(errbuf, errlen, std::string(who) + ": query " + std::to_string(a) + " has " + std::to_string(S.len[(size_t)qi[a]]) + " bases, the class of " +
                                        std::to_string(K) + " words x " + std::to_string(L) + " lanes holds " + std::to_string(64 * K * L));
            return SD_ERR_PARAM;
        }
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
    int W, L;   // L = 0: the lane kernel at W words; else the team kernel <K = W, L>
    int64_t unit0;
    unsigned n_units;
};
// A bench call times one of the two kernels and plans only that kernel's queries.  team, K = L = 0: the queries of the team
// kernel in the classes the library chooses; K, L > 0: every query of at most 64 K L bp in that class.
struct CyBench {
    int warmup, reps, variant;
    float* ms;
    int64_t* info;
    bool team;
    int K, L;
};
// the class of a query of m bp: {W, 0} the lane kernel, {K, L} the team kernel, {0, 0} the host
struct CyClass {
    int W, L;
    int key() const { return L == 0 ? W : 1024 + W * L * 8 + W; }   // classes in launch order: lanes by words, teams by capacity
    int per_group() const { return L == 0 ? sd::CYCLIC_LANES : sd::CYCLIC_LANES / L; }
};
CyClass cy_class(int m, const CyBench* bench) {
    if (bench && bench->team && bench->K > 0) return m <= 64 * bench->K * bench->L ? CyClass{bench->K, bench->L} : CyClass{0, 0};
    if (m <= sd::CYCLIC_QMAX) return bench && bench->team ? CyClass{0, 0} : CyClass{sd::cyclic_class(m), 0};
    if (m <= sd::CYCLIC_QMAX_LONG && !(bench && !bench->team)) {
        const sd::CyclicTeam c = sd::cyclic_team_class(m);
        return CyClass{c.K, c.L};
    }
    return CyClass{0, 0};
}

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
template <int K>
void cy_launch_long(hipStream_t st, unsigned grid, const sd::CyArgs& a, int L) {
    const size_t lds = (size_t)K * 4 * sd::CYCLIC_LANES * sizeof(uint64_t);
    switch (L) {
        case 16: hipLaunchKernelGGL((sd::sd_cyclic_pairs_long<K, 16>), dim3(grid), dim3(sd::CY_T), lds, st, a); break;
        case 32: hipLaunchKernelGGL((sd::sd_cyclic_pairs_long<K, 32>), dim3(grid), dim3(sd::CY_T), lds, st, a); break;
        default: hipLaunchKernelGGL((sd::sd_cyclic_pairs_long<K, 64>), dim3(grid), dim3(sd::CY_T), lds, st, a); break;
    }
}
void cy_launch(hipStream_t st, const CyLaunch& l, sd::CyArgs a, int variant) {
    a.unit0 = l.unit0;
    if (l.L > 0) {
        switch (l.W) {
            case 1: cy_launch_long<1>(st, l.n_units, a, l.L); break;
            case 2: cy_launch_long<2>(st, l.n_units, a, l.L); break;
            case 3: cy_launch_long<3>(st, l.n_units, a, l.L); break;
            default: cy_launch_long<4>(st, l.n_units, a, l.L); break;
        }
        SD_HIP(hipGetLastError());
        return;
    }
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

// The pairs of a checked call on `device`: the in-limit rows x in-limit columns through the kernels -- a row's class
// (cy_class) says which, the lane kernel's groups and launches first, then the team kernel's, on one stream into one set of
// arrays -- the rest on host threads.  Throws HipFail.
void cy_dev(CyCtx& c, hipStream_t st, const CySeqs& S, const int32_t* qi, const int32_t* ti, int32_t m, int32_t k, const int32_t* radius,
            int threads, int32_t* dist, int32_t* end, uint8_t* strand, const CyBench* bench) {
    const int64_t pairs = (int64_t)m * k;
    if (pairs == 0) return;
    std::vector<uint8_t> row_in((size_t)m), col_in((size_t)k);
    std::vector<int32_t> rows, cols;
    auto cls = [&](int32_t a) { return cy_class(S.len[(size_t)qi[a]], bench); };
    for (int32_t a = 0; a < m; ++a)
        if ((row_in[(size_t)a] = cls(a).W > 0)) rows.push_back(a);
    for (int32_t b = 0; b < k; ++b)
        if ((col_in[(size_t)b] = S.len[(size_t)ti[b]] <= sd::CYCLIC_TMAX)) cols.push_back(b);
    const bool on_device = !rows.empty() && !cols.empty();
    if (on_device) {
        // the queries by class; groups of 64 queries with masks as [symbol][word][lane] for the lane kernel, of 64 / L
        // queries with masks as [word of the lane][symbol][lane of the wave] for the team kernel
        std::stable_sort(rows.begin(), rows.end(), [&](int32_t x, int32_t y) { return cls(x).key() < cls(y).key(); });
        const size_t nq = rows.size(), nt = cols.size();
        std::vector<int32_t> q3(3 * nq), t2(2 * nt);
        std::vector<sd::CyGroup> groups;
        std::vector<CyClass> group_w;
        int64_t peq64 = 0;
        for (size_t x = 0; x < nq;) {
            const CyClass W = cls(rows[x]);
            size_t e = x;
            while (e < nq && e - x < (size_t)W.per_group() && cls(rows[e]).key() == W.key()) ++e;
            groups.push_back(sd::CyGroup{(int32_t)peq64, (int32_t)x, (int32_t)(e - x), 0});
            group_w.push_back(W);
            peq64 += 4 * W.W;
            x = e;
        }
        std::vector<uint64_t> peq((size_t)peq64 * 64, 0);
        sd::parallel_for((int64_t)groups.size(), threads, 1, [&](int64_t gi) {
            const sd::CyGroup& g = groups[(size_t)gi];
            const CyClass W = group_w[(size_t)gi];
            uint64_t* base = peq.data() + (size_t)g.peq64 * 64;
            std::vector<uint64_t> team;
            for (int l = 0; l < g.nq; ++l) {
                const int32_t s = qi[rows[(size_t)(g.q0 + l)]];
                if (W.L == 0) {
                    sd::cyclic_masks(S.seq(s), S.len[(size_t)s], W.W, base + l, sd::CYCLIC_LANES);
                    continue;
                }
                const int K = W.W, nw = K * W.L;   // team l of the wave: word w = lane K + b of symbol c at [b][c][l L + lane]
                team.assign(4 * (size_t)nw, 0);
                sd::cyclic_masks(S.seq(s), S.len[(size_t)s], nw, team.data());
                for (int c = 0; c < 4; ++c)
                    for (int w = 0; w < nw; ++w) base[((size_t)(w % K) * 4 + c) * sd::CYCLIC_LANES + (size_t)l * W.L + w / K] = team[(size_t)c * nw + w];
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
        // (the team kernel: a run has a target for each of the workgroup's waves before its columns close it -- a wave there
        // holds 1 to 4 queries, not 64, and two targets of 2 054 bases would leave half the workgroup without work)
        struct Run { int32_t t0, nt; int64_t cols; };
        auto make_runs = [&](int nt_min) {
            std::vector<Run> runs;
            for (size_t y = 0; y < nt;) {
                Run r{(int32_t)y, 0, 0};
                while (y < nt && r.nt < sd::CYCLIC_TB && (r.nt < nt_min || r.cols < sd::CYCLIC_TB_COLS)) {
                    r.cols += 2 * (2 * (int64_t)t2[y] - 1);
                    ++r.nt;
                    ++y;
                }
                runs.push_back(r);
            }
            return runs;
        };
        const std::vector<Run> lane_runs = make_runs(1), team_runs = make_runs(sd::CYCLIC_WAVES);
        // units by class (the groups are in class order), launches closed at CYCLIC_LAUNCH_WORK word steps; a team's steps
        // count its pad words and the L - 1 ramp steps of each strand
        std::vector<sd::CyUnit> units;
        std::vector<CyLaunch> launches;
        int64_t work = 0, steps = 0, n_lane = 0, n_long = 0;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            const CyClass W = group_w[gi];
            for (const Run& r : W.L ? team_runs : lane_runs) {
                const int64_t w = W.L ? (r.cols + 2 * (int64_t)(W.L - 1) * r.nt) * W.W * W.L * groups[gi].nq : r.cols * W.W * groups[gi].nq;
                if (launches.empty() || launches.back().W != W.W || launches.back().L != W.L ||
                    (work + w > sd::CYCLIC_LAUNCH_WORK && launches.back().n_units >= (unsigned)sd::CYCLIC_LAUNCH_WG_MIN)) {
                    launches.push_back(CyLaunch{W.W, W.L, (int64_t)units.size(), 0});
                    ++(W.L ? n_long : n_lane);
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
            g_cy_launches.fetch_add(n_lane);
            g_cy_long_launches.fetch_add(n_long);
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
    const CyBench b{warmup, reps, variant, ms_pairs, info, false, 0, 0};
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

int sd_cyclic_pairs_team_host(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti, int32_t m,
                              int32_t k, int32_t K, int32_t L, int32_t threads, int32_t* dist, int32_t* end, uint8_t* strand, char* errbuf,
                              size_t errlen) try {
    static const char* who = "sd_cyclic_pairs_team_host";
    CySeqs S;
    int rc = cy_seqs(who, text, off, lens, n, INT32_MAX, S, errbuf, errlen);
    if (rc) return rc;
    if ((rc = cy_pair_args(who, S, qi, ti, m, k, !dist || !end || !strand, errbuf, errlen))) return rc;
    if ((rc = cy_team_args(who, S, qi, m, K, L, errbuf, errlen))) return rc;
    sd::parallel_for((int64_t)m * k, std::max(1, threads), 1, [&](int64_t x) {
        const int32_t a = (int32_t)(x / k), b = (int32_t)(x - (int64_t)a * k);
        const int32_t q = qi[a], t = ti[b];
        thread_local sd::CyclicTeamScratch sc;
        sd::cyclic_pair_team(S.seq(q), S.len[(size_t)q], S.seq(t), S.len[(size_t)t], K, L, sc, dist + x, end + x, strand + x);
    });
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_cyclic_long_info(int64_t info[4]) {
    info[0] = sd::CYCLIC_QMAX_LONG;
    info[1] = g_cy_long_launches.load();
    info[2] = sd::CYCLIC_TEAM_N_CLASSES;
    info[3] = sd::CYCLIC_LANES / sd::CYCLIC_TEAM_LS[0];
}

int sd_cyclic_long_kernel_bench(const char* text, const int64_t* off, const int64_t* lens, int32_t n, const int32_t* qi, const int32_t* ti, int32_t m,
                                int32_t k, int32_t device, int32_t K, int32_t L, int32_t warmup, int32_t reps, float* ms_pairs, int64_t info[4],
                                int32_t* dist, int32_t* end, uint8_t* strand) try {
    static const char* who = "sd_cyclic_long_kernel_bench";
    if (warmup < 0 || reps < 1 || !ms_pairs || !info || m <= 0 || k <= 0) return SD_ERR_PARAM;
    for (int i = 0; i < 4; ++i) info[i] = 0;
    for (int i = 0; i < reps; ++i) ms_pairs[i] = 0;
    if (K != 0 || L != 0) {   // a forced class: checked before any device work
        CySeqs S;
        int rc = cy_seqs(who, text, off, lens, n, INT32_MAX, S, nullptr, 0);
        if (rc) return rc;
        if ((rc = cy_pair_args(who, S, qi, ti, m, k, false, nullptr, 0))) return rc;
        if ((rc = cy_team_args(who, S, qi, m, K, L, nullptr, 0))) return rc;
    }
    const CyBench b{warmup, reps, CY_DEFAULT, ms_pairs, info, true, K, L};
    std::vector<int32_t> d, e;
    std::vector<uint8_t> s;
    if (!dist || !end || !strand) {
        d.resize((size_t)m * (size_t)k);
        e.resize(d.size());
        s.resize(d.size());
        dist = d.data(); end = e.data(); strand = s.data();
    }
    return cy_pairs_dev(who, text, off, lens, n, qi, ti, m, k, device, 16, dist, end, strand, nullptr, 0, &b);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
