// sd_cyclic.hpp -- "cyclic pairs" and the merge rule on top of them (--autocorr-merge, bin/sd-merge): which seed monomers
// are the same monomer up to rotation and strand.  One text for host and device, as plain C++ that compiles for both (in
// the manner of sd_motif_edit.hpp): the pair, the limits, the bit-vector column, the team form of the column for queries
// beyond one lane's registers; and, host only, that team schedule run lane by lane, the merge walk and the canonical record.  sd_cyclic.hip holds the kernels, the host form and the C-ABI (sd_cyclic_*, include/sd_hip.h).
//
// The pair.  Sequences are upper-case A C G T only, of length >= 1.  For a query q, a target t and a strand s: t^+ is t,
// t^- its reverse complement; the text is U = t^s t^s without its last base, |U| = 2|t| - 1 -- every rotation of t^s is a
// substring of U, and none occurs twice.  D(j), 0 <= j < |U|, is the smallest unit-cost edit distance (substitution,
// insertion, deletion) of q to a substring of U that ends at j inclusive; the empty substring is allowed, so D(j) <= |q|.
// dist_s = min_j D(j), end_s = the smallest j that attains it.  The pair's result (dist, end, strand) is that of +, unless
// dist_- is strictly smaller.  phase = (end + 1) mod |t|: the position of t^strand just behind the fit, where a query that
// is a whole period begins.
//
// The text is never doubled in memory: column j reads t[j mod |t|], on - the complement of t[|t| - 1 - (j mod |t|)]
// (cyclic_index).  D is Myers' bit vector (J. ACM 46(3), 1999) in its block form (Hyyro 2003), search variant: the row above
// the pattern costs nothing, the pattern lies along the bits of W 64-bit words, the carry between words is the horizontal
// delta of a word's last row.  A query may run on more words than it fills (a wave's lanes run the same W): it is pushed
// to the top of its words over rows that stay 0 (cyclic_pad), so the delta of the bottom row is the top bit of the last word.
//
// The merge rule (host only).  n sequences, an integer weight each, P in 1 .. 100.  R(q) = floor((100 - P) |q| / 100); q
// is close to centre c when abs(|q| - |c|) <= R(q) and dist(q in c) <= R(q) -- the length condition keeps a dimer out of
// its monomer's cluster.  The sequences are visited by weight descending, then index ascending; one that is close to no
// existing centre becomes the next centre, any other joins the close centre of smallest dist, ties to the earliest centre.
// The result is a function of every sequence's pairs against the centres before it, so it is computed in blocks without
// the n x n matrix (cyclic_merge); the block size does not show in it.  A cluster's canonical record is the
// lexicographically smallest sequence among all rotations of the centre and of its reverse complement (cyclic_canon).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#ifndef SD_HD
#define SD_HD __host__ __device__
#endif
#else
#ifndef SD_HD
#define SD_HD
#endif
#endif

namespace sd {

constexpr int CYCLIC_QMAX = 2048;                       // device: the longest query of the lane kernel (32 words)
constexpr int CYCLIC_TMAX = 65535;                      // device: the longest target
constexpr int CYCLIC_WMAX = CYCLIC_QMAX / 64;
constexpr int64_t CYCLIC_PAIRS_MAX = (int64_t)1 << 24;  // pairs of one sd_cyclic_pairs_* call
constexpr int64_t CYCLIC_N_MAX = (int64_t)1 << 20;      // sequences of one sd_cyclic_merge_* call
// The merge's default block.  A block's undecided sequences are compared with each other whether or not they end up in one
// cluster, so a large block costs up to block^2 pairs that the walk does not need: at 1 024 the merge of 1 000 seeds of
// three families took as long as all pairs (profiles/cyclic_timing.md).  128 keeps two full waves of queries per call.
constexpr int CYCLIC_BLOCK = 128;
constexpr int CYCLIC_BLOCK_MAX = 4096;                  // (a block against itself is one pairs call)
// A launch of the pair kernel takes at most this many word steps: columns x words x pairs, summed over its pairs with
// columns = 2 (2 |t| - 1) for the two strands and words = the W of the query's class -- or CYCLIC_LAUNCH_WG_MIN workgroups,
// whichever is more.  The kernel runs about 1e12 word steps a second on an MI355X at three words
// (profiles/cyclic_timing.md), so a launch of short queries is a few milliseconds.  A workgroup of 32-word queries is 3e7
// steps and more (64 queries x 32 words x 16 384 columns), so the step bound alone left 64 workgroups to a launch and
// three quarters of the compute units idle: the workgroup floor fills the device twice.  The longest launch there can be is
// the floor times the largest workgroup, 64 queries x 32 words x one target of 65 535 bases: 5.5e11 steps.
constexpr int64_t CYCLIC_LAUNCH_WORK = (int64_t)1 << 31;
constexpr int CYCLIC_LAUNCH_WG_MIN = 1024;
constexpr int CYCLIC_LANES = 64;                        // queries of a group: one per lane of a wave
constexpr int CYCLIC_WAVES = 4;                         // waves of a workgroup; they share the group's match masks
constexpr int CYCLIC_TB = 8;                            // targets of a workgroup, at most
constexpr int CYCLIC_TB_COLS = 16384;                   // ... and a workgroup's targets end at this many columns

// the word classes: the smallest one that holds the query's words
constexpr int CYCLIC_CLASSES[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
constexpr int CYCLIC_N_CLASSES = 10;
SD_HD inline int cyclic_words(int m) { return (m + 63) >> 6; }
inline int cyclic_class(int m) {
    const int w = cyclic_words(m);
    for (int c = 0; c < CYCLIC_N_CLASSES; ++c)
        if (CYCLIC_CLASSES[c] >= w) return CYCLIC_CLASSES[c];
    return 0;   // (beyond the device's limit)
}

SD_HD inline int cyclic_code(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
// column j of U reads base cyclic_index(p, n, s) of t with p = j mod n, complemented (3 - code) on strand -
SD_HD inline int cyclic_index(int p, int n, int strand) { return strand ? n - 1 - p : p; }
SD_HD inline int cyclic_phase(int end, int n) { return (end + 1) % n; }
SD_HD inline int cyclic_radius(int P, int m) { return (int)((int64_t)(100 - P) * m / 100); }

// Where the query lies in its words.  A query of m rows on nw words is pushed to the top: pad = 64 nw - m rows lie below it,
// at the low bits, which match every symbol (cyclic_pad_eq) and start with a vertical delta of 0 (cyclic_fresh_pv).  Such
// rows hold 0 in every column -- with Pv = Mv = 0 and the match bit set the step gives Ph = Mh = 0 and leaves Pv = Mv = 0,
// and their sum carries nothing upwards -- so they are more copies of the free row above the pattern, and the query's
// first row sees a carry of 0 as it would at bit 0.  The query's last row is then bit 63 of the last word for every query
// of a class: nothing in the step depends on the query's length.
SD_HD inline int cyclic_pad(int m, int nw) { return 64 * nw - m; }
SD_HD inline uint64_t cyclic_low_bits(int pad, int b) {   // the pad rows of word b
    const int k = pad - 64 * b;
    return k <= 0 ? 0ull : k >= 64 ? ~0ull : (1ull << k) - 1;
}
SD_HD inline uint64_t cyclic_fresh_pv(int pad, int b) { return ~cyclic_low_bits(pad, b); }
SD_HD inline uint64_t cyclic_pad_eq(int pad, int b) { return cyclic_low_bits(pad, b); }

// One word of a column: the carry comes in and goes out through hin.
SD_HD inline void cyclic_word(uint64_t& Pv, uint64_t& Mv, uint64_t E, int& hin) {
    constexpr uint64_t top = 1ull << 63;
    const uint64_t pv = Pv, mv = Mv;
    const uint64_t Xv = E | mv;
    if (hin < 0) E |= 1ull;
    const uint64_t Xh = (((E & pv) + pv) ^ pv) | E;
    uint64_t Ph = mv | ~(Xh | pv);
    uint64_t Mh = pv & Xh;
    int hout = 0;
    if (Ph & top) hout = 1;
    if (Mh & top) hout = -1;
    Ph <<= 1;
    Mh <<= 1;
    if (hin < 0) Mh |= 1ull;
    if (hin > 0) Ph |= 1ull;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    hin = hout;
}
// One column of D over a query on nw words (WT > 0: nw = WT, known to the compiler, so that Pv / Mv stay in registers).
// eq(b) = word b of the query's match mask for the column's symbol.  Returns the delta of the bottom row, the top bit of
// the last word.
template <int WT, class Eq>
SD_HD inline int cyclic_step(uint64_t* Pv, uint64_t* Mv, int nw, Eq&& eq) {
    int hin = 0;   // search variant: the row above the pattern costs nothing
    if constexpr (WT > 0) {
#pragma unroll
        for (int b = 0; b < WT; ++b) cyclic_word(Pv[b], Mv[b], eq(b), hin);
    } else {
        for (int b = 0; b < nw; ++b) cyclic_word(Pv[b], Mv[b], eq(b), hin);
    }
    return hin;
}

// the end rule of one strand: the smallest column of the smallest score
struct CyclicBest {
    int score, best, end;
};
SD_HD inline CyclicBest cyclic_fresh(int m) { return CyclicBest{m, m + 1, 0}; }   // (D(0) <= m: column 0 always enters)
SD_HD inline void cyclic_take(CyclicBest& b, int hout, int j) {
    b.score += hout;
    if (b.score < b.best) { b.best = b.score; b.end = j; }
}
// the strand rule: + unless - is strictly smaller
SD_HD inline int cyclic_strand(int dist_plus, int dist_minus) { return dist_minus < dist_plus ? 1 : 0; }

// ---- the team form: a query across the lanes of a wave (queries of CYCLIC_QMAX + 1 .. CYCLIC_QMAX_LONG bp) ----------------
// A query lies over a team of L consecutive lanes, lane l holding words l K .. l K + K - 1 of its K L words, padded as
// above with nw = K L: the bottom row is bit 63 of the last word of the team's last lane, and a lane that is all pad passes a
// carry of 0 (its rows are copies of the free row).  The columns run as a systolic pipeline: at step s lane l computes
// column cyclic_team_column(s, l) = s - l if that is one of the strand's 2 |t| - 1 columns, else it leaves its words as they
// are; a strand takes cyclic_team_steps = 2 |t| - 1 + L - 1 steps.  What lane l hands to lane l + 1 for the next step is one
// register (cyclic_team_pack): the horizontal delta out of its last word as the two bits the halves form has (+1: bit 0,
// -1: bit 1) and the column's symbol above them, so only lane 0 reads the target.  Lane 0 takes a carry of 0 (the search
// variant).  The last lane applies cyclic_take with j = s - (L - 1): the same (score, column) sequence as cyclic_pair sees.
constexpr int CYCLIC_QMAX_LONG = 16384;                 // device: the longest query of the team kernel (256 words)
constexpr int CYCLIC_TEAM_KMAX = 4;                     // words per lane: 1 .. 4
constexpr int CYCLIC_TEAM_LS[] = {16, 32, 64};          // lanes per team
constexpr int CYCLIC_TEAM_N_L = 3;
constexpr int CYCLIC_TEAM_N_CLASSES = CYCLIC_TEAM_KMAX * CYCLIC_TEAM_N_L;
struct CyclicTeam {
    int K, L;   // K = 0: no class (beyond the limit)
};
SD_HD inline bool cyclic_team_is_class(int K, int L) { return K >= 1 && K <= CYCLIC_TEAM_KMAX && (L == 16 || L == 32 || L == 64); }
// A length's class: the (K, L) of smallest K L that holds its words.  Of equal capacities the larger K (the shorter team)
// wins: fewer ramp steps per strand and more queries to a wave (profiles/cyclic_timing.md has 4 x 16 beside 2 x 32).
SD_HD inline CyclicTeam cyclic_team_class(int m) {
    const int w = cyclic_words(m);
    CyclicTeam best{0, 0};
    for (int li = 0; li < CYCLIC_TEAM_N_L; ++li)
        for (int K = 1; K <= CYCLIC_TEAM_KMAX; ++K) {
            const int L = li == 0 ? 16 : li == 1 ? 32 : 64;
            if (K * L >= w && (best.K == 0 || K * L < best.K * best.L || (K * L == best.K * best.L && K > best.K))) best = CyclicTeam{K, L};
        }
    return best;
}
SD_HD inline int cyclic_team_column(int s, int l) { return s - l; }
SD_HD inline int cyclic_team_steps(int cols, int L) { return cols + L - 1; }
SD_HD inline uint32_t cyclic_team_pack(uint32_t cP, uint32_t cM, int sym) { return cP | (cM << 1) | ((uint32_t)sym << 2); }

// cyclic_step in 32-bit halves, as sd_hw_dist_u (sd_filter.hip) has it: on the device the three-input boolean steps are
// single v_bitop3_b32 instructions (truth table over a = 0xF0, b = 0xCC, c = 0xAA), on the host the same functions written
// out; the carries between words are plain 0 / 1 values.  The same column, bit for bit.  cP / cM: the carry into the first
// word (+1 / -1) and, on return, out of the last one.
SD_HD inline uint32_t cyclic_u_xh(uint32_t a, uint32_t b, uint32_t c) {    // (a ^ b) | c
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, (0xF0 ^ 0xCC) | 0xAA);
#else
    return (a ^ b) | c;
#endif
}
SD_HD inline uint32_t cyclic_u_orn(uint32_t a, uint32_t b, uint32_t c) {   // a | ~(b | c)
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xF0 | (~(0xCC | 0xAA) & 0xFF));
#else
    return a | ~(b | c);
#endif
}
SD_HD inline uint32_t cyclic_u_shl1(uint32_t hi, uint32_t lo) {            // the high half of (hi : lo) << 1
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, 31);
#else
    return (hi << 1) | (lo >> 31);
#endif
}
template <int W, class Eq>
SD_HD inline void cyclic_step_uc(uint32_t* PvL, uint32_t* PvH, uint32_t* MvL, uint32_t* MvH, Eq&& eq, uint32_t& cP, uint32_t& cM) {
#pragma unroll
    for (int b = 0; b < W; ++b) {
        const uint64_t E = eq(b);
        uint32_t EqL = (uint32_t)E;
        const uint32_t EqH = (uint32_t)(E >> 32);
        const uint32_t pvL = PvL[b], pvH = PvH[b], mvL = MvL[b], mvH = MvH[b];
        const uint32_t XvL = EqL | mvL, XvH = EqH | mvH;
        EqL |= cM;
        const uint64_t sum = (((uint64_t)(EqH & pvH) << 32) | (EqL & pvL)) + (((uint64_t)pvH << 32) | pvL);
        const uint32_t XhL = cyclic_u_xh((uint32_t)sum, pvL, EqL);
        const uint32_t XhH = cyclic_u_xh((uint32_t)(sum >> 32), pvH, EqH);
        uint32_t PhL = cyclic_u_orn(mvL, XhL, pvL);
        uint32_t PhH = cyclic_u_orn(mvH, XhH, pvH);
        uint32_t MhL = pvL & XhL, MhH = pvH & XhH;
        const uint32_t oP = PhH >> 31, oM = MhH >> 31;
        PhH = cyclic_u_shl1(PhH, PhL);
        MhH = cyclic_u_shl1(MhH, MhL);
        PhL = (PhL << 1) | cP;
        MhL = (MhL << 1) | cM;
        PvL[b] = cyclic_u_orn(MhL, XvL, PhL);
        PvH[b] = cyclic_u_orn(MhH, XvH, PhH);
        MvL[b] = PhL & XvL;
        MvH[b] = PhH & XvH;
        cP = oP;
        cM = oM;
    }
}
// ... a whole column: the carry into the first word is 0; returns the delta of the bottom row
template <int W, class Eq>
SD_HD inline int cyclic_step_u(uint32_t* PvL, uint32_t* PvH, uint32_t* MvL, uint32_t* MvH, Eq&& eq) {
    uint32_t cP = 0, cM = 0;
    cyclic_step_uc<W>(PvL, PvH, MvL, MvH, eq, cP, cM);
    return (int)cP - (int)cM;
}
// One lane of a team at one step: `in` = what the lane above handed down (cyclic_team_pack; lane 0: carry 0 and the column's
// symbol), eq(c, b) = word b of this lane's match mask for symbol c.  Returns what goes to the lane below.
template <int K, class Eq>
SD_HD inline uint32_t cyclic_team_lane(uint32_t* PvL, uint32_t* PvH, uint32_t* MvL, uint32_t* MvH, uint32_t in, Eq&& eq) {
    uint32_t cP = in & 1u, cM = (in >> 1) & 1u;
    const int c = (int)(in >> 2);
    cyclic_step_uc<K>(PvL, PvH, MvL, MvH, [&](int b) { return eq(c, b); }, cP, cM);
    return cyclic_team_pack(cP, cM, c);
}
SD_HD inline int cyclic_team_delta(uint32_t out) { return (int)(out & 1u) - (int)((out >> 1) & 1u); }

// ---- host only ----------------------------------------------------------------------------------------------------------

// The match masks of a query given as codes, on nw >= cyclic_words(m) words: word b of symbol c at peq[(c * nw + b) * pitch].
inline void cyclic_masks(const uint8_t* q, int m, int nw, uint64_t* peq, size_t pitch = 1) {
    const int pad = cyclic_pad(m, nw);
    for (int c = 0; c < 4; ++c)
        for (int b = 0; b < nw; ++b) peq[((size_t)c * nw + b) * pitch] = cyclic_pad_eq(pad, b);
    for (int i = 0; i < m; ++i) peq[((size_t)q[i] * nw + ((i + pad) >> 6)) * pitch] |= 1ull << ((i + pad) & 63);
}

struct CyclicScratch {
    std::vector<uint64_t> peq, pv, mv;
};

// the columns of one strand over Pv / Mv of nw words (WT > 0: nw = WT)
template <int WT>
inline CyclicBest cyclic_strand_run(const uint64_t* peq, int m, int nw, const uint8_t* t, int n, int st, uint64_t* Pv, uint64_t* Mv) {
    for (int b = 0; b < nw; ++b) { Pv[b] = cyclic_fresh_pv(cyclic_pad(m, nw), b); Mv[b] = 0; }
    CyclicBest b = cyclic_fresh(m);
    int p = 0;
    for (int j = 0; j < 2 * n - 1; ++j) {
        const int x = t[cyclic_index(p, n, st)], c = st ? 3 - x : x;
        const uint64_t* e = peq + (size_t)c * nw;
        cyclic_take(b, cyclic_step<WT>(Pv, Mv, nw, [&](int w) { return e[w]; }), j);
        if (++p == n) p = 0;
    }
    return b;
}

// one pair on the host, the same step over the same columns as the kernel.  q, t: codes 0 .. 3.
inline void cyclic_pair(const uint8_t* q, int m, const uint8_t* t, int n, CyclicScratch& s, int32_t* dist, int32_t* end, uint8_t* strand) {
    const int nw = cyclic_words(m);
    s.peq.resize(4 * (size_t)nw);
    s.pv.resize((size_t)nw);
    s.mv.resize((size_t)nw);
    cyclic_masks(q, m, nw, s.peq.data());
    CyclicBest r[2];
    for (int st = 0; st < 2; ++st) {
        uint64_t Pv[4], Mv[4];   // (up to four words: a word count the compiler knows, the vectors in registers)
        switch (nw) {
            case 1: r[st] = cyclic_strand_run<1>(s.peq.data(), m, 1, t, n, st, Pv, Mv); break;
            case 2: r[st] = cyclic_strand_run<2>(s.peq.data(), m, 2, t, n, st, Pv, Mv); break;
            case 3: r[st] = cyclic_strand_run<3>(s.peq.data(), m, 3, t, n, st, Pv, Mv); break;
            case 4: r[st] = cyclic_strand_run<4>(s.peq.data(), m, 4, t, n, st, Pv, Mv); break;
            default: r[st] = cyclic_strand_run<0>(s.peq.data(), m, nw, t, n, st, s.pv.data(), s.mv.data()); break;
        }
    }
    const int st = cyclic_strand(r[0].best, r[1].best);
    *dist = r[st].best;
    *end = r[st].end;
    *strand = (uint8_t)st;
}

// The team schedule on the host: L "lanes" in lock step, lane l's words l K .. l K + K - 1 in 32-bit halves, what a lane
// hands down read by the lane below one step later -- the kernel sd_cyclic_pairs_long<K, L> without a device, for tests and
// sanitizer builds.  m <= 64 K L.
template <int K>
inline CyclicBest cyclic_team_strand(const uint64_t* peq, int m, const uint8_t* t, int n, int st, int L, uint32_t* v, uint32_t* hand) {
    const int nw = K * L, pad = cyclic_pad(m, nw), cols = 2 * n - 1;
    uint32_t *PvL = v, *PvH = v + nw, *MvL = v + 2 * nw, *MvH = v + 3 * nw;
    for (int w = 0; w < nw; ++w) {
        const uint64_t pv = cyclic_fresh_pv(pad, w);
        PvL[w] = (uint32_t)pv; PvH[w] = (uint32_t)(pv >> 32); MvL[w] = MvH[w] = 0u;
    }
    for (int l = 0; l < L; ++l) hand[l] = 0u;
    CyclicBest best = cyclic_fresh(m);
    for (int s = 0; s < cyclic_team_steps(cols, L); ++s)
        for (int l = L - 1; l >= 0; --l) {   // (downwards: hand[l - 1] is still the step before)
            const int j = cyclic_team_column(s, l);
            if (j < 0 || j >= cols) continue;
            uint32_t in;
            if (l == 0) {
                const int x = t[cyclic_index(j % n, n, st)];
                in = cyclic_team_pack(0u, 0u, st ? 3 - x : x);
            } else {
                in = hand[l - 1];
            }
            const int w0 = l * K;
            hand[l] = cyclic_team_lane<K>(PvL + w0, PvH + w0, MvL + w0, MvH + w0, in, [&](int c, int b) { return peq[(size_t)c * nw + w0 + b]; });
            if (l == L - 1) cyclic_take(best, cyclic_team_delta(hand[l]), j);
        }
    return best;
}
struct CyclicTeamScratch {
    std::vector<uint64_t> peq;
    std::vector<uint32_t> v, hand;
};
inline void cyclic_pair_team(const uint8_t* q, int m, const uint8_t* t, int n, int K, int L, CyclicTeamScratch& s, int32_t* dist, int32_t* end,
                             uint8_t* strand) {
    const int nw = K * L;
    s.peq.resize(4 * (size_t)nw);
    s.v.resize(4 * (size_t)nw);
    s.hand.resize((size_t)L);
    cyclic_masks(q, m, nw, s.peq.data());
    CyclicBest r[2];
    for (int st = 0; st < 2; ++st) {
        switch (K) {
            case 1: r[st] = cyclic_team_strand<1>(s.peq.data(), m, t, n, st, L, s.v.data(), s.hand.data()); break;
            case 2: r[st] = cyclic_team_strand<2>(s.peq.data(), m, t, n, st, L, s.v.data(), s.hand.data()); break;
            case 3: r[st] = cyclic_team_strand<3>(s.peq.data(), m, t, n, st, L, s.v.data(), s.hand.data()); break;
            default: r[st] = cyclic_team_strand<4>(s.peq.data(), m, t, n, st, L, s.v.data(), s.hand.data()); break;
        }
    }
    const int st = cyclic_strand(r[0].best, r[1].best);
    *dist = r[st].best;
    *end = r[st].end;
    *strand = (uint8_t)st;
}

// The canonical record: out = the lexicographically smallest among all rotations of seq and of its reverse complement;
// *rotation = the smallest r with out = s[r ..] s[.. r), s = seq on strand + and its reverse complement on strand -;
// strand + where both strands give the same record.  seq: upper-case A C G T, n >= 1.
inline int cyclic_least_rotation(const std::string& s) {
    const int n = (int)s.size();
    int i = 0, j = 1, k = 0;
    while (i < n && j < n && k < n) {
        const char a = s[(size_t)((i + k) % n)], b = s[(size_t)((j + k) % n)];
        if (a == b) { ++k; continue; }
        if (a > b) i += k + 1; else j += k + 1;
        if (i == j) ++j;
        k = 0;
    }
    return std::min(i, j);
}
inline std::string cyclic_revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}
inline std::string cyclic_canon(const std::string& seq, int64_t* rotation, int32_t* strand) {
    const std::string rc = cyclic_revcomp(seq);
    const int r0 = cyclic_least_rotation(seq), r1 = cyclic_least_rotation(rc);
    const std::string a = seq.substr((size_t)r0) + seq.substr(0, (size_t)r0), b = rc.substr((size_t)r1) + rc.substr(0, (size_t)r1);
    const bool minus = b < a;
    *rotation = minus ? r1 : r0;
    *strand = minus ? 1 : 0;
    return minus ? b : a;
}

// The pairs of a merge step: queries x targets (indices of sequences) -> dist / end / strand [queries x targets], a pair
// that fails the length condition under radius[query] left at dist -1.
using CyclicPairsFn = std::function<void(const std::vector<int32_t>& qi, const std::vector<int32_t>& ti, const std::vector<int32_t>& radius,
                                         std::vector<int32_t>& dist, std::vector<int32_t>& end, std::vector<uint8_t>& strand)>;

struct CyclicMergeOut {
    int32_t *cluster, *centre, *dist, *end;
    uint8_t* strand;
    int32_t n_clusters = 0;
};

// The walk, in blocks of `block` sequences of the visiting order: the block against the centres so far, the block
// against its undecided sequences (the only ones that can become centres), then the walk over the block.
inline void cyclic_merge(const int64_t* lens, int32_t n, const int64_t* weight, int P, int block, const CyclicPairsFn& pairs, CyclicMergeOut& o) {
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return weight[a] > weight[b]; });
    std::vector<int32_t> centres;   // sequence index per cluster, in order of creation
    std::vector<int32_t> dist, end, rad, q, t;
    std::vector<uint8_t> strand;
    struct Best { int32_t dist, cluster, end; uint8_t strand; };
    for (int32_t b0 = 0; b0 < n; b0 += block) {
        const int32_t nb = std::min<int32_t>(block, n - b0);
        q.assign(order.begin() + b0, order.begin() + b0 + nb);
        rad.resize((size_t)nb);
        for (int32_t x = 0; x < nb; ++x) rad[(size_t)x] = cyclic_radius(P, (int)lens[q[(size_t)x]]);
        std::vector<Best> best((size_t)nb, Best{-1, -1, 0, 0});
        // a pair's result enters: close, and strictly smaller than what is there (centres come in order of creation)
        auto enter = [&](int32_t x, int32_t cl, int32_t d, int32_t e, uint8_t s) {
            Best& bx = best[(size_t)x];
            if (d >= 0 && d <= rad[(size_t)x] && (bx.cluster < 0 || d < bx.dist)) bx = Best{d, cl, e, s};
        };
        const int32_t n_old = (int32_t)centres.size();
        const int32_t step = (int32_t)std::max<int64_t>(1, CYCLIC_PAIRS_MAX / nb);
        for (int32_t c0 = 0; c0 < n_old; c0 += step) {
            const int32_t nc = std::min(step, n_old - c0);
            t.assign(centres.begin() + c0, centres.begin() + c0 + nc);
            pairs(q, t, rad, dist, end, strand);
            for (int32_t x = 0; x < nb; ++x)
                for (int32_t c = 0; c < nc; ++c) {
                    const size_t at = (size_t)x * nc + c;
                    enter(x, c0 + c, dist[at], end[at], strand[at]);
                }
        }
        std::vector<int32_t> und, und_x;   // the undecided: sequence index, position in the block
        for (int32_t x = 0; x < nb; ++x)
            if (best[(size_t)x].cluster < 0) { und.push_back(q[(size_t)x]); und_x.push_back(x); }
        const int32_t nu = (int32_t)und.size();
        if (nu > 0) pairs(q, und, rad, dist, end, strand);
        std::vector<int32_t> new_c;   // positions in und of the centres made in this block
        size_t u_at = 0;
        for (int32_t x = 0; x < nb; ++x) {
            while (u_at < und_x.size() && und_x[u_at] < x) ++u_at;
            for (size_t i = 0; i < new_c.size(); ++i) {   // (made before x)
                const size_t at = (size_t)x * nu + (size_t)new_c[i];
                enter(x, n_old + (int32_t)i, dist[at], end[at], strand[at]);
            }
            const int32_t s = q[(size_t)x];
            const Best& bx = best[(size_t)x];
            if (bx.cluster < 0) {   // close to no centre: the next one (only an undecided sequence gets here: und[u_at])
                o.cluster[s] = (int32_t)centres.size();
                o.centre[s] = s;
                o.dist[s] = 0;
                o.end[s] = (int32_t)lens[s] - 1;
                o.strand[s] = 0;
                centres.push_back(s);
                new_c.push_back((int32_t)u_at);
            } else {
                o.cluster[s] = bx.cluster;
                o.centre[s] = centres[(size_t)bx.cluster];
                o.dist[s] = bx.dist;
                o.end[s] = bx.end;
                o.strand[s] = bx.strand;
            }
        }
    }
    o.n_clusters = (int32_t)centres.size();
}

}  // namespace sd
