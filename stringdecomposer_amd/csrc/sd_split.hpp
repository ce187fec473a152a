// sd_split.hpp -- subfamilies of a monomer's instances (--split): the rule, written once for the host form and the kernels,
// as plain C++ that compiles for both (in the manner of sd_autocorr.hpp).  sd_split.hip holds the kernels, the host form
// and the C-ABI (sd_split_*, include/sd_hip.h).
//
// Input, for one forward monomer of length L: its n member rows -- the rows of --msa (include/sd_hip.h: SD_MSA_PITCH) with
// status 1 whose pair names the monomer, either strand: a row is already in forward coordinates.  Only bytes [0, L) of a
// row are read, symbols 0..4 = A C G T N and 5 = SD_MSA_DEL (split_sym: a byte above 5, which no computed row holds, reads
// as 5); the insertion slots take no part.  Rows of status 0 or 2 are no members.
//
// Parameters: R >= 1 a radius in columns, 1 <= K <= 64 the most subfamilies, S >= 1 the fewest rows of a new subfamily,
// I >= 1 the Lloyd iterations of a round.
//
// H(x, c) = the columns g of [0, L) with x[g] != c[g] (N equals N, DEL equals DEL).  mode(rows) = per column the most
// frequent symbol, ties to the smallest code (split_mode); a cluster without a member keeps its centre.  assign gives
// every member the centre of smallest H, ties to the smallest centre index (SplitBest), with d1 = that distance and d2 =
// the smallest distance to any other centre, -1 when there is one centre.
//
// Procedure (split_drive):
//   1. centres = [mode(all members)], every member a seed candidate; assign.
//   2. rounds, while there are fewer than K centres and fewer than 4 K rounds have run:
//        i* = the candidate of largest d1, ties to the smallest row index (split_key); stop when d1[i*] < R or no
//        candidate is left; try centres + [x_i*]: assign, then at most I times (mode per cluster, assign), ending early
//        when no assignment changed; a new (last) cluster of fewer than S members discards the trial -- centres and
//        assignment stay as before the round, i* stops being a candidate -- else the trial is kept.
//   3. result: the centres, their count k, per member assign, d1, d2; the cluster sizes, the rounds and the Lloyd
//      iterations (mode, assign) that ran.  n = 0 gives k = 0.
//
// Bit planes: column g of a row is bit g & 63 of word g >> 6 in three planes, the three bits of its symbol; the bits
// beyond L are 0, so H is a sum of popcount((a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2)) over the words (split_word_dist).
#pragma once

#include <cstdint>

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

constexpr int SPLIT_KMAX = 64;                          // 1 <= K <= SPLIT_KMAX
constexpr int SPLIT_LMAX = 512;                         // the device form: the limit of the row kernel of --msa
constexpr int SPLIT_WMAX = SPLIT_LMAX / 64;             // plane words of a row on the device
constexpr int64_t SPLIT_NMAX = (int64_t)1 << 26;        // member rows of one monomer
constexpr int SPLIT_SYMS = 6;                           // A C G T N DEL
constexpr int SPLIT_ROUNDS_PER_K = 4;                   // at most 4 K rounds

SD_HD inline int split_sym(uint8_t b) { return b < SPLIT_SYMS ? (int)b : SPLIT_SYMS - 1; }
SD_HD inline int split_words(int L) { return (L + 63) >> 6; }
SD_HD inline int split_radius(int64_t P, int64_t L) {   // --split P: the radius of a monomer of L bases
    const int64_t r = (P * L + 99) / 100;
    return r < 1 ? 1 : (int)r;
}

SD_HD inline int split_word_dist(uint64_t a0, uint64_t a1, uint64_t a2, uint64_t b0, uint64_t b1, uint64_t b2) {
    return __builtin_popcountll((a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2));
}

// the farthest candidate as a maximum: the larger d1 wins, then the smaller row; 0 = no candidate (a row is below 2^32 - 1)
SD_HD inline uint64_t split_key(int32_t d1, uint32_t row) { return ((uint64_t)(uint32_t)d1 << 32) | (uint64_t)(0xFFFFFFFFu - row); }
SD_HD inline int32_t split_key_d1(uint64_t key) { return (int32_t)(key >> 32); }
SD_HD inline uint32_t split_key_row(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// the most frequent of six counts, ties to the smallest code
template <class C>
SD_HD inline int split_mode(const C* cnt) {
    int b = 0;
    for (int s = 1; s < SPLIT_SYMS; ++s)
        if (cnt[s] > cnt[b]) b = s;
    return b;
}

// centres offered in ascending index: the first of the smallest distances is kept
struct SplitBest {
    int32_t d1 = 0x7fffffff, d2 = 0x7fffffff, at = 0;
    SD_HD void take(int32_t d, int c) {
        if (d < d1) { d2 = d1; d1 = d; at = c; }
        else if (d < d2) d2 = d;
    }
    SD_HD int32_t second() const { return d2 == 0x7fffffff ? -1 : d2; }
};

// what an assign pass reports: O(1) bytes for the host (key, changed, last), the sizes stay with the pass
struct SplitStat {
    unsigned long long key;      // split_key of the farthest candidate, 0 = none
    uint32_t changed;            // rows whose centre differs from the previous pass
    uint32_t last;               // rows of the last centre
    uint32_t sizes[SPLIT_KMAX];
};

// The procedure over a backend B -- the host form or the device passes -- which holds a current and a trial state:
//   start()                  trial: every row in cluster 0
//   modes(k)                 trial: centre c < k = mode of its rows (an empty cluster keeps its centre)
//   assign(k, first)         trial: assign against its k centres -> SplitStat's first three fields; `first`: changed is
//                            measured against the current state (and is not used)
//   accept()                 the trial becomes the current state
//   begin(k, row)            trial centres = the current k centres + member row `row`
//   reject(row)              `row` is no candidate any more -> the key of the current state over those that are
// info = {k, rounds, iterations}
template <class B>
inline void split_drive(B& b, int64_t n, int R, int K, int S, int I, int64_t info[3]) {
    info[0] = info[1] = info[2] = 0;
    if (n <= 0) return;
    b.start();
    b.modes(1);
    SplitStat st = b.assign(1, true);
    b.accept();
    int k = 1;
    int64_t rounds = 0, iters = 0;
    while (k < K && rounds < (int64_t)SPLIT_ROUNDS_PER_K * K) {
        if (st.key == 0 || split_key_d1(st.key) < R) break;
        const uint32_t row = split_key_row(st.key);
        ++rounds;
        b.begin(k, row);
        SplitStat t = b.assign(k + 1, true);
        for (int it = 0; it < I; ++it) {
            b.modes(k + 1);
            t = b.assign(k + 1, false);
            ++iters;
            if (t.changed == 0) break;
        }
        if ((int64_t)t.last < (int64_t)S) {
            st.key = b.reject(row);
        } else {
            b.accept();
            st = t;
            ++k;
        }
    }
    info[0] = k;
    info[1] = rounds;
    info[2] = iters;
}

}  // namespace sd
