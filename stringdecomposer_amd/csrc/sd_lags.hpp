// sd_lags.hpp -- identity of every row of the final TSV to its next D neighbours in the same read (--lags), the parts
// host and device must compute alike, as plain C++ that compiles for both (in the manner of sd_final_dev.hpp): which
// pairs exist, who aligns a pair, the word class of a target, and the period rule.  sd_lags.hip holds the kernels and
// the C-ABI (sd_lag_*, include/sd_hip.h).
//
// Rows in file order; read R owns rows x = 0 .. n_R - 1.  For 1 <= d <= D and x + d < n_R the pair (x, d) aligns
// query = the segment of row x against target = the segment of row x + d, both as they stand in the read (nothing is
// reverse-complemented: a pair across an inversion scores low).  Result index s * D + (d - 1) for row s of the job:
//   dist >= 0     the pair's edit distance and its '=' columns, as sd_nw_identity_batch defines them
//   dist = -1     no partner (the read ends), or a side of the pair is empty (no alignment, main.py:30-33); matches = 0
//   dist = -2     left out by a device-resident call (a pair the lane kernel does not take); matches = 0
// Sums per (read, lag) over the pairs with dist >= 0: {n = pairs, M = sum of matches, C = sum of dist + matches}.
#pragma once

#include "sd_final_prof_dev.hpp"

namespace sd {

constexpr int LAG_DMAX = 255;             // 1 <= D <= LAG_DMAX
constexpr int LAG_TMAX = FPROF_TMAX;      // the lane kernel's limits are those of the profile path
constexpr int LAG_QMAX = FPROF_QMAX;
constexpr int LAG_CLASSES = 6;            // word classes of a target: K = 1, 2, 3, 4, 6, 8

enum : uint8_t { LAG_NONE = 0, LAG_DEV = 1, LAG_HOST = 2 };

SD_HD inline bool lag_d_ok(int64_t D) { return D >= 1 && D <= LAG_DMAX; }

// 64-bit words of a target's match masks (the K of sd_nw_kernel.hpp: 5 and 7 words run as 6 and 8), and its class
SD_HD inline int lag_words(int32_t tl) {
    const int k = (tl + 63) / 64;
    return k <= 4 ? (k < 1 ? 1 : k) : k <= 6 ? 6 : 8;
}
SD_HD inline int lag_class_of_words(int K) { return K <= 4 ? K - 1 : K == 6 ? 4 : 5; }
SD_HD inline int lag_words_of_class(int c) { return c < 4 ? c + 1 : c == 4 ? 6 : 8; }

// who aligns (query of ql bases, target of tl bases) -- text in ACGTN supposed, which the callers check
SD_HD inline uint8_t lag_pair_class(int32_t ql, int32_t tl) {
    if (ql <= 0 || tl <= 0) return LAG_NONE;
    if (tl <= LAG_TMAX && ql <= LAG_QMAX && !final_seg_splits(ql, tl)) return LAG_DEV;
    return LAG_HOST;
}

// a / b > c / d for a, c >= 0 and b, d > 0, by the 128-bit cross products (never in floating point)
SD_HD inline bool lag_ratio_greater(int64_t a, int64_t b, int64_t c, int64_t d) {
    auto mul = [](uint64_t x, uint64_t y, uint64_t& hi, uint64_t& lo) {
        const uint64_t x0 = x & 0xffffffffu, x1 = x >> 32, y0 = y & 0xffffffffu, y1 = y >> 32;
        const uint64_t p00 = x0 * y0, p01 = x0 * y1, p10 = x1 * y0, p11 = x1 * y1;
        const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu);
        lo = (p00 & 0xffffffffu) | (mid << 32);
        hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    };
    uint64_t lh, ll, rh, rl;
    mul((uint64_t)a, (uint64_t)d, lh, ll);
    mul((uint64_t)c, (uint64_t)b, rh, rl);
    return lh > rh || (lh == rh && ll > rl);
}

// The period of a read from its sums (D x {n, M, C}): the lag with the largest pooled identity M / C among the lags with
// n > 0, ties to the smallest lag; 0 when no lag has a pair (fewer than two rows).
SD_HD inline int lag_period(const int64_t* sums, int D) {
    int best = 0;
    for (int d = 1; d <= D; ++d) {
        const int64_t* s = sums + (int64_t)(d - 1) * 3;
        if (s[0] <= 0 || s[2] <= 0) continue;
        if (best == 0 || lag_ratio_greater(s[1], s[2], sums[(int64_t)(best - 1) * 3 + 1], sums[(int64_t)(best - 1) * 3 + 2])) best = d;
    }
    return best;
}

// identity in percent of a pair / pooled identity of a lag, -1 where there is none: the identity column's arithmetic
SD_HD inline double lag_identity(int64_t dist, int64_t matches) {
    return dist < 0 ? -1.0 : final_ident_ratio((double)matches, (double)(dist + matches));
}
SD_HD inline double lag_pooled(const int64_t* s) { return s[0] <= 0 || s[2] <= 0 ? -1.0 : final_ident_ratio((double)s[1], (double)s[2]); }

}  // namespace sd
