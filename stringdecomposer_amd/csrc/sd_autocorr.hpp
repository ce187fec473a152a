// sd_autocorr.hpp -- k-mer autocorrelation of a read against itself (--autocorr), the parts host and device must compute
// alike, as plain C++ that compiles for both (in the manner of sd_heat.hpp): which bytes match, the bit planes of a text,
// a word of k-mer hits, the windows and tiles of a read, the closed form of the positions, and the peak rule.
// sd_autocorr.hip holds the kernels, the host form and the C-ABI (sd_autocorr_*, include/sd_hip.h).
//
// A read is a text T[0 .. n).  Two positions match when they hold the same byte and that byte is one of A C G T (upper
// case); every other byte matches nothing, itself included.  For 1 <= k <= 32 and a lag d >= 1, position i is a hit at
// lag d when 0 <= i <= n - d - k and T[i + j] matches T[i + d + j] for j = 0 .. k - 1.  With a window length W (0: one
// window, the whole read) the read has max(1, ceil(n / W)) windows, window w = [w W, min(n, (w + 1) W)), and
// A[w, d], d = 1 .. D, counts the hits at lag d whose i lies in window w (the partner at i + d may lie beyond it).
//
// Bit planes: base i of a read is bit i & 63 of word i >> 6 in three planes -- lo and hi, the two bits of its code
// (A = 0, C = 1, G = 2, T = 3), and valid, set for A C G T alone.  Bits behind the read's end are 0 in all three, and at
// least one word of zeros follows the last word of a read, so "the partner lies inside the read" is the partner's valid
// bit and nothing in a word loop tests a bound.
#pragma once

#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // hipStream_t of launch_autocorr_prep
#endif

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

constexpr int AUTOCORR_KMAX = 32;                            // 1 <= k <= AUTOCORR_KMAX
constexpr int64_t AUTOCORR_DMAX = (int64_t)1 << 20;          // 1 <= D <= AUTOCORR_DMAX
constexpr int64_t AUTOCORR_CELLS_MAX = (int64_t)1 << 27;     // windows x D of a call: 1 GB of counters
constexpr int AUTOCORR_TILE_WORDS = 64;                      // a workgroup's stretch of a window: 64 words
constexpr int64_t AUTOCORR_TILE = 64 * AUTOCORR_TILE_WORDS;  // = 4096 bases
constexpr int AUTOCORR_LAGS = 256;                           // lags of a workgroup: one per lane
// Workgroups of one launch of sd_autocorr_pairs.  A workgroup is at most AUTOCORR_TILE x AUTOCORR_LAGS base-lag products
// (65 word-steps in each of 256 lanes), so a launch is at most 2^33 of them -- of the order of 100 microseconds on an
// MI355X -- whatever the reads and D are: a long read with many lags becomes many short launches, never one long one.
constexpr int64_t AUTOCORR_LAUNCH_WG = 8192;
constexpr int64_t AUTOCORR_LAUNCH_WORK = AUTOCORR_LAUNCH_WG * AUTOCORR_TILE * AUTOCORR_LAGS;

SD_HD inline bool autocorr_k_ok(int64_t k) { return k >= 1 && k <= AUTOCORR_KMAX; }
SD_HD inline bool autocorr_d_ok(int64_t D) { return D >= 1 && D <= AUTOCORR_DMAX; }
SD_HD inline bool autocorr_w_ok(int64_t W) { return W >= 0; }

// the code of a byte: 0 .. 3 for A C G T, -1 for a byte that matches nothing
SD_HD inline int autocorr_code(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// words of the planes of a read of n bases: its bases, then one word of zeros
SD_HD inline int64_t autocorr_words(int64_t n) { return (n + 63) / 64; }
SD_HD inline int64_t autocorr_plane_words(int64_t n) { return autocorr_words(n) + 1; }

// windows of a read and the bases of window w
SD_HD inline int64_t autocorr_windows(int64_t n, int64_t W) { return W <= 0 || n <= W ? 1 : (n + W - 1) / W; }
SD_HD inline int64_t autocorr_win_start(int64_t w, int64_t W) { return W <= 0 ? 0 : w * W; }
SD_HD inline int64_t autocorr_win_end(int64_t n, int64_t w, int64_t W) { return W <= 0 || (w + 1) * W > n ? n : (w + 1) * W; }

// Tiles: every window is cut into stretches of AUTOCORR_TILE bases from its own start (the last one shorter), so a tile
// belongs to one window.  A full window has autocorr_tiles_per_window tiles; tile j of a read is stretch j % that of window
// j / that.  A read without bases has no tile.
SD_HD inline int64_t autocorr_tiles_per_window(int64_t n, int64_t W) {
    const int64_t len = W <= 0 || W > n ? n : W;
    return len <= 0 ? 1 : (len + AUTOCORR_TILE - 1) / AUTOCORR_TILE;
}
SD_HD inline int64_t autocorr_tiles(int64_t n, int64_t W) {
    if (n <= 0) return 0;
    const int64_t nw = autocorr_windows(n, W), last = n - autocorr_win_start(nw - 1, W);
    return (nw - 1) * autocorr_tiles_per_window(n, W) + (last + AUTOCORR_TILE - 1) / AUTOCORR_TILE;
}

// positions[w, d]: the i of window [ws, we) with i <= n - d - k
SD_HD inline int64_t autocorr_positions(int64_t n, int64_t k, int64_t d, int64_t ws, int64_t we) {
    const int64_t top = n - d - k + 1 < we ? n - d - k + 1 : we;
    return top > ws ? top - ws : 0;
}

// A run of k ones is built from runs of `have` ones by x &= x >> s with s <= have: shifts[] for k, at most 5 of them
SD_HD inline int autocorr_steps(int k, int shifts[5]) {
    int ns = 0;
    for (int have = 1; have < k; ++ns) {
        const int s = have < k - have ? have : k - have;
        shifts[ns] = s;
        have += s;
    }
    return ns;
}

// equality of 64 positions with their partners: the same code, and both A C G T
SD_HD inline uint64_t autocorr_eq(uint64_t lo, uint64_t hi, uint64_t v, uint64_t plo, uint64_t phi, uint64_t pv) {
    return ~((lo ^ plo) | (hi ^ phi)) & v & pv;
}

// bit i of the result: e has k ones from bit i on, in the 96 bits {next (low 32 bits used), cur}; k <= 32
template <int NS>
SD_HD inline uint64_t autocorr_runs(uint64_t cur, uint64_t next, const int* shifts) {
    uint64_t x = cur;
    uint32_t y = (uint32_t)next;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = shifts[i];   // 1 .. 16
        x &= (x >> s) | ((uint64_t)y << (64 - s));
        y &= y >> s;
    }
    return x;
}
SD_HD inline uint64_t autocorr_runs_n(int ns, uint64_t cur, uint64_t next, const int* shifts) {
    switch (ns) {
        case 0: return cur;
        case 1: return autocorr_runs<1>(cur, next, shifts);
        case 2: return autocorr_runs<2>(cur, next, shifts);
        case 3: return autocorr_runs<3>(cur, next, shifts);
        case 4: return autocorr_runs<4>(cur, next, shifts);
        default: return autocorr_runs<5>(cur, next, shifts);
    }
}

// the bits of word t (bases 64 t .. 64 t + 63) that lie in [a, b)
SD_HD inline uint64_t autocorr_word_mask(int64_t t, int64_t a, int64_t b) {
    const int64_t lo = a - 64 * t, hi = b - 64 * t;
    if (hi <= 0 || lo >= 64) return 0;
    uint64_t m = ~(uint64_t)0;
    if (lo > 0) m &= ~(uint64_t)0 << lo;
    if (hi < 64) m &= ~(~(uint64_t)0 << hi);
    return m;
}

// ---- peaks: integers only.  In a spectrum A[1 .. D] (A[d] = a[d - 1]) with smallest lag LO >= 1 and radius R >= 0, lag
// d >= LO is a peak when A[d] > 0, A[d] >= A[e] for every e in [max(LO, d - R), min(D, d + R)], and A[d] > A[e] for every
// such e < d (ties go to the smaller lag).  Peaks are ordered by count descending, then lag ascending.
SD_HD inline bool autocorr_is_peak(const int64_t* a, int64_t D, int64_t LO, int64_t R, int64_t d) {
    if (d < LO || d > D) return false;
    const int64_t c = a[d - 1];
    if (c <= 0) return false;
    const int64_t e0 = d - R > LO ? d - R : LO, e1 = d + R < D ? d + R : D;
    for (int64_t e = e0; e < d; ++e)
        if (a[e - 1] >= c) return false;
    for (int64_t e = d + 1; e <= e1; ++e)
        if (a[e - 1] > c) return false;
    return true;
}
SD_HD inline bool autocorr_peak_before(int64_t count_a, int64_t lag_a, int64_t count_b, int64_t lag_b) {
    return count_a != count_b ? count_a > count_b : lag_a < lag_b;
}

// ---- host only: the planes of one read as sd_autocorr_prep lays them out, for the host forms of the passes that read
// them (sd_autocorr.hip, sd_motif.hip, sd_motif_edit.hip).  Two words of zeros follow the read's own, one more than on the
// device: a shifted partner or the pair (t, t + 1) of the last word of the planes reads inside them.
struct AutocorrPlanes {
    std::vector<uint64_t> lo, hi, v;   // autocorr_words(n) + 2 words
    int64_t rw = 0;                    // autocorr_words(n)
    void build(const uint8_t* t, int64_t n) {
        rw = autocorr_words(n);
        lo.assign((size_t)rw + 2, 0);
        hi.assign((size_t)rw + 2, 0);
        v.assign((size_t)rw + 2, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int c = autocorr_code(t[i]);
            if (c < 0) continue;
            const uint64_t bit = (uint64_t)1 << (i & 63);
            v[(size_t)(i >> 6)] |= bit;
            if (c & 1) lo[(size_t)(i >> 6)] |= bit;
            if (c & 2) hi[(size_t)(i >> 6)] |= bit;
        }
    }
};

#if defined(__HIPCC__)
// sd_autocorr_prep (sd_autocorr.hip) for the other passes that read the planes (sd_motif.hip): the text of n_reads reads
// (read r at text + roff[r], rlen[r] bases, its planes from word pw[r] on; device arrays) into lo | hi | v of `words` words.
void launch_autocorr_prep(hipStream_t st, unsigned grid, const uint8_t* text, const int64_t* roff, const int64_t* rlen, const int64_t* pw,
                          int n_reads, int64_t words, uint64_t* lo, uint64_t* hi, uint64_t* v);
#endif

}  // namespace sd
