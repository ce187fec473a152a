// sd_dotplot.hpp -- windowed k-mer identity of a read against itself (--dotplot), the parts host and device must compute
// alike, as plain C++ that compiles for both (in the manner of sd_autocorr.hpp): the codes of a k-mer, the selection hash,
// the windows and tiles of a read, and the order of the cells.  sd_dotplot.hip holds the kernels, the host form and the
// C-ABI (sd_dotplot_*, include/sd_hip.h).
//
// A read is a text T[0 .. n).  The k-mer at i (1 <= k <= 32) exists when i + k <= n and T[i .. i + k) are all A C G T (the
// byte rule of autocorr_code).  Its forward code f is the 2k-bit number with A C G T = 0 1 2 3, first base most
// significant; its reverse code r is the code of the reverse complement.  k = 32 uses all 64 bits.  Window w of a read
// covers [w W, min(n, (w + 1) W)), nw = ceil(n / W) (a read of 0 bases has none); a k-mer belongs to the window its start
// lies in.  With the modulus M a code x is selected when dotplot_hash(x) % M == 0 -- always the value that is compared:
// S_w = the distinct selected forward codes of window w, R_w = the distinct selected reverse codes (selected by h(r)).
// For windows j <= i of a read (i - j <= B when B > 0) the cell (i, j) holds |S_i & S_j| and, with the reverse strand,
// |S_i & R_j|.  Cells of a read are ordered by i, then j.
#pragma once

#include <cstdint>

#include "sd_autocorr.hpp"

namespace sd {

constexpr int DOTPLOT_KMAX = 32;                             // 1 <= k <= DOTPLOT_KMAX
constexpr int64_t DOTPLOT_WMAX = (int64_t)1 << 30;           // 1 <= W <= DOTPLOT_WMAX
constexpr int64_t DOTPLOT_MMAX = (int64_t)1 << 20;           // 1 <= M <= DOTPLOT_MMAX
constexpr int64_t DOTPLOT_BMAX = (int64_t)1 << 30;           // 0 (all) <= B <= DOTPLOT_BMAX
constexpr int64_t DOTPLOT_CELLS_MAX = (int64_t)1 << 27;      // cells of a call
constexpr int DOTPLOT_SET_MAX = 4096;                        // selected positions of a window and strand: 32 KB of LDS
constexpr int DOTPLOT_TILE = 1024;                           // positions of a workgroup of the count and gather kernels
constexpr int DOTPLOT_JSEG = 64;                             // cells of a row a workgroup of the pair kernel takes
// The most pair-elements -- elements of S_j and R_j looked up in S_i -- one launch of the pair kernel takes, counted with
// the largest set of the call for every set: a chromosome is many short launches, never one long kernel.
constexpr int64_t DOTPLOT_LAUNCH_WORK = (int64_t)1 << 28;
constexpr int64_t DOTPLOT_LAUNCH_TILES = 65536;              // tiles of one launch of the count / gather kernel

SD_HD inline bool dotplot_k_ok(int64_t k) { return k >= 1 && k <= DOTPLOT_KMAX; }
SD_HD inline bool dotplot_w_ok(int64_t W) { return W >= 1 && W <= DOTPLOT_WMAX; }
SD_HD inline bool dotplot_m_ok(int64_t M) { return M >= 1 && M <= DOTPLOT_MMAX; }
SD_HD inline bool dotplot_b_ok(int64_t B) { return B >= 0 && B <= DOTPLOT_BMAX; }

// the splitmix64 finaliser
SD_HD inline uint64_t dotplot_hash(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
SD_HD inline bool dotplot_selected(uint64_t x, uint32_t M) { return M == 1 || dotplot_hash(x) % M == 0; }

// the code of a byte for dotplot_kmer: 0 .. 3 for A C G T, 4 for every other byte and behind the read's end
SD_HD inline uint8_t dotplot_base(uint8_t c) {
    const int x = autocorr_code(c);
    return x < 0 ? 4 : (uint8_t)x;
}

// the codes of the k-mer whose bases are c[0 .. k) (dotplot_base); false when one of them is no base.  No shift by 64:
// the forward code takes 2 bits k times, the reverse code places base t at bit 2 t.
SD_HD inline bool dotplot_kmer(const uint8_t* c, int k, uint64_t& f, uint64_t& r) {
    uint64_t a = 0, b = 0;
    unsigned bad = 0;
    const int top = 2 * (k - 1);
    for (int t = 0; t < k; ++t) {
        const unsigned x = c[t];
        bad |= x >> 2;
        a = (a << 2) | (x & 3);
        b = (b >> 2) | ((uint64_t)(3 - (x & 3)) << top);
    }
    f = a;
    r = b;
    return bad == 0;
}

// windows of a read; rows of cells: row i (a window of the read) holds the cells (i, j) for j = i - cells + 1 .. i
SD_HD inline int64_t dotplot_windows(int64_t n, int64_t W) { return n <= 0 ? 0 : (n + W - 1) / W; }
SD_HD inline int64_t dotplot_row_cells(int64_t i, int64_t B) { return B <= 0 || i <= B ? i + 1 : B + 1; }
// cells of the rows before row i (i <= 2^31: the product stays in 63 bits)
SD_HD inline int64_t dotplot_row_off(int64_t i, int64_t B) {
    return B <= 0 || i <= B + 1 ? i * (i + 1) / 2 : (B + 1) * (B + 2) / 2 + (i - B - 1) * (B + 1);
}

// Tiles: every window is cut into stretches of DOTPLOT_TILE positions from its own start (the last one shorter), so a tile
// belongs to one window.  Every window of a read but the last has dotplot_tiles_per_window tiles.
SD_HD inline int64_t dotplot_tiles_per_window(int64_t W) { return (W + DOTPLOT_TILE - 1) / DOTPLOT_TILE; }
SD_HD inline int64_t dotplot_tiles(int64_t n, int64_t W) {
    const int64_t nw = dotplot_windows(n, W);
    if (nw <= 0) return 0;
    return (nw - 1) * dotplot_tiles_per_window(W) + (n - (nw - 1) * W + DOTPLOT_TILE - 1) / DOTPLOT_TILE;
}

// the last x in [0, n) with off[x] <= v (off ascending, off[0] <= v)
SD_HD inline int dotplot_find(const int64_t* off, int n, int64_t v) {
    int a = 0, b = n;
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (off[m] <= v) a = m; else b = m;
    }
    return a;
}

}  // namespace sd
