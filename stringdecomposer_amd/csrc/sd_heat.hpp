// sd_heat.hpp -- all-against-all identity of the rows of a read, kept as sums per bin (--heatmap), the parts host and
// device must compute alike, as plain C++ that compiles for both (in the manner of sd_lags.hpp): which pairs exist, the
// bin of a row, the cell of a pair, the strips of a target, and the closed forms of the layout.  sd_heat.hip holds the
// kernels and the C-ABI (sd_heat_*, include/sd_hip.h).
//
// Rows in file order; a group (read) owns rows x = 0 .. n - 1.  B rows per bin: row x lies in bin x / B, the group has
// nb = ceil(n / B) bins.  The pairs of a group are all (x, y) with x < y, and with y - x <= W when W > 0; query = the
// segment of row x (the earlier one), target = the segment of row y, so pair (x, y) is the pair (x, d = y - x) of --lags,
// bit for bit.  A pair with an empty side does not exist.  Cell (I, J), I <= J, holds {n, M, C} = the pair count, the sum
// of matches and the sum of dist + matches over the pairs with x in bin I and y in bin J.  The cells of a group are the
// row-major upper triangle: I * nb - I (I - 1) / 2 + (J - I); group g starts at cell_off[g], the prefix sum of
// nb (nb + 1) / 2.  Who aligns a pair is lag_pair_class(ql, tl), unchanged.
#pragma once

#include "sd_lags.hpp"

namespace sd {

constexpr int64_t HEAT_BMAX = (int64_t)1 << 20;        // 1 <= B <= HEAT_BMAX
constexpr int64_t HEAT_CELLS_MAX = (int64_t)1 << 25;   // cells of a call: 805 MB of sums
constexpr int HEAT_STRIP = 64;                         // queries of a work item: one per lane of a wave

// Within the kernel's limits no pair is split by edlib (final_seg_splits at its largest operands), so for a target of
// 1 .. LAG_TMAX bases the class of a pair depends on the query alone: LAG_NONE (empty), LAG_HOST (over LAG_QMAX), else
// LAG_DEV.  The closed-form class counts of sd_heat.hip rest on this.
static_assert(20ll * ((LAG_QMAX + 63) / 64) * LAG_TMAX + 8ll * LAG_TMAX < 1024 * 1024, "a pair inside the limits that edlib splits");

SD_HD inline bool heat_b_ok(int64_t B) { return B >= 1 && B <= HEAT_BMAX; }
SD_HD inline bool heat_w_ok(int64_t W) { return W >= 0; }

SD_HD inline int64_t heat_bins(int64_t n, int64_t B) { return (n + B - 1) / B; }
SD_HD inline int64_t heat_cells(int64_t nb) { return nb * (nb + 1) / 2; }
SD_HD inline int64_t heat_cell(int64_t nb, int64_t I, int64_t J) { return I * nb - I * (I - 1) / 2 + (J - I); }

// the first query of target y (both counted inside the group), and its strips of up to HEAT_STRIP consecutive queries
SD_HD inline int64_t heat_first_query(int64_t y, int64_t W) { return W > 0 && y > W ? y - W : 0; }
SD_HD inline int64_t heat_strips(int64_t y, int64_t W) { return (y - heat_first_query(y, W) + HEAT_STRIP - 1) / HEAT_STRIP; }

// the word class of a target the kernel takes; -1 for a target no lane walks (empty, or over LAG_TMAX bases)
SD_HD inline int heat_target_class(int32_t tl) { return tl >= 1 && tl <= LAG_TMAX ? lag_class_of_words(lag_words(tl)) : -1; }

SD_HD inline double heat_pooled(const int64_t* s) { return lag_pooled(s); }

// pairs of a group of n rows: sum over y of min(y, W) -- n (n - 1) / 2 without a limit; false when the total leaves 64 bits
inline bool heat_add_pairs(int64_t n, int64_t W, uint64_t& total) {
    if (n < 2) return true;
    const unsigned __int128 N = (unsigned __int128)n, w = (unsigned __int128)W;
    const unsigned __int128 p = (W <= 0 || W >= n - 1) ? N * (N - 1) / 2 : w * (w + 1) / 2 + (N - 1 - w) * w;
    const unsigned __int128 t = p + total;
    if (t >> 64) return false;
    total = (uint64_t)t;
    return true;
}

}  // namespace sd
