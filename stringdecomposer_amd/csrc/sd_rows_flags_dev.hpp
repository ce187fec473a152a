// sd_rows_flags_dev.hpp -- device text shared by the units that compact flagged items (sd_rows_dev.hip: the records the
// seam merge keeps; sd_final_dev.hip: the rows the final selection keeps): byte flags in tiles of ROWS_TILE, counted per
// tile (sd_rows_count), scanned by scan_bases (sd_scan_dev.hpp), and the helpers a scatter places its items with.
// sd_rows_count is static: every unit that includes this launches its own copy.
#pragma once

#include "sd_scan_dev.hpp"

namespace sd {

constexpr int ROWS_T = SCAN_T;                // threads per workgroup of every kernel of these units
constexpr int ROWS_TILE = ROWS_T * 4;         // items per tile of the count / scatter (4 flags = one word per lane)

// the four flags of a lane as one word (keep is allocated and zeroed in whole words), and how many are set
__device__ inline uint32_t rows_flags(const uint8_t* __restrict__ keep, int64_t n, int64_t i0) {
    return i0 < n ? *reinterpret_cast<const uint32_t*>(keep + i0) : 0u;
}
__device__ inline int rows_flag_count(uint32_t f) { return (int)((f * 0x01010101u) >> 24); }

static __global__ __launch_bounds__(ROWS_T) void sd_rows_count(const uint8_t* __restrict__ keep, int64_t n, int32_t* __restrict__ bsum) {
    int total;
    (void)block_scan<int>(rows_flag_count(rows_flags(keep, n, (int64_t)blockIdx.x * ROWS_TILE + threadIdx.x * 4)), &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// flags set in keep[0 .. idx), from the tile bases
__device__ inline int64_t rows_flags_before(const uint8_t* __restrict__ keep, const int64_t* __restrict__ bbase, int64_t idx) {
    const int64_t t0 = idx / ROWS_TILE;
    int64_t s = bbase[t0];
    int64_t x = t0 * ROWS_TILE;
    for (; x + 4 <= idx; x += 4) s += rows_flag_count(*reinterpret_cast<const uint32_t*>(keep + x));
    for (; x < idx; ++x) s += keep[x];
    return s;
}

}  // namespace sd
