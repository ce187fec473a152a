// sd_rows_scan_dev.hpp -- device text shared by the units that compact flagged items (sd_rows_dev.hip: the records the
// seam merge keeps; sd_final_dev.hip: the rows the final selection keeps): byte flags in tiles of ROWS_TILE, counted per
// tile (sd_rows_count), scanned by one workgroup (sd_rows_scan), and the helpers a scatter places its items with.  The
// two kernels are static: every unit that includes this launches its own copy.
#pragma once

#include <cstdint>

namespace sd {

constexpr int ROWS_T = 256;                   // threads per workgroup of every kernel of these units
constexpr int ROWS_TILE = ROWS_T * 4;         // items per tile of the count / scatter (4 flags = one word per lane)

// exclusive scan of v over the workgroup; *total = the sum (valid in every thread)
__device__ inline int rows_block_scan(int v, int* total) {
    __shared__ int wsum[ROWS_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int sc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int s2 = __shfl_up(sc, off);
        if (lane >= off) sc += s2;
    }
    __syncthreads();   // (the last call's readers are through)
    if (lane == 63) wsum[w] = sc;
    __syncthreads();
    int pre = 0, all = 0;
    for (int x = 0; x < ROWS_T / 64; ++x) {
        if (x < w) pre += wsum[x];
        all += wsum[x];
    }
    *total = all;
    return pre + sc - v;
}

// the four flags of a lane as one word (keep is allocated and zeroed in whole words), and how many are set
__device__ inline uint32_t rows_flags(const uint8_t* __restrict__ keep, int64_t n, int64_t i0) {
    return i0 < n ? *reinterpret_cast<const uint32_t*>(keep + i0) : 0u;
}
__device__ inline int rows_flag_count(uint32_t f) { return (int)((f * 0x01010101u) >> 24); }

static __global__ __launch_bounds__(ROWS_T) void sd_rows_count(const uint8_t* __restrict__ keep, int64_t n, int32_t* __restrict__ bsum) {
    int total;
    (void)rows_block_scan(rows_flag_count(rows_flags(keep, n, (int64_t)blockIdx.x * ROWS_TILE + threadIdx.x * 4)), &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bbase[b] = rows before tile b, bbase[n_tiles] = the row count
static __global__ __launch_bounds__(ROWS_T) void sd_rows_scan(const int32_t* __restrict__ bsum, int64_t n_tiles, int64_t* __restrict__ bbase) {
    int64_t run = 0;
    for (int64_t b0 = 0; b0 < n_tiles; b0 += ROWS_T) {
        const int64_t b = b0 + threadIdx.x;
        int total;
        const int ex = rows_block_scan(b < n_tiles ? bsum[b] : 0, &total);   // (a round holds at most 256 * 1024 rows)
        if (b < n_tiles) bbase[b] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) bbase[n_tiles] = run;
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
