// sd_scan_dev.hpp -- the device prefix scan of the post-pass units: "counts per item -> place of each item, plus the total".
//   block_scan<T>     exclusive scan over the lanes of a workgroup: a shuffle scan per wave, the wave sums through LDS
//   scan_bases<T>     one workgroup: the sums of tiles (int32 or int64) -> int64 bases before each tile, the total behind them
//   scan_tiles<Src>, scan_place   for a caller without a kernel of its own to produce the tile sums in: per tile of SCAN_T
//                     items the exclusive values inside the tile and the tile's sum; then the tile's base added to each
//   exclusive_scan_dev   the three launches on a stream: out[i] = src(0) + .. + src(i - 1), out[n] = the total
// A unit that counts in a kernel of its own (the flag counts, the text lengths, the motif items) writes the tile sums there
// and launches scan_bases alone.  The kernels are templates: every unit that launches one holds its own copy.  Nothing is
// allocated and nothing waits here: the buffers and the stream are the caller's.
#pragma once

#include <cstdint>

namespace sd {

constexpr int SCAN_T = 256;   // threads per workgroup of the scan kernels = items per tile of scan_tiles

// exclusive scan of v over the workgroup; *total = the sum (valid in every thread)
template <class T, int THREADS = SCAN_T>
__device__ inline T block_scan(T v, T* total) {
    __shared__ T wsum[THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T sc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const T s2 = __shfl_up(sc, off);
        if (lane >= off) sc += s2;
    }
    __syncthreads();   // (the last call's readers are through)
    if (lane == 63) wsum[w] = sc;
    __syncthreads();
    T pre = 0, all = 0;
    for (int x = 0; x < THREADS / 64; ++x) {
        if (x < w) pre += wsum[x];
        all += wsum[x];
    }
    *total = all;
    return pre + sc - v;
}

// one workgroup: tbase[b] = the sum of the tiles before tile b, tbase[n_tiles] = the sum of all; SCAN_T tiles per round.
// A round is summed in T (int32 tiles: 64-bit shuffles cost the motif size pass 3 to 6 %, profiles/scan_timing.md), so with
// int32 tiles the SCAN_T sums of a round must stay below 2^31 together -- they do where a tile is at most 2^23: 1 024
// flags, the hits of 256 words, 256 x 1 024 in the self-test; the running base is 64-bit whatever T is
template <class T>
__global__ __launch_bounds__(SCAN_T) void scan_bases(const T* __restrict__ tsum, int64_t n_tiles, int64_t* __restrict__ tbase) {
    int64_t run = 0;
    for (int64_t b0 = 0; b0 < n_tiles; b0 += SCAN_T) {
        const int64_t b = b0 + threadIdx.x;
        T total;
        const T ex = block_scan<T>(b < n_tiles ? tsum[b] : 0, &total);
        if (b < n_tiles) tbase[b] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) tbase[n_tiles] = run;
}

// the plain source of a scan: an array of counts (out itself, for a scan in place: a lane reads its item before it writes it)
template <class T>
struct ScanArray {
    const T* v;
    __device__ int64_t operator()(int64_t i) const { return v[i]; }
};

// a workgroup per tile: out[i] = the items of the tile before i, tsum[tile] = the tile's sum (T: int32 or int64)
template <class Src, class T>
__global__ __launch_bounds__(SCAN_T) void scan_tiles(Src src, int64_t n, int64_t* out, T* __restrict__ tsum) {
    const int64_t i = (int64_t)blockIdx.x * SCAN_T + threadIdx.x;
    int64_t total;
    const int64_t ex = block_scan<int64_t>(i < n ? src(i) : 0, &total);
    if (i < n) out[i] = ex;
    if (threadIdx.x == 0) tsum[blockIdx.x] = (T)total;
}

// out[i] += the base of its tile, out[n] = the total; at least one workgroup (n = 0: out[0] = 0).  T: the type of out
template <class T>
__global__ __launch_bounds__(SCAN_T) void scan_place(T* __restrict__ out, int64_t n, const int64_t* __restrict__ tbase, int64_t n_tiles) {
    const int64_t i = (int64_t)blockIdx.x * SCAN_T + threadIdx.x;
    if (i < n) out[i] += (T)tbase[blockIdx.x];
    if (i == 0) out[n] = (T)tbase[n_tiles];
}

inline int64_t scan_tiles_of(int64_t n) { return (n + SCAN_T - 1) / SCAN_T; }

// tsum: scan_tiles_of(n) entries (at least one), tbase: one more, out: n + 1
template <class Src, class T>
inline void exclusive_scan_dev(hipStream_t st, Src src, int64_t n, int64_t* out, T* tsum, int64_t* tbase) {
    const int64_t n_tiles = scan_tiles_of(n);
    if (n_tiles > 0) hipLaunchKernelGGL((scan_tiles<Src, T>), dim3((unsigned)n_tiles), dim3(SCAN_T), 0, st, src, n, out, tsum);
    hipLaunchKernelGGL(scan_bases<T>, dim3(1), dim3(SCAN_T), 0, st, tsum, n_tiles, tbase);
    hipLaunchKernelGGL(scan_place<int64_t>, dim3((unsigned)(n_tiles > 0 ? n_tiles : 1)), dim3(SCAN_T), 0, st, out, n, tbase, n_tiles);
}

}  // namespace sd
