// sd_group_dev.hpp -- grouping on the device: the scatter half of a counting sort, shared by the column profiles of a
// device-final job (sd_final_prof_dev.hip: pairs grouped by forward monomer) and the lag identities (sd_lags.hip: pairs
// grouped by the word class of their target).  The counts per group come from the caller's plan kernel, the exclusive
// prefix from sd_fprof_scan (group_scan); this is the pass that places every element:
//   elements of kind GROUP_IN    -> order[], grouped -- a workgroup counts its elements per group in LDS and reserves its
//                                   range of each group with ONE atomic per group; groups behind GROUP_HIST reserve per element
//   elements of kind GROUP_ASIDE -> a compact list of the source's own (src.aside(m, place)), its cursor at cursor[M]
// Order inside a group depends on the atomics; what is computed per element does not.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sd {

constexpr int GROUP_T = 256;        // threads per workgroup of a kernel that calls group_scatter
constexpr int GROUP_HIST = 1024;    // groups with a bin in LDS

enum : int { GROUP_OUT = 0, GROUP_IN = 1, GROUP_ASIDE = 2 };

// Called by every thread of a workgroup of GROUP_T threads; element m = blockIdx.x * GROUP_T + threadIdx.x of n.
// Src: int kind(int64_t m), int group(int64_t m) (kind GROUP_IN: 0 <= group < M), void aside(int64_t m, int64_t place).
template <class Src>
__device__ __forceinline__ void group_scatter(const Src& src, int64_t n, int64_t cap, int M, int32_t* __restrict__ cursor,
                                              int32_t* __restrict__ order) {
    __shared__ int hist[GROUP_HIST];
    __shared__ int nh_s, nh_base;
    const int nb = M < GROUP_HIST ? M : GROUP_HIST;
    for (int i = threadIdx.x; i < nb; i += GROUP_T) hist[i] = 0;
    if (threadIdx.x == 0) { nh_s = 0; nh_base = 0; }
    __syncthreads();
    const int64_t m = (int64_t)blockIdx.x * GROUP_T + threadIdx.x;
    const int c = m < n ? src.kind(m) : (int)GROUP_OUT;
    int g = -1, rank = 0;
    if (c == GROUP_IN) {
        g = src.group(m);
        if (g < GROUP_HIST) rank = atomicAdd(&hist[g], 1);
    } else if (c == GROUP_ASIDE) {
        rank = atomicAdd(&nh_s, 1);
    }
    __syncthreads();
    // the workgroup's range in each group: hist[i] becomes its first place
    for (int i = threadIdx.x; i < nb; i += GROUP_T) {
        const int k = hist[i];
        if (k) hist[i] = atomicAdd(&cursor[i], k);
    }
    if (threadIdx.x == 0 && nh_s) nh_base = atomicAdd(&cursor[M], nh_s);
    __syncthreads();
    if (c == GROUP_IN) {
        const int64_t pos = g < GROUP_HIST ? hist[g] + rank : atomicAdd(&cursor[g], 1);
        if (pos < cap) order[pos] = (int32_t)m;
    } else if (c == GROUP_ASIDE) {
        const int64_t pos = (int64_t)nh_base + rank;
        if (pos < cap) src.aside(m, pos);
    }
}

}  // namespace sd
