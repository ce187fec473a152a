// sd_fast_launch.hpp -- host: one launch of a fill kernel of the fast family with the operands of a FillArgs, its dynamic
// LDS limit raised to what the launch asks for first.  The units of the kernel families (sd_fast*.hip) instantiate their
// kernels at their P values through these.
#pragma once

#include "sd_fast_fill.hpp"
#include "sd_fast_wide_fill.hpp"
#include "sd_fast_wn_fill.hpp"

namespace sd {

// narrow layout (sd_fast_fill), the RANKED form where the batch has --ed_thr ranks
template <int P, int CF, int FL, bool ONE, int FLS>
void launch_narrow(hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, uint32_t hx, uint64_t levels = 0) {
    with_bool(a.cendoff != nullptr, [&](auto rk) {
        constexpr bool RK = decltype(rk)::value;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sd_fast_fill<P, RK, CF, FL, ONE, FLS>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((sd_fast_fill<P, RK, CF, FL, ONE, FLS>), dim3(grid), dim3(nw * 64), lds, st, a.chunks, a.n_chunks,
                           a.bases2, a.nmask, a.table, a.lane_consts, a.sc, hx, levels, a.B, a.argV, a.ckpt, a.ckbase, a.queue,
                           a.order, a.cendoff, a.crank);
    });
}

// wide layout (sd_fast_fill_wide), 8 waves per workgroup, the RANKED form where the batch has --ed_thr ranks
template <int P, bool F16, int FL>
void launch_wide(hipStream_t st, const FillArgs& a, int grid, size_t lds) {
    with_bool(a.cendoff != nullptr, [&](auto rk) {
        constexpr bool RK = decltype(rk)::value;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sd_fast_fill_wide<P, RK, F16, FL>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((sd_fast_fill_wide<P, RK, F16, FL>), dim3(grid), dim3(512), lds, st, a.chunks, a.n_chunks, a.bases2,
                           a.nmask, a.table, a.lane_consts, a.sc, a.B, a.ckpt, a.ckbase, a.queue, a.order, a.cendoff, a.crank);
    });
}

// multi-wave layouts (sd_fast_fill_wn), nw waves per workgroup.  The W-wave forms fill the chunks of a.order with the whole
// set (RANKED where the batch has --ed_thr ranks); the compacted ones a class of chunks with its kept templates.
template <int P, int FL, bool COMPACT, bool TILED, bool F16>
void launch_wn(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds) {
    auto go = [&](auto rk) {
        constexpr bool RK = decltype(rk)::value;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sd_fast_fill_wn<P, RK, FL, COMPACT, TILED, F16>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((sd_fast_fill_wn<P, RK, FL, COMPACT, TILED, F16>), dim3(grid), dim3(64 * nw), lds, st, a.chunks,
                           COMPACT ? 0 : a.n_chunks, a.bases2, a.nmask, COMPACT ? nullptr : a.table, a.lane_consts, a.sc,
                           plan.waves, plan.bf8_match, plan.bf8_mismatch, a.B, a.ckpt, a.ckbase, a.queue, a.order,
                           COMPACT ? nullptr : a.cendoff, COMPACT ? nullptr : a.crank, a.n_ptr,
                           COMPACT && !TILED ? a.klist : nullptr, COMPACT ? a.tcodes : nullptr, COMPACT ? a.toff : nullptr,
                           COMPACT ? a.tlen : nullptr, COMPACT ? plan.T : 0,
                           TILED ? (int)(plan.H | fast_has_1bp(plan) << 8) : 0, COMPACT && TILED ? a.lane_t : nullptr);
    };
    if constexpr (COMPACT) go(std::false_type());   // (the compacted form has no ranks)
    else with_bool(a.cendoff != nullptr, go);
}

}  // namespace sd
