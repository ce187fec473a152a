// sd_fast_fl.hip -- instantiations of sd_fast_fill (sd_fast_fill.hpp) that take the maximum of a slot's
// diagonal input with the start term only in the first FL slots of a lane.
//
// In the recurrence  S'[x] = max3(S'[x-1], max(S[x-1], KB) + tbl[x], S[x])  the term KB + tbl[x] (KB = the
// row's start term B_i + del joined with the lane's lazy carry) is one more candidate of slot x.  S' is a
// prefix maximum along the slots, and tbl takes two values per read symbol, so KB + tbl[x] can only raise
// S'[x] where tbl[x] exceeds every tbl[x'] of an earlier slot x' >= 1 of the lane -- slot 1 and the first
// slot holding the read's base (main.cpp:187-207 evaluates the start term in every cell; this is the same
// maximum with the dominated candidates left out).  fast_plan_build finds the last such slot over all lanes
// and the five read symbols (FastPlan::floor_slots: 16 on the synthetic 12-monomer set, 24 on the DXZ1
// monomers of the reference's test data); behind it a slot costs 2 packed ops instead of 3.
//
// Only slot counts P >= 30 (P = 30..40 here, 42..64 in sd_fast_fl_long.hip) and the fp16 cell format get these
// variants; everything else runs the full kernels of sd_fast.hip.
#include "sd_fast_launch.hpp"

// (sd_fast_fl_u16.hip and sd_fast_fl_u16s.hip compile this file again for the biased-u16 cell format: SD_FL_CF = CF_U16,
// their own entry names)
#ifndef SD_FL_CF
#define SD_FL_CF CF_F16
#define SD_FL_STEP 0      /* one floor level for every row; sd_fast_fl_u16.hip sets 4: levels by read symbol */
#define SD_FL_ENTRY launch_fast_fill_fl
#endif

namespace sd {

void SD_FL_ENTRY(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl) {
    const uint64_t levels = fast_fill_levels(plan, fl, SD_FL_STEP);
    with_p(FastFlP(), plan.P, [&](auto p) {
        with_p(FlLevels(), fl, [&](auto f) {
            launch_narrow<decltype(p)::value, SD_FL_CF, decltype(f)::value, false, SD_FL_STEP>(st, a, grid, nw, lds, plan.Hx, levels);
        });
    });
}

}  // namespace sd
