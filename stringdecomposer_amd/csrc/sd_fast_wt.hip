// sd_fast_wt.hip -- tiled multi-wave variant of the fast fill: template sets that neither the narrow layout (at most
// 128 virtual lanes of up to 64 slots) nor the wide ones (one template per virtual lane of up to 224 slots) hold --
// e.g. sixty 340-bp templates, or two hundred 500-bp ones (the reference takes any monomer set, main.cpp:187-207).
//
// The kernel is sd_fast_fill_wn (sd_fast_wn_fill.hpp: W waves per chunk, template base codes in LDS, table bytes made
// on the fly, one workgroup barrier per row for B_i) with its TILED parameter: a template lies over V = ceil(L / P)
// consecutive virtual lanes of one plane of one wave and the deletion chain crosses the lanes through the lazily
// applied carry of the narrow fills (sd_fast_fill.hpp).  fast_plan_build() picks P from FastTiledP as the slot
// count with the least SIMD time per row at the occupancy it gets, among those that fit eight waves and the LDS of a CU;
// W may be 1.
//
// Outputs as the multi-wave wide fill: checkpoints [checkpoint][wave][P][64] (true values, max(cell, carry)), one word
// per row (B_i << 10) | (wave << 7 | virtual lane) -> sd_fast_trace (bshift = 10), whose cell -> (wave, lane, slot) map
// (FastPlan::slot_of) knows the tiling.  --ed_thr: the chunks whose kept templates need fewer than W waves are filled by
// that many (launch_fast_fill_wt_compact below: per-chunk lane table from sd_tiled_place), the others by the ranked form
// (per-chunk end offsets and ranks on every lane of a template, sd_rank_keep).
#include "sd_fast_launch.hpp"

namespace sd {

void launch_fast_fill_wt(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds, int fl) {
    with_p(FastTiledP(), plan.P, [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (fl == 48) launch_wn<P, 48, false, true, true>(plan, st, a, grid, plan.waves, lds);
        else launch_wn<P, P, false, true, true>(plan, st, a, grid, plan.waves, lds);
    });
}

// --ed_thr: the chunks whose kept templates need wb < W waves, filled by wb waves that hold exactly those (the point of
// the reference's prefilter, main.cpp:128-149: less DP work) -- the compacted form of sd_fast_wn_ck.hip with the
// per-chunk lane table of sd_tiled_place in place of "one kept template per lane".
void launch_fast_fill_wt_compact(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int wb, size_t lds, int fl) {
    with_p(FastTiledP(), plan.P, [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (fl == 48) launch_wn<P, 48, true, true, true>(plan, st, a, grid, wb, lds);
        else launch_wn<P, P, true, true, true>(plan, st, a, grid, wb, lds);
    });
}

}  // namespace sd
