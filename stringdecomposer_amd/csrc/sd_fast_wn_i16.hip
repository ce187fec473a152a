// sd_fast_wn_i16.hip -- the multi-wave fills (sd_fast_wn_fill.hpp) with packed int16 cells and int8 table bytes: the form a
// template set beyond one wave takes when its scoring leaves the exact-integer range of fp16 (or its table values are not
// exact in bf8), and the form an engine repeats a batch in after its fp16 range guard tripped.  The reference takes any
// scoring on any monomer set (main.cpp:187-207: long long cells); until round 5 these cases ran on the generic family.
#include "sd_fast_launch.hpp"

namespace sd {

// plain W-wave layout: one template per virtual lane, more than 128 templates
void launch_fast_fill_wn_i16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds) {
    with_p(FastWideP(), plan.P, [&](auto p) {
        constexpr int P = decltype(p)::value;
        launch_wn<P, P, false, false, false>(plan, st, a, grid, plan.waves, lds);
    });
}

// tiled layout: a template over consecutive virtual lanes
void launch_fast_fill_wt_i16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds) {
    with_p(FastTiledP(), plan.P, [&](auto p) {
        constexpr int P = decltype(p)::value;
        launch_wn<P, P, false, true, false>(plan, st, a, grid, plan.waves, lds);
    });
}

}  // namespace sd
