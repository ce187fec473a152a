// sd_fast_wn_fl.hip -- instantiations of sd_fast_fill_wn (sd_fast_wn_fill.hpp) that take the maximum of a slot's
// diagonal input with the start term only in the first 48 slots (see sd_fast_fl.hip for the argument): 3.5
// instead of 4.5 packed ops per slot behind them.
#include "sd_fast_launch.hpp"

namespace sd {

void launch_fast_fill_wn_fl(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds) {
    with_p(FastWideP(), plan.P, [&](auto p) {
        launch_wn<decltype(p)::value, 48, false, false, true>(plan, st, a, grid, plan.waves, lds);
    });
}

}  // namespace sd
