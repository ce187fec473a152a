// sd_fast_fl_i16.hip -- the variants of sd_fast_fl.hip / sd_fast_fl_long.hip for the packed-int16 cell format
// (scorings whose range does not fit fp16): 3 instead of 4 packed ops per slot behind the first FL slots.
// Fewer levels than the fp16 variants: FL = 16 / 24 for P = 30..40, FL = 24 for P = 42..64.
#include "sd_fast_launch.hpp"

namespace sd {

void launch_fast_fill_fl_i16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl) {
    auto go = [&](auto p, auto f) {
        launch_narrow<decltype(p)::value, CF_I16, decltype(f)::value, false, 0>(st, a, grid, nw, lds, plan.Hx);
    };
    with_p(FastFlP(), plan.P, [&](auto p) { with_p(FlI16Levels(), fl, [&](auto f) { go(p, f); }); });
    with_p(FastFlLongP(), plan.P, [&](auto p) { with_p(FlLongI16Levels(), fl, [&](auto f) { go(p, f); }); });
}

}  // namespace sd
