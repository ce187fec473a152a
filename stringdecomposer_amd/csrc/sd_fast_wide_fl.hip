// sd_fast_wide_fl.hip -- instantiations of sd_fast_fill_wide (sd_fast_wide_fill.hpp) that take the maximum of a
// slot's diagonal input with the start term only in the first FL slots (see sd_fast_fl.hip for the argument).
// In the wide layout a virtual lane holds a whole template, so FastPlan::floor_slots is the latest first
// occurrence of a base in any template: behind it a slot costs 3 packed ops (table conversion, add, maximum3)
// instead of 4.  fp16 cells only.
#include "sd_fast_launch.hpp"

namespace sd {

void launch_fast_fill_wide_fl(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds, int fl) {
    with_p(FastWideP(), plan.P, [&](auto p) {
        with_p(FlWideLevels(), fl, [&](auto f) { launch_wide<decltype(p)::value, true, decltype(f)::value>(st, a, grid, lds); });
    });
}

}  // namespace sd
