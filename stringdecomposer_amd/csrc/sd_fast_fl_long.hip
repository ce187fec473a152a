// sd_fast_fl_long.hip -- the variants of sd_fast_fl.hip for P = 42..64 slots per lane (sets of 13 to 23 monomers
// of ~170 bp, or longer monomers), in their own translation unit so that the library builds in parallel.
#include "sd_fast_launch.hpp"

// (sd_fast_fl_long_u16.hip and sd_fast_fl_long_u16s.hip compile this file again for the biased-u16 cell format)
#ifndef SD_FL_CF
#define SD_FL_CF CF_F16
#define SD_FL_STEP 0      /* one floor level for every row; sd_fast_fl_long_u16.hip sets 4: levels by read symbol */
#define SD_FL_ENTRY launch_fast_fill_fl_long
#endif

namespace sd {

void SD_FL_ENTRY(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl) {
    const uint64_t levels = fast_fill_levels(plan, fl, SD_FL_STEP);
    with_p(FastFlLongP(), plan.P, [&](auto p) {
        with_p(FlLongLevels(), fl, [&](auto f) {
            launch_narrow<decltype(p)::value, SD_FL_CF, decltype(f)::value, false, SD_FL_STEP>(st, a, grid, nw, lds, plan.Hx, levels);
        });
    });
}

}  // namespace sd
