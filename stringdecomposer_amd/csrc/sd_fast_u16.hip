// sd_fast_u16.hip -- the narrow fill with the start-term maximum in every slot (what sd_fast.hip instantiates for fp16 and
// int16 cells) for the biased-u16 cell format (CellOps<CF_U16>, sd_fast_dev.hpp): slot counts below 30, template sets whose
// floor_slots exceeds every FL level of sd_fast_fl_u16.hip, sets with 1-bp templates (the FLC_ONE form), SD_FLAG_FULL_FLOOR.
#include "sd_fast_launch.hpp"

namespace sd {

void launch_fast_fill_full_u16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, bool one) {
    with_p(FastP(), plan.P, [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (one) launch_narrow<P, CF_U16, P, true, 0>(st, a, grid, nw, lds, plan.Hx);
        else launch_narrow<P, CF_U16, P, false, 0>(st, a, grid, nw, lds, plan.Hx);
    });
}

}  // namespace sd
