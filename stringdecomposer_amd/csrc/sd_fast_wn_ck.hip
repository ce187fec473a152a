// sd_fast_wn_ck.hip -- the compacted form of the multi-wave wide fill (sd_fast_wn_fill.hpp, COMPACT): with
// --ed_thr and more than 128 templates, a chunk is filled by ceil(kept / 128) waves holding exactly its kept
// templates, in their filtered order, instead of W waves holding all of them.
#include "sd_fast_launch.hpp"

namespace sd {

void launch_fast_fill_wn_compact(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int wb, size_t lds, int fl) {
    with_p(FastWideP(), plan.P, [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (fl == 48) launch_wn<P, 48, true, false, true>(plan, st, a, grid, wb, lds);
        else launch_wn<P, P, true, false, true>(plan, st, a, grid, wb, lds);
    });
}

}  // namespace sd
