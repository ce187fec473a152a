// sd_fast_wide.hip -- wide variant of the fast fill for large template sets (up to 128 templates,
// e.g. the 64-monomer suprachromosomal-family configuration): ONE template per virtual lane
// (P >= Lmax slots, no cross-lane chain, no lazy carry).
//
// The (mm - del - ins) table is int8 ({lo plane, hi plane} byte pairs) so that 128 x 176 cells x
// 5 read symbols fit the 160 KB LDS; it is streamed 16 slots at a time into a double-buffered
// 16-register window.  5 VALU ops per cell pair (the add is two SDWA byte adds).  Tail slots behind
// a template's last cell hold the table byte -128: in the row-shifted domain
// S_new[last] >= max(S_old[last], KB) - 127, so such a slot is a transparent copy of the last cell
// and the template end is always read from slot P-1.
//
// Same outputs as sd_fast_fill (packed B/arg-max words, checkpoints) -> same traceback kernel.
// Replaces reference stringdecomposer/src/main.cpp:171-216 like sd_fast_fill does.
#include "sd_fast_launch.hpp"

namespace sd {

void launch_fast_fill_wide(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds) {
    with_p(FastWideP(), plan.P, [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (plan.f16) launch_wide<P, true, P>(st, a, grid, lds);
        else launch_wide<P, false, P>(st, a, grid, lds);
    });
}

}  // namespace sd
