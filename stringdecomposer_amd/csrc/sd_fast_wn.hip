// sd_fast_wn.hip -- multi-wave wide variant of the fast fill: template sets beyond 128 templates
// (hundreds of monomers; the reference takes any monomer set, main.cpp:187-207).
//
// A workgroup of W waves (W = ceil(T / 128), up to 8 = 1024 templates) owns one chunk at a time; wave w
// holds templates [128 w, 128 w + 128), ONE template per virtual lane as in sd_fast_wide.hip (P >= Lmax
// slots in registers, no cross-lane chain).  Rows are strictly sequential because B_i is the maximum over
// ALL template ends (main.cpp:184-186): every wave reduces its own ends (DPP), the wave results meet in
// LDS, one workgroup barrier per row, and every wave derives the same B_i / arg-max.
//
// The per-symbol score table of the single-wave kernel (5 x 128 x P bf8 bytes = 112 KB of LDS) cannot be
// replicated per wave, so LDS holds, per wave, the template base CODES only (one byte per slot and plane,
// symbol-independent, 22.5 KB at P = 176), and the row's table bytes are produced on the fly: the eight
// bf8 bytes {code c == row symbol ? match : mismatch (c = 0..4), -inf for padding (code 7)} sit in two
// registers and ONE v_perm_b32 turns a dword of four codes into the four bf8 table bytes of two slots;
// v_cvt_scalef32_pk_f16_bf8 then expands a slot's {lo, hi} pair as in the single-wave kernel.  4.5 VALU
// ops per slot (perm/2 + cvt + max + add + max3) instead of 4.
//
// Outputs as sd_fast_fill_wide (checkpoints every FAST_R rows: [checkpoint][wave][P][64]; one word per
// row, here (B_i << 10) | (wave << 7 | virtual lane)) -> the same traceback kernel (bshift = 10).
#include "sd_fast_launch.hpp"

namespace sd {

void launch_fast_fill_wn(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds) {
    with_p(FastWideP(), plan.P, [&](auto p) {
        constexpr int P = decltype(p)::value;
        launch_wn<P, P, false, false, true>(plan, st, a, grid, plan.waves, lds);
    });
}

}  // namespace sd
