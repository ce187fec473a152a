// sd_fast.hpp -- layout plan + launch wrappers of the fast kernel family (sd_fast.hip).
//
// Lane layout ("virtual lanes"): a wave owns one chunk.  Every 32-bit VGPR holds two int16 DP
// cells, one of the "lo plane" (bits 0..15) and one of the "hi plane" (bits 16..31); plane h,
// lane l is virtual lane v = 64*h + l and owns P consecutive slots of the flattened template axis
// (P registers).  Template j occupies V_j = ceil(L_j / P) consecutive virtual lanes of ONE plane,
// starting at slot 0 of its first virtual lane; the unused tail slots of its last virtual lane are
// "transparent" padding cells that carry E[L_j-1] to the last slot.  Templates 0..s-1 live in the
// lo plane, s..T-1 in the hi plane, in order, so that "smallest virtual lane" == "first template".
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "sd_device.hpp"

namespace sd {

constexpr int FAST_R = 32;          // checkpoint interval (rows)
constexpr int FAST_REBASE = 128;    // int16 rebase interval (rows), a multiple of FAST_R
constexpr int FAST_LANE_WORDS = 8;  // dwords of per-lane constants

// per-lane constant block (dword index), every dword = packed {lo plane, hi plane} int16
enum FastLaneConst {
    FLC_STARTMASK = 0, // 0xffff where the virtual lane starts a template (or is idle)
    FLC_CONTMASK,      // 0xffff where virtual lane v-1 belongs to the same template
    FLC_ENDOFF,        // (L-1)*del on the last virtual lane of a template, NEG elsewhere
    FLC_ROW0,          // row-0 adjustment of slot 0: ins+del on start lanes, ins elsewhere
    FLC_TMPL,          // template index per plane (for the traceback: vlane -> template)
    FLC_CONT2,         // 0xffff where virtual lane v-2 belongs to the same template
    FLC_ENDALL,        // (L-1)*del on EVERY virtual lane of a template, NEG on idle lanes
    FLC_ONE,           // 0xffff where the virtual lane holds a 1-bp template: its end is slot 0, not the last slot
};

struct FastPlan {
    bool ok = false;
    bool wide = false;    // one template per virtual lane, int8 table streamed from LDS (P > 64)
    bool f16 = false;     // narrow layout with packed-fp16 cells (3 ops per cell pair, v_pk_maximum3_f16)
    bool u16 = false;     // narrow layout with biased unsigned 16-bit cells (CellOps<CF_U16>: the same 3 ops, the add a plain
                          // v_add_u32, exact range +-15 k); takes precedence over f16 and int16 where the range fits
    int u16_lim = 0;      // |stored cell| the u16 format's run-time guard allows (>= range_bound)
    int P = 0;            // slots per virtual lane
    int P4 = 0;           // P rounded up to a multiple of 4 (LDS table row)
    int H = 0;            // carry hops of the cross-lane chain: Vmax-1
    // what the narrow fills get as their `int Hx` (the same bits):
    //   bits 0..7    H
    //   bit 8        the carry scan takes its shifted operands from ds_bpermute (both planes segment alike, bits 16..21)
    //   bit 9        ... in the last round too (developer A/B: SD_FILL_BPERM_TAIL)
    //   bit 10       the set has 1-bp templates (FLC_ONE: fast_has_1bp)
    //   bit 11       rebase every 64 rows instead of 128 (FastPlan::rebase)
    //   bits 16..21  with bit 8: a virtual lane that is idle in both planes
    //   bits 22..31  0 (the floor levels of the u16 fills travel in a kernel argument of their own: fast_fill_levels)
    uint32_t Hx = 0;
    int T = 0;
    int split = 0;        // templates [0,split) in the lo plane
    int Lmax = 0;
    int Qk = 0;           // traceback: template cells per lane = ceil(Lmax/64)
    int waves = 1;        // waves per chunk: 1, or ceil(T/128) for the multi-wave wide layout (sd_fast_wn.hip)
    bool tiled = false;   // multi-wave layout with templates tiled over consecutive virtual lanes (sd_fast_wt.hip); wide is set too
    bool filter_only = false;   // tiled, and the whole set does NOT fit eight waves: only with --ed_thr, every chunk in the
                                // compacted form (its kept templates re-dealt, sd_tiled_place); a chunk whose kept templates
                                // do not fit either raises the guard flag and the batch is repeated on the generic family
    int bshift = 7;       // B words: (B_i << bshift) | arg-max (wave << 7 | virtual lane)
    int rebase = FAST_REBASE;  // rows between two rebases of the stored cells (ScoreArgs::rebase_mask + 1; the narrow fills read it from Hx bit 11): 128 or 64
    int range_bound = 0;       // proven bound on |stored cell| between two rebases (fp16 formats need <= 2040)
    bool full_floor = false;   // launch the fills that take the start-term maximum in every slot (SD_FLAG_FULL_FLOOR: A/B, parity test)
    int floor_slots = 0;  // last slot of a lane whose diagonal input needs the max with the start term (see sd_fast_fill)
    int floor_sym[5] = {0, 0, 0, 0, 0};   // the same per read symbol (A C G T N); floor_slots = their maximum
    bool table_nonneg = false;            // every table value (mm - del - ins) >= 0: the fills may apply the floor in place (sd_fast_fill: FLS)
    int floor_pair[5][5] = {};            // [previous][current read symbol]: the last slot that needs the floor in a row whose neighbour above had
                                          // symbol `previous` (<= floor_sym[current]; == floor_sym[current] on the diagonal and behind an N)
    bool pair_rule = false;               // the conditions of the pair levels hold (table_nonneg, del <= 0, end offsets + del <= 0); else
                                          // floor_pair[a][b] == floor_sym[b]
    std::vector<std::vector<int32_t>> lane_bounds;   // narrow layout, per template: first cell of each of its lanes, then its length
    uint32_t bf8_match = 0, bf8_mismatch = 0;   // multi-wave wide layout: the two table values as bf8 bytes (f16) or int8 bytes (integer cells)
    std::vector<int32_t> vlane0;         // first virtual lane of template j
    std::vector<uint32_t> table;         // narrow: [5][P4/4][64][4] packed int16 (mm - del - ins), NEG on padding
                                         // wide:   [5][P/16][2][64][4] dwords of int8 {lo,hi} pairs, -128 on padding
    std::vector<uint32_t> lane_consts;   // [64][FAST_LANE_WORDS]
    std::vector<uint32_t> slot_of;       // per template cell x=toff[j]+k: (wave << 16) | (slot << 7) | vlane
    std::vector<uint8_t> tcodes;         // per template cell: base code
    std::vector<int32_t> end_vlane;      // virtual lane holding the end of template j
    std::vector<int32_t> end_off;        // (L_j - 1) * del
    // traceback, second form (sd_fast_trace2.hip): packed 16-bit recomputation, two blocks per wave
    bool tr2_ok = false;                 // one wave per chunk in the fill (narrow layout, wide / tiled layouts of one wave), templates <= 256 bp, scores inside the 16-bit tagged range
    int tr2_qm = 0;                      // ceil(Lmax / 64): registers per lane at the widest level
    int tr2_xlim = 0;                    // |E' - base| a checkpoint cell may have (run-time check of the range proof)
    int tr2_bound = 0;                   // the proven bound on |E' - base| for this template set and scoring (<= tr2_xlim)
    std::vector<uint32_t> tr2_tab;       // per template and level: table [5][QQ][32] + checkpoint map [QQ][2][32]
};

// the tables of sd_fast_trace_pk for a built narrow plan (tr2_ok = false when it does not apply)
void fast_plan_trace2(const std::vector<std::string>& tseq, ScoreArgs sc, FastPlan& plan);

// the set has 1-bp templates (FastPlan::Hx bit 10): only the full narrow fills and the tiled ones know that form
inline bool fast_has_1bp(const FastPlan& plan) { return (plan.Hx >> 10) & 1; }

// The values a kernel template is instantiated for.  with_p(List(), v, f) calls f(std::integral_constant<int, v>()) when v
// is in the list, else nothing: a launcher maps a run-time P or floor level onto the template argument with it.
template <int... Vs> struct PList { static constexpr int v[] = {Vs...}; };
template <int... Vs, typename F> void with_p(PList<Vs...>, int v, F&& f) {
    (void)((v == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...);
}
template <typename F> void with_bool(bool b, F&& f) { b ? f(std::true_type()) : f(std::false_type()); }

// slots per virtual lane: the narrow layout, the P of its FL kernels (P <= 40, P > 40), the wide and the tiled layouts
using FastP = PList<4, 8, 12, 16, 20, 24, 28, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 42, 44, 46, 48, 52, 56, 60, 64>;
using FastFlP = PList<30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40>;
using FastFlLongP = PList<42, 44, 46, 48, 52, 56, 60, 64>;
using FastWideP = PList<80, 96, 112, 128, 144, 160, 176, 192, 208, 224>;
using FastTiledP = PList<96, 128, 160, 192, 224>;
// floor levels FL of the FL kernels: narrow fp16 / u16 cells (P <= 40, P > 40), narrow int16 cells (the same), wide layout
using FlLevels = PList<12, 16, 20, 24, 28>;
using FlLongLevels = PList<16, 24, 32>;
using FlI16Levels = PList<16, 24>;
using FlLongI16Levels = PList<24>;
using FlWideLevels = PList<32, 64>;

// Builds the plan; returns false (with the reason) when the fast family cannot represent the
// input exactly (then the generic family is used).
bool fast_plan_build(const std::vector<std::string>& tseq, ScoreArgs sc, int max_rows,
                     FastPlan& plan, std::string& why, bool allow_f16 = true, bool allow_tr2 = true,
                     bool filter_only_ok = false,    // --ed_thr is on: a set beyond eight waves may take the filter-only form
                     bool allow_u16 = true);         // false: SD_FLAG_NO_U16 (the narrow layout's fp16 / int16 cells as in rounds 1-5)

// --ed_thr prefilter on the device (sd_filter.hip): infix edit distances, kept set and ranks per
// chunk -> per-chunk lane constants of the fast family (cendoff, crank: [chunk][64] packed {lo,hi}
// int16; grank == nullptr) or the rank table of the generic family (grank: [chunk][T], 0xffff = dropped)
void build_peq(const std::vector<std::string>& tseq, std::vector<unsigned long long>& peq);
struct FilterArgs {
    const ChunkDesc* chunks;
    int n_chunks;
    int T;
    int Lmax;
    int ed_thr;
    const uint32_t* bases2;
    const uint32_t* nmask;
    const unsigned long long* peq;
    const int32_t* tlen;
    int32_t* dist;                     // [chunk][T] infix edit distances
    int uniform_half = -1;             // 0 / 1: every template ends in the low / high half of word ceil(L/64)-1
                                       // and all have that many words (sd_hw_dist_u); -1: general kernel
    // fast family: the templates' end lanes and offsets in, the per-chunk lane constants out
    const int32_t* end_vlane = nullptr;
    const int32_t* end_off = nullptr;
    const int32_t* vlane0 = nullptr;   // first virtual lane of each template (narrow layout)
    uint32_t* cendoff = nullptr;
    uint32_t* crank = nullptr;
    int waves = 1;
    // ... its compacted classes (more than 128 templates): every template's place, the kept templates in filtered
    // order and their count per chunk
    uint16_t* kpos = nullptr;
    uint16_t* klist = nullptr;
    int32_t* nkept = nullptr;
    uint16_t* grank = nullptr;         // generic family: the rank table (set: cendoff / crank are not written)
    // the screen (sd_screen.hip): set, the launch reduces the distances to key[chunk] = (min distance << 16) | first
    // template that has it and writes nothing else (dist, ranks and ed_thr are not used)
    uint32_t* screen_key = nullptr;
    bool dist_only = false;            // the distance kernel alone into dist: no fills, no sd_rank_keep (tools/screen_bench.py)
};
void launch_edthr_filter(hipStream_t st, const FilterArgs& a);
// --ed_thr with more than 128 templates: the chunk order split into W classes by ceil(kept templates / 128)
// --ed_thr on the tiled multi-wave layout: per chunk, the kept templates' lanes (sd_filter.hip: sd_tiled_place)
void launch_tiled_place(hipStream_t st, int n_chunks, int T, int P, int W, const uint16_t* klist, int32_t* nkept,
                        const int32_t* tlen, uint16_t* kpos, uint32_t* lane_t, int* overflow_flag = nullptr);
void launch_split_order(hipStream_t st, const int* order, int n, const int32_t* nkept, int* orders, int* counts,
                        int W);   // orders: [W][n] -- class w-1 = the chunks that need w waves, in the given order

// number of checkpoint rows of the batch; fills ChunkDesc::pad with each chunk's first checkpoint
int64_t fast_ckpt_rows_total(const FastPlan& plan, std::vector<ChunkDesc>& chunks);

// Operands of one batch's fill.  Every fill launcher takes (plan, stream, FillArgs) and, beside them, only what its
// chooser decides (launch_fast_fill, launch_fast_fill_compact: sd_fast.hip): the launch geometry -- grid, nw (or wb) waves
// per workgroup, lds bytes -- and the kernel form -- fl = the floor level (P: the full kernel), one = the 1-bp form.
struct FillArgs {
    const ChunkDesc* chunks;
    int n_chunks;                      // (where n_ptr is set: the bound the launch geometry is sized by)
    const int* n_ptr = nullptr;        // the number of chunks lives on the device (order = a class list of launch_split_order)
    const uint32_t* bases2;
    const uint32_t* nmask;
    const uint32_t* table;             // FastPlan::table on the device
    const uint32_t* lane_consts;
    ScoreArgs sc;
    int32_t* B;
    int32_t* argV;
    uint32_t* ckpt;
    int32_t* ckbase;
    int* queue;                        // a zeroed work-queue head that no earlier launch has used: no memset between launches
    const int* order;
    int n_cu;
    const uint32_t* cendoff = nullptr; // --ed_thr: per-chunk end offsets and ranks (the RANKED kernels)
    const uint32_t* crank = nullptr;
    // the compacted classes of --ed_thr: a chunk's kept templates, one per lane (klist) or over the lanes of the tiled
    // layout (lane_t: sd_tiled_place), and the templates' codes, offsets and lengths
    const uint16_t* klist = nullptr;
    const uint32_t* lane_t = nullptr;
    const uint8_t* tcodes = nullptr;
    const int32_t* toff = nullptr;
    const int32_t* tlen = nullptr;
};

// Operands of one batch's traceback (launch_fast_trace)
struct TraceArgs {
    const ChunkDesc* chunks;
    int n_chunks;
    const uint32_t* bases2;
    const uint32_t* nmask;
    const uint32_t* slot_of;
    const uint8_t* tcodes;
    const uint32_t* lane_consts;
    const int32_t* toff;
    const int32_t* tlen;
    ScoreArgs sc;
    const int32_t* B;
    const int32_t* argV;
    const uint32_t* ckpt;
    const int32_t* ckbase;
    DevRec* recs;
    int32_t* rec_cnt;
    int* queue;
    const int* order;
    int n_cu;
    const uint32_t* tr2_tab = nullptr; // device copy of FastPlan::tr2_tab: the packed two-block form where it applies
    // chunks filled in the compacted form: kept templates, their places and count per chunk; the tiled layout's lane table
    // (kpos = first lanes then; FastPlan::filter_only: every chunk is one, or skipped)
    const uint16_t* klist = nullptr;
    const uint16_t* kpos = nullptr;
    const int32_t* nkept = nullptr;
    const uint32_t* lane_t = nullptr;
};

// The fill of one batch: chooses the kernel -- layout, cell format, floor form -- and its launch geometry (min_lds,
// pipeline mode 2: what the narrow fills ask for at least, so that a third workgroup never fits a CU)
void launch_fast_fill(const FastPlan& plan, hipStream_t st, const FillArgs& a, size_t min_lds = 0);
// --ed_thr, multi-wave layouts: one class of chunks (a.order, a.n_ptr) filled by wb waves holding their kept templates
void launch_fast_fill_compact(const FastPlan& plan, hipStream_t st, const FillArgs& a, int wb);
// the `levels` argument of a narrow FL launch with levels per row (step > 0; else 0): two bits per (previous, current) read
// symbol at bit 2 * (5 * previous + current), level l = the start-term maximum in the first fl - l * step slots
// (sd_fast_fill.hpp: FLS).  From FastPlan::floor_pair; with SD_FILL_SYMBOL_LEVEL set from floor_sym[current] for every
// previous symbol (developer A/B, parity test).
uint64_t fast_fill_levels(const FastPlan& plan, int fl, int step);

// The kernels of one family at plan.P, launched by the two choosers above.
// Narrow layout, the start-term maximum in the first fl slots of a lane only: fp16 cells (sd_fast_fl.hip: P <= 40,
// sd_fast_fl_long.hip: P > 40), u16 cells with levels by read symbol (_u16) or one level (_u16s), int16 cells (_i16)
void launch_fast_fill_fl(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl);
void launch_fast_fill_fl_long(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl);
void launch_fast_fill_fl_u16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl);
void launch_fast_fill_fl_long_u16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl);
void launch_fast_fill_fl_u16s(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl);
void launch_fast_fill_fl_long_u16s(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl);
void launch_fast_fill_fl_i16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, int fl);
// ... and in every slot, u16 cells (sd_fast_u16.hip; fp16 and int16 cells: sd_fast.hip)
void launch_fast_fill_full_u16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int nw, size_t lds, bool one);
// wide layout: every slot (sd_fast_wide.hip), fp16 cells with fl = 32 / 64 (sd_fast_wide_fl.hip)
void launch_fast_fill_wide(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds);
void launch_fast_fill_wide_fl(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds, int fl);
// multi-wave layouts, plan.waves waves per workgroup: wide (sd_fast_wn.hip, sd_fast_wn_fl.hip: fl = 48) and tiled
// (sd_fast_wt.hip: fl = 48 or P) with fp16 cells, both with int16 cells (sd_fast_wn_i16.hip)
void launch_fast_fill_wn(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds);
void launch_fast_fill_wn_fl(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds);
void launch_fast_fill_wt(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds, int fl);
void launch_fast_fill_wn_i16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds);
void launch_fast_fill_wt_i16(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, size_t lds);
// their compacted forms, wb waves per workgroup (sd_fast_wn_ck.hip, sd_fast_wt.hip): fl = 48 or P
void launch_fast_fill_wn_compact(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int wb, size_t lds, int fl);
void launch_fast_fill_wt_compact(const FastPlan& plan, hipStream_t st, const FillArgs& a, int grid, int wb, size_t lds, int fl);

// The traceback of one batch: the packed two-block form (sd_fast_trace2.hip) where the plan has it, else sd_fast_trace
void launch_fast_trace(const FastPlan& plan, hipStream_t st, const TraceArgs& a);
void launch_fast_trace2(const FastPlan& plan, hipStream_t st, const TraceArgs& a);

}  // namespace sd
