// sd_final_prof_ws.hpp -- internal to libsd_hip.so: the column profiles of a device-final stream on the device
// (SD_FLAG_DEVICE_PROFILE; sd_final_prof_dev.hip).  Behind the selection of a job one kernel plans the pair of every kept
// row (sd_final_prof_dev.hpp: the host's text), the pairs of sd_nw_profile are grouped by forward monomer (a scan over
// the monomer counts and a scatter: the counting sort nw_profile_device does on the host), and the counts, the longest
// segment and the number of host pairs travel to pinned memory -- 4 (M + 2) bytes, no base, record or row.  From that
// summary the host sizes the checkpoints, the work items and the grid, and the fold (sd_nw_profile, sd_nw.hip) adds
// into the stream's own 64-bit counters in HBM.
#pragma once

#include "sd_final_prof_dev.hpp"
#include "sd_pipeline.hpp"

namespace sdi {

// Per stream: the templates as the fold reads them, the counters, the checkpoints of the fold's lanes.
struct ProfDev {
    int M = 0, K = 1, tmax = 1, n_cu = 256;
    int64_t total = 0;                        // counters (profile_offsets)
    DevBuf<unsigned long long> peq;           // match masks of the interleaved templates
    DevBuf<unsigned long long> counts;        // total counters; the 64 bytes behind them: the fold's failure count
    DevBuf<int32_t> tlen, own_il;             // interleaved lengths; DP template -> interleaved index
    DevBuf<int64_t> poff;                     // per forward monomer: its first counter
    DevBuf<uint8_t> ck;                       // checkpoints of the fold in flight (folds run on ONE stream)
    DevBuf<int> ckpos;
    // uploads on st, which is waited for; the counters are zeroed.  il: m0, rc(m0), m1, ...; own: DP template -> il
    void setup(const std::vector<std::string>& il, const std::vector<int32_t>& own, hipStream_t st);
    int* fails() const { return reinterpret_cast<int*>(counts.p + total); }
};

// Per job (a member of FinalWS: it is reused under FinalWS's rules).  Everything per merged row is indexed by the row,
// so order[] holds row numbers and the fold reads seg_start / seg_len / pair_il through it.
struct ProfWS {
    DevBuf<int64_t> seg_start, text_off;      // per merged row: first base in the job's text; per read: its first base
    DevBuf<int32_t> seg_len, pair_il, order;
    DevBuf<uint8_t> cls;                      // per merged row: sd::FPROF_*
    DevBuf<int32_t> sum;                      // [0, M) kernel pairs per forward monomer, [M] longest such segment, [M + 1] host pairs
    DevBuf<int32_t> base, cursor;             // exclusive prefix of the counts (M + 1); scatter cursors, [M]: the host list's
    DevBuf<sd::FProfHostPair> hlist;          // the host pairs, compacted
    DevBuf<int4> items;
    PinBuf<int32_t> h_sum;
    PinBuf<int64_t> h_text_off;
    PinBuf<sd::FProfHostPair> h_hlist;
    PinBuf<uint8_t> h_text;                   // staging of the reads of a job submitted from host memory
    bool planned = false;
};

// (all throw HipFail)
// Plan and group on st: rows [0, min(*n_ptr, cap)), row m = recs[src ? src[m] : m] where keep[m]; its read from moff
// (n_reads + 1), rlen and w.text_off per read (w.text_off uploaded on st before).  Leaves the summary on its way to w.h_sum.
void prof_plan(ProfWS& w, const ProfDev& d, hipStream_t st, const sd::DevRec* recs, const int64_t* src, const uint8_t* keep,
               const int64_t* moff, const int64_t* rlen, int32_t n_reads, int64_t cap, const int64_t* n_ptr);
// The grouping alone, on a plan already in w (cls, pair_il, seg_start, seg_len per row and the counts w.sum[0 .. M)): the
// scan of the monomer counts and, over rows [0, min(*n_ptr, cap)), the scatter into w.order / w.hlist (cap 0: the scan only).
void prof_group(ProfWS& w, int M, hipStream_t st, int64_t cap, const int64_t* n_ptr);
// The scan alone: base[0 .. M] = the exclusive prefix of sum[0 .. M), cursor[0 .. M) = base, cursor[M] = 0 (one lane: M is
// tens to hundreds) -- the start of every grouping (sd_group_dev.hpp).
void group_scan(hipStream_t st, const int32_t* sum, int M, int32_t* base, int32_t* cursor);
// w.items[0 .. n_items) = the work items of up to `per` pairs from w.base.  clear: n_items is an upper bound taken without
// the counts -- the entries behind the last item are empty items (no pair).
void prof_items(ProfWS& w, int M, int per, int64_t n_items, hipStream_t st, bool clear);
// The work items and the fold on st, sized from w.h_sum (the host has seen the plan end).  text: the job's text on the
// device, readable up to the next multiple of 4 past its end.  Returns the pairs folded.  Grows d.ck after waiting for st.
int64_t prof_fold(ProfWS& w, ProfDev& d, hipStream_t st, const uint8_t* text);
// dst[i] += add[i] on st
void prof_add(hipStream_t st, unsigned long long* dst, const unsigned long long* add, int64_t n);

}  // namespace sdi
