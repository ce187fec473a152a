// sd_final_ws.hpp -- internal to libsd_hip.so: the final selection on the device (sd_final_dev.hip; SD_FLAG_DEVICE_FINAL
// streams, sd_final_select_dev).  A job of such a stream keeps, beside its record store (RowsWS), the identity words of
// every record at the record's index; behind the seam merge one kernel writes where each merged row came from, the
// selection kernels turn every merged row into an sd_final_row (sd_final_dev.hpp: the host's rule) and a keep flag,
// and the flags are counted and scanned.  The kept rows, their offsets per read and their key identities are copied
// into the caller's buffers on the CALLER's stream (final_scatter), so the rules of RowsWS hold here too: the host
// waits for ev_free before any of these buffers is reallocated or released.
#pragma once

#include "sd_final_dev.hpp"
#include "sd_final_prof_ws.hpp"
#include "sd_pipeline.hpp"

namespace sdi {

// the tables of a PostProcessor in device memory, uploaded once per stream
struct FinalDevTables {
    DevBuf<int32_t> key_of_t, kcol, key_of_il;
    sd::FinalTables tb;   // device pointers
    void upload(const sd::FinalTables& h) {
        auto up = [](DevBuf<int32_t>& d, const int32_t* p, size_t n) {
            d.alloc(n);
            if (n) SD_HIP(hipMemcpy(d.p, p, n * sizeof(int32_t), hipMemcpyHostToDevice));
        };
        up(key_of_t, h.key_of_t, (size_t)h.n_tmpl);
        up(kcol, h.kcol, (size_t)h.n_keys);
        up(key_of_il, h.key_of_il, (size_t)h.n_tmpl);
        tb = h;
        tb.key_of_t = key_of_t.p;
        tb.kcol = kcol.p;
        tb.key_of_il = key_of_il.p;
    }
};

struct FinalWS {
    DevBuf<uint32_t> words, hwords;   // per record of the job's store: its identity words, plain / homopolymer-compressed
    DevBuf<int64_t> src;              // per merged row: its record in the store (and so its words)
    DevBuf<int64_t> moff;             // per read: its first merged row (n_reads + 1)
    DevBuf<int64_t> rlen;             // per read: its length
    DevBuf<sd::DevRec> mrows;         // text-based path only: the merged raw rows on their way to the host
    DevBuf<sd_final_row> rows;        // per merged row: the selected row (valid where keep is set)
    DevBuf<double> alt;               // per merged row: its key identities (second_best)
    DevBuf<uint8_t> keep;             // per merged row: kept by the selection
    DevBuf<int64_t> dst;              // per merged row: its place among the kept rows, or -1 (written by the scatter)
    DevBuf<int32_t> bsum;             // kept rows per tile
    DevBuf<int64_t> bbase;            // kept rows before each tile; [tiles] = the kept rows
    DevBuf<unsigned long long> und;   // rows the words do not decide
    PinBuf<int64_t> h_counts;         // [0] kept rows [1] undecided rows
    PinBuf<int64_t> h_rlen;
    hipEvent_t ev_sel = nullptr, ev_free = nullptr;
    bool free_recorded = false;
    bool settled = true;              // (as RowsWS::settled)
    int64_t cap_rows = 0, n_tiles = 0;
    int32_t n_reads = 0, n_keys = 0;
    const int64_t* n_ptr = nullptr;   // device: the number of merged rows
    const int64_t* d_moff = nullptr;
    // SD_FLAG_DEVICE_PROFILE: the plan of the job's pairs (sd_final_prof_ws.hpp).  The fold runs on the stream's own
    // stream after collect has returned and reads prof and the job's text; the upload of a host job's text runs there
    // too.  ev_prof is recorded behind either (ev_f0 before a fold: its time), and the rule of ev_free holds for it:
    // the host has seen it before this workspace is reused or released.  The job's text (StreamJob::din.text) waits here
    // meanwhile, and goes back to the stream's spare list with the workspace's next job.
    ProfWS prof;
    hipEvent_t ev_f0 = nullptr, ev_prof = nullptr;
    bool prof_recorded = false, fold_timed = false;
    std::unique_ptr<DevBuf<uint8_t>> held_text;
    bool idle() {
        if (free_recorded && hipEventQuery(ev_free) != hipErrorNotReady) { (void)hipGetLastError(); free_recorded = false; }
        if (prof_recorded && hipEventQuery(ev_prof) != hipErrorNotReady) { (void)hipGetLastError(); prof_recorded = false; }
        return !free_recorded && !prof_recorded;
    }
    void wait_idle() {
        if (free_recorded) { if (hipEventSynchronize(ev_free) != hipSuccess) (void)hipGetLastError(); free_recorded = false; }
        if (prof_recorded) { if (hipEventSynchronize(ev_prof) != hipSuccess) (void)hipGetLastError(); prof_recorded = false; }
    }
    ~FinalWS() {
        wait_idle();
        if (ev_sel) (void)hipEventDestroy(ev_sel);
        if (ev_free) (void)hipEventDestroy(ev_free);
        if (ev_f0) (void)hipEventDestroy(ev_f0);
        if (ev_prof) (void)hipEventDestroy(ev_prof);
    }
};

// (all throw HipFail)
// where the merged rows of an assembled store came from: f.src and f.moff from the keep flags of ws (behind rows_assemble
// on the same stream)
void final_sources(FinalWS& f, RowsWS& ws, hipStream_t st);
// The selection of up to cap_rows rows (*n_ptr of them, read on the device): row m = recs[ridx ? ridx[m] : m], its words
// at words / hwords + widx[m] * per, its read from moff (n_reads + 1, device); d_rlen may be null.  Leaves the selected
// rows, flags and counts in f, the two counts on their way to f.h_counts, and records f.ev_sel.
void final_select(FinalWS& f, hipStream_t st, const sd::FinalTables& dtb, const sd::DevRec* recs, const int64_t* ridx,
                  const int64_t* widx, const uint32_t* words, const uint32_t* hwords, const int64_t* moff,
                  const int64_t* d_rlen, int32_t n_reads, int64_t cap_rows, const int64_t* n_ptr);
// the kept rows into out[0 .. cap), their offsets per read and (alt != null) their key identities; records f.ev_free
void final_scatter(FinalWS& f, hipStream_t st, sd_final_row* out, int64_t cap, int64_t* row_off, double* alt);

}  // namespace sdi
