// sd_engine.hip -- host engine + C-ABI of libsd_hip.so (include/sd_hip.h).
//
// Host side of the reference's AlignReadsSet (stringdecomposer/src/main.cpp:67-122): chunk table,
// device batches, ordered gather, per-read assembly, raw TSV.  The DP itself runs only in the HIP
// kernels (sd_generic.hip, sd_fast.hip); there is no CPU implementation of it in this library.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <chrono>
#include <functional>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sd_hip.h"
#include "sd_convert.hpp"
#include "sd_ident.hpp"
#include "sd_nw.hpp"
#include "sd_device.hpp"
#include "sd_fast.hpp"
#include "sd_host.hpp"
#include "sd_kernels.hpp"
#include "sd_records.hpp"
#include "sd_seam.hpp"
#include "sd_engine_int.hpp"
#include "sd_devices.hpp"

namespace sdi {
DevPool g_pool;
std::atomic<long long> g_alloc_ns{0};   // time spent in hipMalloc / hipHostMalloc (SD_TIMING report)
PinPool g_pinpool;
}  // namespace sdi


// Developer overrides of sd_params.reserved[] from the environment, read HERE and nowhere else (the switches are part
// of the parameters; the variables exist so that a test or an A/B run can flip one without touching the caller):
// SD_PIPE_MODE=0|1|2, SD_FILL_CELLS=i16, SD_FILL_FULLFLOOR=1, SD_EDTHR_COMPACT=0, SD_FILTER_GENERAL=1, SD_IDENT_STREAM=0, SD_TRACE=1,
// SD_F16_GUARD=<limit>.
void apply_env_overrides(sd_params& p) {
    if (p.reserved[0] == 0)
        if (const char* ev = getenv("SD_PIPE_MODE")) p.reserved[0] = std::max(0, std::min(2, atoi(ev))) + 1;
    auto on = [](const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; };
    if (on("SD_FILL_CELLS", 'i')) p.reserved[1] |= SD_FLAG_NO_F16;
    if (on("SD_FILL_CELLS", 'f')) p.reserved[1] |= SD_FLAG_NO_U16;   // f16: the narrow layout's cells of rounds 1-5 (A/B)
    if (getenv("SD_FILL_FULLFLOOR")) p.reserved[1] |= SD_FLAG_FULL_FLOOR;
    if (on("SD_EDTHR_COMPACT", '0')) p.reserved[1] |= SD_FLAG_NO_EDTHR_COMPACT;
    if (getenv("SD_FILTER_GENERAL")) p.reserved[1] |= SD_FLAG_FILTER_GENERAL;
    if (on("SD_IDENT_STREAM", '0')) p.reserved[1] |= SD_FLAG_NO_STREAM_IDENT;
    if (on("SD_TRACE", '1')) p.reserved[1] |= SD_FLAG_TRACE_V1;
    if (on("SD_IDENT_PRUNE", '0')) p.reserved[1] |= SD_FLAG_NO_IDENT_PRUNE;
    if (p.reserved[2] == 0)
        if (const char* ev = getenv("SD_F16_GUARD")) p.reserved[2] = std::max(0, atoi(ev));
}


namespace {

int device_count_checked() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void ensure_events(std::vector<hipEvent_t>& v, size_t count, unsigned flags = hipEventDefault) {
    while (v.size() < count) {
        hipEvent_t e;
        SD_HIP(hipEventCreateWithFlags(&e, flags));
        v.push_back(e);
    }
}

// Everything must stay above the reference's INF = -1e6 sentinel (main.cpp:156), which makes its
// `> INF` guards vacuous, and below 2^24 so that its float arithmetic on scores is exact.
int check_score_range(const sd_params& p, int Lmax, std::string& err) {
    auto a = [](int v) { return (int64_t)(v < 0 ? -v : v); };
    const int64_t n = (int64_t)p.part_size + p.overlap;
    const int64_t ms = std::max(std::max(a(p.ins), a(p.match)), a(p.mismatch));
    const int64_t bound = n * ms + (int64_t)Lmax * a(p.del) + a(p.mismatch);
    if (bound >= 1000000) {
        err = "scores x chunk length reach the reference's INF sentinel (-1e6): unsupported";
        return SD_ERR_UNSUPPORTED;
    }
    return SD_OK;
}

// What a monomer set and a scoring come to on the host, before any device call: the engine's reduced scores (score_scale,
// sc) and its template set (tseq: the monomers, then their reverse complements, main.cpp:364-371; tlen, toff, T, sumL,
// Lmax).  sd_engine_create starts from it, and sd_plan_info on an engine that never meets a device, so the plan a test
// without a GPU sees is the engine's.  SD_OK, or the code and text of the first monomer that is empty, has a symbol
// outside the alphabet or no complement.
int host_templates(sd_engine* e, const sd_params& p, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, std::string& err) {
    // A common factor of the four scores scales every DP value, every difference and every tie alike:
    // the device works with the reduced scores (more scorings fit the packed fp16 / int16 cells) and
    // the record scores are multiplied back when they are fetched.
    auto gcd = [](int a, int b) { a = a < 0 ? -a : a; b = b < 0 ? -b : b; while (b) { const int t = a % b; a = b; b = t; } return a; };
    const int g = std::max(1, gcd(gcd(p.ins, p.del), gcd(p.mismatch, p.match)));
    e->score_scale = g;
    e->sc = sd::ScoreArgs{p.ins / g, p.del / g, p.mismatch / g, p.match / g};
    e->T = 2 * n_mono;
    e->tseq.resize((size_t)e->T);
    for (int j = 0; j < n_mono; ++j) {
        if (mono_lens[j] <= 0) { err = "ERROR: empty monomer sequence"; return SD_ERR_EMPTY; }
        e->tseq[j].assign(mono_seqs[j], (size_t)mono_lens[j]);
        const int rc = sd::check_alphabet("<monomer>", mono_seqs[j], mono_lens[j], err);
        if (rc) return rc;
        if (!sd::reverse_complement(e->tseq[j], e->tseq[(size_t)n_mono + j])) { err = "map::at"; return SD_ERR_SYMBOL; }
    }
    e->tlen.resize((size_t)e->T);
    e->toff.resize((size_t)e->T + 1);
    for (int j = 0; j < e->T; ++j) {
        e->tlen[j] = (int32_t)e->tseq[j].size();
        e->toff[j + 1] = e->toff[j] + e->tlen[j];
        e->Lmax = std::max(e->Lmax, (int)e->tlen[j]);
    }
    e->sumL = e->toff[e->T];
    return SD_OK;
}

// The fast family's layout plan of a template set: sd_params.reserved[1] (after apply_env_overrides) as the arguments of
// fast_plan_build.  allow_f16 = false: no fp16 cell format; allow_tr2 = false: no packed two-block traceback.
bool plan_fast_family(const sd_params& p, const std::vector<std::string>& tseq, sd::ScoreArgs sc, bool allow_f16, bool allow_tr2,
                      sd::FastPlan& plan, std::string& why) {
    return sd::fast_plan_build(tseq, sc, p.part_size + p.overlap, plan, why, allow_f16 && !(p.reserved[1] & SD_FLAG_NO_F16), allow_tr2,
                               p.ed_thr > -1 && !(p.reserved[1] & SD_FLAG_NO_EDTHR_COMPACT), !(p.reserved[1] & SD_FLAG_NO_U16));
}

// the "cells" code of a plan's layout and cell format (sd_plan_info [2], sd_engine_info [4] >> 8)
int layout_code(const sd::FastPlan& f) {
    return f.tiled ? (f.f16 ? 6 : 8) : f.waves > 1 ? (f.f16 ? 5 : 7) : f.wide ? (f.f16 ? 4 : 3) : f.u16 ? 9 : f.f16 ? 2 : 1;
}

void build_generic_tables(sd_engine* e) {
    const int Q = e->Q;
    const int64_t need = (e->sumL + Q - 1) / Q;
    int threads = (int)((need + 63) / 64 * 64);
    if (threads < 64) threads = 64;
    e->n_tiles = 1;
    if (threads > 1024) {  // more than 32 768 cells: tiles of 1024 threads x 32 cells, processed in order
        e->n_tiles = (int)((need + 1023) / 1024);
        threads = 1024;
    }
    e->threads = threads;
    const int64_t cells = (int64_t)e->n_tiles * threads * Q;
    e->rowBytes = (int)(cells / 4);
    std::vector<uint8_t> meta((size_t)cells, (uint8_t)(7 | sd::CELL_START));
    std::vector<int32_t> kd((size_t)cells, 0), tj((size_t)cells, 0);
    for (int j = 0; j < e->T; ++j) {
        for (int k = 0; k < e->tlen[j]; ++k) {
            const size_t x = (size_t)e->toff[j] + k;
            uint8_t m = (uint8_t)sd::base_code(e->tseq[j][k]);
            if (k == 0) m |= sd::CELL_START;
            if (k == e->tlen[j] - 1) {
                m |= sd::CELL_END;
                kd[x] = (e->tlen[j] - 1) * e->sc.del;
                tj[x] = j;
            }
            meta[x] = m;
        }
    }
    e->d_tmeta.upload(meta);
    e->d_tend_kd.upload(kd);
    e->d_tend_j.upload(tj);
}

}  // namespace

// Kernel family and layout plan of an engine (sd_params.kernel: 0 auto, 1 generic, 2 fast) and their tables on the
// device.  allow_f16 = false: no fp16 cell format (the fills' range guard tripped, or sd_params.reserved[1] bit 0).
static int engine_pick_family(sd_engine* e, bool allow_f16, std::string& err) {
    const sd_params* p = &e->p;
    int family = p->kernel;
    std::string why;
    // the packed two-block traceback unless switched off, and not after a range guard tripped (its own check raises the same flag)
    const bool tr2 = allow_f16 && !(p->reserved[1] & SD_FLAG_TRACE_V1);
    const bool fast_ok = plan_fast_family(*p, e->tseq, e->sc, allow_f16, tr2, e->fplan, why);
    e->fplan.full_floor = (p->reserved[1] & SD_FLAG_FULL_FLOOR) != 0;
    e->sc.rebase_mask = fast_ok ? e->fplan.rebase - 1 : 127;
    if (family == 0) family = fast_ok ? 2 : 1;
    if (family == 2 && !fast_ok) { err = "fast kernel family not applicable: " + why; return SD_ERR_UNSUPPORTED; }
    if (family != 1 && family != 2) { err = "bad kernel family"; return SD_ERR_PARAM; }
    if (p->ed_thr > -1 && e->Lmax > 2048) { err = "--ed_thr supports templates of up to 2048 bp"; return SD_ERR_UNSUPPORTED; }
    if (e->T > 65534) { err = "more than 65534 templates"; return SD_ERR_UNSUPPORTED; }
    e->family = family;
    e->d_toff.upload(e->toff);
    e->d_tlen.upload(e->tlen);
    if (family == 1) {
        e->Q = sd::generic_pick_q(e->sumL);
        build_generic_tables(e);
    } else {
        e->d_ftable.upload(e->fplan.table);
        e->d_flane.upload(e->fplan.lane_consts);
        e->d_fslot.upload(e->fplan.slot_of);
        e->d_ftcodes.upload(e->fplan.tcodes);
        if (e->fplan.tr2_ok) e->d_ftr2.upload(e->fplan.tr2_tab);
        if (p->ed_thr > -1) {
            e->d_endvl.upload(e->fplan.end_vlane);
            e->d_endoff.upload(e->fplan.end_off);
            e->d_vlane0.upload(e->fplan.vlane0);
        }
        // run-time guard of the fp16 cell formats (sd_fast_dev.hpp: F16Guard); reserved[2]: a smaller limit (tests)
        // (biased-u16 cells: the window the plan left around the bias, FastPlan::u16_lim)
        e->sc.guard_lim = p->reserved[2] > 0 ? p->reserved[2] : e->fplan.u16 ? e->fplan.u16_lim : 2040;
        // the same hook lowers the range check of the packed traceback's 16-bit words (its own run-time guard: a
        // checkpoint cell or start term beyond it raises the same flag, and the batch is repeated with sd_fast_trace)
        if (p->reserved[2] > 0 && e->fplan.tr2_ok) e->fplan.tr2_xlim = std::min(e->fplan.tr2_xlim, (int)p->reserved[2]);
        e->d_guard.alloc(1);
        SD_HIP(hipMemset(e->d_guard.p, 0, sizeof(int)));
        e->sc.guard_flag = e->d_guard.p;
    }
    return SD_OK;
}

// In-stream identities (sd_ident.hip).  il_seq = the monomers and their reverse complements interleaved (m0, m0', m1,
// ..., main.py:79-84), own[t] = interleaved index of the DP's template t; second_best = every template, plain and
// homopolymer-compressed, instead of the record's own.  Returns false (mode stays 0: the post-processing computes the
// identities from the read text as before) for template sets the kernel does not take.
bool engine_set_identity(sd_engine* e, const std::vector<std::string>& il_seq, const std::vector<int32_t>& own,
                         bool second_best) {
    e->ident_mode = 0;
    if (il_seq.empty() || (int)own.size() != e->T) return false;
    auto hpc = [](const std::string& x) {
        std::string o;
        for (size_t i = 0; i < x.size(); ++i)
            if (i == 0 || x[i] != x[i - 1]) o.push_back(x[i]);
        return o;
    };
    std::vector<std::string> hs;
    size_t tmax = 1, hmax = 1;
    for (const std::string& t : il_seq) {
        for (char c : t)
            if (!(c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N')) return false;
        if (t.empty()) return false;
        hs.push_back(hpc(t));
        tmax = std::max(tmax, t.size());
        hmax = std::max(hmax, hs.back().size());
    }
    if (tmax > 512) return false;
    auto words = [](size_t L) { int k = (int)((L + 63) / 64); return k == 5 ? 6 : k == 7 ? 8 : k; };
    if ((int64_t)e->p.part_size + e->p.overlap > 60000) return false;   // dist / matches travel as 16-bit fields
    try {
        SD_HIP(hipSetDevice(e->device));
        std::vector<unsigned long long> peq;
        std::vector<int32_t> tl;
        e->iT = (int)il_seq.size();
        e->iK = words(tmax);
        sd::nw_build_masks(il_seq, e->iK, peq, tl);
        e->d_ipeq.upload(peq);
        e->d_itlen.upload(tl);
        e->d_iown.upload(own);
        if (second_best) {
            e->iKh = words(hmax);
            sd::nw_build_masks(hs, e->iKh, peq, tl);
            e->d_ihpeq.upload(peq);
            e->d_ihtlen.upload(tl);
        }
        if (!e->ev_id0) SD_HIP(hipEventCreate(&e->ev_id0));
        if (!e->ev_id1) SD_HIP(hipEventCreate(&e->ev_id1));
    } catch (const HipFail&) {
        return false;
    }
    e->ident_mode = second_best ? 2 : 1;
    return true;
}

// The operands of one identity pass over the batch (homo: the homopolymer-compressed templates), with the buffers only
// that pass uses; maxlen = the longest chunk.  The checkpoint workspace the two passes share is set by alloc_identity.
static void set_ident_args(sd_engine* e, sd::IdentArgs& a, bool homo, int32_t maxlen) {
    const int per = e->ident_words();
    a = sd::IdentArgs{};
    a.chunks = e->dp_chunks; a.bases2 = e->dp_bases2; a.nmask = e->dp_nmask;
    a.dense = e->d_dense.p; a.rec_chunk = e->d_recchunk.p; a.total = e->d_roff.p + e->chunks.size();
    a.rec_cap = e->ident_cap;
    a.T = per; a.own = e->ident_mode == 1 ? e->d_iown.p : nullptr;
    a.peq = homo ? e->d_ihpeq.p : e->d_ipeq.p;
    a.tlen = homo ? e->d_ihtlen.p : e->d_itlen.p;
    a.Tmask = e->iT; a.K = homo ? e->iKh : e->iK; a.homo = homo ? 1 : 0;
    const int S = sd::nw_block_cols(a.K);
    a.short_max = std::min<int>(512, maxlen);
    a.cap_short = (a.short_max + S - 1) / S;
    a.grid_short = e->n_cu * 3;
    a.cap_long = (maxlen + S - 1) / S;
    // the long launch: as many lanes as 192 MB of checkpoints allow, at most one workgroup per CU
    const size_t per_block = (size_t)a.cap_long * 256 * ((size_t)a.K * 16 + 4);
    a.grid_long = (int)std::max<size_t>(1, std::min<size_t>((size_t)e->n_cu, ((size_t)192 << 20) / per_block));
    a.long_cnt = e->d_ilongcnt.p; a.long_list = e->d_ilong.p;
    a.out = homo ? e->d_identh.p : e->d_ident.p;
    // the homopolymer pass in its pruned form (distances, bounds, full alignments of the possible two best only)
    if (homo && per >= 3 && (int64_t)e->ident_cap * per < ((int64_t)1 << 32) && !(e->p.reserved[1] & SD_FLAG_NO_IDENT_PRUNE)) {
        e->d_icand.alloc((size_t)e->ident_cap * per);
        e->d_icandcnt.alloc(64);
        a.cand_list = e->d_icand.p;
        a.cand_cnt = e->d_icandcnt.p;
        a.grid_cand = e->n_cu * 3;
        e->d_ick2.alloc((size_t)a.grid_cand * 256 * (size_t)a.cap_short * (size_t)a.K);
        e->d_ickpos2.alloc((size_t)a.grid_cand * 256 * (size_t)a.cap_short);
        a.ck_cand = e->d_ick2.p;
        a.ckpos_cand = e->d_ickpos2.p;
    }
}

// identity workspace of the batch: outputs, long-pair list, checkpoints; fills ia_plain / ia_homo
static void alloc_identity(sd_engine* e) {
    // identity outputs for up to one record per 48 rows (a block is about a monomer long: ~170 rows); a batch
    // with more records falls back to the text-based identities of the post-processing
    int32_t maxlen = 1;
    for (const sd::ChunkDesc& cd : e->chunks) maxlen = std::max(maxlen, cd.n);
    e->ident_cap = std::min<int64_t>(e->dense_cap, std::max<int64_t>(4096, e->rows / 48));
    e->d_recchunk.alloc((size_t)e->dense_cap);
    e->d_ilong.alloc((size_t)e->ident_cap);
    e->d_ilongcnt.alloc(1);
    e->d_ident.alloc((size_t)e->ident_cap * e->ident_words());
    if (e->ident_mode == 2) e->d_identh.alloc((size_t)e->ident_cap * e->ident_words());
    set_ident_args(e, e->ia_plain, false, maxlen);
    size_t lanes = sd::ident_ck_lanes(e->ia_plain) * (size_t)e->ia_plain.K;
    size_t pos = sd::ident_ck_lanes(e->ia_plain);
    if (e->ident_mode == 2) {
        set_ident_args(e, e->ia_homo, true, maxlen);
        lanes = std::max(lanes, sd::ident_ck_lanes(e->ia_homo) * (size_t)e->ia_homo.K);
        pos = std::max(pos, sd::ident_ck_lanes(e->ia_homo));
    }
    e->d_ick.alloc(lanes);
    e->d_ickpos.alloc(pos);
    e->ia_plain.ck = e->d_ick.p; e->ia_plain.ckpos = e->d_ickpos.p;
    e->ia_homo.ck = e->d_ick.p; e->ia_homo.ckpos = e->d_ickpos.p;
}

// what the kernel family needs per batch: the generic pointer workspace in sub-batches, or the fast family's
// checkpoints (nck rows) and --ed_thr tables; the event pairs of the fills and tracebacks
static void alloc_family(sd_engine* e, int64_t nck) {
    const size_t C = e->chunks.size();
    e->subs.clear();
    if (e->family == 1) {
        // pointer workspace: sub-batches of consecutive chunks within the budget
        size_t free_b = 0, total_b = 0;
        SD_HIP(hipMemGetInfo(&free_b, &total_b));
        size_t budget = std::min<size_t>(free_b / 2 + e->d_ptr.bytes(), (size_t)48 << 30);
        size_t max_sub = 0, cur = 0;
        int begin = 0;
        for (size_t c = 0; c < C; ++c) {
            const size_t need = (size_t)e->chunks[c].n * (size_t)e->rowBytes;
            if (cur + need > budget && cur > 0) {
                e->subs.emplace_back(begin, (int)c);
                max_sub = std::max(max_sub, cur);
                begin = (int)c;
                cur = 0;
            }
            cur += need;
        }
        if (C > 0) { e->subs.emplace_back(begin, (int)C); max_sub = std::max(max_sub, cur); }
        e->d_ptr.alloc(max_sub);
        if (e->n_tiles > 1) {
            size_t most = 0;
            for (const auto& sb : e->subs) most = std::max(most, (size_t)(sb.second - sb.first));
            e->d_estate.alloc(most * (size_t)e->n_tiles * 1024 * 32);
        }
        if (e->p.ed_thr > -1) {
            e->d_dist.alloc(C * (size_t)e->T);
            e->d_grank.alloc(C * (size_t)e->T);
        }
    } else {
        if (e->p.ed_thr > -1) {
            e->d_dist.alloc(C * (size_t)e->T);
            e->d_cendoff.alloc(C * 64 * (size_t)e->fplan.waves);
            e->d_crank.alloc(C * 64 * (size_t)e->fplan.waves);
            // SD_FLAG_NO_EDTHR_COMPACT (SD_EDTHR_COMPACT=0 arrives as that flag through apply_env_overrides):
            // every chunk on the W-wave ranked kernel (A/B, tests)
            e->compact_edthr = e->fplan.wide && e->fplan.waves > 1 && e->fplan.f16 && !(e->p.reserved[1] & SD_FLAG_NO_EDTHR_COMPACT);
            if (e->compact_edthr && e->fplan.tiled) e->d_lanet.alloc(C * (size_t)e->fplan.waves * 128);
            if (e->compact_edthr) {
                e->d_klist.alloc(C * (size_t)e->T + 2);
                e->d_kpos.alloc(C * (size_t)e->T);
                e->d_nkept.alloc(C);
                e->d_orders.alloc((size_t)e->fplan.waves * C);
                e->d_cls.alloc(8);
            }
        }
        e->d_fckpt.alloc((size_t)nck * (size_t)e->fplan.P * 64 * (size_t)e->fplan.waves);
        e->d_fckbase.alloc((size_t)nck + 1);
    }
    const size_t pairs = e->family == 1 ? e->subs.size() : 1;   // (as sd_engine_timings reads them)
    ensure_events(e->ev_fill, 2 * pairs);
    ensure_events(e->ev_trace, 2 * pairs);
}

// Device buffers of the loaded batch (throws HipFail): what every batch needs, then the identity workspace and what depends
// on the kernel family and its layout plan.  Separate from the packing / upload of load_chunks_impl because a batch is
// re-run under another plan when the fp16 range guard of the fills trips (fetch_begin).
static void engine_alloc_batch(sd_engine* e, int64_t nck) {
    const size_t C = e->chunks.size();
    e->d_B.alloc((size_t)e->rows + C);
    e->d_argB.alloc((size_t)e->rows + C);
    e->d_cnt.alloc(C);
    e->d_roff.alloc(C + 1);
    e->h_roff.alloc(C + 1);
    e->d_recs.alloc((size_t)e->rows);
    e->dense_cap = std::max<int64_t>(4096, e->rows / 16);
    e->d_dense.alloc((size_t)e->dense_cap);
    e->dense_cap = (int64_t)e->d_dense.cap;
    if (e->ident_mode) alloc_identity(e);
    alloc_family(e, nck);
}

// Packs the given chunks (pointer + length each) into the pinned staging buffer, starts their copy to
// the device on `st` (asynchronous) and sizes the per-batch device buffers.  Chunk c refers to
// cptr[c][0 .. clen[c]).  The kernels of sd_engine_run must be enqueued on the same stream (or after
// a synchronisation with it).
// With a DevSrc the pointers are device addresses: the host builds the same table, order and sizes -- every chunk with
// the mask offset it would have if every chunk held an N -- uploads them with the addresses, and the packer
// (sd_pack_dev.hip) fills bases2 / nmask on `st` once the caller's stream has produced the text; no base is read here.
int load_chunks_impl(sd_engine* e, const std::vector<const char*>& cptr,
                     const std::vector<int32_t>& clen, hipStream_t st, char* errbuf, size_t errlen, const DevSrc* ds) {
    e->ran = false;
    e->fetched = false;
    e->rows_done = false;
    e->dev_src = ds != nullptr;
    e->dev_cum = ds ? ds->cum : nullptr;
    e->chunks.clear();
    const size_t C = cptr.size();
    e->chunks.resize(C);
    uint64_t row0 = 0;
    size_t words_total = 0;
    for (size_t c = 0; c < C; ++c) {
        sd::ChunkDesc& cd = e->chunks[c];
        cd = sd::ChunkDesc{};
        cd.woff = (uint32_t)words_total;
        cd.n = clen[c];
        cd.noff = -1;
        cd.row0 = row0;
        row0 += (uint64_t)clen[c];
        words_total += ((size_t)clen[c] + 15) / 16;
    }
    if (words_total >= (1ull << 31)) {
        set_err(errbuf, errlen, "batch too large: split the reads into smaller groups");
        return SD_ERR_UNSUPPORTED;
    }
    e->rows = (int64_t)row0;
    try {
        SD_HIP(hipSetDevice(e->device));
        if (e->in_pending) {  // the previous batch's copy still reads the staging buffer
            SD_HIP(hipEventSynchronize(e->ev_in));
            e->in_pending = false;
        }
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_chunks = 0;
        const size_t o_order = al(o_chunks + C * sizeof(sd::ChunkDesc));
        // device source: [chunk addresses][chunk positions][alphabet flag] between the order and the bases
        const size_t o_src = al(o_order + C * sizeof(int));
        const size_t o_gpos = o_src + (ds ? C * sizeof(uint64_t) : 0);
        const size_t o_bad = o_gpos + (ds ? C * sizeof(int64_t) : 0);
        const size_t o_bases = ds ? al(o_bad + sizeof(uint64_t)) : o_src;
        const size_t o_nmask = al(o_bases + words_total * sizeof(uint32_t));
        // worst-case N mask (every chunk has N): one bit per base
        size_t nwords_max = 0;
        for (size_t c = 0; c < C; ++c) nwords_max += ((size_t)clen[c] + 31) / 32;
        e->h_in.alloc(ds ? o_bases : o_nmask + nwords_max * sizeof(uint32_t) + 256);
        uint32_t* bases2 = reinterpret_cast<uint32_t*>(e->h_in.p + o_bases);
        uint32_t* nmask = reinterpret_cast<uint32_t*>(e->h_in.p + o_nmask);
        size_t nwords = 0;
        if (ds) {
            uint64_t* src = reinterpret_cast<uint64_t*>(e->h_in.p + o_src);
            int64_t* gpos = reinterpret_cast<int64_t*>(e->h_in.p + o_gpos);
            for (size_t c = 0; c < C; ++c) {
                e->chunks[c].noff = (int32_t)nwords;
                nwords += ((size_t)clen[c] + 31) / 32;
                src[c] = (uint64_t)reinterpret_cast<uintptr_t>(cptr[c]);
                gpos[c] = ds->gpos[c];
            }
            *reinterpret_cast<uint64_t*>(e->h_in.p + o_bad) = ~0ull;
        } else {
            std::vector<uint8_t> hasn(C, 0);
            sd::parallel_for((int64_t)C, e->p.threads, 16, [&](int64_t c) {
                const sd::ChunkDesc& cd = e->chunks[(size_t)c];
                hasn[(size_t)c] = sd::pack_chunk(cptr[(size_t)c], cd.n, bases2 + cd.woff) ? 1 : 0;
            });
            for (size_t c = 0; c < C; ++c)
                if (hasn[c]) {
                    e->chunks[c].noff = (int32_t)nwords;
                    nwords += ((size_t)e->chunks[c].n + 31) / 32;
                }
            if (nwords) {
                std::memset(nmask, 0, nwords * sizeof(uint32_t));
                sd::parallel_for((int64_t)C, e->p.threads, 16, [&](int64_t c) {
                    const sd::ChunkDesc& cd = e->chunks[(size_t)c];
                    if (cd.noff < 0) return;
                    const char* s = cptr[(size_t)c];
                    for (int32_t i = 0; i < cd.n; ++i)
                        if (s[i] == 'N') nmask[(size_t)cd.noff + (size_t)(i >> 5)] |= 1u << (i & 31);
                });
            }
        }
        const int64_t nck = e->family == 2 ? sd::fast_ckpt_rows_total(e->fplan, e->chunks) : 0;
        if (C) std::memcpy(e->h_in.p + o_chunks, e->chunks.data(), C * sizeof(sd::ChunkDesc));
        {
            // longest chunks first; almost every chunk has the full length, so a counting pass over the
            // two or three distinct lengths would do as well -- the sort is O(C log C) on ints
            int* order = reinterpret_cast<int*>(e->h_in.p + o_order);
            for (size_t c = 0; c < C; ++c) order[c] = (int)c;
            std::stable_sort(order, order + C, [&](int a, int b) { return e->chunks[(size_t)a].n > e->chunks[(size_t)b].n; });
        }
        const size_t in_bytes = ds ? o_bad + sizeof(uint64_t) : o_nmask + nwords * sizeof(uint32_t);
        e->d_in.alloc(o_nmask + nwords_max * sizeof(uint32_t) + 256);
        e->dp_chunks = reinterpret_cast<sd::ChunkDesc*>(e->d_in.p + o_chunks);
        e->dp_order = reinterpret_cast<int*>(e->d_in.p + o_order);
        e->dp_bases2 = reinterpret_cast<uint32_t*>(e->d_in.p + o_bases);
        e->dp_nmask = reinterpret_cast<uint32_t*>(e->d_in.p + o_nmask);
        e->dp_bad = ds ? reinterpret_cast<unsigned long long*>(e->d_in.p + o_bad) : nullptr;
        SD_HIP(hipMemcpyAsync(e->d_in.p, e->h_in.p, in_bytes, hipMemcpyHostToDevice, st));
        if (ds) {
            if (ds->ready) SD_HIP(hipStreamWaitEvent(st, ds->ready, 0));
            sd::PackDevArgs pa{};
            pa.chunks = e->dp_chunks; pa.n_chunks = (int)C; pa.bases2 = e->dp_bases2; pa.nmask = e->dp_nmask;
            pa.src = reinterpret_cast<const unsigned long long*>(e->d_in.p + o_src);
            pa.gpos = reinterpret_cast<const long long*>(e->d_in.p + o_gpos);
            pa.bad = e->dp_bad;
            sd::launch_pack_dev(st, pa);
            SD_HIP(hipGetLastError());
            e->h_bad.alloc(1);
            e->h_bad.p[0] = ~0ull;
        }
        SD_HIP(hipEventRecord(e->ev_in, st));
        // whatever the caller enqueues on its stream from here on follows the packer: it may overwrite or free the text
        if (ds && ds->release) SD_HIP(hipStreamWaitEvent(ds->user, e->ev_in, 0));
        e->in_pending = true;
        engine_alloc_batch(e, nck);
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

// ---- what one run enqueues, stage by stage (each throws HipFail; engine_run2 calls them in order) -------------------

// --ed_thr with more than 128 templates: the fast family fills and traces the batch in its compacted classes
static bool compacted(const sd_engine* e) { return e->p.ed_thr > -1 && e->compact_edthr; }

// the operands of the --ed_thr prefilter (main.cpp:91-93: per-chunk template prefilter) with the outputs of the engine's family
static sd::FilterArgs filter_args(const sd_engine* e) {
    sd::FilterArgs a{};
    a.chunks = e->dp_chunks; a.n_chunks = (int)e->chunks.size(); a.T = e->T; a.Lmax = e->Lmax; a.ed_thr = e->p.ed_thr;
    a.bases2 = e->dp_bases2; a.nmask = e->dp_nmask; a.peq = e->d_peq.p; a.tlen = e->d_tlen.p; a.dist = e->d_dist.p;
    a.uniform_half = e->filter_uniform;
    if (e->family == 1) { a.grank = e->d_grank.p; return a; }
    a.end_vlane = e->d_endvl.p; a.end_off = e->d_endoff.p; a.vlane0 = e->d_vlane0.p;
    a.cendoff = e->d_cendoff.p; a.crank = e->d_crank.p; a.waves = e->fplan.waves;
    if (compacted(e)) { a.kpos = e->d_kpos.p; a.klist = e->d_klist.p; a.nkept = e->d_nkept.p; }
    return a;
}

// Generic family: the prefilter with its rank table, then fill + traceback per sub-batch of the pointer workspace
static void enqueue_generic(sd_engine* e, hipStream_t st) {
    const bool ranked = e->p.ed_thr > -1;
    if (ranked) sd::launch_edthr_filter(st, filter_args(e));
    for (size_t s = 0; s < e->subs.size(); ++s) {
        const int b = e->subs[s].first, n_sub = e->subs[s].second - b;
        const uint64_t row0_base = e->chunks[(size_t)b].row0;
        SD_HIP(hipEventRecord(e->ev_fill[2 * s], st));
        sd::launch_generic_fill(e->Q, e->threads, n_sub, st, e->dp_chunks, b,
                                e->dp_bases2, e->dp_nmask, e->d_tmeta.p,
                                e->d_tend_kd.p, e->d_tend_j.p, e->sc, e->rowBytes,
                                e->d_ptr.p, row0_base, e->d_B.p, e->d_argB.p,
                                ranked ? e->d_grank.p : nullptr, e->T, e->n_tiles, e->d_estate.p);
        SD_HIP(hipEventRecord(e->ev_fill[2 * s + 1], st));
        SD_HIP(hipEventRecord(e->ev_trace[2 * s], st));
        sd::launch_generic_trace(n_sub, st, e->dp_chunks, b, e->d_ptr.p, row0_base,
                                 e->rowBytes, e->d_B.p, e->d_argB.p, e->d_toff.p,
                                 e->d_tlen.p, e->d_recs.p, e->d_cnt.p);
        SD_HIP(hipEventRecord(e->ev_trace[2 * s + 1], st));
        ++e->fill_launches;
    }
}

// the operands of the batch's fill / traceback; queue = the zeroed head the launch draws its chunks from
static sd::FillArgs fill_args(const sd_engine* e, int* queue) {
    sd::FillArgs fa{};
    fa.chunks = e->dp_chunks; fa.n_chunks = (int)e->chunks.size(); fa.bases2 = e->dp_bases2; fa.nmask = e->dp_nmask;
    fa.table = e->d_ftable.p; fa.lane_consts = e->d_flane.p; fa.sc = e->sc;
    fa.B = e->d_B.p; fa.argV = e->d_argB.p; fa.ckpt = e->d_fckpt.p; fa.ckbase = e->d_fckbase.p;
    fa.queue = queue; fa.order = e->dp_order; fa.n_cu = e->n_cu;
    if (e->p.ed_thr > -1) { fa.cendoff = e->d_cendoff.p; fa.crank = e->d_crank.p; }
    if (compacted(e)) { fa.klist = e->d_klist.p; fa.lane_t = e->fplan.tiled ? e->d_lanet.p : nullptr; }
    fa.tcodes = e->d_ftcodes.p; fa.toff = e->d_toff.p; fa.tlen = e->d_tlen.p;
    return fa;
}

static sd::TraceArgs trace_args(const sd_engine* e, int* queue) {
    sd::TraceArgs ta{};
    ta.chunks = e->dp_chunks; ta.n_chunks = (int)e->chunks.size(); ta.bases2 = e->dp_bases2; ta.nmask = e->dp_nmask;
    ta.slot_of = e->d_fslot.p; ta.tcodes = e->d_ftcodes.p; ta.lane_consts = e->d_flane.p;
    ta.toff = e->d_toff.p; ta.tlen = e->d_tlen.p; ta.sc = e->sc;
    ta.B = e->d_B.p; ta.argV = e->d_argB.p; ta.ckpt = e->d_fckpt.p; ta.ckbase = e->d_fckbase.p;
    ta.recs = e->d_recs.p; ta.rec_cnt = e->d_cnt.p; ta.queue = queue; ta.order = e->dp_order; ta.n_cu = e->n_cu;
    ta.tr2_tab = e->fplan.tr2_ok ? e->d_ftr2.p : nullptr;
    if (compacted(e)) { ta.klist = e->d_klist.p; ta.kpos = e->d_kpos.p; ta.nkept = e->d_nkept.p; ta.lane_t = e->fplan.tiled ? e->d_lanet.p : nullptr; }
    return ta;
}

// More than 128 templates: a chunk is filled by as many waves as its kept templates need, holding exactly those (the
// point of the reference's prefilter, main.cpp:128-149: less DP work); chunks that need all W waves by the W-wave
// ranked kernel.  The class sizes stay on the device.  fa = the batch's operands, fa.queue the run's first head.
static void enqueue_class_fills(sd_engine* e, hipStream_t st, const sd::FillArgs& fa) {
    const int C = (int)e->chunks.size(), W = e->fplan.waves;
    int* ord = e->d_orders.p;   // [W][C]: class w-1 = the chunks whose kept templates need w waves
    // tiled layout: the kept templates' lanes per chunk (d_kpos becomes "first lane", d_nkept "lanes used")
    if (e->fplan.tiled)
        sd::launch_tiled_place(st, C, e->T, e->fplan.P, W, e->d_klist.p, e->d_nkept.p, e->d_tlen.p,
                               e->d_kpos.p, e->d_lanet.p, e->fplan.filter_only ? e->d_guard.p : nullptr);
    sd::launch_split_order(st, e->dp_order, C, e->d_nkept.p, ord, e->d_cls.p, W);
    for (int w = 1; w <= W; ++w) {
        sd::FillArgs cw = fa;   // class w; queue heads: class 1 the run's fill head, class W the third
        cw.queue = w == 1 ? fa.queue : w == W ? fa.queue + 2 : fa.queue + 1 + w;
        cw.order = ord + (size_t)(w - 1) * C;
        cw.n_ptr = e->d_cls.p + (w - 1);
        // (FastPlan::filter_only: no layout of the whole set, the chunks that need all W waves are compacted too)
        if (w < W || e->fplan.filter_only) sd::launch_fast_fill_compact(e->fplan, st, cw, w);
        else sd::launch_fast_fill(e->fplan, st, cw);
    }
}

// Fast family: the prefilter, the fill -- plain or in the classes of --ed_thr -- on st, the traceback behind it on ts
static void enqueue_fast(sd_engine* e, hipStream_t st, hipStream_t ts) {
    if (e->q_run == sd_engine::QN) {  // every queue head used once: zero them again (no kernel of this
        SD_HIP(hipMemsetAsync(e->d_queue.p, 0, sizeof(int) * sd_engine::QS * (size_t)sd_engine::QN, st));  // engine is running)
        e->q_run = 0;
    }
    int* heads = e->d_queue.p + sd_engine::QS * e->q_run++;   // heads of this run: fill, traceback, fill classes 2..8
    if (e->p.ed_thr > -1) sd::launch_edthr_filter(st, filter_args(e));
    SD_HIP(hipEventRecord(e->ev_fill[0], st));
    if (compacted(e)) enqueue_class_fills(e, st, fill_args(e, heads));
    else sd::launch_fast_fill(e->fplan, st, fill_args(e, heads), e->lds_gate ? 54 * 1024 : 0);
    SD_HIP(hipEventRecord(e->ev_fill[1], st));
    if (ts != st) SD_HIP(hipStreamWaitEvent(ts, e->ev_fill[1], 0));
    SD_HIP(hipEventRecord(e->ev_trace[0], ts));
    sd::launch_fast_trace(e->fplan, ts, trace_args(e, heads + 1));
    SD_HIP(hipEventRecord(e->ev_trace[1], ts));
    e->fill_launches = 1;
}

// record offsets + compaction of the batch's records in one launch (sd_scan_compact); its workspace on first use
static void enqueue_compact(sd_engine* e, hipStream_t ts) {
    SD_HIP(hipEventRecord(e->ev_cmp0, ts));
    if (!e->d_scanws.p) {
        e->d_scanws.alloc(520);
        SD_HIP(hipMemsetAsync(e->d_scanws.p, 0, 520 * sizeof(long long), ts));
        e->scan_tickets = 0;
    }
    sd::launch_compact(ts, e->dp_chunks, (int)e->chunks.size(), e->d_cnt.p, e->d_roff.p, e->d_recs.p,
                       e->d_dense.p, e->dense_cap, true, e->ident_mode ? e->d_recchunk.p : nullptr,
                       e->d_scanws.p, ++e->scan_epoch, &e->scan_tickets);
    SD_HIP(hipEventRecord(e->ev_cmp1, ts));
}

// the record offsets travel right behind the compaction: the fetch then knows the record
// count as soon as the stream is idle, without a second round trip
static void copy_offsets(sd_engine* e, hipStream_t ts) {
    SD_HIP(hipMemcpyAsync(e->h_roff.p, e->d_roff.p, sizeof(int64_t) * (e->chunks.size() + 1), hipMemcpyDeviceToHost, ts));
    if (e->dev_src)         // the device packer's alphabet flag
        SD_HIP(hipMemcpyAsync(e->h_bad.p, e->dp_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, ts));
    if (e->family == 2) {   // and the fp16 range guard of the fills (reset for the next run behind the copy)
        e->h_guard.alloc(1);
        SD_HIP(hipMemcpyAsync(e->h_guard.p, e->d_guard.p, sizeof(int), hipMemcpyDeviceToHost, ts));
        SD_HIP(hipMemsetAsync(e->d_guard.p, 0, sizeof(int), ts));
    }
}

// identities of the whole batch in one pass per form
static void enqueue_ident_batch(sd_engine* e, hipStream_t ts) {
    e->ia_plain.rec_lo = e->ia_homo.rec_lo = e->ia_plain.rec_hi = e->ia_homo.rec_hi = nullptr;
    sd::launch_ident(ts, e->ia_plain);
    if (e->ident_mode == 2) {
        e->ia_homo.cand_cnt = e->ia_homo.cand_list ? e->d_icandcnt.p : nullptr;
        sd::launch_ident_pruned(ts, e->ia_homo);
    }
}

// ... and slice by slice (sd_engine::slice_end), an event behind each slice
static void enqueue_ident_slices(sd_engine* e, hipStream_t ts) {
    ensure_events(e->ev_slice, e->slice_end.size(), hipEventBlockingSync | hipEventDisableTiming);
    // the candidate stage of slice s on its own stream, beside the kernels of slice s + 1 (per-slice counter,
    // per-slice region of the list, its own checkpoint workspace)
    const bool side = e->ident_mode == 2 && e->ia_homo.cand_list && e->slice_end.size() <= 64 && !getenv("SD_IDENT_CAND_INLINE");
    if (side) {
        if (!e->cand_st) SD_HIP(hipStreamCreateWithFlags(&e->cand_st, hipStreamNonBlocking));
        ensure_events(e->ev_cand, e->slice_end.size(), hipEventDisableTiming);
        SD_HIP(hipMemsetAsync(e->d_icandcnt.p, 0, 64 * sizeof(int), ts));
    }
    int c_lo = 0;
    bool on_side = false;
    for (size_t sl = 0; sl < e->slice_end.size(); ++sl) {
        const int c_hi = e->slice_end[sl];
        e->ia_plain.rec_lo = e->ia_homo.rec_lo = e->d_roff.p + c_lo;
        e->ia_plain.rec_hi = e->ia_homo.rec_hi = e->d_roff.p + c_hi;
        sd::launch_ident(ts, e->ia_plain);
        bool rec_on_side = false;
        if (e->ident_mode == 2) {
            e->ia_homo.cand_cnt = e->ia_homo.cand_list ? e->d_icandcnt.p + (side ? sl : 0) : nullptr;
            if (side) {
                if (sd::launch_ident_pruned_front(ts, e->ia_homo)) {
                    SD_HIP(hipEventRecord(e->ev_cand[sl], ts));
                    SD_HIP(hipStreamWaitEvent(e->cand_st, e->ev_cand[sl], 0));
                    sd::launch_ident_pruned_back(e->cand_st, e->ia_homo);
                    rec_on_side = on_side = true;
                }
            } else {
                sd::launch_ident_pruned(ts, e->ia_homo);
            }
        }
        SD_HIP(hipEventRecord(e->ev_slice[sl], rec_on_side ? e->cand_st : ts));
        c_lo = c_hi;
    }
    if (on_side) SD_HIP(hipStreamWaitEvent(ts, e->ev_slice.back(), 0));   // what follows on ts follows the last candidates
}

// identities of the final TSV on the batch's compact records (sd_ident.hip)
static void enqueue_identities(sd_engine* e, hipStream_t ts) {
    SD_HIP(hipEventRecord(e->ev_id0, ts));
    e->ia_plain.dense = e->ia_homo.dense = e->d_dense.p;            // (a fetch may have grown them)
    e->ia_plain.rec_chunk = e->ia_homo.rec_chunk = e->d_recchunk.p;
    e->ia_plain.dense_cap = e->ia_homo.dense_cap = e->dense_cap;
    if (e->sliced_run) enqueue_ident_slices(e, ts);
    else enqueue_ident_batch(e, ts);
    SD_HIP(hipEventRecord(e->ev_id1, ts));
}

// One pass over the loaded batch.  `st` carries the fill (and, for the generic family, everything);
// with a distinct `ts` the traceback + compaction of the fast family go there behind an event, so that
// a pipeline can put the next batch's fill on `st` right behind this one: the traceback of batch b
// then shares the machine with the fill of batch b+1 and runs in the slots its drain leaves free.
int engine_run2(sd_engine* e, hipStream_t st, hipStream_t ts, char* errbuf, size_t errlen) {
    const int C = (int)e->chunks.size();
    if (e->family == 1) ts = st;
    try {
        SD_HIP(hipSetDevice(e->device));
        if (e->in_pending) SD_HIP(hipStreamWaitEvent(st, e->ev_in, 0));
        SD_HIP(hipEventRecord(e->ev_run0, st));
        e->fill_launches = 0;
        if (C > 0) {
            if (e->family == 1) enqueue_generic(e, st);
            else enqueue_fast(e, st, ts);
            enqueue_compact(e, ts);
            e->sliced_run = e->ident_mode != 0 && !e->slice_end.empty() && e->slice_end.back() == C;
            if (e->sliced_run) {
                copy_offsets(e, ts);
                if (!e->ev_dp) SD_HIP(hipEventCreateWithFlags(&e->ev_dp, hipEventBlockingSync));
                SD_HIP(hipEventRecord(e->ev_dp, ts));
            }
            if (e->ident_mode) enqueue_identities(e, ts);
            if (!e->sliced_run) copy_offsets(e, ts);
        }
        SD_HIP(hipEventRecord(e->ev_run1, ts));
        SD_HIP(hipGetLastError());
    } catch (const HipFail& f) {
        // sd_scan_compact takes its range from (device ticket counter - the host's count of tickets handed out): a launch
        // that was rejected, or a kernel that died before every workgroup drew its ticket, leaves the two apart for the
        // life of the workspace -- later launches would then wait on counts nobody publishes.  After any error the
        // workspace is dropped: the next run allocates and zeroes a new one and counts from zero.
        e->d_scanws.free_();
        e->scan_tickets = 0;
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    e->run_st = st;
    e->run_ts = ts;
    e->ran = true;
    e->fetched = false;
    e->rows_done = false;
    return SD_OK;
}

// The alphabet flag of a device-packed batch as a message: read index within the job, 0-based position, the byte.
static std::string dev_symbol_message(unsigned long long key, const std::vector<int64_t>* cum) {
    const int64_t pos = (int64_t)(key >> 8);
    const unsigned byte = (unsigned)(key & 0xff);
    int64_t r = 0, at = pos;
    if (cum && cum->size() > 1) {
        r = (int64_t)(std::upper_bound(cum->begin(), cum->end(), pos) - cum->begin()) - 1;
        r = std::min<int64_t>(std::max<int64_t>(r, 0), (int64_t)cum->size() - 2);
        at = pos - (*cum)[(size_t)r];
    }
    char txt[160];
    std::snprintf(txt, sizeof txt, "ERROR: Sequence #%lld contains undefined symbol (not ACGT) at position %lld: byte %u (0x%02x)",
                  (long long)r, (long long)at, byte, byte);
    return txt;
}

static std::atomic<long long> g_guard_trips{0};   // batches repeated after a tripped range guard (sd_guard_trips)

// First half of a fetch: wait until the DP of the last run is done and its record offsets are on the host (a sliced run:
// ev_dp, the identity slices may still be running; else the whole run), repeat the batch if a guard tripped, size the
// host buffer of the records.
int fetch_begin(sd_engine* e, int64_t& total, char* errbuf, size_t errlen) {
    total = 0;
    if (!e->ran) { set_err(errbuf, errlen, "sd_engine_fetch before sd_engine_run"); return SD_ERR_PARAM; }
    const size_t C = e->chunks.size();
    try {
        SD_HIP(hipSetDevice(e->device));
        SD_HIP(hipEventSynchronize(e->sliced_run ? e->ev_dp : e->ev_run1));
        e->in_pending = false;
        if (C == 0) { e->h_roff.alloc(1); e->h_roff.p[0] = 0; return SD_OK; }
        if (e->dev_src && e->h_bad.p[0] != ~0ull) {   // (nothing of the run is used; it ran on masked codes)
            set_err(errbuf, errlen, dev_symbol_message(e->h_bad.p[0], e->dev_cum.get()));
            return SD_ERR_SYMBOL;
        }
        // (a batch packed on the device: which chunks run maskless is in the device's table only)
        const bool dev_table = e->dev_src;
        if (e->family == 2 && e->h_guard.p && e->h_guard.p[0] != 0) {
            // A wave's fp16 cells left the range in which they are exact integers (F16Guard, sd_fast_dev.hpp): the
            // layout plan's bound did not hold for this input.  Nothing of the run is used; the batch (still packed on
            // the device) is repeated with integer cells, which this engine keeps from now on.
            ++g_guard_trips;
            e->replanned = true;
            if (e->sliced_run) SD_HIP(hipEventSynchronize(e->ev_run1));   // (the identity slices of the dropped run)
            std::string err2;
            int rc2 = engine_pick_family(e, false, err2);
            if (rc2) { set_err(errbuf, errlen, "fp16 cell range exceeded, and no integer-cell layout: " + err2); return rc2; }
            const int64_t nck = e->family == 2 ? sd::fast_ckpt_rows_total(e->fplan, e->chunks) : 0;
            if (dev_table) SD_HIP(hipMemcpy(e->chunks.data(), e->dp_chunks, C * sizeof(sd::ChunkDesc), hipMemcpyDeviceToHost));
            SD_HIP(hipMemcpy(e->dp_chunks, e->chunks.data(), C * sizeof(sd::ChunkDesc), hipMemcpyHostToDevice));
            engine_alloc_batch(e, nck);
            rc2 = engine_run2(e, e->run_st, e->run_ts, errbuf, errlen);
            if (rc2) return rc2;
            SD_HIP(hipEventSynchronize(e->ev_run1));
            if (e->family == 2 && e->h_guard.p[0] != 0) {
                set_err(errbuf, errlen, "cell range exceeded in the integer-cell fill");
                return SD_ERR_INTERNAL;
            }
        }
        total = e->h_roff.p[C];
        e->ident_valid = e->ident_mode != 0 && total <= e->ident_cap && total <= e->dense_cap;
        if (total > e->dense_cap) {
            if (e->sliced_run) SD_HIP(hipEventSynchronize(e->ev_run1));
            e->d_dense.alloc((size_t)total);
            e->dense_cap = (int64_t)e->d_dense.cap;
            if (e->ident_mode) e->d_recchunk.alloc((size_t)e->dense_cap);   // a later run of the same load compacts into it
            sd::launch_compact(e->run_ts, e->dp_chunks, (int)C, e->d_cnt.p, e->d_roff.p,
                               e->d_recs.p, e->d_dense.p, e->dense_cap, false);
            SD_HIP(hipStreamSynchronize(e->run_ts));
        }
        e->h_recs.alloc((size_t)std::max<int64_t>(total, 1));
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

// Second half: the records [r_lo, r_hi) into h_recs (at their own indices) and, if the run has them and the caller gives
// room (pinned, word 0 = record r_lo), their identity words.
int fetch_range(sd_engine* e, int64_t r_lo, int64_t r_hi, uint32_t* id_dst, uint32_t* idh_dst, char* errbuf, size_t errlen) {
    static_assert(sizeof(sd_rec) == sizeof(sd::DevRec), "record layout");
    const int64_t n = r_hi - r_lo;
    if (n <= 0) return SD_OK;
    try {
        hipStream_t cs = e->copy_stream ? e->copy_stream : e->run_ts;
        SD_HIP(hipMemcpyAsync(e->h_recs.p + r_lo, e->d_dense.p + r_lo, sizeof(sd_rec) * (size_t)n, hipMemcpyDeviceToHost, cs));
        if (e->ident_valid && id_dst) {
            const size_t per = (size_t)e->ident_words();
            const size_t nb = sizeof(uint32_t) * (size_t)n * per;
            SD_HIP(hipMemcpyAsync(id_dst, e->d_ident.p + (size_t)r_lo * per, nb, hipMemcpyDeviceToHost, cs));
            if (e->ident_mode == 2 && idh_dst)
                SD_HIP(hipMemcpyAsync(idh_dst, e->d_identh.p + (size_t)r_lo * per, nb, hipMemcpyDeviceToHost, cs));
        }
        SD_HIP(hipStreamSynchronize(cs));
        if (e->score_scale != 1)
            for (int64_t x = r_lo; x < r_hi; ++x) e->h_recs.p[x].score *= e->score_scale;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

// the engine's own identity blocks, large enough for `total` records (throws HipFail)
static void engine_grow_ident(sd_engine* e, int64_t total) {
    if (!e->ident_valid || total <= 0) return;
    const size_t nb = sizeof(uint32_t) * (size_t)total * (size_t)e->ident_words();
    auto grow = [&](uint32_t** p, size_t* have) {
        if (*have >= nb) return;
        g_pinpool.give(*p, *have);
        *p = nullptr;
        *have = 0;   // take() may throw: no stale size beside a null pointer
        *p = static_cast<uint32_t*>(g_pinpool.take(nb, *have));
    };
    grow(&e->h_ident, &e->h_ident_bytes);
    if (e->ident_mode == 2) grow(&e->h_identh, &e->h_identh_bytes);
}

// The whole batch in one piece, after fetch_begin: waits for the end of the run where the identities ran in slices, then
// brings the compact records (and identities) into the pinned buffers h_recs / h_ident (valid until the next load / run
// of this engine).
int fetch_whole(sd_engine* e, int64_t total, char* errbuf, size_t errlen) {
    if (e->sliced_run && hipEventSynchronize(e->ev_run1) != hipSuccess) { set_err(errbuf, errlen, "device run failed"); return SD_ERR_HIP; }
    try {
        engine_grow_ident(e, total);
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return fetch_range(e, 0, total, e->h_ident, e->h_identh, errbuf, errlen);
}


// Pipelines of finished jobs (sd_run_files*, the raw calls; taken and given back by JobPipes only), kept for the next job with the same parameters and monomer set: creating
// the engines (layout plan, tables, identity masks, streams, events, pinned staging) is 25-40 ms per call, a quarter of
// a C4 --second-best job.  A process that decomposes many read sets against one monomer set (a service behind the
// C-ABI, bench.py's steps) pays it once; sd_release_cache() drops them.  At most two are kept per device entry (the
// pipelines of an sd_run_files_devices job are keyed by ordinal and entry), none that holds more
// than SD_PIPE_CACHE_GB (default 96) GB of device memory, and none whose engines left the layout they were created
// with (a tripped fp16 guard, an overflowing filter-only batch: the next job should start from the plan again).
// The entries are never destroyed at process exit (as g_pool / g_pinpool: the HIP runtime may be gone by then);
// sd_release_cache() is the only place that tears them down.
namespace {
struct PipeCacheEntry { std::string key; std::unique_ptr<Pipeline> pipe; int entry; };
struct PipeCache { std::mutex m; std::vector<PipeCacheEntry> v; };
PipeCache& pipe_cache() { static PipeCache* c = new PipeCache; return *c; }   // leaked on purpose
}  // namespace
// the cache key, field by field (the raw bytes of an sd_params would carry its padding and the host-thread count)
std::string pipe_cache_key(const sd_params& pe, char kind, const std::vector<const char*>& mseq, const std::vector<int32_t>& mlen) {
    std::string k;
    for (int32_t v : {pe.ins, pe.del, pe.mismatch, pe.match, pe.part_size, pe.overlap, pe.ed_thr, pe.device, pe.kernel,
                      pe.max_batch_rows, pe.reserved[0], pe.reserved[1], pe.reserved[2], pe.reserved[3], pe.reserved[4]}) {
        k += std::to_string(v);
        k.push_back(',');
    }
    k.push_back(kind);
    for (size_t m = 0; m < mseq.size(); ++m) { k.append(mseq[m], (size_t)mlen[m]); k.push_back('\n'); }
    return k;
}
std::unique_ptr<Pipeline> pipe_cache_take(const std::string& key) {
    PipeCache& c = pipe_cache();
    std::lock_guard<std::mutex> g(c.m);
    for (size_t i = 0; i < c.v.size(); ++i)
        if (c.v[i].key == key) {
            std::unique_ptr<Pipeline> q = std::move(c.v[i].pipe);
            c.v.erase(c.v.begin() + (long)i);
            return q;
        }
    return nullptr;
}
void pipe_cache_give(const std::string& key, std::unique_ptr<Pipeline> q, int entry) {
    static const size_t cap = [] { const char* e = getenv("SD_PIPE_CACHE_GB"); return (size_t)(e ? std::max(0, atoi(e)) : 96) << 30; }();
    if (!q || q->degraded() || q->held_bytes() > cap) return;   // (destroyed here, outside the lock)
    std::vector<PipeCacheEntry> drop;   // destroyed outside the lock
    {
        PipeCache& c = pipe_cache();
        std::lock_guard<std::mutex> g(c.m);
        c.v.push_back(PipeCacheEntry{key, std::move(q), entry});
        // at most two per device entry (sd_run_files_devices keeps one pipeline per entry of its device list)
        size_t same = 0;
        for (const PipeCacheEntry& x : c.v) same += x.entry == entry;
        for (size_t i = 0; same > 2 && i < c.v.size();)
            if (c.v[i].entry == entry) { drop.push_back(std::move(c.v[i])); c.v.erase(c.v.begin() + (long)i); --same; }
            else ++i;
    }
}
void pipe_cache_clear() {
    std::vector<PipeCacheEntry> drop;
    {
        PipeCache& c = pipe_cache();
        std::lock_guard<std::mutex> g(c.m);
        drop.swap(c.v);
    }
}

namespace {
// Records of a chunk range as the C-ABI hands them out (malloc'ed records + offsets), filled batch by batch straight
// from the pipeline's pinned buffers: one copy per record (a std::vector + a final copy cost 6 ms per 200-Mb job).
struct RangeCollector {
    sd_rec* recs = nullptr;
    int64_t* off = nullptr;
    size_t cap = 0, n = 0, c_lo, n_chunks;
    bool failed = false;
    RangeCollector(size_t chunks, size_t first) : c_lo(first), n_chunks(chunks) {
        off = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * (chunks + 1)));
        cap = std::max<size_t>(4096, chunks * 40);   // ~32 records per 5.5-kb chunk of satellite DNA
        recs = static_cast<sd_rec*>(std::malloc(sizeof(sd_rec) * cap));
        if (!off || !recs) failed = true; else off[0] = 0;
    }
    void add(size_t c0, size_t c1, const sd_rec* r, const int64_t* ro, int threads) {
        if (failed) return;
        const size_t k = (size_t)ro[c1 - c0];
        if (n + k > cap) {
            cap = std::max(n + k, cap + cap / 2);
            sd_rec* q = static_cast<sd_rec*>(std::realloc(recs, sizeof(sd_rec) * cap));
            if (!q) { failed = true; return; }
            recs = q;
        }
        const size_t pieces = (k + 65535) / 65536;
        sd::parallel_for((int64_t)pieces, threads, 1, [&](int64_t x) {
            const size_t a = (size_t)x * 65536, b = std::min(k, a + 65536);
            std::memcpy(recs + n + a, r + a, sizeof(sd_rec) * (b - a));
        });
        for (size_t c = 1; c <= c1 - c0; ++c) off[c0 - c_lo + c] = (int64_t)n + ro[c];
        n += k;
    }
    void release(sd_rec** r, int64_t** o) { *r = recs; *o = off; recs = nullptr; off = nullptr; }
    ~RangeCollector() { std::free(recs); std::free(off); }
};

// The raw calls' job (sd_decompose*, the chunk-range calls): the reads' chunk table against a template set.  run() takes
// the chunks [lo, hi) through the device in batches of consecutive chunks sized to the free HBM, so a single 200-Mb
// sequence and a million reads take the same path, on one pipeline of its own kind ('C': JobPipes with the one entry
// {p->device}, driven on the calling thread); the records of every batch go to `sink(c0, c1, recs, rec_off)` in table
// order (chunk-local coordinates, rec_off relative to the batch), and a sink that returns false stops the dealing.
// `check` (may be empty) runs on the calling thread once the last batch is enqueued, i.e. while the device works
// (drive_entry's busy): the chunk-range calls check their share's alphabet there instead of before the first upload (a
// bad symbol still fails the call -- the records of the run are dropped -- it just no longer delays the device by the
// 0.2 ms the check of 27 Mb takes; the packer maps any byte to a 2-bit code, so the kernels run on whatever the bytes are).
using BatchSink = std::function<bool(size_t, size_t, const sd_rec*, const int64_t*)>;
using BusyCheck = std::function<int(std::string&)>;
struct RawJob {
    const std::vector<ReadView>& reads;
    const sd_params* p;
    TemplateSet ts;
    std::vector<CRef> table;
    std::vector<int32_t> nch;
    RawJob(const std::vector<ReadView>& r, const std::vector<sd::Seq>& monos, const sd_params* pp) : reads(r), p(pp), ts(monos) {
        build_chunk_table(reads, p, table, nch);
    }
    int run(size_t lo, size_t hi, const BatchSink& sink, const BusyCheck& check, std::string& err) {
        const bool timing = getenv("SD_TIMING") != nullptr;  // developer knob: stage times on stderr
        const double t_begin = now_s();
        JobPipes jp({p->device});
        int rc = jp.open(p, 'C', ts, nullptr, err);
        if (rc) return rc;
        int64_t rows = 0;
        for (size_t c = lo; c < hi; ++c) rows += table[c].len;
        const int64_t budget = jp.budget[0];   // (a new pipeline: fresh_row_budget; a job of one batch stays one batch)
        std::vector<std::pair<size_t, size_t>> batches;
        plan_batches(table, lo, hi, jp.reused() || rows <= budget ? budget : fresh_row_budget(budget, rows), 1, batches);
        std::atomic<int> sink_rc{SD_OK};
        int busy_rc = SD_OK;
        std::string busy_err;
        double t_busy = 0;
        rc = jp.drive(reads, table, batches, sink_rc, [](size_t, size_t, std::vector<int>&) {},
                      [&](Pipeline&, size_t c0, size_t c1, const sd_rec* r, const int64_t* ro) { if (!sink(c0, c1, r, ro)) sink_rc = SD_ERR_IO; },
                      [&] { t_busy = now_s(); if (check) busy_rc = check(busy_err); t_busy = now_s() - t_busy; }, err);
        // an undefined symbol in the share is the reference's own diagnostic (main.cpp:335): it is what the caller sees,
        // also when the device run over those bytes failed as well
        if (busy_rc) { rc = busy_rc; err = busy_err; }
        const PipeCounters& t = jp.pipes[0]->cnt;
        if (timing) {
            std::fprintf(stderr, "[sd timing] host work under the device: %.2f ms\n", t_busy * 1e3);
            std::fprintf(stderr, "[sd timing] %zu batches: pack+enqueue %.1f ms, wait %.1f ms, sink %.1f ms, kernels fill %.1f "
                         "trace %.1f compact %.2f ms, total %.1f ms\n", batches.size(), t.pack_s * 1e3, t.wait_s * 1e3,
                         t.sink_s * 1e3, t.fill_ms, t.trace_ms, t.compact_ms, (now_s() - t_begin) * 1e3);
        }
        jp.give_back(rc == SD_OK);
        return rc;
    }
    // The chunk-range calls: the records of [lo, hi) as the C-ABI hands them out (*recs / *rec_off, set on success only).
    int collect(size_t lo, size_t hi, const BusyCheck& check, sd_rec** recs, int64_t** rec_off, std::string& err) {
        RangeCollector col(hi - lo, lo);
        int rc = run(lo, hi, [&](size_t c0, size_t c1, const sd_rec* r, const int64_t* ro) {
            col.add(c0, c1, r, ro, p->threads);
            return !col.failed;
        }, check, err);
        if (rc == SD_OK && col.failed) { rc = SD_ERR_INTERNAL; err = "out of host memory"; }
        if (rc == SD_OK) col.release(recs, rec_off);
        return rc;
    }
};
}  // namespace

static int decompose_impl(const std::vector<ReadView>& reads, const std::vector<sd::Seq>& monos,
                          const sd_params* p, std::string& tsv, std::string& err, const char* records_out = nullptr,
                          std::vector<std::string>* parts_out = nullptr,   // parts_out: the text in pieces instead of `tsv`
                          const std::function<bool(std::vector<std::string>&)>& flush_parts = nullptr) {   // ... handed over after every batch
    if (monos.empty()) { err = "no monomers"; return SD_ERR_PARAM; }
    for (const ReadView& r : reads)
        if (r.len <= 0) { err = "ERROR: Sequence " + std::string(r.name, r.name_len) + " is empty"; return SD_ERR_EMPTY; }
    RawJob job(reads, monos, p);
    ReadAssembler as(reads, job.table, job.nch, job.ts.tnames, p->threads, tsv);
    as.part_sink = parts_out;
    sd::RecordsWriter rw;
    if (records_out) {
        const int orc = rw.open(records_out, *p, job.ts.tnames, err);
        if (orc) return orc;
        as.rec_out = &rw;
    }
    bool flush_ok = true;   // (a failed write stops the dealing)
    int rc = job.run(0, job.table.size(), [&](size_t c0, size_t c1, const sd_rec* recs, const int64_t* roff) {
        as.add(c0, c1, recs, roff);
        if (flush_parts && parts_out && flush_ok) flush_ok = flush_parts(*parts_out);
        return flush_ok;
    }, nullptr, err);
    if (rc == SD_OK && !flush_ok) { rc = SD_ERR_IO; err = "short write"; }
    if (records_out && rc == SD_OK) rc = rw.close(err, records_out);
    return rc;
}

// raw_tsv_out: the text `dp` prints; records_out: the same rows as the binary record stream (sd_records.hpp), no text made
static int decompose_files_impl(const char* reads_fa, const char* monomers_fa, const sd_params* p,
                                const char* raw_tsv_out, const char* records_out, char* errbuf, size_t errlen) {
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (!reads_fa || !monomers_fa || (!raw_tsv_out && !records_out)) return SD_ERR_PARAM;
    sd::FastaFile rf, mf;
    rc = rf.open(reads_fa, p->threads, err, lenient_of(p));                   // main.cpp:394
    if (rc == SD_OK) rc = rf.validate(0, rf.recs.size(), p->threads, err);
    if (rc == SD_OK) rc = mf.open(monomers_fa, p->threads, err, lenient_of(p));   // main.cpp:395
    if (rc == SD_OK) rc = mf.validate(0, mf.recs.size(), p->threads, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    sd_note_input_stats(rf, mf, lenient_of(p));
    sd_params p_job = *p;   // (the files are read: the pipelines and their cache keys never see the flag)
    p_job.reserved[1] &= ~SD_FLAG_LENIENT;
    p = &p_job;
    std::vector<sd::Seq> monos;
    for (const auto& r : mf.recs) monos.push_back(sd::Seq{std::string(r.name, r.name_len), std::string(r.seq, (size_t)r.len)});
    std::string out;
    std::vector<ReadView> views;
    views.reserve(rf.recs.size());
    for (const auto& r : rf.recs) views.push_back(ReadView{r.name, r.name_len, r.seq, r.len});
    // The text stays in the pieces the threads formatted and goes to the file after every device batch (write_parts: no
    // gather), i.e. while the next batch is on the device -- for a chromosome-sized read too, whose rows are merged and
    // formatted as its chunks arrive (ReadAssembler::stream_advance).
    std::vector<std::string> parts;
    int fd = -1;
    if (raw_tsv_out) {
        fd = ::open(raw_tsv_out, O_RDWR | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) { set_err(errbuf, errlen, std::string("cannot write ") + raw_tsv_out); return SD_ERR_IO; }
    }
    int64_t off = 0;
    auto flush = [&](std::vector<std::string>& ps) {
        const bool ok = fd < 0 || sd::write_parts(fd, off, ps, p->threads);
        ps.clear();
        return ok;
    };
    rc = decompose_impl(views, monos, p, out, err, records_out, &parts, flush);
    const bool closed = fd < 0 || ::close(fd) == 0;
    if (rc) { set_err(errbuf, errlen, err == "short write" ? std::string("short write to ") + raw_tsv_out : err); return rc; }
    if (!closed) { set_err(errbuf, errlen, std::string("short write to ") + raw_tsv_out); return SD_ERR_IO; }
    return SD_OK;
}

// File form of the chunk-range call for a job sharded over ranks: every rank maps and indexes the FASTA
// (no copy of the sequences), takes the contiguous share block_range(n_chunks, rank, world) of the global
// chunk table and checks the alphabet of the reads that share touches only (main.cpp:329-341 reports the
// first offending read in file order: the caller raises the error of the lowest failing rank).

// edge / hout set: the share's records stay with a range assembler (sd_decompose_files_range_begin)
static int decompose_files_range_impl(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank,
                                      int32_t world, sd_rec** recs, int64_t** rec_off, int64_t* chunk_lo, int64_t* chunk_hi,
                                      int64_t* n_chunks_total, sd_seam_edge* edge, sd_range_asm** hout, char* errbuf, size_t errlen) {
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    sd::FastaFile rf, mf;
    rc = rf.open(reads_fa, p->threads, err, lenient_of(p));
    if (rc == SD_OK) rc = mf.open(monomers_fa, p->threads, err, lenient_of(p));
    if (rc == SD_OK) rc = mf.validate(0, mf.recs.size(), p->threads, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    sd_note_input_stats(rf, mf, lenient_of(p));
    sd_params p_job = *p;   // (the files are read: the pipelines and their cache keys never see the flag)
    p_job.reserved[1] &= ~SD_FLAG_LENIENT;
    p = &p_job;
    std::vector<sd::Seq> monos;
    for (const auto& r : mf.recs) monos.push_back(sd::Seq{std::string(r.name, r.name_len), std::string(r.seq, (size_t)r.len)});
    if (monos.empty()) { set_err(errbuf, errlen, "no monomers"); return SD_ERR_PARAM; }
    std::vector<ReadView> reads;
    reads.reserve(rf.recs.size());
    for (const auto& r : rf.recs) {
        if (r.len <= 0) { set_err(errbuf, errlen, "ERROR: Sequence " + std::string(r.name, r.name_len) + " is empty"); return SD_ERR_EMPTY; }
        reads.push_back(ReadView{r.name, r.name_len, r.seq, r.len});
    }
    RawJob job(reads, monos, p);
    const int64_t n = (int64_t)job.table.size();
    const int64_t base = n / world, extra = n % world;
    const int64_t lo = rank * base + std::min<int64_t>(rank, extra);
    const int64_t hi = lo + base + (rank < extra ? 1 : 0);
    if (chunk_lo) *chunk_lo = lo;
    if (chunk_hi) *chunk_hi = hi;
    if (n_chunks_total) *n_chunks_total = n;
    // the reads this share touches are checked under the device's work
    auto validate = [&](std::string& verr) -> int {
        return hi > lo ? rf.validate((size_t)job.table[(size_t)lo].read, (size_t)job.table[(size_t)hi - 1].read + 1, p->threads, verr) : SD_OK;
    };
    sd_rec* r = nullptr;
    int64_t* o = nullptr;
    rc = job.collect((size_t)lo, (size_t)hi, validate, &r, &o, err);
    if (rc == SD_OK && hout) rc = range_asm_from_files(rf, mf, p, lo, hi, r, o, edge, hout, err);   // (takes r / o over, also when it fails)
    else if (rc == SD_OK) { *recs = r; *rec_off = o; }
    if (rc) set_err(errbuf, errlen, err);
    return rc;
}

// ---- the C entry points (include/sd_hip.h) ---------------------------------------------------------------------------
extern "C" {

void sd_params_default(sd_params* p) {
    std::memset(p, 0, sizeof *p);
    p->ins = -1; p->del = -1; p->mismatch = -1; p->match = 1;
    p->part_size = 5000; p->overlap = 500; p->ed_thr = -1; p->threads = 1; p->device = 0;
    p->kernel = 0;
}

const char* sd_version(void) { return "stringdecomposer_amd 0.1.0 (gfx950)"; }

int sd_device_count(void) { return device_count_checked(); }

void sd_free(void* p) { std::free(p); }

// Host only: the layout the fast kernel family would use for a monomer set and scoring -- what sd_engine_create
// decides before it touches the device.  For tests without a GPU and for users who want to know which kernels a
// set will run on.
int sd_plan_info(const sd_params* p, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                 int64_t info[8], char* errbuf, size_t errlen) {
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_mono <= 0 || !mono_seqs || !mono_lens || !info) { set_err(errbuf, errlen, "no monomers"); return SD_ERR_PARAM; }
    sd_engine e;   // (host fields only: nothing here or in its destructor calls the device)
    rc = host_templates(&e, *p, mono_seqs, mono_lens, n_mono, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    sd::FastPlan& plan = e.fplan;
    std::string why;
    e.p = *p;
    apply_env_overrides(e.p);
    const bool ok = plan_fast_family(e.p, e.tseq, e.sc, true, true, plan, why);
    for (int i = 0; i < 8; ++i) info[i] = 0;
    info[0] = ok ? 2 : 1;                       // kernel family "auto" would take: 2 fast, 1 generic
    if (!ok) { set_err(errbuf, errlen, why); return SD_OK; }
    info[1] = plan.P;
    info[2] = layout_code(plan);
    info[3] = plan.floor_slots;
    info[4] = plan.waves | ((int64_t)plan.range_bound << 8) | ((int64_t)plan.rebase << 40);
    // narrow layout: cells in the shortest first lane of a template and in the fullest lane (from slot_of)
    int64_t min_first = 1 << 30, max_lane = 0, x = 0;
    for (size_t j = 0; j < e.tseq.size(); ++j) {
        const int64_t L = (int64_t)e.tseq[j].size();
        int64_t run = 0, lanes_seen = 0;
        for (int64_t k = 0; k < L; ++k, ++x) {
            const uint32_t so = plan.slot_of[(size_t)x];
            const bool new_lane = k == 0 || (so & 127u) != (plan.slot_of[(size_t)x - 1] & 127u) || (so >> 16) != (plan.slot_of[(size_t)x - 1] >> 16);
            if (new_lane && k > 0) {
                if (lanes_seen == 0) min_first = std::min(min_first, run);
                max_lane = std::max(max_lane, run);
                ++lanes_seen;
                run = 0;
            }
            ++run;
        }
        if (lanes_seen == 0) min_first = std::min(min_first, run);
        max_lane = std::max(max_lane, run);
    }
    info[5] = min_first;
    info[6] = max_lane;
    info[7] = (int64_t)e.score_scale | ((int64_t)(plan.tr2_ok ? plan.tr2_qm : 0) << 16) | ((int64_t)(plan.tr2_ok ? plan.tr2_bound : 0) << 24) |
              ((int64_t)((plan.Hx >> 8) & 1) << 56);
    return SD_OK;
}

// Host only: the floor levels of the narrow fills for a monomer set and scoring, and the lane layout they were computed
// over (FastPlan::floor_sym, floor_pair, lane_bounds).
int sd_plan_floor_levels(const sd_params* p, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                         int32_t floor_sym[5], int32_t floor_pair[25], int32_t* lane_off, int32_t* lane_start, int64_t lane_cap,
                         int64_t info[4], char* errbuf, size_t errlen) {
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_mono <= 0 || !mono_seqs || !mono_lens || !floor_sym || !floor_pair || !lane_off || !lane_start || !info) {
        set_err(errbuf, errlen, "no monomers");
        return SD_ERR_PARAM;
    }
    sd_engine e;   // (host fields only, as in sd_plan_info)
    rc = host_templates(&e, *p, mono_seqs, mono_lens, n_mono, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    sd::FastPlan& plan = e.fplan;
    std::string why;
    e.p = *p;
    apply_env_overrides(e.p);
    const bool ok = plan_fast_family(e.p, e.tseq, e.sc, true, true, plan, why);
    for (int i = 0; i < 4; ++i) info[i] = 0;
    for (int i = 0; i < 5; ++i) floor_sym[i] = 0;
    for (int i = 0; i < 25; ++i) floor_pair[i] = 0;
    for (int j = 0; j <= e.T; ++j) lane_off[j] = 0;
    info[0] = ok ? 2 : 1;
    if (!ok) { set_err(errbuf, errlen, why); return SD_OK; }
    info[1] = plan.P;
    info[2] = plan.pair_rule ? 1 : 0;
    for (int b = 0; b < 5; ++b) floor_sym[b] = plan.floor_sym[b];
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b) floor_pair[5 * a + b] = plan.floor_pair[a][b];
    int64_t n = 0;
    for (int j = 0; j < e.T; ++j) {
        const std::vector<int32_t>& bj = plan.lane_bounds[(size_t)j];
        for (size_t u = 0; u + 1 < bj.size(); ++u, ++n)
            if (n < lane_cap) lane_start[n] = bj[u];
        lane_off[j + 1] = (int32_t)n;
    }
    info[3] = n;
    if (n > lane_cap) { set_err(errbuf, errlen, "lane_start too small"); return SD_ERR_PARAM; }
    return SD_OK;
}

int sd_engine_create(sd_engine** out, const sd_params* p, const char* const* mono_seqs,
                     const int32_t* mono_lens, int32_t n_mono, char* errbuf, size_t errlen) {
    if (!out) return SD_ERR_PARAM;
    *out = nullptr;
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_mono <= 0) { set_err(errbuf, errlen, "no monomers"); return SD_ERR_PARAM; }
    std::unique_ptr<sd_engine> e(new sd_engine);
    e->p = *p;
    apply_env_overrides(e->p);
    rc = host_templates(e.get(), *p, mono_seqs, mono_lens, n_mono, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    {
        const int w0 = (e->tlen[0] - 1) >> 6, h0 = ((e->tlen[0] - 1) >> 5) & 1;
        bool same = true;
        for (int j = 1; j < e->T; ++j) same = same && ((e->tlen[j] - 1) >> 6) == w0 && (((e->tlen[j] - 1) >> 5) & 1) == h0;
        e->filter_uniform = same && w0 == ((e->Lmax + 63) / 64) - 1 ? h0 : -1;
        if (e->p.reserved[1] & SD_FLAG_FILTER_GENERAL) e->filter_uniform = -1;
    }
    rc = check_score_range(*p, e->Lmax, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }

    if (device_count_checked() <= 0) {
        set_err(errbuf, errlen, "no HIP device available (libsd_hip has no CPU fallback)");
        return SD_ERR_NO_DEVICE;
    }
    try {
        SD_HIP(hipSetDevice(p->device));
        {
            // Host threads that wait for the device sleep instead of spinning.  A rank of the pipelined path waits
            // ~14 of every 16 ms; spinning, it burns a whole CPU for that (measured: 34.5 -> 21.5 ms of CPU time
            // per 16.3-ms step and rank, same step time), which an 8-GPU node whose ranks share the host CPUs
            // (or a container CPU quota) cannot spare.  SD_HOST_WAIT=spin keeps the runtime's default.
            const char* hw = getenv("SD_HOST_WAIT");
            if (!(hw && hw[0] == 's') && hipSetDeviceFlags(hipDeviceScheduleBlockingSync) != hipSuccess)
                (void)hipGetLastError();
        }
        e->device = p->device;
        {
            // (hipGetDeviceProperties fills a 1.5-KB struct from the driver: milliseconds; one attribute is enough)
            static std::atomic<int> cu_of[64];
            int ncu = (p->device >= 0 && p->device < 64) ? cu_of[p->device].load() : 0;
            if (ncu <= 0) {
                SD_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p->device));
                if (p->device >= 0 && p->device < 64) cu_of[p->device].store(ncu);
            }
            e->n_cu = ncu > 0 ? ncu : 256;
            e->d_queue.alloc(sd_engine::QS * (size_t)sd_engine::QN);
            SD_HIP(hipMemset(e->d_queue.p, 0, sizeof(int) * sd_engine::QS * (size_t)sd_engine::QN));
        }
        rc = engine_pick_family(e.get(), true, err);
        if (rc) { set_err(errbuf, errlen, err); return rc; }
        if (p->ed_thr > -1) {
            std::vector<unsigned long long> peq;
            sd::build_peq(e->tseq, peq);
            e->d_peq.upload(peq);
        }
        SD_HIP(hipEventCreate(&e->ev_run0));
        // the events the host waits on put the waiting thread to sleep (interrupt) instead of spinning: a rank
        // waits ~14 of 16 ms per step, and on a node where the host CPUs are shared by 8 ranks (or capped by a
        // cgroup quota) a spinning waiter per rank takes the time the packers need
        SD_HIP(hipEventCreateWithFlags(&e->ev_run1, hipEventBlockingSync));
        SD_HIP(hipEventCreate(&e->ev_cmp0));
        SD_HIP(hipEventCreate(&e->ev_cmp1));
        SD_HIP(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming | hipEventBlockingSync));
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    *out = e.release();
    return SD_OK;
}

void sd_engine_destroy(sd_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    delete e;
}

int sd_engine_load_reads(sd_engine* e, const char* const* read_seqs, const int64_t* read_lens,
                         int32_t n_reads, int64_t* n_chunks, char* errbuf, size_t errlen) {
    if (!e) return SD_ERR_PARAM;
    e->chunk_read.clear();
    e->chunk_off.clear();
    e->read_nchunks.assign((size_t)std::max(n_reads, 0), 0);
    e->n_reads = n_reads;
    // chunk table (main.cpp:70-81)
    std::vector<const char*> cptr;
    std::vector<int32_t> clen;
    for (int32_t r = 0; r < n_reads; ++r) {
        int cnt = sd::chunk_plan(read_lens[r], e->p.part_size, e->p.overlap, [&](int64_t off, int32_t l) {
            cptr.push_back(read_seqs[r] + off);
            clen.push_back(l);
            e->chunk_read.push_back(r);
            e->chunk_off.push_back(off);
        });
        if (cnt == 0) {
            set_err(errbuf, errlen, "ERROR: Sequence #" + std::to_string(r) + " is empty");
            return SD_ERR_EMPTY;
        }
        e->read_nchunks[(size_t)r] = cnt;
    }
    if (n_chunks) *n_chunks = (int64_t)cptr.size();
    // default (null) stream: a later sd_engine_run on any blocking stream is ordered behind the copy;
    // the explicit wait also covers non-blocking streams
    const int rc = load_chunks_impl(e, cptr, clen, nullptr, errbuf, errlen);
    if (rc == SD_OK && hipEventSynchronize(e->ev_in) != hipSuccess) {
        set_err(errbuf, errlen, "H2D copy of the packed reads failed");
        return SD_ERR_HIP;
    }
    e->in_pending = false;
    return rc;
}

int sd_engine_load_reads_dev(sd_engine* e, const void* d_bases, const int64_t* read_off, const int64_t* read_lens,
                             int32_t n_reads, void* hip_stream, int64_t* n_chunks, char* errbuf, size_t errlen) {
    if (!e || n_reads < 0 || (n_reads > 0 && (!d_bases || !read_off || !read_lens))) return SD_ERR_PARAM;
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_lens[r] <= 0) {
            set_err(errbuf, errlen, "ERROR: Sequence #" + std::to_string(r) + " is empty");
            return SD_ERR_EMPTY;
        }
    std::string err;
    int dev = -1;
    int rc = n_reads > 0 ? device_pointer(d_bases, dev, err) : SD_OK;
    if (rc == SD_OK && n_reads > 0 && dev != e->device) {
        err = "the reads lie in the memory of device " + std::to_string(dev) + ", the engine runs on device " + std::to_string(e->device);
        rc = SD_ERR_UNSUPPORTED;
    }
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    e->chunk_read.clear();
    e->chunk_off.clear();
    e->read_nchunks.assign((size_t)n_reads, 0);
    e->n_reads = n_reads;
    std::vector<const char*> cptr;
    std::vector<int32_t> clen;
    std::vector<int64_t> gpos;
    auto cum = std::make_shared<std::vector<int64_t>>((size_t)n_reads + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) {
        (*cum)[(size_t)r + 1] = (*cum)[(size_t)r] + read_lens[r];
        e->read_nchunks[(size_t)r] = sd::chunk_plan(read_lens[r], e->p.part_size, e->p.overlap, [&](int64_t off, int32_t l) {
            cptr.push_back(static_cast<const char*>(d_bases) + read_off[r] + off);
            clen.push_back(l);
            gpos.push_back((*cum)[(size_t)r] + off);
            e->chunk_read.push_back(r);
            e->chunk_off.push_back(off);
        });
    }
    if (n_chunks) *n_chunks = (int64_t)cptr.size();
    DevSrc ds;
    ds.user = reinterpret_cast<hipStream_t>(hip_stream);
    ds.gpos = gpos.data();
    ds.cum = cum;
    hipEvent_t ready = nullptr;
    if (hipSetDevice(e->device) != hipSuccess || hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess ||
        hipEventRecord(ready, ds.user) != hipSuccess) {
        (void)hipGetLastError();
        if (ready) (void)hipEventDestroy(ready);
        set_err(errbuf, errlen, "cannot record an event on the caller's stream");
        return SD_ERR_HIP;
    }
    ds.ready = ready;
    rc = load_chunks_impl(e, cptr, clen, nullptr, errbuf, errlen, &ds);
    if (rc == SD_OK && hipEventSynchronize(e->ev_in) != hipSuccess) {
        set_err(errbuf, errlen, "packing the reads on the device failed");
        rc = SD_ERR_HIP;
    }
    (void)hipEventDestroy(ready);
    e->in_pending = false;
    return rc;
}

int sd_pack_bases_dev(const void* d_bases, const int64_t* chunk_off, const int32_t* chunk_len, int32_t n_chunks,
                      int32_t device, void* hip_stream, uint32_t* bases2, uint32_t* nmask, int32_t* has_n,
                      int64_t* first_bad) {
    if (n_chunks < 0 || (n_chunks > 0 && (!d_bases || !chunk_off || !chunk_len || !bases2 || !nmask))) return SD_ERR_PARAM;
    for (int32_t c = 0; c < n_chunks; ++c)
        if (chunk_len[c] <= 0 || chunk_off[c] < 0) return SD_ERR_PARAM;
    if (first_bad) *first_bad = -1;
    if (n_chunks == 0) return SD_OK;
    std::string err;
    int dev = -1;
    int rc = device_pointer(d_bases, dev, err);
    if (rc) return rc;
    if (dev != device) return SD_ERR_UNSUPPORTED;
    try {
        SD_HIP(hipSetDevice(device));
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        const size_t C = (size_t)n_chunks;
        std::vector<sd::ChunkDesc> tab(C);
        std::vector<unsigned long long> src(C);
        std::vector<long long> gpos(C);
        size_t words = 0, nwords = 0;
        for (size_t c = 0; c < C; ++c) {
            tab[c] = sd::ChunkDesc{};
            tab[c].woff = (uint32_t)words;
            tab[c].n = chunk_len[c];
            tab[c].noff = (int32_t)nwords;
            words += ((size_t)chunk_len[c] + 15) / 16;
            nwords += ((size_t)chunk_len[c] + 31) / 32;
            src[c] = (unsigned long long)reinterpret_cast<uintptr_t>(static_cast<const char*>(d_bases) + chunk_off[c]);
            gpos[c] = chunk_off[c];
        }
        if (words >= (1ull << 31)) return SD_ERR_UNSUPPORTED;
        DevBuf<sd::ChunkDesc> d_tab;
        DevBuf<unsigned long long> d_src, d_bad;
        DevBuf<long long> d_gpos;
        DevBuf<uint32_t> d_w, d_m;
        d_tab.alloc(C); d_src.alloc(C); d_gpos.alloc(C); d_bad.alloc(1); d_w.alloc(words); d_m.alloc(nwords);
        unsigned long long bad = ~0ull;
        // (the caller's words go up first: what the packer leaves alone comes back as it was)
        SD_HIP(hipMemcpyAsync(d_tab.p, tab.data(), C * sizeof(sd::ChunkDesc), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(d_src.p, src.data(), C * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(d_gpos.p, gpos.data(), C * sizeof(long long), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(d_bad.p, &bad, sizeof bad, hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(d_w.p, bases2, words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(d_m.p, nmask, nwords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        sd::PackDevArgs pa{};
        pa.chunks = d_tab.p; pa.src = d_src.p; pa.gpos = d_gpos.p; pa.n_chunks = n_chunks;
        pa.bases2 = d_w.p; pa.nmask = d_m.p; pa.bad = d_bad.p;
        sd::launch_pack_dev(st, pa);
        SD_HIP(hipGetLastError());
        SD_HIP(hipMemcpyAsync(tab.data(), d_tab.p, C * sizeof(sd::ChunkDesc), hipMemcpyDeviceToHost, st));
        SD_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, st));
        SD_HIP(hipMemcpyAsync(bases2, d_w.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SD_HIP(hipMemcpyAsync(nmask, d_m.p, nwords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));
        if (has_n)
            for (size_t c = 0; c < C; ++c) has_n[c] = tab[c].noff >= 0 ? 1 : 0;
        if (first_bad && bad != ~0ull) *first_bad = (int64_t)(bad >> 8);
    } catch (const HipFail&) {
        return SD_ERR_HIP;
    }
    return SD_OK;
}

int sd_engine_run(sd_engine* e, void* hip_stream, char* errbuf, size_t errlen) {
    if (!e) return SD_ERR_PARAM;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return engine_run2(e, st, st, errbuf, errlen);
}

int64_t sd_guard_trips(void) { return (int64_t)g_guard_trips.load(); }

int sd_engine_fetch(sd_engine* e, sd_rec** recs, int64_t** rec_off, char* errbuf, size_t errlen) {
    if (!e || !recs || !rec_off) return SD_ERR_PARAM;
    *recs = nullptr;
    *rec_off = nullptr;
    int64_t total = 0;
    int rc = fetch_begin(e, total, errbuf, errlen);
    if (rc == SD_OK && !e->chunks.empty()) rc = fetch_whole(e, total, errbuf, errlen);
    if (rc) return rc;
    const size_t C = e->chunks.size();
    int64_t* off = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * (C + 1)));
    sd_rec* out = static_cast<sd_rec*>(std::malloc(sizeof(sd_rec) * (size_t)std::max<int64_t>(total, 1)));
    if (!off || !out) { std::free(off); std::free(out); set_err(errbuf, errlen, "out of host memory"); return SD_ERR_INTERNAL; }
    std::memcpy(off, e->h_roff.p, sizeof(int64_t) * (C + 1));
    if (total > 0) std::memcpy(out, e->h_recs.p, sizeof(sd_rec) * (size_t)total);
    *recs = out;
    *rec_off = off;
    e->fetched = true;
    return SD_OK;
}

// The prefilter's tables of the run whose rows the last sd_engine_fetch brought (a batch repeated after a guard trip: the
// repeat's -- the engine's family and plan are those of the repeat, and it wrote the tables last).  No kernel: copies
// and a host decode of whichever rank form sd_rank_keep wrote for the family.
int sd_engine_filter_result(sd_engine* e, int32_t* dist, uint16_t* rank, int64_t cap, int64_t* n_chunks, int32_t* n_templates,
                            char* errbuf, size_t errlen) {
    if (!e) return SD_ERR_PARAM;
    if (e->p.ed_thr < 0) { set_err(errbuf, errlen, "sd_engine_filter_result: the engine runs without --ed_thr"); return SD_ERR_PARAM; }
    if (!e->ran || !e->fetched) { set_err(errbuf, errlen, "sd_engine_filter_result before sd_engine_fetch"); return SD_ERR_PARAM; }
    const size_t C = e->chunks.size(), T = (size_t)e->T;
    if (n_chunks) *n_chunks = (int64_t)C;
    if (n_templates) *n_templates = e->T;
    if (!dist || !rank || cap < (int64_t)(C * T)) {
        set_err(errbuf, errlen, "sd_engine_filter_result: room for n_chunks x n_templates entries is needed");
        return SD_ERR_PARAM;
    }
    if (C == 0) return SD_OK;
    try {
        SD_HIP(hipSetDevice(e->device));
        SD_HIP(hipEventSynchronize(e->ev_run1));
        SD_HIP(hipMemcpy(dist, e->d_dist.p, C * T * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (e->family == 1) {   // rank table [chunk][T], 0xffff = dropped
            SD_HIP(hipMemcpy(rank, e->d_grank.p, C * T * sizeof(uint16_t), hipMemcpyDeviceToHost));
        } else if (compacted(e)) {
            // the kept templates of a chunk in their filtered order, behind them the 0xffff the launcher filled (d_kpos
            // and d_nkept are not read: the tiled layout turns them into first lanes / lanes used, sd_tiled_place)
            std::vector<uint16_t> kl(C * T);
            SD_HIP(hipMemcpy(kl.data(), e->d_klist.p, C * T * sizeof(uint16_t), hipMemcpyDeviceToHost));
            std::fill(rank, rank + C * T, (uint16_t)0xffff);
            for (size_t c = 0; c < C; ++c)
                for (size_t r = 0; r < T && kl[c * T + r] != 0xffff; ++r) {
                    if (kl[c * T + r] >= T) { set_err(errbuf, errlen, "sd_engine_filter_result: template index beyond the set in the kept list"); return SD_ERR_INTERNAL; }
                    rank[c * T + kl[c * T + r]] = (uint16_t)r;
                }
        } else {
            // per-lane constants of the ranked fills: the rank at the lane that holds the template's end (sd_rank_keep)
            const size_t W = (size_t)e->fplan.waves;
            std::vector<uint16_t> cr(C * W * 64 * 2);
            SD_HIP(hipMemcpy(cr.data(), e->d_crank.p, cr.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
            for (size_t c = 0; c < C; ++c)
                for (size_t j = 0; j < T; ++j) {
                    const int v = e->fplan.end_vlane[j];
                    const size_t at = ((c * W + (size_t)(v >> 7)) * 64 + (size_t)(v & 63)) * 2 + (size_t)((v >> 6) & 1);
                    rank[c * T + j] = cr[at] == 0x7fff ? (uint16_t)0xffff : cr[at];
                }
        }
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

int sd_engine_assemble(sd_engine* e, const sd_rec* recs, const int64_t* rec_off, sd_rec** rows,
                       int64_t** row_off, char* errbuf, size_t errlen) {
    (void)errbuf; (void)errlen;
    if (!e || !rows || !row_off) return SD_ERR_PARAM;
    std::vector<sd_rec> all;
    std::vector<int64_t> offs((size_t)e->n_reads + 1, 0);
    std::vector<sd_rec> batch;
    size_t c = 0;
    for (int32_t r = 0; r < e->n_reads; ++r) {
        batch.clear();
        for (int a = 0; a < e->read_nchunks[(size_t)r]; ++a, ++c) {
            const int32_t add = (int32_t)e->chunk_off[c];  // main.cpp:109-111
            for (int64_t x = rec_off[c]; x < rec_off[c + 1]; ++x) {
                sd_rec t = recs[x];
                t.start += add;
                t.end += add;
                batch.push_back(t);
            }
        }
        sd::seam_merge(batch);  // main.cpp:116
        all.insert(all.end(), batch.begin(), batch.end());
        offs[(size_t)r + 1] = (int64_t)all.size();
    }
    sd_rec* o = static_cast<sd_rec*>(std::malloc(sizeof(sd_rec) * std::max<size_t>(all.size(), 1)));
    if (!all.empty()) std::memcpy(o, all.data(), sizeof(sd_rec) * all.size());
    int64_t* ro = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * offs.size()));
    std::memcpy(ro, offs.data(), sizeof(int64_t) * offs.size());
    *rows = o;
    *row_off = ro;
    return SD_OK;
}

int sd_engine_timings(sd_engine* e, float ms[4]) {
    if (!e || !e->ran) return SD_ERR_PARAM;
    ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
    if (hipSetDevice(e->device) != hipSuccess) return SD_ERR_HIP;
    if (hipEventSynchronize(e->ev_run1) != hipSuccess) return SD_ERR_HIP;
    const size_t pairs = e->family == 1 ? e->subs.size() : (e->chunks.empty() ? 0 : 1);
    for (size_t s = 0; s < pairs; ++s) {
        float a = 0.f, b = 0.f;
        (void)hipEventElapsedTime(&a, e->ev_fill[2 * s], e->ev_fill[2 * s + 1]);
        (void)hipEventElapsedTime(&b, e->ev_trace[2 * s], e->ev_trace[2 * s + 1]);
        ms[0] += a;
        ms[1] += b;
    }
    if (!e->chunks.empty()) (void)hipEventElapsedTime(&ms[2], e->ev_cmp0, e->ev_cmp1);
    (void)hipEventElapsedTime(&ms[3], e->ev_run0, e->ev_run1);
    return SD_OK;
}

int sd_engine_info(sd_engine* e, int64_t info[8]) {
    if (!e) return SD_ERR_PARAM;
    info[0] = e->T;
    info[1] = e->sumL;
    info[2] = (int64_t)e->chunks.size();
    info[3] = e->rows;
    info[4] = e->family | ((e->family == 1 ? 0 : layout_code(e->fplan)) << 8);
    info[5] = e->family == 1 ? e->Q : (e->fplan.P | ((int64_t)e->fplan.floor_slots << 16));
    info[6] = (int64_t)e->workspace_bytes();
    info[7] = (e->family == 1 ? (int64_t)e->subs.size() : 1) |
              ((int64_t)(e->family == 1 ? 0 : (e->fplan.tr2_ok && !e->compact_edthr) ? 2 : 1) << 16);
    return SD_OK;
}

int sd_decompose(const char* const* read_names, const char* const* read_seqs,
                 const int64_t* read_lens, int32_t n_reads, const char* const* mono_names,
                 const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                 const sd_params* p, char** tsv, size_t* tsv_len, char* errbuf, size_t errlen) {
    if (!tsv || !tsv_len) return SD_ERR_PARAM;
    *tsv = nullptr;
    *tsv_len = 0;
    std::string err;
    {
        const int vrc = validate_params(p, err);  // before anything walks the chunk table (part_size > 0)
        if (vrc) { set_err(errbuf, errlen, err); return vrc; }
        if (n_reads < 0 || n_mono < 0 || (n_reads && (!read_names || !read_seqs || !read_lens)) ||
            (n_mono && (!mono_names || !mono_seqs || !mono_lens))) {
            set_err(errbuf, errlen, "null input array");
            return SD_ERR_PARAM;
        }
    }
    std::vector<ReadView> reads((size_t)std::max(n_reads, 0));
    std::vector<sd::Seq> monos((size_t)std::max(n_mono, 0));
    {
        // alphabet check of all reads on the host threads; the first offending read (in input
        // order) is reported, as load_fasta does (main.cpp:329-341)
        std::vector<int> bad((size_t)std::max(n_reads, 0), 0);
        sd::parallel_for(n_reads, p->threads, 8, [&](int64_t r) {
            reads[(size_t)r] = ReadView{read_names[r], std::strlen(read_names[r]), read_seqs[r], read_lens[r]};
            std::string e2;
            bad[(size_t)r] = sd::check_alphabet(read_names[r], read_seqs[r], read_lens[r], e2) != SD_OK;
        });
        for (int32_t r = 0; r < n_reads; ++r)
            if (bad[(size_t)r]) {
                int rc = sd::check_alphabet(read_names[r], read_seqs[r], read_lens[r], err);
                set_err(errbuf, errlen, err);
                return rc;
            }
    }
    for (int32_t m = 0; m < n_mono; ++m) {
        monos[(size_t)m].name = mono_names[m];
        monos[(size_t)m].seq.assign(mono_seqs[m], (size_t)mono_lens[m]);
        int rc = sd::check_alphabet(mono_names[m], mono_seqs[m], mono_lens[m], err);
        if (rc) { set_err(errbuf, errlen, err); return rc; }
    }
    std::string out;
    int rc = decompose_impl(reads, monos, p, out, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    char* o = static_cast<char*>(std::malloc(out.size() + 1));
    std::memcpy(o, out.data(), out.size());
    o[out.size()] = 0;
    *tsv = o;
    *tsv_len = out.size();
    return SD_OK;
}

int sd_decompose_files(const char* reads_fa, const char* monomers_fa, const sd_params* p,
                       const char* raw_tsv_out, char* errbuf, size_t errlen) {
    if (!raw_tsv_out) return SD_ERR_PARAM;
    return decompose_files_impl(reads_fa, monomers_fa, p, raw_tsv_out, nullptr, errbuf, errlen);
}

int sd_decompose_files_records(const char* reads_fa, const char* monomers_fa, const sd_params* p,
                               const char* records_out, char* errbuf, size_t errlen) {
    if (!records_out) return SD_ERR_PARAM;
    return decompose_files_impl(reads_fa, monomers_fa, p, nullptr, records_out, errbuf, errlen);
}

// Host only (CPU test): the two pieces of pipeline logic that decide WHICH engines a job meets and HOW it is cut, checked
// against their contracts without a device --
//   pipe_cache_key: two jobs share cached engines exactly when every parameter that shapes an engine and the monomer set
//     agree; the host-thread count does not shape one; ("AC", "G") and ("A", "CG") are different sets;
//   plan_batches / fresh_row_budget: consecutive, complete, in order; no batch above the budget unless one chunk alone
//     is; at least half of min_batches when there are that many chunks (a share carries a slack of one chunk); no small
//     remainder (the smallest batch of a job of equal chunks, 16 or more per batch, holds at least half the rows of the largest).
// Returns SD_OK or SD_ERR_INTERNAL with the broken property in errbuf.
int sd_pipeline_logic_selftest(char* errbuf, size_t errlen) {
    auto fail = [&](const std::string& m) { set_err(errbuf, errlen, m); return SD_ERR_INTERNAL; };
    sd_params a;
    sd_params_default(&a);
    const char* m1[] = {"ACGT", "GG"};
    const std::vector<const char*> ms(m1, m1 + 2);
    const std::vector<int32_t> ml = {4, 2};
    const std::string k0 = pipe_cache_key(a, '1', ms, ml);
    {
        sd_params b = a;
        b.threads = 17;
        if (pipe_cache_key(b, '1', ms, ml) != k0) return fail("cache key depends on the host-thread count");
    }
    int32_t* fields[] = {&a.ins, &a.del, &a.mismatch, &a.match, &a.part_size, &a.overlap, &a.ed_thr, &a.device, &a.kernel,
                         &a.max_batch_rows, &a.reserved[0], &a.reserved[1], &a.reserved[2], &a.reserved[3], &a.reserved[4]};
    for (size_t f = 0; f < sizeof fields / sizeof fields[0]; ++f) {
        const int32_t keep = *fields[f];
        *fields[f] = keep + 1;
        const std::string k = pipe_cache_key(a, '1', ms, ml);
        *fields[f] = keep;
        if (k == k0) return fail("cache key ignores parameter field " + std::to_string(f));
    }
    if (pipe_cache_key(a, '2', ms, ml) == k0) return fail("cache key ignores the job kind");
    {
        const char* m2[] = {"ACGTG", "G"};
        if (pipe_cache_key(a, '1', std::vector<const char*>(m2, m2 + 2), {5, 1}) == k0) return fail("cache key: monomer boundaries");
        const char* m3[] = {"GG", "ACGT"};
        if (pipe_cache_key(a, '1', std::vector<const char*>(m3, m3 + 2), {2, 4}) == k0) return fail("cache key: monomer order");
    }
    if (pipe_cache_take(std::string("no such key\x01")) != nullptr) return fail("cache returned a pipeline for an unknown key");
    // batch plans over random chunk tables
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t n) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint64_t)(rng % n); };
    for (int trial = 0; trial < 400; ++trial) {
        const size_t n = 1 + (size_t)rnd(300);
        const bool equal = rnd(3) == 0;
        std::vector<CRef> table(n);
        for (size_t c = 0; c < n; ++c) table[c] = CRef{(int32_t)c, 0, equal ? 5500 : (int32_t)(1 + rnd(5500))};
        const size_t lo = (size_t)rnd(n), hi = lo + 1 + (size_t)rnd(n - lo);
        const int64_t budget = 1 + (int64_t)rnd(200000);
        const int minb = 1 + (int)rnd(9);
        std::vector<std::pair<size_t, size_t>> out;
        plan_batches(table, lo, hi, budget, minb, out);
        size_t at = lo;
        int64_t small = INT64_MAX, big = 0;
        for (const auto& b : out) {
            if (b.first != at || b.second <= b.first) return fail("batches are not consecutive and non-empty");
            int64_t rows = 0;
            for (size_t c = b.first; c < b.second; ++c) rows += table[c].len;
            if (rows > budget && b.second - b.first > 1) return fail("a batch of several chunks exceeds the budget");
            small = std::min(small, rows);
            big = std::max(big, rows);
            at = b.second;
        }
        if (at != hi) return fail("batches do not cover the range");
        // (the shares carry a slack of one chunk, so a batch may take one chunk more than its share: at least half of what was asked for)
        if (equal && budget >= (int64_t)5500 * (int64_t)(hi - lo) && 2 * out.size() < (size_t)std::min<int>(minb, (int)(hi - lo)))
            return fail("far fewer batches than min_batches although the chunks allow them");
        // (with a handful of chunks per batch the one-chunk slack itself is a large fraction: 10 chunks in 4 batches are 3, 3, 3, 1)
        if (equal && out.size() > 1 && hi - lo >= 16 * out.size() && small * 2 < big) return fail("a small remainder batch");
    }
    if (fresh_row_budget(100 << 20, 1000) > (100 << 20)) return fail("fresh_row_budget raised the budget");
    for (int64_t rows : {(int64_t)1 << 20, (int64_t)60 << 20, (int64_t)500 << 20, (int64_t)5000 << 20, (int64_t)30000 << 20}) {
        const int64_t b = fresh_row_budget((int64_t)64 << 20, rows);
        if (b <= 0 || b > ((int64_t)64 << 20)) return fail("fresh_row_budget outside (0, budget]");
    }
    return SD_OK;
}

void sd_release_cache(void) { pipe_cache_clear(); g_pool.release_all(); g_pinpool.release_all(); g_deferred.drain(); text_pool_clear(); }

// -------------------------------------------------------------------------------------------
// chunk-range form: multi-GPU sharding of one job, one process per GPU
// -------------------------------------------------------------------------------------------
int sd_decompose_chunk_range(const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads,
                             const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                             const sd_params* p, int64_t chunk_lo, int64_t chunk_hi, sd_rec** recs,
                             int64_t** rec_off, char* errbuf, size_t errlen) {
    if (!recs || !rec_off || !read_seqs || !read_lens || !mono_seqs || !mono_lens) return SD_ERR_PARAM;
    *recs = nullptr;
    *rec_off = nullptr;
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_mono <= 0) { set_err(errbuf, errlen, "no monomers"); return SD_ERR_PARAM; }
    std::vector<ReadView> reads((size_t)std::max(n_reads, 0));
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] <= 0) { set_err(errbuf, errlen, "ERROR: Sequence #" + std::to_string(r) + " is empty"); return SD_ERR_EMPTY; }
        reads[(size_t)r] = ReadView{"", 0, read_seqs[r], read_lens[r]};
    }
    std::vector<sd::Seq> monos((size_t)n_mono);
    for (int32_t m = 0; m < n_mono; ++m) {
        monos[(size_t)m].name = "m" + std::to_string(m);
        monos[(size_t)m].seq.assign(mono_seqs[m], (size_t)mono_lens[m]);
        rc = sd::check_alphabet(monos[(size_t)m].name.c_str(), mono_seqs[m], mono_lens[m], err);
        if (rc) { set_err(errbuf, errlen, err); return rc; }
    }
    RawJob job(reads, monos, p);
    const std::vector<CRef>& table = job.table;
    if (chunk_lo < 0 || chunk_hi < chunk_lo || (size_t)chunk_hi > table.size()) {
        set_err(errbuf, errlen, "chunk range outside the chunk table");
        return SD_ERR_PARAM;
    }
    // only the bases this range touches are validated (every rank validates its own share) -- under the device's work
    auto validate = [&](std::string& verr) -> int {
        std::vector<int> bad((size_t)(chunk_hi - chunk_lo), 0);
        sd::parallel_for(chunk_hi - chunk_lo, p->threads, 64, [&](int64_t i) {
            const CRef& c = table[(size_t)(chunk_lo + i)];
            std::string e2;
            bad[(size_t)i] = sd::check_alphabet("", reads[(size_t)c.read].seq + c.off, c.len, e2) != SD_OK;
        });
        for (size_t i = 0; i < bad.size(); ++i)
            if (bad[i]) {
                const CRef& c = table[(size_t)chunk_lo + i];
                const std::string nm = "#" + std::to_string(c.read);
                return sd::check_alphabet(nm.c_str(), reads[(size_t)c.read].seq + c.off, c.len, verr);
            }
        return SD_OK;
    };
    rc = job.collect((size_t)chunk_lo, (size_t)chunk_hi, validate, recs, rec_off, err);
    if (rc) set_err(errbuf, errlen, err);
    return rc;
}

int sd_decompose_files_range(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank,
                             int32_t world, sd_rec** recs, int64_t** rec_off, int64_t* chunk_lo, int64_t* chunk_hi,
                             int64_t* n_chunks_total, char* errbuf, size_t errlen) {
    if (!recs || !rec_off || !reads_fa || !monomers_fa || world < 1 || rank < 0 || rank >= world) return SD_ERR_PARAM;
    *recs = nullptr;
    *rec_off = nullptr;
    return decompose_files_range_impl(reads_fa, monomers_fa, p, rank, world, recs, rec_off, chunk_lo, chunk_hi, n_chunks_total,
                                      nullptr, nullptr, errbuf, errlen);
}

int sd_decompose_files_range_begin(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank,
                                   int32_t world, sd_seam_edge* edge, sd_range_asm** h, int64_t* chunk_lo, int64_t* chunk_hi,
                                   int64_t* n_chunks_total, char* errbuf, size_t errlen) {
    if (!edge || !h || !reads_fa || !monomers_fa || world < 1 || rank < 0 || rank >= world) return SD_ERR_PARAM;
    *h = nullptr;
    return decompose_files_range_impl(reads_fa, monomers_fa, p, rank, world, nullptr, nullptr, chunk_lo, chunk_hi, n_chunks_total,
                                      edge, h, errbuf, errlen);
}

}  // extern "C"
