// sd_job_dev.hpp -- internal to libsd_hip.so: the host-side frame that the analyses on final rows, segments and reads share
// (sd_lags.hip, sd_heat.hip, sd_autocorr.hip, sd_split.hip, sd_dotplot.hip; sd_hits_job.hpp for the two motif searches).
// Header-only, no kernel: per-device work areas kept between calls, the argument checks and their texts, the read tables,
// the upload of a host-memory call's reads, the stream of such a call and the timed repetitions of a bench entry.
// DESIGN.md, "The frame of an analysis", says who owns what.
#pragma once

#include <map>
#include <mutex>
#include <type_traits>

#include "sd_pipeline.hpp"

namespace sdi {

// Base of a per-device work area that is kept between calls.  A device-resident call returns with its kernels in flight on
// the caller's stream, so the buffers cannot be the call's own: in_flight() records ev_use behind the last kernel and the
// next call on the device settle()s before it touches them.  m serialises the calls on one device.
struct DevWork {
    std::mutex m;
    hipEvent_t ev_use = nullptr;
    bool used = false;
    int n_cu = 256;
    void settle() {
        if (used && hipEventSynchronize(ev_use) != hipSuccess) (void)hipGetLastError();
        used = false;
    }
    void in_flight(hipStream_t st) {
        ensure_event(ev_use, hipEventDisableTiming);
        SD_HIP(hipEventRecord(ev_use, st));
        used = true;
    }
    void waited() { used = false; }   // (the caller has synchronised the stream)
};

// the work area of type Ctx (a DevWork) of `device`, made at its first use
template <class Ctx>
Ctx& device_ctx(int device) {
    static std::mutex m;
    static std::map<int, Ctx*>* all = new std::map<int, Ctx*>;   // (never destroyed: no HIP call at process exit)
    std::lock_guard<std::mutex> g(m);
    Ctx*& c = (*all)[device];
    if (!c) {
        c = new Ctx;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
        else (void)hipGetLastError();
    }
    return *c;
}

// is `device` a device; errbuf may be null
inline int device_check(int32_t device, char* errbuf, size_t errlen) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); set_err(errbuf, errlen, "no usable HIP device"); return SD_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_err(errbuf, errlen, "device " + std::to_string(device) + " does not exist"); return SD_ERR_PARAM; }
    return SD_OK;
}

// no byte of the text outside ACGTN (the bytes the pair kernels read)
inline bool text_is_acgtn(const char* t, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (t[i] != 'A' && t[i] != 'C' && t[i] != 'G' && t[i] != 'T' && t[i] != 'N') return false;
    return true;
}

// The checked segments of a segment call: start (in seq + lo) and length per segment, [lo, hi) the text they cover, and in
// *grp (may be null) the group of every segment.  seg_limit: the segments the caller can number, too_many: what it says
// of a job with that many.  The caller's results and the order inside group_off are the caller's to check.
inline int segment_args(const char* who, const char* seq, int64_t seqlen, const int64_t* starts, const int64_t* ends, int64_t n_seg,
                        const int64_t* group_off, int32_t n_groups, const void* sums, int64_t seg_limit, const char* too_many,
                        std::vector<int64_t>& st, std::vector<int32_t>& ln, std::vector<int32_t>* grp, int64_t& lo, int64_t& hi, char* errbuf,
                        size_t errlen) {
    if (n_seg < 0 || n_groups < 0 || seqlen < 0 || !group_off || !sums || (seqlen > 0 && !seq) || (n_seg > 0 && (!starts || !ends))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    if (group_off[0] != 0 || group_off[n_groups] != n_seg) { set_err(errbuf, errlen, std::string(who) + ": the groups do not cover the segments"); return SD_ERR_PARAM; }
    if (n_seg >= seg_limit) { set_err(errbuf, errlen, std::string(who) + ": " + too_many); return SD_ERR_UNSUPPORTED; }
    st.resize((size_t)n_seg);
    ln.resize((size_t)n_seg);
    lo = seqlen;
    hi = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        if (starts[s] < 0 || ends[s] >= seqlen) { set_err(errbuf, errlen, std::string(who) + ": segment " + std::to_string(s) + " lies outside the text"); return SD_ERR_PARAM; }
        const int64_t l = std::max<int64_t>(0, ends[s] - starts[s] + 1);
        if (l >= ((int64_t)1 << 27)) { set_err(errbuf, errlen, std::string(who) + ": a segment of 2^27 bases or more"); return SD_ERR_UNSUPPORTED; }
        ln[(size_t)s] = (int32_t)l;
        if (l > 0) { lo = std::min(lo, starts[s]); hi = std::max(hi, ends[s] + 1); }
    }
    if (hi < lo) { lo = 0; hi = 0; }
    for (int64_t s = 0; s < n_seg; ++s) st[(size_t)s] = ln[(size_t)s] > 0 ? starts[s] - lo : 0;
    if (grp) {
        grp->assign((size_t)n_seg, 0);
        for (int32_t g = 0; g < n_groups; ++g)   // (offsets out of order are refused later: stay inside the segments)
            for (int64_t s = std::max<int64_t>(0, group_off[g]); s < std::min(n_seg, group_off[g + 1]); ++s) (*grp)[(size_t)s] = g;
    }
    return SD_OK;
}

// A table of `cols` columns of n_reads + 1 int64 (the last row is the terminator), pinned and on the device.  The caller
// fills the columns h(0 .. cols) and uploads; the kernels read d(0 .. cols).
struct ReadTable {
    PinBuf<int64_t> h_reads;
    DevBuf<int64_t> reads;
    size_t nr = 0;
    void shape(int cols, int32_t n_reads) {
        nr = (size_t)n_reads + 1;
        h_reads.alloc((size_t)cols * nr);
        reads.alloc((size_t)cols * nr);
    }
    int64_t* h(int col) { return h_reads.p + (size_t)col * nr; }
    const int64_t* d(int col) const { return reads.p + (size_t)col * nr; }
    void upload(int cols, hipStream_t st) { SD_HIP(hipMemcpyAsync(reads.p, h_reads.p, (size_t)cols * nr * sizeof(int64_t), hipMemcpyHostToDevice, st)); }
};

// the text arguments of a reads call (k-mer analyses); no_output: the caller's own "an output is missing"
inline int reads_text_args(const char* who, const void* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, bool no_output,
                           char* errbuf, size_t errlen) {
    int64_t bases = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        if (!read_off || read_off[r] < 0) { set_err(errbuf, errlen, std::string(who) + ": missing or negative read offset"); return SD_ERR_PARAM; }
        bases += read_lens[r];
    }
    if ((bases > 0 && !text) || no_output) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    return SD_OK;
}

// The reads of a host-memory call up into dst on st, back to back, whatever their order and gaps in the caller's buffer
// -> where each lies in dst (n_reads + 1: the last entry is the bases of all)
inline std::vector<int64_t> reads_upload(DevBuf<uint8_t>& dst, hipStream_t st, const char* text, const int64_t* read_off, const int64_t* read_lens,
                                         int32_t n_reads) {
    std::vector<int64_t> off((size_t)n_reads + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) off[(size_t)r + 1] = off[(size_t)r] + read_lens[r];
    dst.alloc((size_t)off[(size_t)n_reads]);
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_lens[r] > 0)
            SD_HIP(hipMemcpyAsync(dst.p + off[(size_t)r], text + read_off[r], (size_t)read_lens[r], hipMemcpyHostToDevice, st));
    return off;
}

// ---- a call on final rows in device memory: the reads as [roff | rlen | toff] and their text back to back ----------------
struct FinalText : ReadTable {
    DevBuf<uint8_t> text;   // 8 zero bytes behind the last base
    const int64_t* rlen() const { return d(1); }
    const int64_t* toff() const { return d(2); }
};

// the read table of the caller checked; text = the bases of all reads
inline int final_reads_args(const char* who, const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, int64_t& text,
                            char* errbuf, size_t errlen) {
    text = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_off[r] < 0 || read_lens[r] < 0) { set_err(errbuf, errlen, std::string(who) + ": negative read offset or length"); return SD_ERR_PARAM; }
        text += read_lens[r];
    }
    if (text > 0 && !d_text) { set_err(errbuf, errlen, std::string(who) + ": missing text"); return SD_ERR_PARAM; }
    return SD_OK;
}

// table up, the reads of d_text gathered into t.text on st
inline void final_text_gather(FinalText& t, hipStream_t st, const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                              int64_t text) {
    t.shape(3, n_reads);
    t.text.alloc((size_t)text + 8);
    int64_t *roff = t.h(0), *rlen = t.h(1), *toff = t.h(2);
    int64_t at = 0;
    for (int32_t r = 0; r < n_reads; ++r) { roff[r] = read_off[r]; rlen[r] = read_lens[r]; toff[r] = at; at += read_lens[r]; }
    roff[n_reads] = 0; rlen[n_reads] = 0; toff[n_reads] = at;
    t.upload(3, st);
    SD_HIP(hipMemsetAsync(t.text.p + text, 0, 8, st));
    sd::launch_text_gather(st, static_cast<const uint8_t*>(d_text), t.d(0), t.toff(), (int)n_reads, text, t.text.p);
}

// The stream of a call on host memory: the call's own, waited for and destroyed when the call leaves, however it leaves.
// (A call that reads results synchronises itself first and reports that error; this wait is for the other exits.)
struct OwnedStream {
    hipStream_t st = nullptr;
    OwnedStream() { SD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    operator hipStream_t() const { return st; }
};

// The timed repetitions of a bench entry's stages.  time(): warmup + reps rounds of body() between two events on st, the
// rounds from `warmup` on into ms[]; before() runs ahead of each round, untimed.
struct StageClock {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    StageClock() = default;
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
    ~StageClock() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    template <class Body, class Before>
    void time(hipStream_t st, int warmup, int reps, float* ms, Body body, Before before) {
        ensure_event(e0);
        ensure_event(e1);
        for (int it = 0; it < warmup + reps; ++it) {
            before();
            SD_HIP(hipEventRecord(e0, st));
            body();
            SD_HIP(hipEventRecord(e1, st));
            SD_HIP(hipEventSynchronize(e1));
            if (it >= warmup) SD_HIP(hipEventElapsedTime(&ms[it - warmup], e0, e1));
        }
    }
    template <class Body>
    void time(hipStream_t st, int warmup, int reps, float* ms, Body body) { time(st, warmup, reps, ms, body, [] {}); }
};

// f(std::integral_constant<int, K>) for the word classes of the pair walks: 1, 2, 3, 4, 6, 8 (anything else: 8)
template <class F>
void with_words(int K, F&& f) {
    switch (K) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}

}  // namespace sdi
