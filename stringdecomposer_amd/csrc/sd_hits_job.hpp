// sd_hits_job.hpp -- internal to libsd_hip.so: the frame of a hit search over the bit planes of the reads (sd_motif.hip,
// sd_motif_edit.hip), on top of sd_job_dev.hpp.  A search counts its hits per (read, pattern-strand, tile) item in launches
// of at most LAUNCH_WG (tile, pattern block) units, scan_bases turns the counts into bases, per[read][motif][strand] is
// derived from them, and the units are run again to write 16-byte records from each item's base on.  Everything around the
// kernels' inner work is here, once: the checks and their texts, the work area with the size / write handshake, setup,
// prep, the launch loop, both passes, the host form's collection and the bodies of the five entries.  DESIGN.md, "The frame
// of an analysis", says what a search brings.  A search is described by a struct S:
//   Set, Hit, Args       the compiled request, the 16-byte record, the kernels' argument block.  Args has the fields the
//                        frame fills: lo hi v, rlen pw tile_off, n_reads n_ps n_psb, unit0 n_units, cnt base cap
//   PB, LAUNCH_WG        pattern-strands of a unit, units of a launch
//   size_entry           the name of its size entry, for the write entry's refusal
//   launches             its launch counter (std::atomic<int64_t>)
//   compile(patterns, n_motifs, budget, set, err), strands(set), n_motifs(set), tiles(n)
//   Request              the request's device and pinned buffers; upload(set, st, a) sends it and sets its fields of a
//   size(set, grid, st, a), write(set, grid, st, a, hits)   one launch of `grid` units
//   host_item(set, planes, n, r, q, out)   the hits of pattern-strand q on read r, by start
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "sd_motif.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"
#include "sd_scan_dev.hpp"

namespace sd {

// The unit of a workgroup into the search's own lane struct (r ps0 nq, n item0 tiles_r): its pattern block [ps0, ps0 + nq),
// its read r of n bases and tile tl of that read.  The item of pattern-strand ps is item0 + ps * tiles_r.  false: nothing to
// do.  (The fields stay in the search's struct, in its order: a shared base struct changed sd_motif_edit_write's registers.
// The size kernels' tail -- wave sum, LDS, the store of cnt -- stays in each kernel for the same reason: shared, it changed
// sd_motif_size's scalar registers and schedule.)
template <int PB, class Args, class Lane>
__device__ inline bool hits_unit(const Args& a, Lane& l, int64_t& tl) {
    const int64_t u = a.unit0 + blockIdx.x;
    if (u >= a.n_units) return false;
    const int64_t tile = u / a.n_psb;
    l.ps0 = (int)(u - tile * a.n_psb) * PB;
    l.nq = a.n_ps - l.ps0 < PB ? a.n_ps - l.ps0 : PB;
    int r = 0, rb = a.n_reads;   // the read of the tile: the last one whose tiles start at or before it
    while (rb - r > 1) {
        const int m = (r + rb) >> 1;
        if (a.tile_off[m] <= tile) r = m; else rb = m;
    }
    l.r = r;
    l.n = a.rlen[r];
    l.tiles_r = a.tile_off[r + 1] - a.tile_off[r];
    tl = tile - a.tile_off[r];
    l.item0 = (int64_t)a.n_ps * a.tile_off[r] + tl;
    return true;
}

// per[(r * n_motifs + motif) * 2 + strand] = the hits of the items of (read r, pattern-strand).  tag[ps * STRIDE] = motif |
// strand << 16 of pattern-strand ps.  (A template, as the kernels of sd_scan_dev.hpp are: each unit holds its own copy.)
template <int STRIDE>
__global__ void sd_hits_per(const int* tag, const int64_t* tile_off, const int64_t* base, int n_reads, int n_ps, int n_motifs, int64_t* per) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (int64_t)n_reads * n_ps) return;
    const int r = (int)(x / n_ps), ps = (int)(x - (int64_t)r * n_ps);
    const int64_t tiles_r = tile_off[r + 1] - tile_off[r], i0 = (int64_t)n_ps * tile_off[r] + ps * tiles_r;
    const int t = tag[(int64_t)ps * STRIDE];
    per[((int64_t)r * n_motifs + (t & 0xffff)) * 2 + (t >> 16)] = base[i0 + tiles_r] - base[i0];
}

}  // namespace sd

namespace sdi {

// Per device and search, kept between calls (sd_job_dev.hpp: DevWork): the planes, the per-read tables
// [roff | rlen | pw | tile_off], the request, the items' counts and bases, and what the last size call was for (the write
// call must match it).
template <class S>
struct HitsCtx : DevWork, ReadTable {
    DevBuf<uint64_t> planes;
    DevBuf<uint8_t> text;        // the _dev entry: the reads, back to back
    typename S::Request req;
    DevBuf<int32_t> cnt;
    DevBuf<int64_t> base, per;
    DevBuf<uint4> hits;          // the _dev entry
    PinBuf<int64_t> h_total;
    typename S::Args a{};
    bool sized = false;
    const void* s_text = nullptr;
    int s_device = -1;
    std::vector<int64_t> s_off, s_len;
    std::string s_key;
    int64_t s_total = 0;
};

inline std::string hits_key(const char* const* patterns, int32_t n_motifs, int32_t budget) {
    std::string k = std::to_string(budget);
    for (int32_t m = 0; m < n_motifs; ++m) { k += '|'; k += patterns[m]; }
    return k;
}

// the request and the reads checked, before any device work; tiles / items / words of the call
template <class S>
struct HitsJob {
    typename S::Set set;
    std::vector<int64_t> tile_off, pw;
    int64_t tiles = 0, items = 0, words = 0, bases = 0;
};
template <class S>
int hits_job(const char* who, const char* const* patterns, int32_t n_motifs, int32_t budget, const int64_t* read_lens, int32_t n_reads,
             HitsJob<S>& j, char* errbuf, size_t errlen) {
    std::string err;
    if (n_motifs > 0 && !patterns) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    if (!S::compile(patterns, n_motifs, budget, j.set, err)) { set_err(errbuf, errlen, std::string(who) + ": " + err); return SD_ERR_PARAM; }
    if (n_reads < 0 || (n_reads > 0 && !read_lens)) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    j.tile_off.assign((size_t)n_reads + 1, 0);
    j.pw.assign((size_t)n_reads + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] < 0 || read_lens[r] >= ((int64_t)1 << 40)) { set_err(errbuf, errlen, std::string(who) + ": a negative read length, or one of 2^40 bases or more"); return SD_ERR_PARAM; }
        j.tile_off[(size_t)r] = j.tiles;
        j.pw[(size_t)r] = j.words;
        j.tiles += S::tiles(read_lens[r]);
        j.words += sd::autocorr_plane_words(read_lens[r]);
        j.bases += read_lens[r];
    }
    j.tile_off[(size_t)n_reads] = j.tiles;
    j.pw[(size_t)n_reads] = j.words;
    const int64_t n_ps = (int64_t)S::strands(j.set).size();
    if (j.tiles > sd::MOTIF_ITEMS_MAX / n_ps) {
        set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(j.tiles) + " read tiles x " + std::to_string(n_ps) + " pattern-strands, the cap is " +
                                    std::to_string(sd::MOTIF_ITEMS_MAX) + " items (MOTIF_ITEMS_MAX): use fewer reads or fewer motifs per call");
        return SD_ERR_PARAM;
    }
    j.items = j.tiles * n_ps;
    return SD_OK;
}
inline int hits_cap(const char* who, int64_t total, char* errbuf, size_t errlen) {
    if (total <= sd::MOTIF_HITS_MAX) return SD_OK;
    set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(total) + " hits, the cap is " + std::to_string(sd::MOTIF_HITS_MAX) +
                                " (MOTIF_HITS_MAX): use fewer reads or fewer motifs per call");
    return SD_ERR_PARAM;
}

// ---- the host form: the items by S::host_item, then hits in canonical order (malloc'ed) and per --------------------------
template <class S>
int hits_host(const char* who, const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
              int32_t n_motifs, int32_t budget, int32_t threads, typename S::Hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
              size_t errlen) {
    using Hit = typename S::Hit;
    HitsJob<S> j;
    int rc = hits_job<S>(who, patterns, n_motifs, budget, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, text, read_off, read_lens, n_reads, !hits || !n_hits || (n_reads > 0 && !per), errbuf, errlen))) return rc;
    threads = std::max(1, threads);
    const std::vector<sd::MotifStrand>& ps = S::strands(j.set);
    const int64_t n_ps = (int64_t)ps.size();
    const size_t nm = (size_t)S::n_motifs(j.set);
    std::vector<sd::AutocorrPlanes> planes((size_t)n_reads);
    sd::parallel_for(n_reads, threads, 1, [&](int64_t r) { planes[(size_t)r].build(reinterpret_cast<const uint8_t*>(text) + read_off[r], read_lens[r]); });
    std::vector<std::vector<Hit>> found((size_t)(n_reads * n_ps));   // (read, pattern-strand): the canonical order
    sd::parallel_for(n_reads * n_ps, threads, 1, [&](int64_t it) {
        const int32_t r = (int32_t)(it / n_ps);
        S::host_item(j.set, planes[(size_t)r], read_lens[r], r, (size_t)(it - r * n_ps), found[(size_t)it]);
    });
    int64_t total = 0;
    std::vector<int64_t> at(found.size() + 1, 0);
    for (size_t i = 0; i < found.size(); ++i) { at[i] = total; total += (int64_t)found[i].size(); }
    if ((rc = hits_cap(who, total, errbuf, errlen))) return rc;
    std::memset(per, 0, sizeof(int64_t) * (size_t)n_reads * nm * 2);
    Hit* out = static_cast<Hit*>(std::malloc(sizeof(Hit) * (size_t)std::max<int64_t>(total, 1)));
    if (!out) throw std::bad_alloc();
    sd::parallel_for((int64_t)found.size(), threads, 8, [&](int64_t i) {
        if (!found[(size_t)i].empty()) std::memcpy(out + at[(size_t)i], found[(size_t)i].data(), sizeof(Hit) * found[(size_t)i].size());
    });
    for (size_t i = 0; i < found.size(); ++i) {
        const sd::MotifStrand& q = ps[i % (size_t)n_ps];
        per[((i / (size_t)n_ps) * nm + (size_t)q.motif) * 2 + (size_t)q.strand] = (int64_t)found[i].size();
    }
    *hits = out;
    *n_hits = total;
    return SD_OK;
}

// ---- the device passes --------------------------------------------------------------------------------------------------
// tables and request up on st; c.a ready for the launches.  d_text + roff[r] = read r.
template <class S>
void hits_setup(HitsCtx<S>& c, hipStream_t st, const HitsJob<S>& j, const int64_t* roff, const int64_t* read_lens, int32_t n_reads) {
    const int n_ps = (int)S::strands(j.set).size();
    c.shape(4, n_reads);
    int64_t *h_off = c.h(0), *h_len = c.h(1), *h_pw = c.h(2), *h_tile = c.h(3);
    for (int32_t r = 0; r < n_reads; ++r) { h_off[r] = roff[r]; h_len[r] = read_lens[r]; h_pw[r] = j.pw[(size_t)r]; h_tile[r] = j.tile_off[(size_t)r]; }
    h_off[n_reads] = 0; h_len[n_reads] = 0; h_pw[n_reads] = j.words; h_tile[n_reads] = j.tiles;
    c.upload(4, st);
    typename S::Args& a = c.a;
    a = typename S::Args{};
    c.req.upload(j.set, st, a);
    c.planes.alloc(3 * (size_t)j.words);
    c.cnt.alloc((size_t)j.items);
    c.base.alloc((size_t)j.items + 1);
    c.h_total.alloc(1);
    uint64_t* lo = c.planes.p;
    a.lo = lo; a.hi = lo + j.words; a.v = lo + 2 * j.words;
    a.rlen = c.d(1); a.pw = c.d(2); a.tile_off = c.d(3);
    a.n_reads = (int)n_reads; a.n_ps = n_ps; a.n_psb = (n_ps + S::PB - 1) / S::PB;
    a.n_units = j.tiles * a.n_psb;
    a.cnt = c.cnt.p; a.base = c.base.p;
}

template <class S>
void hits_prep(HitsCtx<S>& c, hipStream_t st, const uint8_t* d_text, const HitsJob<S>& j, int32_t n_reads) {
    if (j.words == 0 || n_reads == 0) return;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((j.words + 3) / 4, (int64_t)c.n_cu * 32));
    sd::launch_autocorr_prep(st, grid, d_text, c.d(0), c.d(1), c.d(2), (int)n_reads, j.words, c.planes.p, c.planes.p + j.words, c.planes.p + 2 * j.words);
    SD_HIP(hipGetLastError());
}

template <class S, class Launch>
void hits_units(HitsCtx<S>& c, Launch&& launch) {
    int64_t launches = 0;
    for (int64_t u0 = 0; u0 < c.a.n_units; u0 += S::LAUNCH_WG) {
        c.a.unit0 = u0;
        launch((unsigned)std::min<int64_t>(S::LAUNCH_WG, c.a.n_units - u0));
        SD_HIP(hipGetLastError());
        ++launches;
    }
    S::launches.fetch_add(launches);
}

// counts, scan, per (d_per: n_reads x n_motifs x 2) and the total on its way to c.h_total; nothing waits
template <class S>
void hits_size(HitsCtx<S>& c, hipStream_t st, const HitsJob<S>& j, int32_t n_reads, int64_t* d_per) {
    hits_units(c, [&](unsigned grid) { S::size(j.set, grid, st, c.a); });
    hipLaunchKernelGGL(sd::scan_bases<int32_t>, dim3(1), dim3(sd::SCAN_T), 0, st, c.cnt.p, j.items, c.base.p);
    SD_HIP(hipGetLastError());
    const int n_motifs = S::n_motifs(j.set);
    const int64_t cells = (int64_t)n_reads * n_motifs * 2, rp = (int64_t)n_reads * c.a.n_ps;
    if (cells) {
        SD_HIP(hipMemsetAsync(d_per, 0, sizeof(int64_t) * (size_t)cells, st));   // (the - strand of a palindrome has no item)
        constexpr int stride = (int)(sizeof(*c.a.ps) / sizeof(int));
        hipLaunchKernelGGL(sd::sd_hits_per<stride>, dim3((unsigned)((rp + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const int*>(c.a.ps) + 1,
                           c.a.tile_off, c.a.base, c.a.n_reads, c.a.n_ps, n_motifs, d_per);
        SD_HIP(hipGetLastError());
    }
    SD_HIP(hipMemcpyAsync(c.h_total.p, c.base.p + j.items, sizeof(int64_t), hipMemcpyDeviceToHost, st));
}

template <class S>
void hits_write(HitsCtx<S>& c, hipStream_t st, const HitsJob<S>& j, uint4* d_hits, int64_t cap) {
    c.a.cap = cap;
    hits_units(c, [&](unsigned grid) { S::write(j.set, grid, st, c.a, d_hits); });
}

struct HitsBench {
    int warmup, reps;
    float *ms_prep, *ms_size, *ms_write;
    int64_t* info;
};

// the reads of host memory: up, both passes, hits (malloc'ed) and per back
template <class S>
int hits_dev(const char* who, const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
             int32_t n_motifs, int32_t budget, int32_t device, typename S::Hit** hits, int64_t* n_hits, int64_t* per, char* errbuf, size_t errlen,
             const HitsBench* bench = nullptr) {
    using Hit = typename S::Hit;
    HitsJob<S> j;
    int rc = hits_job<S>(who, patterns, n_motifs, budget, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, text, read_off, read_lens, n_reads, !hits || !n_hits || (n_reads > 0 && !per), errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    const size_t cells = (size_t)n_reads * (size_t)S::n_motifs(j.set) * 2;
    try {
        DeviceScope on(device);
        HitsCtx<S>& c = device_ctx<HitsCtx<S>>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        c.sized = false;
        OwnedStream st;
        c.per.alloc(cells);
        const std::vector<int64_t> off = reads_upload(c.text, st, text, read_off, read_lens, n_reads);
        hits_setup(c, st, j, off.data(), read_lens, n_reads);
        StageClock clock;
        if (bench) {
            clock.time(st, bench->warmup, bench->reps, bench->ms_prep, [&]() { hits_prep(c, st, c.text.p, j, n_reads); });
            clock.time(st, bench->warmup, bench->reps, bench->ms_size, [&]() { hits_size(c, st, j, n_reads, c.per.p); });
        } else {
            hits_prep(c, st, c.text.p, j, n_reads);
            hits_size(c, st, j, n_reads, c.per.p);
        }
        c.in_flight(st);
        SD_HIP(hipStreamSynchronize(st));
        c.waited();
        const int64_t total = c.h_total.p[0];
        if ((rc = hits_cap(who, total, errbuf, errlen))) return rc;
        c.hits.alloc((size_t)total);
        Hit* out = static_cast<Hit*>(std::malloc(sizeof(Hit) * (size_t)std::max<int64_t>(total, 1)));
        if (!out) throw std::bad_alloc();
        struct Free { Hit* p; ~Free() { std::free(p); } } keep{out};
        if (bench) {
            const int64_t before = S::launches.load();
            clock.time(st, bench->warmup, bench->reps, bench->ms_write, [&]() { hits_write(c, st, j, c.hits.p, total); });
            bench->info[0] = (S::launches.load() - before) / (bench->warmup + bench->reps);
            bench->info[1] = j.items;
            bench->info[2] = total;
            bench->info[3] = j.words;
        } else {
            hits_write(c, st, j, c.hits.p, total);
        }
        c.in_flight(st);
        if (total) SD_HIP(hipMemcpyAsync(out, c.hits.p, sizeof(Hit) * (size_t)total, hipMemcpyDeviceToHost, st));
        if (cells) SD_HIP(hipMemcpyAsync(per, c.per.p, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));
        c.waited();
        keep.p = nullptr;
        *hits = out;
        *n_hits = total;
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
}

// the reads of device memory, the size pass: per filled on the caller's stream, the number of hits waited for
template <class S>
int hits_reads_size_dev(const char* who, const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                        const char* const* patterns, int32_t n_motifs, int32_t budget, int32_t device, void* hip_stream, int64_t* d_per,
                        int64_t* n_hits, char* errbuf, size_t errlen) {
    HitsJob<S> j;
    int rc = hits_job<S>(who, patterns, n_motifs, budget, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, d_text, read_off, read_lens, n_reads, !n_hits || (n_reads > 0 && !d_per), errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        if (n_reads > 0 && (rc = buffer_on_device(d_per, device, who, "per", errbuf, errlen))) return rc;
        if (j.bases > 0 && (rc = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return rc;
        HitsCtx<S>& c = device_ctx<HitsCtx<S>>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();   // the previous call's kernels read the buffers this one overwrites
        c.sized = false;
        hits_setup(c, st, j, read_off, read_lens, n_reads);
        hits_prep(c, st, static_cast<const uint8_t*>(d_text), j, n_reads);
        hits_size(c, st, j, n_reads, d_per);
        c.in_flight(st);
        SD_HIP(hipStreamSynchronize(st));   // the 8 bytes of the total: the call's only wait
        c.waited();
        *n_hits = c.h_total.p[0];
        if ((rc = hits_cap(who, *n_hits, errbuf, errlen))) return rc;
        c.sized = true;
        c.s_text = d_text;
        c.s_device = device;
        c.s_off.assign(read_off, read_off + n_reads);
        c.s_len.assign(read_lens, read_lens + n_reads);
        c.s_key = hits_key(patterns, n_motifs, budget);
        c.s_total = *n_hits;
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
}

// the write pass of the size call before it: the records into d_hits on the caller's stream, nothing waits
template <class S>
int hits_reads_write_dev(const char* who, const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                         const char* const* patterns, int32_t n_motifs, int32_t budget, int32_t device, void* hip_stream, typename S::Hit* d_hits,
                         int64_t cap, char* errbuf, size_t errlen) {
    HitsJob<S> j;
    int rc = hits_job<S>(who, patterns, n_motifs, budget, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, d_text, read_off, read_lens, n_reads, false, errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        HitsCtx<S>& c = device_ctx<HitsCtx<S>>(device);
        std::lock_guard<std::mutex> g(c.m);
        if (!c.sized || c.s_text != d_text || c.s_device != device || (int32_t)c.s_off.size() != n_reads ||
            !std::equal(c.s_off.begin(), c.s_off.end(), read_off) || !std::equal(c.s_len.begin(), c.s_len.end(), read_lens) ||
            c.s_key != hits_key(patterns, n_motifs, budget)) {
            set_err(errbuf, errlen, std::string(who) + ": the last " + S::size_entry + " call on this device was not for these reads and motifs");
            return SD_ERR_PARAM;
        }
        if (cap < c.s_total) {
            set_err(errbuf, errlen, std::string(who) + ": capacity " + std::to_string(cap) + " records, the hits need " + std::to_string(c.s_total));
            return SD_ERR_PARAM;
        }
        if (c.s_total == 0) return SD_OK;
        if (!d_hits) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
        if ((rc = buffer_on_device(d_hits, device, who, "hit", errbuf, errlen))) return rc;
        hits_write(c, st, j, reinterpret_cast<uint4*>(d_hits), c.s_total);
        c.in_flight(st);   // (the kernels read the work area: the next size call on the device settles first)
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
}

// the stages of hits_dev, timed
template <class S>
int hits_kernel_bench(const char* who, const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                      const char* const* patterns, int32_t n_motifs, int32_t budget, int32_t device, int32_t warmup, int32_t reps, float* ms_prep,
                      float* ms_size, float* ms_write, int64_t info[4]) {
    if (warmup < 0 || reps < 1 || !ms_prep || !ms_size || !ms_write || !info || n_reads <= 0) return SD_ERR_PARAM;
    for (int i = 0; i < 4; ++i) info[i] = 0;
    const HitsBench b{warmup, reps, ms_prep, ms_size, ms_write, info};
    typename S::Hit* hits = nullptr;
    int64_t n_hits = 0;
    std::vector<int64_t> per((size_t)n_reads * (size_t)std::max(n_motifs, 1) * 2);
    const int rc = hits_dev<S>(who, text, read_off, read_lens, n_reads, patterns, n_motifs, budget, device, &hits, &n_hits, per.data(), nullptr, 0, &b);
    std::free(hits);
    return rc;
}

}  // namespace sdi
