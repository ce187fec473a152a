// sd_motif_edit.hip -- IUPAC motif hits with insertions and deletions (--motif-edits): a CENP-B box that a noisy read
// holds with an indel.  sd_motif_edit.hpp holds the rule and everything host and device compute alike; this file holds the
// kernels, the host form and the C-ABI (include/sd_hip.h: sd_motif_edit_*).
//   sd_autocorr_prep     (sd_autocorr.hip, through launch_autocorr_prep) the byte text -> the bit planes lo | hi | valid
//   sd_motif_edit_size   a workgroup (256 lanes) per (tile of 256 stretches of a read, block of MOTIF_EDIT_PB
//                        pattern-strands).  A lane owns a stretch of MOTIF_EDIT_STRETCH consecutive ends.  Per
//                        pattern-strand -- its header and five match words are the same in every lane and come through
//                        scalar loads -- the lane runs Myers' bit-vector column with the search boundary over the L + K
//                        bases before its stretch (never before the read's first base), its stretch, and one base more,
//                        on one 32-bit word for L <= 32 and one 64-bit word above (motif_edit_scan), and counts the ends
//                        the rule takes.  The workgroup's sum is the int32 count of the item (read, pattern-strand,
//                        tile), laid out in canonical order.
//   scan_bases           (sd_scan_dev.hpp) one workgroup: the items' bases and the total
//   sd_motif_edit_per    per[read][motif][strand] from the bases
//   sd_motif_edit_write  the work item of the size kernel again, for the items with a count: the lane recomputes its hits
//                        as a bit mask over its stretch, the lanes' counts are scanned within the workgroup, and for each
//                        hit the owning lane runs the recurrence anchored at the end backwards over the reversed pattern
//                        for start and edits (motif_edit_start) and stores one 16-byte record.
// No atomics anywhere: the hit array is a function of the input.  A launch takes at most MOTIF_EDIT_LAUNCH_WG work items.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "sd_motif_edit.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"
#include "sd_scan_dev.hpp"

static_assert(sizeof(sd_motif_edit_hit) == 16, "a hit is one 16-byte store");
static_assert(SD_MOTIF_KMAX == sd::MOTIF_EDIT_KMAX && SD_MOTIF_EDIT_TILE_WORDS == sd::MOTIF_EDIT_TILE_WORDS, "include/sd_hip.h states the limits");
static_assert(sd::MOTIF_LMAX + sd::MOTIF_EDIT_KMAX <= 255, "the matched length is one byte of the record");

namespace sd {

constexpr int ME_T = MOTIF_EDIT_LANES;
constexpr int ME_SW = MOTIF_EDIT_STRETCH_WORDS;
static_assert(ME_T == SCAN_T, "block_scan scans a workgroup of SCAN_T lanes");

struct MeArgs {
    const uint64_t *lo, *hi, *v;                 // the planes of the job
    const int64_t *rlen, *pw, *tile_off;         // per read (pw, tile_off: n_reads + 1)
    int n_reads, n_ps, n_psb, K;
    const int2* ps;                              // per pattern-strand {L, motif | strand << 16}
    const uint64_t* eq;                          // MOTIF_EDIT_WORDS per pattern-strand
    int64_t unit0, n_units;                      // the launch: its first (tile, pattern block) unit
    int32_t* cnt;                                // per item
    const int64_t* base;                         // per item + 1: the scan
    int64_t cap;
};

// The unit of a workgroup: its read, the planes of that read and the lane's stretch [a, a + MOTIF_EDIT_STRETCH).
struct MeLane {
    int r, ps0, nq;
    int64_t n, a, item0, tiles_r;   // item of pattern-strand ps: item0 + ps * tiles_r
    const uint64_t *lo, *hi, *v;    // word 0 of the read
};
__device__ inline bool me_lane(const MeArgs& a, MeLane& l) {
    const int64_t u = a.unit0 + blockIdx.x;
    if (u >= a.n_units) return false;
    const int64_t tile = u / a.n_psb;
    l.ps0 = (int)(u - tile * a.n_psb) * MOTIF_EDIT_PB;
    l.nq = a.n_ps - l.ps0 < MOTIF_EDIT_PB ? a.n_ps - l.ps0 : MOTIF_EDIT_PB;
    int r = 0, rb = a.n_reads;   // the read of the tile: the last one whose tiles start at or before it
    while (rb - r > 1) {
        const int m = (r + rb) >> 1;
        if (a.tile_off[m] <= tile) r = m; else rb = m;
    }
    l.r = r;
    l.n = a.rlen[r];
    l.tiles_r = a.tile_off[r + 1] - a.tile_off[r];
    const int64_t tl = tile - a.tile_off[r];
    l.item0 = (int64_t)a.n_ps * a.tile_off[r] + tl;
    l.a = tl * MOTIF_EDIT_TILE + (int64_t)threadIdx.x * MOTIF_EDIT_STRETCH;   // (at or behind n: the scan does nothing)
    const int64_t x = a.pw[r];
    l.lo = a.lo + x; l.hi = a.hi + x; l.v = a.v + x;
    return true;
}

// the header and the match words of pattern-strand ps, word by word so that each is a scalar load
struct MeHead {
    int L, tag;
};
__device__ inline MeHead me_head(const MeArgs& a, int ps) {
    const int* h = reinterpret_cast<const int*>(a.ps + ps);
    return MeHead{motif_request_word(h), motif_request_word(h + 1)};
}
template <class W>
__device__ inline MotifEditEq<W> me_words(const MeArgs& a, int ps, bool reversed) {
    return motif_edit_words<W>(a.eq + (int64_t)ps * MOTIF_EDIT_WORDS + (reversed ? MOTIF_EDIT_CLASSES : 0));
}

template <class W>
__device__ inline int me_count(const MeArgs& a, const MeLane& l, int ps, int L) {
    const MotifEditEq<W> eq = me_words<W>(a, ps, false);
    int c = 0;
    motif_edit_scan<W>(l.lo, l.hi, l.v, l.n, l.a, l.a + MOTIF_EDIT_STRETCH, eq, L, a.K, [&](int64_t) { ++c; });
    return c;
}

__global__ __launch_bounds__(ME_T) void sd_motif_edit_size(MeArgs a) {
    __shared__ int wsum[MOTIF_EDIT_PB][ME_T / 64];
    MeLane l;
    if (!me_lane(a, l)) return;
    for (int q = 0; q < l.nq; ++q) {
        const MeHead P = me_head(a, l.ps0 + q);
        int c = P.L <= 32 ? me_count<uint32_t>(a, l, l.ps0 + q, P.L) : me_count<uint64_t>(a, l, l.ps0 + q, P.L);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if ((threadIdx.x & 63) == 0) wsum[q][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x < l.nq) {
        int s = 0;
        for (int w = 0; w < ME_T / 64; ++w) s += wsum[threadIdx.x][w];
        a.cnt[l.item0 + (int64_t)(l.ps0 + (int)threadIdx.x) * l.tiles_r] = s;
    }
}

// the hits of the lane's stretch as a mask, bit p - l.a of word (p - l.a) / 64
template <class W>
__device__ inline void me_mask(const MeArgs& a, const MeLane& l, int ps, int L, uint64_t* hm) {
    const MotifEditEq<W> eq = me_words<W>(a, ps, false);
    motif_edit_scan<W>(l.lo, l.hi, l.v, l.n, l.a, l.a + MOTIF_EDIT_STRETCH, eq, L, a.K, [&](int64_t p) {
        const int x = (int)(p - l.a);
#pragma unroll
        for (int k = 0; k < ME_SW; ++k)   // (unrolled: the mask stays in registers)
            hm[k] |= k == (x >> 6) ? (uint64_t)1 << (x & 63) : 0;
    });
}
// the records of the mask from hits[o] on
template <class W>
__device__ inline void me_records(const MeArgs& a, const MeLane& l, int ps, const MeHead& P, const uint64_t* hm, int64_t o, uint4* __restrict__ hits) {
    const MotifEditEq<W> eq = me_words<W>(a, ps, true);
    const uint32_t tag = (uint32_t)P.tag;   // motif | strand << 16
#pragma unroll
    for (int k = 0; k < ME_SW; ++k) {   // (unrolled: the mask stays in registers)
        uint64_t h = hm[k];
        while (h) {
            const int bit = __ffsll((unsigned long long)h) - 1;
            h &= h - 1;
            const int64_t j = l.a + 64 * k + bit + 1;
            int len, ed;
            motif_edit_start<W>(P.L, a.K, j, [&](int64_t p) { return motif_edit_eq_at<W>(l.lo, l.hi, l.v, p, eq); }, &len, &ed);
            const int64_t start = j - len;
            if (o < a.cap)   // (the capacity was checked against the total: never taken)
                hits[o] = make_uint4((uint32_t)start, (uint32_t)(start >> 32), (uint32_t)l.r,
                                     (tag & 0xffff) | (uint32_t)len << 16 | (uint32_t)ed << 24 | (tag >> 16) << 31);
            ++o;
        }
    }
}

// (hits is a parameter of its own so that it can be __restrict__, as in sd_motif_write)
__global__ __launch_bounds__(ME_T) void sd_motif_edit_write(MeArgs a, uint4* __restrict__ hits) {
    MeLane l;
    if (!me_lane(a, l)) return;
    for (int q = 0; q < l.nq; ++q) {
        const int64_t item = l.item0 + (int64_t)(l.ps0 + q) * l.tiles_r;
        if (motif_request_word(a.cnt + item) == 0) continue;   // (the same in every lane; the size pass wrote it, this kernel does not)
        const MeHead P = me_head(a, l.ps0 + q);
        uint64_t hm[ME_SW];
        for (int k = 0; k < ME_SW; ++k) hm[k] = 0;
        if (P.L <= 32) me_mask<uint32_t>(a, l, l.ps0 + q, P.L, hm); else me_mask<uint64_t>(a, l, l.ps0 + q, P.L, hm);
        int c = 0, total;
        for (int k = 0; k < ME_SW; ++k) c += __popcll(hm[k]);
        const int64_t o = motif_request_word(a.base + item) + block_scan<int>(c, &total);
        if (P.L <= 32) me_records<uint32_t>(a, l, l.ps0 + q, P, hm, o, hits); else me_records<uint64_t>(a, l, l.ps0 + q, P, hm, o, hits);
    }
}

// per[(r * n_motifs + motif) * 2 + strand] = the hits of the items of (read r, pattern-strand)
__global__ void sd_motif_edit_per(MeArgs a, int n_motifs, int64_t* per) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (int64_t)a.n_reads * a.n_ps) return;
    const int r = (int)(x / a.n_ps), ps = (int)(x - (int64_t)r * a.n_ps);
    const int64_t tiles_r = a.tile_off[r + 1] - a.tile_off[r], i0 = (int64_t)a.n_ps * a.tile_off[r] + ps * tiles_r;
    const int tag = a.ps[ps].y;
    per[((int64_t)r * n_motifs + (tag & 0xffff)) * 2 + (tag >> 16)] = a.base[i0 + tiles_r] - a.base[i0];
}

}  // namespace sd

namespace sdi {
namespace {

std::atomic<int64_t> g_me_launches{0};   // launches of the size and the write kernel in this process (sd_motif_edit_info)

// Per device, kept between calls (sd_job_dev.hpp: DevWork): the planes, the per-read tables [roff | rlen | pw | tile_off],
// the request, the items' counts and bases, and what the last size call was for (the write call must match it).
struct MeCtx : DevWork, ReadTable {
    DevBuf<uint64_t> planes;
    DevBuf<uint8_t> text;        // sd_motif_edit_dev: the reads, back to back
    DevBuf<int2> ps;
    DevBuf<uint64_t> eq;
    DevBuf<int32_t> cnt;
    DevBuf<int64_t> base, per;
    DevBuf<uint4> hits;          // sd_motif_edit_dev
    PinBuf<int64_t> h_total;
    PinBuf<int2> h_ps;
    PinBuf<uint64_t> h_eq;
    sd::MeArgs a{};
    bool sized = false;
    const void* s_text = nullptr;
    int s_device = -1;
    std::vector<int64_t> s_off, s_len;
    std::string s_key;
    int64_t s_total = 0;
};

std::string me_key(const char* const* patterns, int32_t n_motifs, int32_t K) {
    std::string k = std::to_string(K);
    for (int32_t m = 0; m < n_motifs; ++m) { k += '|'; k += patterns[m]; }
    return k;
}

// the request and the reads checked, before any device work; tiles / items / words of the call
struct MeJob {
    sd::MotifEditSet set;
    std::vector<int64_t> tile_off, pw;
    int64_t tiles = 0, items = 0, words = 0, bases = 0;
};
int me_job(const char* who, const char* const* patterns, int32_t n_motifs, int32_t K, const int64_t* read_lens, int32_t n_reads, MeJob& j,
           char* errbuf, size_t errlen) {
    std::string err;
    if (n_motifs > 0 && !patterns) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    if (!sd::motif_edit_compile(patterns, n_motifs, K, j.set, err)) { set_err(errbuf, errlen, std::string(who) + ": " + err); return SD_ERR_PARAM; }
    if (n_reads < 0 || (n_reads > 0 && !read_lens)) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    j.tile_off.assign((size_t)n_reads + 1, 0);
    j.pw.assign((size_t)n_reads + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] < 0 || read_lens[r] >= ((int64_t)1 << 40)) { set_err(errbuf, errlen, std::string(who) + ": a negative read length, or one of 2^40 bases or more"); return SD_ERR_PARAM; }
        j.tile_off[(size_t)r] = j.tiles;
        j.pw[(size_t)r] = j.words;
        j.tiles += sd::motif_edit_tiles(read_lens[r]);
        j.words += sd::autocorr_plane_words(read_lens[r]);
        j.bases += read_lens[r];
    }
    j.tile_off[(size_t)n_reads] = j.tiles;
    j.pw[(size_t)n_reads] = j.words;
    const int64_t n_ps = (int64_t)j.set.set.ps.size();
    if (j.tiles > sd::MOTIF_ITEMS_MAX / n_ps) {
        set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(j.tiles) + " read tiles x " + std::to_string(n_ps) + " pattern-strands, the cap is " +
                                    std::to_string(sd::MOTIF_ITEMS_MAX) + " items (MOTIF_ITEMS_MAX): use fewer reads or fewer motifs per call");
        return SD_ERR_PARAM;
    }
    j.items = j.tiles * n_ps;
    return SD_OK;
}
int me_hits_cap(const char* who, int64_t total, char* errbuf, size_t errlen) {
    if (total <= sd::MOTIF_HITS_MAX) return SD_OK;
    set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(total) + " hits, the cap is " + std::to_string(sd::MOTIF_HITS_MAX) +
                                " (MOTIF_HITS_MAX): use fewer reads or fewer motifs per call");
    return SD_ERR_PARAM;
}

// ---- the host form ------------------------------------------------------------------------------------------------------
struct MePlanes {
    std::vector<uint64_t> lo, hi, v;   // autocorr_plane_words(n) words
    void build(const uint8_t* t, int64_t n) {
        const size_t w = (size_t)sd::autocorr_plane_words(n);
        lo.assign(w, 0);
        hi.assign(w, 0);
        v.assign(w, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int c = sd::autocorr_code(t[i]);
            if (c < 0) continue;
            const uint64_t bit = (uint64_t)1 << (i & 63);
            v[(size_t)(i >> 6)] |= bit;
            if (c & 1) lo[(size_t)(i >> 6)] |= bit;
            if (c & 2) hi[(size_t)(i >> 6)] |= bit;
        }
    }
};

// one pattern-strand over one read: the scan from the read's first base, the same step and the same start as the kernels
template <class W>
void me_host_item(const MePlanes& p, int64_t n, int32_t r, const sd::MotifStrand& q, const uint64_t* eq64, int K, std::vector<sd_motif_edit_hit>& out) {
    const sd::MotifEditEq<W> eq = sd::motif_edit_words<W>(eq64), rq = sd::motif_edit_words<W>(eq64 + sd::MOTIF_EDIT_CLASSES);
    const uint64_t *lo = p.lo.data(), *hi = p.hi.data(), *v = p.v.data();
    sd::motif_edit_scan<W>(lo, hi, v, n, 0, n, eq, q.L, K, [&](int64_t e) {
        int len, ed;
        sd::motif_edit_start<W>(q.L, K, e + 1, [&](int64_t x) { return sd::motif_edit_eq_at<W>(lo, hi, v, x, rq); }, &len, &ed);
        out.push_back(sd_motif_edit_hit{e + 1 - len, r, (uint16_t)q.motif, (uint8_t)len, (uint8_t)(q.strand << 7 | ed)});
    });
}

// hits in canonical order (malloc'ed) and per
int me_host(const uint8_t* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const sd::MotifEditSet& set, int threads,
            sd_motif_edit_hit** hits, int64_t* n_hits, int64_t* per, const char* who, char* errbuf, size_t errlen) {
    const std::vector<sd::MotifStrand>& ps = set.set.ps;
    const int64_t n_ps = (int64_t)ps.size();
    std::vector<MePlanes> planes((size_t)n_reads);
    sd::parallel_for(n_reads, threads, 1, [&](int64_t r) { planes[(size_t)r].build(text + read_off[r], read_lens[r]); });
    std::vector<std::vector<sd_motif_edit_hit>> found((size_t)(n_reads * n_ps));   // (read, pattern-strand): the canonical order
    sd::parallel_for(n_reads * n_ps, threads, 1, [&](int64_t it) {
        const int32_t r = (int32_t)(it / n_ps);
        const size_t q = (size_t)(it - r * n_ps);
        const uint64_t* eq = set.eq.data() + q * sd::MOTIF_EDIT_WORDS;
        if (ps[q].L <= 32) me_host_item<uint32_t>(planes[(size_t)r], read_lens[r], r, ps[q], eq, set.K, found[(size_t)it]);
        else me_host_item<uint64_t>(planes[(size_t)r], read_lens[r], r, ps[q], eq, set.K, found[(size_t)it]);
    });
    int64_t total = 0;
    std::vector<int64_t> at(found.size() + 1, 0);
    for (size_t i = 0; i < found.size(); ++i) { at[i] = total; total += (int64_t)found[i].size(); }
    const int rc = me_hits_cap(who, total, errbuf, errlen);
    if (rc) return rc;
    std::memset(per, 0, sizeof(int64_t) * (size_t)n_reads * (size_t)set.set.n_motifs * 2);
    sd_motif_edit_hit* out = static_cast<sd_motif_edit_hit*>(std::malloc(sizeof(sd_motif_edit_hit) * (size_t)std::max<int64_t>(total, 1)));
    if (!out) throw std::bad_alloc();
    sd::parallel_for((int64_t)found.size(), threads, 8, [&](int64_t i) {
        if (!found[(size_t)i].empty()) std::memcpy(out + at[(size_t)i], found[(size_t)i].data(), sizeof(sd_motif_edit_hit) * found[(size_t)i].size());
    });
    for (size_t i = 0; i < found.size(); ++i) {
        const sd::MotifStrand& q = ps[i % (size_t)n_ps];
        per[((i / (size_t)n_ps) * (size_t)set.set.n_motifs + (size_t)q.motif) * 2 + (size_t)q.strand] = (int64_t)found[i].size();
    }
    *hits = out;
    *n_hits = total;
    return SD_OK;
}

// ---- the device passes --------------------------------------------------------------------------------------------------
// tables and request up on st; c.a ready for the launches.  d_text + roff[r] = read r.
void me_setup(MeCtx& c, hipStream_t st, const MeJob& j, const int64_t* roff, const int64_t* read_lens, int32_t n_reads) {
    const std::vector<sd::MotifStrand>& ps = j.set.set.ps;
    const int n_ps = (int)ps.size();
    c.shape(4, n_reads);
    int64_t *h_off = c.h(0), *h_len = c.h(1), *h_pw = c.h(2), *h_tile = c.h(3);
    for (int32_t r = 0; r < n_reads; ++r) { h_off[r] = roff[r]; h_len[r] = read_lens[r]; h_pw[r] = j.pw[(size_t)r]; h_tile[r] = j.tile_off[(size_t)r]; }
    h_off[n_reads] = 0; h_len[n_reads] = 0; h_pw[n_reads] = j.words; h_tile[n_reads] = j.tiles;
    c.upload(4, st);
    c.h_ps.alloc((size_t)n_ps);
    c.h_eq.alloc(j.set.eq.size());
    c.ps.alloc((size_t)n_ps);
    c.eq.alloc(j.set.eq.size());
    for (int q = 0; q < n_ps; ++q) c.h_ps.p[q] = make_int2(ps[(size_t)q].L, ps[(size_t)q].motif | ps[(size_t)q].strand << 16);
    std::memcpy(c.h_eq.p, j.set.eq.data(), sizeof(uint64_t) * j.set.eq.size());
    SD_HIP(hipMemcpyAsync(c.ps.p, c.h_ps.p, sizeof(int2) * (size_t)n_ps, hipMemcpyHostToDevice, st));
    SD_HIP(hipMemcpyAsync(c.eq.p, c.h_eq.p, sizeof(uint64_t) * j.set.eq.size(), hipMemcpyHostToDevice, st));
    c.planes.alloc(3 * (size_t)j.words);
    c.cnt.alloc((size_t)j.items);
    c.base.alloc((size_t)j.items + 1);
    c.h_total.alloc(1);
    uint64_t* lo = c.planes.p;
    sd::MeArgs& a = c.a;
    a = sd::MeArgs{};
    a.lo = lo; a.hi = lo + j.words; a.v = lo + 2 * j.words;
    a.rlen = c.d(1); a.pw = c.d(2); a.tile_off = c.d(3);
    a.n_reads = (int)n_reads; a.n_ps = n_ps; a.n_psb = (n_ps + sd::MOTIF_EDIT_PB - 1) / sd::MOTIF_EDIT_PB; a.K = j.set.K;
    a.ps = c.ps.p; a.eq = c.eq.p;
    a.n_units = j.tiles * a.n_psb;
    a.cnt = c.cnt.p; a.base = c.base.p;
}

void me_prep(MeCtx& c, hipStream_t st, const uint8_t* d_text, const MeJob& j, int32_t n_reads) {
    if (j.words == 0 || n_reads == 0) return;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((j.words + 3) / 4, (int64_t)c.n_cu * 32));
    sd::launch_autocorr_prep(st, grid, d_text, c.d(0), c.d(1), c.d(2), (int)n_reads, j.words, c.planes.p, c.planes.p + j.words, c.planes.p + 2 * j.words);
    SD_HIP(hipGetLastError());
}

template <class Launch>
void me_units(MeCtx& c, Launch&& launch) {
    int64_t launches = 0;
    for (int64_t u0 = 0; u0 < c.a.n_units; u0 += sd::MOTIF_EDIT_LAUNCH_WG) {
        c.a.unit0 = u0;
        launch((unsigned)std::min<int64_t>(sd::MOTIF_EDIT_LAUNCH_WG, c.a.n_units - u0));
        SD_HIP(hipGetLastError());
        ++launches;
    }
    g_me_launches.fetch_add(launches);
}

// counts, scan, per (d_per: n_reads x n_motifs x 2) and the total on its way to c.h_total; nothing waits
void me_size(MeCtx& c, hipStream_t st, const MeJob& j, int32_t n_reads, int64_t* d_per) {
    me_units(c, [&](unsigned grid) { hipLaunchKernelGGL(sd::sd_motif_edit_size, dim3(grid), dim3(sd::ME_T), 0, st, c.a); });
    hipLaunchKernelGGL(sd::scan_bases<int32_t>, dim3(1), dim3(sd::SCAN_T), 0, st, c.cnt.p, j.items, c.base.p);
    SD_HIP(hipGetLastError());
    const int64_t cells = (int64_t)n_reads * j.set.set.n_motifs * 2, rp = (int64_t)n_reads * c.a.n_ps;
    if (cells) {
        SD_HIP(hipMemsetAsync(d_per, 0, sizeof(int64_t) * (size_t)cells, st));   // (the - strand of a palindrome has no item)
        hipLaunchKernelGGL(sd::sd_motif_edit_per, dim3((unsigned)((rp + 255) / 256)), dim3(256), 0, st, c.a, (int)j.set.set.n_motifs, d_per);
        SD_HIP(hipGetLastError());
    }
    SD_HIP(hipMemcpyAsync(c.h_total.p, c.base.p + j.items, sizeof(int64_t), hipMemcpyDeviceToHost, st));
}

void me_write(MeCtx& c, hipStream_t st, uint4* d_hits, int64_t cap) {
    c.a.cap = cap;
    me_units(c, [&](unsigned grid) { hipLaunchKernelGGL(sd::sd_motif_edit_write, dim3(grid), dim3(sd::ME_T), 0, st, c.a, d_hits); });
}

struct MeBench {
    int warmup, reps;
    float *ms_prep, *ms_size, *ms_write;
    int64_t* info;
};

int me_dev(const char* who, const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
           int32_t n_motifs, int32_t K, int32_t device, sd_motif_edit_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf, size_t errlen,
           const MeBench* bench) {
    MeJob j;
    int rc = me_job(who, patterns, n_motifs, K, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, text, read_off, read_lens, n_reads, !hits || !n_hits || (n_reads > 0 && !per), errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    std::vector<int64_t> off((size_t)n_reads + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) off[(size_t)r + 1] = off[(size_t)r] + read_lens[r];
    const size_t cells = (size_t)n_reads * (size_t)j.set.set.n_motifs * 2;
    try {
        DeviceScope on(device);
        MeCtx& c = device_ctx<MeCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        c.sized = false;
        OwnedStream st;
        c.text.alloc((size_t)j.bases);
        c.per.alloc(cells);
        for (int32_t r = 0; r < n_reads; ++r)   // the reads back to back, whatever their order and gaps in the caller's buffer
            if (read_lens[r] > 0)
                SD_HIP(hipMemcpyAsync(c.text.p + off[(size_t)r], text + read_off[r], (size_t)read_lens[r], hipMemcpyHostToDevice, st));
        me_setup(c, st, j, off.data(), read_lens, n_reads);
        StageClock clock;
        if (bench) {
            clock.time(st, bench->warmup, bench->reps, bench->ms_prep, [&]() { me_prep(c, st, c.text.p, j, n_reads); });
            clock.time(st, bench->warmup, bench->reps, bench->ms_size, [&]() { me_size(c, st, j, n_reads, c.per.p); });
        } else {
            me_prep(c, st, c.text.p, j, n_reads);
            me_size(c, st, j, n_reads, c.per.p);
        }
        c.in_flight(st);
        SD_HIP(hipStreamSynchronize(st));
        c.waited();
        const int64_t total = c.h_total.p[0];
        if ((rc = me_hits_cap(who, total, errbuf, errlen))) return rc;
        c.hits.alloc((size_t)total);
        sd_motif_edit_hit* out = static_cast<sd_motif_edit_hit*>(std::malloc(sizeof(sd_motif_edit_hit) * (size_t)std::max<int64_t>(total, 1)));
        if (!out) throw std::bad_alloc();
        struct Free { sd_motif_edit_hit* p; ~Free() { std::free(p); } } keep{out};
        if (bench) {
            const int64_t before = g_me_launches.load();
            clock.time(st, bench->warmup, bench->reps, bench->ms_write, [&]() { me_write(c, st, c.hits.p, total); });
            bench->info[0] = (g_me_launches.load() - before) / (bench->warmup + bench->reps);
            bench->info[1] = j.items;
            bench->info[2] = total;
            bench->info[3] = j.words;
        } else {
            me_write(c, st, c.hits.p, total);
        }
        c.in_flight(st);
        if (total) SD_HIP(hipMemcpyAsync(out, c.hits.p, sizeof(sd_motif_edit_hit) * (size_t)total, hipMemcpyDeviceToHost, st));
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

}  // namespace
}  // namespace sdi

extern "C" {

int sd_motif_edit_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                       int32_t n_motifs, int32_t K, int32_t threads, sd_motif_edit_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
                       size_t errlen) try {
    static const char* who = "sd_motif_edit_host";
    MeJob j;
    int rc = me_job(who, patterns, n_motifs, K, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, text, read_off, read_lens, n_reads, !hits || !n_hits || (n_reads > 0 && !per), errbuf, errlen))) return rc;
    return me_host(reinterpret_cast<const uint8_t*>(text), read_off, read_lens, n_reads, j.set, std::max(1, threads), hits, n_hits, per, who, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_edit_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                      int32_t n_motifs, int32_t K, int32_t device, sd_motif_edit_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
                      size_t errlen) try {
    return me_dev("sd_motif_edit_dev", text, read_off, read_lens, n_reads, patterns, n_motifs, K, device, hits, n_hits, per, errbuf, errlen, nullptr);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_edit_reads_size_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                                 const char* const* patterns, int32_t n_motifs, int32_t K, int32_t device, void* hip_stream, int64_t* d_per,
                                 int64_t* n_hits, char* errbuf, size_t errlen) try {
    static const char* who = "sd_motif_edit_reads_size_dev";
    MeJob j;
    int rc = me_job(who, patterns, n_motifs, K, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, d_text, read_off, read_lens, n_reads, !n_hits || (n_reads > 0 && !d_per), errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        if (n_reads > 0 && (rc = buffer_on_device(d_per, device, who, "per", errbuf, errlen))) return rc;
        if (j.bases > 0 && (rc = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return rc;
        MeCtx& c = device_ctx<MeCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();   // the previous call's kernels read the buffers this one overwrites
        c.sized = false;
        me_setup(c, st, j, read_off, read_lens, n_reads);
        me_prep(c, st, static_cast<const uint8_t*>(d_text), j, n_reads);
        me_size(c, st, j, n_reads, d_per);
        c.in_flight(st);
        SD_HIP(hipStreamSynchronize(st));   // the 8 bytes of the total: the call's only wait
        c.waited();
        *n_hits = c.h_total.p[0];
        if ((rc = me_hits_cap(who, *n_hits, errbuf, errlen))) return rc;
        c.sized = true;
        c.s_text = d_text;
        c.s_device = device;
        c.s_off.assign(read_off, read_off + n_reads);
        c.s_len.assign(read_lens, read_lens + n_reads);
        c.s_key = me_key(patterns, n_motifs, K);
        c.s_total = *n_hits;
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_edit_reads_write_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                                  const char* const* patterns, int32_t n_motifs, int32_t K, int32_t device, void* hip_stream,
                                  sd_motif_edit_hit* d_hits, int64_t cap, char* errbuf, size_t errlen) try {
    static const char* who = "sd_motif_edit_reads_write_dev";
    MeJob j;
    int rc = me_job(who, patterns, n_motifs, K, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, d_text, read_off, read_lens, n_reads, false, errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        MeCtx& c = device_ctx<MeCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        if (!c.sized || c.s_text != d_text || c.s_device != device || (int32_t)c.s_off.size() != n_reads ||
            !std::equal(c.s_off.begin(), c.s_off.end(), read_off) || !std::equal(c.s_len.begin(), c.s_len.end(), read_lens) ||
            c.s_key != me_key(patterns, n_motifs, K)) {
            set_err(errbuf, errlen, std::string(who) + ": the last sd_motif_edit_reads_size_dev call on this device was not for these reads and motifs");
            return SD_ERR_PARAM;
        }
        if (cap < c.s_total) {
            set_err(errbuf, errlen, std::string(who) + ": capacity " + std::to_string(cap) + " records, the hits need " + std::to_string(c.s_total));
            return SD_ERR_PARAM;
        }
        if (c.s_total == 0) return SD_OK;
        if (!d_hits) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
        if ((rc = buffer_on_device(d_hits, device, who, "hit", errbuf, errlen))) return rc;
        me_write(c, st, reinterpret_cast<uint4*>(d_hits), c.s_total);
        c.in_flight(st);   // (the kernels read the work area: the next size call on the device settles first)
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_motif_edit_info(int64_t info[6]) {
    info[0] = sd::MOTIF_EDIT_STRETCH;
    info[1] = sd::MOTIF_EDIT_TILE_WORDS;
    info[2] = sd::MOTIF_EDIT_PB;
    info[3] = sd::MOTIF_EDIT_LAUNCH_WORK;
    info[4] = g_me_launches.load();
    info[5] = sd::MOTIF_EDIT_LAUNCH_WG;
}

int sd_motif_edit_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                               int32_t n_motifs, int32_t K, int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_size,
                               float* ms_write, int64_t info[4]) try {
    if (warmup < 0 || reps < 1 || !ms_prep || !ms_size || !ms_write || !info || n_reads <= 0) return SD_ERR_PARAM;
    for (int i = 0; i < 4; ++i) info[i] = 0;
    const MeBench b{warmup, reps, ms_prep, ms_size, ms_write, info};
    sd_motif_edit_hit* hits = nullptr;
    int64_t n_hits = 0;
    std::vector<int64_t> per((size_t)n_reads * (size_t)std::max(n_motifs, 1) * 2);
    const int rc = me_dev("sd_motif_edit_kernel_bench", text, read_off, read_lens, n_reads, patterns, n_motifs, K, device, &hits, &n_hits, per.data(), nullptr, 0, &b);
    std::free(hits);
    return rc;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
