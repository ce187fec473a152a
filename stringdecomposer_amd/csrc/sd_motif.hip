// sd_motif.hip -- IUPAC motif hits on both strands of every read (--motif): where a short pattern such as the CENP-B box
// NTTCGNNNNANNCGGGN lies, with a budget of mismatches.  sd_motif.hpp holds the definition and everything host and device
// compute alike; this file holds the kernels, the host form and the C-ABI (include/sd_hip.h: sd_motif_*).
//   sd_autocorr_prep  (sd_autocorr.hip, through launch_autocorr_prep) the byte text -> the bit planes lo | hi | valid
//   sd_motif_size     a workgroup (256 lanes) per (tile of 256 words of a read, block of MOTIF_PB pattern-strands).  A lane
//                     owns one word: it loads its planes and the next word's once and keeps them in registers over the
//                     block.  The pattern-strand and its constrained positions are the same in every lane and come through
//                     scalar loads; per position the three planes are shifted across the word boundary (v_alignbit on the
//                     32-bit halves), the set's match word is formed and added to the bit-sliced mismatch counter
//                     (motif_word).  The hit word is masked to i + L <= n, counted, and the workgroup's sum is the int32
//                     count of the item (read, pattern-strand, tile), laid out in canonical order.
//   scan_bases        (sd_scan_dev.hpp) one workgroup: the items' bases and the total
//   sd_motif_per      per[read][motif][strand] from the bases
//   sd_motif_write    the work item of sd_motif_size again, for the items with a count: the hit words are recomputed, the
//                     lanes' counts scanned within the workgroup, and every lane writes its own hits as 16-byte records
//                     (one vector store each) from the item's base on.
// No atomics anywhere: the hit array is a function of the input.  Launches: the work items are (tile, pattern block) pairs;
// a launch takes at most MOTIF_LAUNCH_WG of them (sd_motif.hpp).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "sd_motif.hpp"
#include "sd_host.hpp"
#include "sd_job_dev.hpp"
#include "sd_scan_dev.hpp"

static_assert(sizeof(sd_motif_hit) == 16, "a hit is one 16-byte store");

namespace sd {

constexpr int MT_T = MOTIF_TILE_WORDS;   // threads per workgroup: one word per lane
static_assert(MT_T == SCAN_T, "block_scan scans a workgroup of SCAN_T lanes");

struct MtArgs {
    const uint64_t *lo, *hi, *v;                 // the planes of the job
    const int64_t *rlen, *pw, *tile_off;         // per read (pw, tile_off: n_reads + 1)
    int n_reads, n_ps, n_psb;
    const int4* ps;                              // per pattern-strand {L, motif | strand << 16, pos_off, npos}
    const uint32_t* pos;                         // motif_pos
    int64_t unit0, n_units;                      // the launch: its first (tile, pattern block) unit
    int32_t* cnt;                                // per item
    const int64_t* base;                         // per item + 1: the scan
    int64_t cap;
};

// The unit of a workgroup: its read, the lane's word and the planes of that word and the next one.  false: nothing to do.
struct MtLane {
    int r, ps0, nq;
    int64_t n, t, item0, tiles_r;   // item of pattern-strand ps: item0 + ps * tiles_r
    uint64_t lo0, hi0, v0, lo1, hi1, v1;
    bool active;
};
__device__ inline bool mt_lane(const MtArgs& a, MtLane& l) {
    const int64_t u = a.unit0 + blockIdx.x;
    if (u >= a.n_units) return false;
    const int64_t tile = u / a.n_psb;
    l.ps0 = (int)(u - tile * a.n_psb) * MOTIF_PB;
    l.nq = a.n_ps - l.ps0 < MOTIF_PB ? a.n_ps - l.ps0 : MOTIF_PB;
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
    l.t = tl * MOTIF_TILE_WORDS + threadIdx.x;
    l.active = l.t < autocorr_words(l.n);   // (word t + 1 exists: the zero word behind the read at the latest)
    const int64_t x = a.pw[r] + l.t;
    l.lo0 = l.active ? a.lo[x] : 0; l.hi0 = l.active ? a.hi[x] : 0; l.v0 = l.active ? a.v[x] : 0;
    l.lo1 = l.active ? a.lo[x + 1] : 0; l.hi1 = l.active ? a.hi[x + 1] : 0; l.v1 = l.active ? a.v[x + 1] : 0;
    return true;
}

// the header of pattern-strand ps, word by word so that each is a scalar load
struct MtHead {
    int L, tag, off, np;
};
__device__ inline MtHead mt_head(const MtArgs& a, int ps) {
    const int* h = reinterpret_cast<const int*>(a.ps + ps);
    return MtHead{motif_request_word(h), motif_request_word(h + 1), motif_request_word(h + 2), motif_request_word(h + 3)};
}

template <int E1>
__global__ __launch_bounds__(MT_T) void sd_motif_size(MtArgs a) {
    __shared__ int wsum[MOTIF_PB][MT_T / 64];
    MtLane l;
    if (!mt_lane(a, l)) return;
    for (int q = 0; q < l.nq; ++q) {
        const MtHead P = mt_head(a, l.ps0 + q);
        uint64_t cp[4];
        const uint64_t h = motif_word<E1>(a.pos + P.off, P.np, l.lo0, l.hi0, l.v0, l.lo1, l.hi1, l.v1, cp) & autocorr_word_mask(l.t, 0, l.n - P.L + 1);
        int c = l.active ? __popcll(h) : 0;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if ((threadIdx.x & 63) == 0) wsum[q][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x < l.nq) {
        int s = 0;
        for (int w = 0; w < MT_T / 64; ++w) s += wsum[threadIdx.x][w];
        a.cnt[l.item0 + (int64_t)(l.ps0 + (int)threadIdx.x) * l.tiles_r] = s;
    }
}

// (hits is a parameter of its own so that it can be __restrict__: the records are stored inside the loops, and only a store
// that cannot alias them leaves the request and the counts in scalar loads)
template <int E1>
__global__ __launch_bounds__(MT_T) void sd_motif_write(MtArgs a, uint4* __restrict__ hits) {
    constexpr int B = E1 >= 8 ? 4 : E1 >= 4 ? 3 : E1 >= 2 ? 2 : 1;
    MtLane l;
    if (!mt_lane(a, l)) return;
    for (int q = 0; q < l.nq; ++q) {
        const int64_t item = l.item0 + (int64_t)(l.ps0 + q) * l.tiles_r;
        if (motif_request_word(a.cnt + item) == 0) continue;   // (the same in every lane; the size pass wrote it, this kernel does not)
        const MtHead P = mt_head(a, l.ps0 + q);
        uint64_t cp[4];
        uint64_t h = motif_word<E1>(a.pos + P.off, P.np, l.lo0, l.hi0, l.v0, l.lo1, l.hi1, l.v1, cp) & autocorr_word_mask(l.t, 0, l.n - P.L + 1);
        if (!l.active) h = 0;
        int total;
        int64_t o = motif_request_word(a.base + item) + block_scan<int>(__popcll(h), &total);
        const uint32_t tag = (uint32_t)P.tag;   // motif | strand << 16
        while (h) {
            const int bit = __ffsll((unsigned long long)h) - 1;
            h &= h - 1;
            const int64_t start = l.t * 64 + bit;
            if (o < a.cap)   // (the capacity was checked against the total: never taken)
                hits[o] = make_uint4((uint32_t)start, (uint32_t)(start >> 32), (uint32_t)l.r, tag | (uint32_t)motif_count_at(cp, B, bit) << 24);
            ++o;
        }
    }
}

// per[(r * n_motifs + motif) * 2 + strand] = the hits of the items of (read r, pattern-strand)
__global__ void sd_motif_per(MtArgs a, int n_motifs, int64_t* per) {
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

std::atomic<int64_t> g_mt_launches{0};   // launches of sd_motif_size and sd_motif_write in this process (sd_motif_info)

// Per device, kept between calls (sd_job_dev.hpp: DevWork): the planes, the per-read tables [roff | rlen | pw | tile_off],
// the request, the items' counts and bases, and what the last size call was for (the write call must match it).
struct MtCtx : DevWork, ReadTable {
    DevBuf<uint64_t> planes;
    DevBuf<uint8_t> text;        // sd_motif_dev: the reads, back to back
    DevBuf<int4> ps;
    DevBuf<uint32_t> pos;
    DevBuf<int32_t> cnt;
    DevBuf<int64_t> base, per;
    DevBuf<uint4> hits;          // sd_motif_dev
    PinBuf<int64_t> h_total;
    PinBuf<int4> h_ps;
    PinBuf<uint32_t> h_pos;
    sd::MtArgs a{};
    bool sized = false;
    const void* s_text = nullptr;
    int s_device = -1;
    std::vector<int64_t> s_off, s_len;
    std::string s_key;
    int64_t s_total = 0;
};

std::string mt_key(const char* const* patterns, int32_t n_motifs, int32_t E) {
    std::string k = std::to_string(E);
    for (int32_t m = 0; m < n_motifs; ++m) { k += '|'; k += patterns[m]; }
    return k;
}

// the request and the reads checked, before any device work; tiles / items / words of the call
struct MtJob {
    sd::MotifSet set;
    std::vector<int64_t> tile_off, pw;
    int64_t tiles = 0, items = 0, words = 0, bases = 0;
};
int mt_job(const char* who, const char* const* patterns, int32_t n_motifs, int32_t E, const int64_t* read_lens, int32_t n_reads, MtJob& j,
           char* errbuf, size_t errlen) {
    std::string err;
    if (n_motifs > 0 && !patterns) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    if (!sd::motif_compile(nullptr, patterns, n_motifs, E, j.set, err)) { set_err(errbuf, errlen, std::string(who) + ": " + err); return SD_ERR_PARAM; }
    if (n_reads < 0 || (n_reads > 0 && !read_lens)) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    j.tile_off.assign((size_t)n_reads + 1, 0);
    j.pw.assign((size_t)n_reads + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] < 0 || read_lens[r] >= ((int64_t)1 << 40)) { set_err(errbuf, errlen, std::string(who) + ": a negative read length, or one of 2^40 bases or more"); return SD_ERR_PARAM; }
        j.tile_off[(size_t)r] = j.tiles;
        j.pw[(size_t)r] = j.words;
        j.tiles += sd::motif_tiles(read_lens[r]);
        j.words += sd::autocorr_plane_words(read_lens[r]);
        j.bases += read_lens[r];
    }
    j.tile_off[(size_t)n_reads] = j.tiles;
    j.pw[(size_t)n_reads] = j.words;
    const int64_t n_ps = (int64_t)j.set.ps.size();
    if (j.tiles > sd::MOTIF_ITEMS_MAX / n_ps) {
        set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(j.tiles) + " read tiles x " + std::to_string(n_ps) + " pattern-strands, the cap is " +
                                    std::to_string(sd::MOTIF_ITEMS_MAX) + " items (MOTIF_ITEMS_MAX): use fewer reads or fewer motifs per call");
        return SD_ERR_PARAM;
    }
    j.items = j.tiles * n_ps;
    return SD_OK;
}
int mt_hits_cap(const char* who, int64_t total, char* errbuf, size_t errlen) {
    if (total <= sd::MOTIF_HITS_MAX) return SD_OK;
    set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(total) + " hits, the cap is " + std::to_string(sd::MOTIF_HITS_MAX) +
                                " (MOTIF_HITS_MAX): use fewer reads or fewer motifs per call");
    return SD_ERR_PARAM;
}

// ---- the host form ------------------------------------------------------------------------------------------------------
struct MtPlanes {
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

template <int E1>
void mt_host_item(const MtPlanes& p, int64_t n, int32_t r, const sd::MotifStrand& q, const uint32_t* pos, std::vector<sd_motif_hit>& out) {
    constexpr int B = E1 >= 8 ? 4 : E1 >= 4 ? 3 : E1 >= 2 ? 2 : 1;
    if (n < q.L) return;
    const int64_t tl = (n - q.L) >> 6;   // the word of the last start
    for (int64_t t = 0; t <= tl; ++t) {
        uint64_t cp[4];
        uint64_t h = sd::motif_word<E1>(pos + q.pos_off, q.npos, p.lo[(size_t)t], p.hi[(size_t)t], p.v[(size_t)t], p.lo[(size_t)t + 1],
                                        p.hi[(size_t)t + 1], p.v[(size_t)t + 1], cp) &
                     sd::autocorr_word_mask(t, 0, n - q.L + 1);
        while (h) {
            const int bit = __builtin_ctzll(h);
            h &= h - 1;
            out.push_back(sd_motif_hit{t * 64 + bit, r, (uint16_t)q.motif, (uint8_t)q.strand, (uint8_t)sd::motif_count_at(cp, B, bit)});
        }
    }
}

// hits in canonical order (malloc'ed) and per
int mt_host(const uint8_t* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const sd::MotifSet& set, int threads,
            sd_motif_hit** hits, int64_t* n_hits, int64_t* per, const char* who, char* errbuf, size_t errlen) {
    const int64_t n_ps = (int64_t)set.ps.size();
    std::vector<MtPlanes> planes((size_t)n_reads);
    sd::parallel_for(n_reads, threads, 1, [&](int64_t r) { planes[(size_t)r].build(text + read_off[r], read_lens[r]); });
    std::vector<std::vector<sd_motif_hit>> found((size_t)(n_reads * n_ps));   // (read, pattern-strand): the canonical order
    sd::motif_with_budget(set.E, [&](auto e1) {
        sd::parallel_for(n_reads * n_ps, threads, 1, [&](int64_t it) {
            const int32_t r = (int32_t)(it / n_ps);
            mt_host_item<decltype(e1)::value>(planes[(size_t)r], read_lens[r], r, set.ps[(size_t)(it - r * n_ps)], set.pos.data(), found[(size_t)it]);
        });
    });
    int64_t total = 0;
    std::vector<int64_t> at(found.size() + 1, 0);
    for (size_t i = 0; i < found.size(); ++i) { at[i] = total; total += (int64_t)found[i].size(); }
    const int rc = mt_hits_cap(who, total, errbuf, errlen);
    if (rc) return rc;
    std::memset(per, 0, sizeof(int64_t) * (size_t)n_reads * (size_t)set.n_motifs * 2);
    sd_motif_hit* out = static_cast<sd_motif_hit*>(std::malloc(sizeof(sd_motif_hit) * (size_t)std::max<int64_t>(total, 1)));
    if (!out) throw std::bad_alloc();
    sd::parallel_for((int64_t)found.size(), threads, 8, [&](int64_t i) {
        if (!found[(size_t)i].empty()) std::memcpy(out + at[(size_t)i], found[(size_t)i].data(), sizeof(sd_motif_hit) * found[(size_t)i].size());
    });
    for (size_t i = 0; i < found.size(); ++i) {
        const sd::MotifStrand& q = set.ps[i % (size_t)n_ps];
        per[((i / (size_t)n_ps) * (size_t)set.n_motifs + (size_t)q.motif) * 2 + (size_t)q.strand] = (int64_t)found[i].size();
    }
    *hits = out;
    *n_hits = total;
    return SD_OK;
}

// ---- the device passes --------------------------------------------------------------------------------------------------
// tables and request up on st; c.a ready for the launches.  d_text + roff[r] = read r.
void mt_setup(MtCtx& c, hipStream_t st, const MtJob& j, const int64_t* roff, const int64_t* read_lens, int32_t n_reads) {
    const int n_ps = (int)j.set.ps.size();
    c.shape(4, n_reads);
    int64_t *h_off = c.h(0), *h_len = c.h(1), *h_pw = c.h(2), *h_tile = c.h(3);
    for (int32_t r = 0; r < n_reads; ++r) { h_off[r] = roff[r]; h_len[r] = read_lens[r]; h_pw[r] = j.pw[(size_t)r]; h_tile[r] = j.tile_off[(size_t)r]; }
    h_off[n_reads] = 0; h_len[n_reads] = 0; h_pw[n_reads] = j.words; h_tile[n_reads] = j.tiles;
    c.upload(4, st);
    c.h_ps.alloc((size_t)n_ps);
    c.h_pos.alloc(j.set.pos.size());
    c.ps.alloc((size_t)n_ps);
    c.pos.alloc(j.set.pos.size());
    for (int q = 0; q < n_ps; ++q) {
        const sd::MotifStrand& s = j.set.ps[(size_t)q];
        c.h_ps.p[q] = make_int4(s.L, s.motif | s.strand << 16, s.pos_off, s.npos);
    }
    std::memcpy(c.h_pos.p, j.set.pos.data(), sizeof(uint32_t) * j.set.pos.size());
    SD_HIP(hipMemcpyAsync(c.ps.p, c.h_ps.p, sizeof(int4) * (size_t)n_ps, hipMemcpyHostToDevice, st));
    SD_HIP(hipMemcpyAsync(c.pos.p, c.h_pos.p, sizeof(uint32_t) * j.set.pos.size(), hipMemcpyHostToDevice, st));
    c.planes.alloc(3 * (size_t)j.words);
    c.cnt.alloc((size_t)j.items);
    c.base.alloc((size_t)j.items + 1);
    c.h_total.alloc(1);
    uint64_t* lo = c.planes.p;
    sd::MtArgs& a = c.a;
    a = sd::MtArgs{};
    a.lo = lo; a.hi = lo + j.words; a.v = lo + 2 * j.words;
    a.rlen = c.d(1); a.pw = c.d(2); a.tile_off = c.d(3);
    a.n_reads = (int)n_reads; a.n_ps = n_ps; a.n_psb = (n_ps + sd::MOTIF_PB - 1) / sd::MOTIF_PB;
    a.ps = c.ps.p; a.pos = c.pos.p;
    a.n_units = j.tiles * a.n_psb;
    a.cnt = c.cnt.p; a.base = c.base.p;
}

void mt_prep(MtCtx& c, hipStream_t st, const uint8_t* d_text, const MtJob& j, int32_t n_reads) {
    if (j.words == 0 || n_reads == 0) return;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((j.words + 3) / 4, (int64_t)c.n_cu * 32));
    sd::launch_autocorr_prep(st, grid, d_text, c.d(0), c.d(1), c.d(2), (int)n_reads, j.words, c.planes.p, c.planes.p + j.words, c.planes.p + 2 * j.words);
    SD_HIP(hipGetLastError());
}

template <class Launch>
void mt_units(MtCtx& c, Launch&& launch) {
    int64_t launches = 0;
    for (int64_t u0 = 0; u0 < c.a.n_units; u0 += sd::MOTIF_LAUNCH_WG) {
        c.a.unit0 = u0;
        launch((unsigned)std::min<int64_t>(sd::MOTIF_LAUNCH_WG, c.a.n_units - u0));
        SD_HIP(hipGetLastError());
        ++launches;
    }
    g_mt_launches.fetch_add(launches);
}

// counts, scan, per (d_per: n_reads x n_motifs x 2) and the total on its way to c.h_total; nothing waits
void mt_size(MtCtx& c, hipStream_t st, const MtJob& j, int32_t n_reads, int64_t* d_per) {
    sd::motif_with_budget(j.set.E, [&](auto e1) {
        mt_units(c, [&](unsigned grid) { hipLaunchKernelGGL(sd::sd_motif_size<decltype(e1)::value>, dim3(grid), dim3(sd::MT_T), 0, st, c.a); });
    });
    hipLaunchKernelGGL(sd::scan_bases<int32_t>, dim3(1), dim3(sd::SCAN_T), 0, st, c.cnt.p, j.items, c.base.p);
    SD_HIP(hipGetLastError());
    const int64_t cells = (int64_t)n_reads * j.set.n_motifs * 2, rp = (int64_t)n_reads * c.a.n_ps;
    if (cells) {
        SD_HIP(hipMemsetAsync(d_per, 0, sizeof(int64_t) * (size_t)cells, st));   // (the - strand of a palindrome has no item)
        hipLaunchKernelGGL(sd::sd_motif_per, dim3((unsigned)((rp + 255) / 256)), dim3(256), 0, st, c.a, (int)j.set.n_motifs, d_per);
        SD_HIP(hipGetLastError());
    }
    SD_HIP(hipMemcpyAsync(c.h_total.p, c.base.p + j.items, sizeof(int64_t), hipMemcpyDeviceToHost, st));
}

void mt_write(MtCtx& c, hipStream_t st, int E, uint4* d_hits, int64_t cap) {
    c.a.cap = cap;
    sd::motif_with_budget(E, [&](auto e1) {
        mt_units(c, [&](unsigned grid) { hipLaunchKernelGGL(sd::sd_motif_write<decltype(e1)::value>, dim3(grid), dim3(sd::MT_T), 0, st, c.a, d_hits); });
    });
}

struct MtBench {
    int warmup, reps;
    float *ms_prep, *ms_size, *ms_write;
    int64_t* info;
};

int mt_dev(const char* who, const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
           int32_t n_motifs, int32_t E, int32_t device, sd_motif_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf, size_t errlen,
           const MtBench* bench) {
    MtJob j;
    int rc = mt_job(who, patterns, n_motifs, E, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, text, read_off, read_lens, n_reads, !hits || !n_hits || (n_reads > 0 && !per), errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    std::vector<int64_t> off((size_t)n_reads + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) off[(size_t)r + 1] = off[(size_t)r] + read_lens[r];
    const size_t cells = (size_t)n_reads * (size_t)j.set.n_motifs * 2;
    try {
        DeviceScope on(device);
        MtCtx& c = device_ctx<MtCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();
        c.sized = false;
        OwnedStream st;
        c.text.alloc((size_t)j.bases);
        c.per.alloc(cells);
        for (int32_t r = 0; r < n_reads; ++r)   // the reads back to back, whatever their order and gaps in the caller's buffer
            if (read_lens[r] > 0)
                SD_HIP(hipMemcpyAsync(c.text.p + off[(size_t)r], text + read_off[r], (size_t)read_lens[r], hipMemcpyHostToDevice, st));
        mt_setup(c, st, j, off.data(), read_lens, n_reads);
        StageClock clock;
        if (bench) {
            clock.time(st, bench->warmup, bench->reps, bench->ms_prep, [&]() { mt_prep(c, st, c.text.p, j, n_reads); });
            clock.time(st, bench->warmup, bench->reps, bench->ms_size, [&]() { mt_size(c, st, j, n_reads, c.per.p); });
        } else {
            mt_prep(c, st, c.text.p, j, n_reads);
            mt_size(c, st, j, n_reads, c.per.p);
        }
        c.in_flight(st);
        SD_HIP(hipStreamSynchronize(st));
        c.waited();
        const int64_t total = c.h_total.p[0];
        if ((rc = mt_hits_cap(who, total, errbuf, errlen))) return rc;
        c.hits.alloc((size_t)total);
        sd_motif_hit* out = static_cast<sd_motif_hit*>(std::malloc(sizeof(sd_motif_hit) * (size_t)std::max<int64_t>(total, 1)));
        if (!out) throw std::bad_alloc();
        struct Free { sd_motif_hit* p; ~Free() { std::free(p); } } keep{out};
        if (bench) {
            const int64_t before = g_mt_launches.load();
            clock.time(st, bench->warmup, bench->reps, bench->ms_write, [&]() { mt_write(c, st, j.set.E, c.hits.p, total); });
            bench->info[0] = (g_mt_launches.load() - before) / (bench->warmup + bench->reps);
            bench->info[1] = j.items;
            bench->info[2] = total;
            bench->info[3] = j.words;
        } else {
            mt_write(c, st, j.set.E, c.hits.p, total);
        }
        c.in_flight(st);
        if (total) SD_HIP(hipMemcpyAsync(out, c.hits.p, sizeof(sd_motif_hit) * (size_t)total, hipMemcpyDeviceToHost, st));
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

int sd_motif_compile(const char* const* names, const char* const* patterns, int32_t n_motifs, int32_t E, int32_t* n_strands, int32_t* table,
                     char* errbuf, size_t errlen) try {
    static const char* who = "sd_motif_compile";
    if (!n_strands || (n_motifs > 0 && (!patterns || !names))) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
    sd::MotifSet set;
    std::string err;
    if (!sd::motif_compile(names, patterns, n_motifs, E, set, err)) { set_err(errbuf, errlen, std::string(who) + ": " + err); return SD_ERR_PARAM; }
    *n_strands = (int32_t)set.ps.size();
    if (table)
        for (size_t q = 0; q < set.ps.size(); ++q) {
            const sd::MotifStrand& s = set.ps[q];
            table[5 * q] = s.motif; table[5 * q + 1] = s.strand; table[5 * q + 2] = s.L; table[5 * q + 3] = s.npos; table[5 * q + 4] = s.palindrome;
        }
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                  int32_t n_motifs, int32_t E, int32_t threads, sd_motif_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
                  size_t errlen) try {
    static const char* who = "sd_motif_host";
    MtJob j;
    int rc = mt_job(who, patterns, n_motifs, E, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, text, read_off, read_lens, n_reads, !hits || !n_hits || (n_reads > 0 && !per), errbuf, errlen))) return rc;
    return mt_host(reinterpret_cast<const uint8_t*>(text), read_off, read_lens, n_reads, j.set, std::max(1, threads), hits, n_hits, per, who, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                 int32_t n_motifs, int32_t E, int32_t device, sd_motif_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf, size_t errlen) try {
    return mt_dev("sd_motif_dev", text, read_off, read_lens, n_reads, patterns, n_motifs, E, device, hits, n_hits, per, errbuf, errlen, nullptr);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_reads_size_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                            int32_t n_motifs, int32_t E, int32_t device, void* hip_stream, int64_t* d_per, int64_t* n_hits, char* errbuf,
                            size_t errlen) try {
    static const char* who = "sd_motif_reads_size_dev";
    MtJob j;
    int rc = mt_job(who, patterns, n_motifs, E, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, d_text, read_off, read_lens, n_reads, !n_hits || (n_reads > 0 && !d_per), errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        if (n_reads > 0 && (rc = buffer_on_device(d_per, device, who, "per", errbuf, errlen))) return rc;
        if (j.bases > 0 && (rc = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return rc;
        MtCtx& c = device_ctx<MtCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        c.settle();   // the previous call's kernels read the buffers this one overwrites
        c.sized = false;
        mt_setup(c, st, j, read_off, read_lens, n_reads);
        mt_prep(c, st, static_cast<const uint8_t*>(d_text), j, n_reads);
        mt_size(c, st, j, n_reads, d_per);
        c.in_flight(st);
        SD_HIP(hipStreamSynchronize(st));   // the 8 bytes of the total: the call's only wait
        c.waited();
        *n_hits = c.h_total.p[0];
        if ((rc = mt_hits_cap(who, *n_hits, errbuf, errlen))) return rc;
        c.sized = true;
        c.s_text = d_text;
        c.s_device = device;
        c.s_off.assign(read_off, read_off + n_reads);
        c.s_len.assign(read_lens, read_lens + n_reads);
        c.s_key = mt_key(patterns, n_motifs, E);
        c.s_total = *n_hits;
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_reads_write_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                             int32_t n_motifs, int32_t E, int32_t device, void* hip_stream, sd_motif_hit* d_hits, int64_t cap, char* errbuf,
                             size_t errlen) try {
    static const char* who = "sd_motif_reads_write_dev";
    MtJob j;
    int rc = mt_job(who, patterns, n_motifs, E, read_lens, n_reads, j, errbuf, errlen);
    if (rc) return rc;
    if ((rc = reads_text_args(who, d_text, read_off, read_lens, n_reads, false, errbuf, errlen))) return rc;
    if ((rc = device_check(device, errbuf, errlen))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    try {
        DeviceScope on(device);
        MtCtx& c = device_ctx<MtCtx>(device);
        std::lock_guard<std::mutex> g(c.m);
        if (!c.sized || c.s_text != d_text || c.s_device != device || (int32_t)c.s_off.size() != n_reads ||
            !std::equal(c.s_off.begin(), c.s_off.end(), read_off) || !std::equal(c.s_len.begin(), c.s_len.end(), read_lens) ||
            c.s_key != mt_key(patterns, n_motifs, E)) {
            set_err(errbuf, errlen, std::string(who) + ": the last sd_motif_reads_size_dev call on this device was not for these reads and motifs");
            return SD_ERR_PARAM;
        }
        if (cap < c.s_total) {
            set_err(errbuf, errlen, std::string(who) + ": capacity " + std::to_string(cap) + " records, the hits need " + std::to_string(c.s_total));
            return SD_ERR_PARAM;
        }
        if (c.s_total == 0) return SD_OK;
        if (!d_hits) { set_err(errbuf, errlen, std::string(who) + ": missing argument"); return SD_ERR_PARAM; }
        if ((rc = buffer_on_device(d_hits, device, who, "hit", errbuf, errlen))) return rc;
        mt_write(c, st, j.set.E, reinterpret_cast<uint4*>(d_hits), c.s_total);
        c.in_flight(st);   // (the kernels read the work area: the next size call on the device settles first)
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_motif_info(int64_t info[4]) {
    info[0] = sd::MOTIF_TILE_WORDS;
    info[1] = sd::MOTIF_PB;
    info[2] = sd::MOTIF_LAUNCH_WORK;
    info[3] = g_mt_launches.load();
}

int sd_motif_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                          int32_t n_motifs, int32_t E, int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_size,
                          float* ms_write, int64_t info[4]) try {
    if (warmup < 0 || reps < 1 || !ms_prep || !ms_size || !ms_write || !info || n_reads <= 0) return SD_ERR_PARAM;
    for (int i = 0; i < 4; ++i) info[i] = 0;
    const MtBench b{warmup, reps, ms_prep, ms_size, ms_write, info};
    sd_motif_hit* hits = nullptr;
    int64_t n_hits = 0;
    std::vector<int64_t> per((size_t)n_reads * (size_t)std::max(n_motifs, 1) * 2);
    const int rc = mt_dev("sd_motif_kernel_bench", text, read_off, read_lens, n_reads, patterns, n_motifs, E, device, &hits, &n_hits, per.data(), nullptr, 0, &b);
    std::free(hits);
    return rc;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
