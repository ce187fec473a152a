// sd_motif.hip -- IUPAC motif hits on both strands of every read (--motif): where a short pattern such as the CENP-B box
// NTTCGNNNNANNCGGGN lies, with a budget of mismatches.  sd_motif.hpp holds the definition and everything host and device
// compute alike; sd_hits_job.hpp holds the frame of a hit search (checks, work area, passes, the bodies of the entries);
// this file holds what is the Hamming search's own: the kernels, one item of the host form, the request's upload and the
// C-ABI names (include/sd_hip.h: sd_motif_*).
//   sd_autocorr_prep  (sd_autocorr.hip, through launch_autocorr_prep) the byte text -> the bit planes lo | hi | valid
//   sd_motif_size     a workgroup (256 lanes) per (tile of 256 words of a read, block of MOTIF_PB pattern-strands).  A lane
//                     owns one word: it loads its planes and the next word's once and keeps them in registers over the
//                     block.  The pattern-strand and its constrained positions are the same in every lane and come through
//                     scalar loads; per position the three planes are shifted across the word boundary (v_alignbit on the
//                     32-bit halves), the set's match word is formed and added to the bit-sliced mismatch counter
//                     (motif_word).  The hit word is masked to i + L <= n, counted, and the workgroup's sum is the int32
//                     count of the item (read, pattern-strand, tile), laid out in canonical order.
//   scan_bases        (sd_scan_dev.hpp) one workgroup: the items' bases and the total
//   sd_hits_per       (sd_hits_job.hpp) per[read][motif][strand] from the bases
//   sd_motif_write    the work item of sd_motif_size again, for the items with a count: the hit words are recomputed, the
//                     lanes' counts scanned within the workgroup, and every lane writes its own hits as 16-byte records
//                     (one vector store each) from the item's base on.
// No atomics anywhere: the hit array is a function of the input.  Launches: the work items are (tile, pattern block) pairs;
// a launch takes at most MOTIF_LAUNCH_WG of them (sd_motif.hpp).
#include "sd_motif.hpp"
#include "sd_hits_job.hpp"

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

// The unit of a workgroup (hits_unit), the lane's word and the planes of that word and the next one.
struct MtLane {
    int r, ps0, nq;
    int64_t n, t, item0, tiles_r;   // item of pattern-strand ps: item0 + ps * tiles_r
    uint64_t lo0, hi0, v0, lo1, hi1, v1;
    bool active;
};
__device__ inline bool mt_lane(const MtArgs& a, MtLane& l) {
    int64_t tl;
    if (!hits_unit<MOTIF_PB>(a, l, tl)) return false;
    l.t = tl * MOTIF_TILE_WORDS + threadIdx.x;
    l.active = l.t < autocorr_words(l.n);   // (word t + 1 exists: the zero word behind the read at the latest)
    const int64_t x = a.pw[l.r] + l.t;
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

}  // namespace sd

namespace sdi {
namespace {

// the Hamming search as sd_hits_job.hpp takes it
struct MtSearch {
    using Set = sd::MotifSet;
    using Hit = sd_motif_hit;
    using Args = sd::MtArgs;
    static constexpr int T = sd::MT_T, PB = sd::MOTIF_PB;
    static constexpr int64_t LAUNCH_WG = sd::MOTIF_LAUNCH_WG;
    static constexpr const char* size_entry = "sd_motif_reads_size_dev";
    static inline std::atomic<int64_t> launches{0};   // launches of sd_motif_size and sd_motif_write in this process (sd_motif_info)

    static bool compile(const char* const* patterns, int32_t n_motifs, int32_t E, Set& set, std::string& err) {
        return sd::motif_compile(nullptr, patterns, n_motifs, E, set, err);
    }
    static const std::vector<sd::MotifStrand>& strands(const Set& set) { return set.ps; }
    static int n_motifs(const Set& set) { return set.n_motifs; }
    static int64_t tiles(int64_t n) { return sd::motif_tiles(n); }

    struct Request {   // the headers as int4 and the constrained positions
        DevBuf<int4> ps;
        DevBuf<uint32_t> pos;
        PinBuf<int4> h_ps;
        PinBuf<uint32_t> h_pos;
        void upload(const Set& set, hipStream_t st, Args& a) {
            const size_t n_ps = set.ps.size();
            h_ps.alloc(n_ps);
            h_pos.alloc(set.pos.size());
            ps.alloc(n_ps);
            pos.alloc(set.pos.size());
            for (size_t q = 0; q < n_ps; ++q) {
                const sd::MotifStrand& s = set.ps[q];
                h_ps.p[q] = make_int4(s.L, s.motif | s.strand << 16, s.pos_off, s.npos);
            }
            std::memcpy(h_pos.p, set.pos.data(), sizeof(uint32_t) * set.pos.size());
            SD_HIP(hipMemcpyAsync(ps.p, h_ps.p, sizeof(int4) * n_ps, hipMemcpyHostToDevice, st));
            SD_HIP(hipMemcpyAsync(pos.p, h_pos.p, sizeof(uint32_t) * set.pos.size(), hipMemcpyHostToDevice, st));
            a.ps = ps.p; a.pos = pos.p;
        }
    };

    static void size(const Set& set, unsigned grid, hipStream_t st, const Args& a) {
        sd::motif_with_budget(set.E, [&](auto e1) { hipLaunchKernelGGL(sd::sd_motif_size<decltype(e1)::value>, dim3(grid), dim3(T), 0, st, a); });
    }
    static void write(const Set& set, unsigned grid, hipStream_t st, const Args& a, uint4* hits) {
        sd::motif_with_budget(set.E, [&](auto e1) { hipLaunchKernelGGL(sd::sd_motif_write<decltype(e1)::value>, dim3(grid), dim3(T), 0, st, a, hits); });
    }

    template <int E1>
    static void item(const sd::AutocorrPlanes& p, int64_t n, int32_t r, const sd::MotifStrand& q, const uint32_t* pos, std::vector<Hit>& out) {
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
                out.push_back(Hit{t * 64 + bit, r, (uint16_t)q.motif, (uint8_t)q.strand, (uint8_t)sd::motif_count_at(cp, B, bit)});
            }
        }
    }
    static void host_item(const Set& set, const sd::AutocorrPlanes& p, int64_t n, int32_t r, size_t q, std::vector<Hit>& out) {
        sd::motif_with_budget(set.E, [&](auto e1) { item<decltype(e1)::value>(p, n, r, set.ps[q], set.pos.data(), out); });
    }
};

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
    return sdi::hits_host<sdi::MtSearch>("sd_motif_host", text, read_off, read_lens, n_reads, patterns, n_motifs, E, threads, hits, n_hits, per, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                 int32_t n_motifs, int32_t E, int32_t device, sd_motif_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf, size_t errlen) try {
    return sdi::hits_dev<sdi::MtSearch>("sd_motif_dev", text, read_off, read_lens, n_reads, patterns, n_motifs, E, device, hits, n_hits, per, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_reads_size_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                            int32_t n_motifs, int32_t E, int32_t device, void* hip_stream, int64_t* d_per, int64_t* n_hits, char* errbuf,
                            size_t errlen) try {
    return sdi::hits_reads_size_dev<sdi::MtSearch>("sd_motif_reads_size_dev", d_text, read_off, read_lens, n_reads, patterns, n_motifs, E, device, hip_stream, d_per, n_hits, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_reads_write_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                             int32_t n_motifs, int32_t E, int32_t device, void* hip_stream, sd_motif_hit* d_hits, int64_t cap, char* errbuf,
                             size_t errlen) try {
    return sdi::hits_reads_write_dev<sdi::MtSearch>("sd_motif_reads_write_dev", d_text, read_off, read_lens, n_reads, patterns, n_motifs, E, device, hip_stream, d_hits, cap, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_motif_info(int64_t info[4]) {
    info[0] = sd::MOTIF_TILE_WORDS;
    info[1] = sd::MOTIF_PB;
    info[2] = sd::MOTIF_LAUNCH_WORK;
    info[3] = sdi::MtSearch::launches.load();
}

int sd_motif_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                          int32_t n_motifs, int32_t E, int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_size,
                          float* ms_write, int64_t info[4]) try {
    return sdi::hits_kernel_bench<sdi::MtSearch>("sd_motif_kernel_bench", text, read_off, read_lens, n_reads, patterns, n_motifs, E, device, warmup, reps, ms_prep, ms_size, ms_write, info);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
