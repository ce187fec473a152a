// sd_motif_edit.hip -- IUPAC motif hits with insertions and deletions (--motif-edits): a CENP-B box that a noisy read
// holds with an indel.  sd_motif_edit.hpp holds the rule and everything host and device compute alike; sd_hits_job.hpp holds
// the frame of a hit search (checks, work area, passes, the bodies of the entries); this file holds what is the edit
// search's own: the kernels, one item of the host form, the request's upload and the C-ABI names (include/sd_hip.h:
// sd_motif_edit_*).
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
//   sd_hits_per          (sd_hits_job.hpp) per[read][motif][strand] from the bases
//   sd_motif_edit_write  the work item of the size kernel again, for the items with a count: the lane recomputes its hits
//                        as a bit mask over its stretch, the lanes' counts are scanned within the workgroup, and for each
//                        hit the owning lane runs the recurrence anchored at the end backwards over the reversed pattern
//                        for start and edits (motif_edit_start) and stores one 16-byte record.
// No atomics anywhere: the hit array is a function of the input.  A launch takes at most MOTIF_EDIT_LAUNCH_WG work items.
#include "sd_motif_edit.hpp"
#include "sd_hits_job.hpp"

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

// The unit of a workgroup (hits_unit), the planes of its read and the lane's stretch [a, a + MOTIF_EDIT_STRETCH).
struct MeLane {
    int r, ps0, nq;
    int64_t n, a, item0, tiles_r;   // item of pattern-strand ps: item0 + ps * tiles_r
    const uint64_t *lo, *hi, *v;    // word 0 of the read
};
__device__ inline bool me_lane(const MeArgs& a, MeLane& l) {
    int64_t tl;
    if (!hits_unit<MOTIF_EDIT_PB>(a, l, tl)) return false;
    l.a = tl * MOTIF_EDIT_TILE + (int64_t)threadIdx.x * MOTIF_EDIT_STRETCH;   // (at or behind n: the scan does nothing)
    const int64_t x = a.pw[l.r];
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

}  // namespace sd

namespace sdi {
namespace {

// the edit search as sd_hits_job.hpp takes it
struct MeSearch {
    using Set = sd::MotifEditSet;
    using Hit = sd_motif_edit_hit;
    using Args = sd::MeArgs;
    static constexpr int T = sd::ME_T, PB = sd::MOTIF_EDIT_PB;
    static constexpr int64_t LAUNCH_WG = sd::MOTIF_EDIT_LAUNCH_WG;
    static constexpr const char* size_entry = "sd_motif_edit_reads_size_dev";
    static inline std::atomic<int64_t> launches{0};   // launches of the size and the write kernel in this process (sd_motif_edit_info)

    static bool compile(const char* const* patterns, int32_t n_motifs, int32_t K, Set& set, std::string& err) {
        return sd::motif_edit_compile(patterns, n_motifs, K, set, err);
    }
    static const std::vector<sd::MotifStrand>& strands(const Set& set) { return set.set.ps; }
    static int n_motifs(const Set& set) { return set.set.n_motifs; }
    static int64_t tiles(int64_t n) { return sd::motif_edit_tiles(n); }

    struct Request {   // the headers as int2 and the match words
        DevBuf<int2> ps;
        DevBuf<uint64_t> eq;
        PinBuf<int2> h_ps;
        PinBuf<uint64_t> h_eq;
        void upload(const Set& set, hipStream_t st, Args& a) {
            const std::vector<sd::MotifStrand>& s = set.set.ps;
            h_ps.alloc(s.size());
            h_eq.alloc(set.eq.size());
            ps.alloc(s.size());
            eq.alloc(set.eq.size());
            for (size_t q = 0; q < s.size(); ++q) h_ps.p[q] = make_int2(s[q].L, s[q].motif | s[q].strand << 16);
            std::memcpy(h_eq.p, set.eq.data(), sizeof(uint64_t) * set.eq.size());
            SD_HIP(hipMemcpyAsync(ps.p, h_ps.p, sizeof(int2) * s.size(), hipMemcpyHostToDevice, st));
            SD_HIP(hipMemcpyAsync(eq.p, h_eq.p, sizeof(uint64_t) * set.eq.size(), hipMemcpyHostToDevice, st));
            a.ps = ps.p; a.eq = eq.p; a.K = set.K;
        }
    };

    static void size(const Set&, unsigned grid, hipStream_t st, const Args& a) {
        hipLaunchKernelGGL(sd::sd_motif_edit_size, dim3(grid), dim3(T), 0, st, a);
    }
    static void write(const Set&, unsigned grid, hipStream_t st, const Args& a, uint4* hits) {
        hipLaunchKernelGGL(sd::sd_motif_edit_write, dim3(grid), dim3(T), 0, st, a, hits);
    }

    // one pattern-strand over one read: the scan from the read's first base, the same step and the same start as the kernels
    template <class W>
    static void item(const sd::AutocorrPlanes& p, int64_t n, int32_t r, const sd::MotifStrand& q, const uint64_t* eq64, int K, std::vector<Hit>& out) {
        const sd::MotifEditEq<W> eq = sd::motif_edit_words<W>(eq64), rq = sd::motif_edit_words<W>(eq64 + sd::MOTIF_EDIT_CLASSES);
        const uint64_t *lo = p.lo.data(), *hi = p.hi.data(), *v = p.v.data();
        sd::motif_edit_scan<W>(lo, hi, v, n, 0, n, eq, q.L, K, [&](int64_t e) {
            int len, ed;
            sd::motif_edit_start<W>(q.L, K, e + 1, [&](int64_t x) { return sd::motif_edit_eq_at<W>(lo, hi, v, x, rq); }, &len, &ed);
            out.push_back(Hit{e + 1 - len, r, (uint16_t)q.motif, (uint8_t)len, (uint8_t)(q.strand << 7 | ed)});
        });
    }
    static void host_item(const Set& set, const sd::AutocorrPlanes& p, int64_t n, int32_t r, size_t q, std::vector<Hit>& out) {
        const sd::MotifStrand& s = set.set.ps[q];
        const uint64_t* eq = set.eq.data() + q * sd::MOTIF_EDIT_WORDS;
        if (s.L <= 32) item<uint32_t>(p, n, r, s, eq, set.K, out);
        else item<uint64_t>(p, n, r, s, eq, set.K, out);
    }
};

}  // namespace
}  // namespace sdi

extern "C" {

int sd_motif_edit_host(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                       int32_t n_motifs, int32_t K, int32_t threads, sd_motif_edit_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
                       size_t errlen) try {
    return sdi::hits_host<sdi::MeSearch>("sd_motif_edit_host", text, read_off, read_lens, n_reads, patterns, n_motifs, K, threads, hits, n_hits, per, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_edit_dev(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                      int32_t n_motifs, int32_t K, int32_t device, sd_motif_edit_hit** hits, int64_t* n_hits, int64_t* per, char* errbuf,
                      size_t errlen) try {
    return sdi::hits_dev<sdi::MeSearch>("sd_motif_edit_dev", text, read_off, read_lens, n_reads, patterns, n_motifs, K, device, hits, n_hits, per, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_edit_reads_size_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                                 const char* const* patterns, int32_t n_motifs, int32_t K, int32_t device, void* hip_stream, int64_t* d_per,
                                 int64_t* n_hits, char* errbuf, size_t errlen) try {
    return sdi::hits_reads_size_dev<sdi::MeSearch>("sd_motif_edit_reads_size_dev", d_text, read_off, read_lens, n_reads, patterns, n_motifs, K, device, hip_stream, d_per, n_hits, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_motif_edit_reads_write_dev(const void* d_text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                                  const char* const* patterns, int32_t n_motifs, int32_t K, int32_t device, void* hip_stream,
                                  sd_motif_edit_hit* d_hits, int64_t cap, char* errbuf, size_t errlen) try {
    return sdi::hits_reads_write_dev<sdi::MeSearch>("sd_motif_edit_reads_write_dev", d_text, read_off, read_lens, n_reads, patterns, n_motifs, K, device, hip_stream, d_hits, cap, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_motif_edit_info(int64_t info[6]) {
    info[0] = sd::MOTIF_EDIT_STRETCH;
    info[1] = sd::MOTIF_EDIT_TILE_WORDS;
    info[2] = sd::MOTIF_EDIT_PB;
    info[3] = sd::MOTIF_EDIT_LAUNCH_WORK;
    info[4] = sdi::MeSearch::launches.load();
    info[5] = sd::MOTIF_EDIT_LAUNCH_WG;
}

int sd_motif_edit_kernel_bench(const char* text, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads, const char* const* patterns,
                               int32_t n_motifs, int32_t K, int32_t device, int32_t warmup, int32_t reps, float* ms_prep, float* ms_size,
                               float* ms_write, int64_t info[4]) try {
    return sdi::hits_kernel_bench<sdi::MeSearch>("sd_motif_edit_kernel_bench", text, read_off, read_lens, n_reads, patterns, n_motifs, K, device, warmup, reps, ms_prep, ms_size, ms_write, info);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
