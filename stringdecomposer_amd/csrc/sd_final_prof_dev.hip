// sd_final_prof_dev.hip -- the column profiles of a device-final job on the device (SD_FLAG_DEVICE_PROFILE): the part
// between the selection (sd_final_dev.hip) and the fold (sd_nw_profile, sd_nw.hip), which nw_profile_device does on the
// host from host vectors.
//   sd_fprof_plan      one lane per merged row: the pair of a kept row (sd_final_prof_dev.hpp), its class, and per
//                      forward monomer the number of kernel pairs (workgroup histogram in LDS, then global adds), the
//                      longest such segment, the number of host pairs
//   sd_fprof_scan      exclusive prefix of the monomer counts, the scatter's cursors
//   sd_fprof_scatter   kernel pairs -> order[], grouped by forward monomer (group_scatter of sd_group_dev.hpp: a workgroup
//                      reserves its ranges with one atomic per monomer); host pairs -> a compact list of (start, len, template)
//   sd_fprof_items     work items {monomer, first, end} of up to `per` pairs from the same prefix
// Order inside a group depends on the atomics; the counters are integer sums, so the profile does not.
#include "sd_final_ws.hpp"
#include "sd_group_dev.hpp"
#include "sd_job_dev.hpp"

namespace sd {

constexpr int FPROF_T = 256;       // threads per workgroup of the row kernels
constexpr int FPROF_HIST = 1024;   // forward monomers with a bin in LDS; those behind go to the global counters directly

struct FProfArgs {
    const DevRec* recs;
    const int64_t* src;        // null: row m is recs[m]
    const uint8_t* keep;
    const int64_t* moff;
    const int64_t* rlen;
    const int64_t* text_off;
    int n_reads;
    const int64_t* n_ptr;
    int64_t cap;
    const int32_t* own_il;
    const int32_t* tlen;
    int n_tmpl, tmax, M;
    int64_t* seg_start;
    int32_t* seg_len;
    int32_t* pair_il;
    uint8_t* cls;
    int32_t* sum;              // M + 2
};

// the read that owns merged row m: the first r with moff[r + 1] > m (fin_read_of of sd_final_dev.hip)
__device__ inline int fprof_read_of(const int64_t* __restrict__ moff, int n_reads, int64_t m) {
    int lo = 0, hi = n_reads - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (moff[mid + 1] > m) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(FPROF_T) void sd_fprof_plan(FProfArgs a) {
    __shared__ int hist[FPROF_HIST];
    __shared__ int qmax_s, nh_s;
    const int nb = a.M < FPROF_HIST ? a.M : FPROF_HIST;
    for (int i = threadIdx.x; i < nb; i += FPROF_T) hist[i] = 0;
    if (threadIdx.x == 0) { qmax_s = 0; nh_s = 0; }
    __syncthreads();
    const int64_t m = (int64_t)blockIdx.x * FPROF_T + threadIdx.x;
    const int64_t n = *a.n_ptr < a.cap ? *a.n_ptr : a.cap;
    if (m < n) {
        uint8_t c = FPROF_NONE;
        if (a.keep[m]) {
            const DevRec x = a.recs[a.src ? a.src[m] : m];
            if (x.tmpl >= 0 && x.tmpl < a.n_tmpl) {
                const int r = fprof_read_of(a.moff, a.n_reads, m);
                const int il = a.own_il[x.tmpl];
                const FProfPair p = final_prof_pair(x.start, x.end, a.rlen[r], a.text_off[r], il, a.tlen[il], a.tmax);
                a.seg_start[m] = p.start;
                a.seg_len[m] = p.len;
                a.pair_il[m] = p.il;
                c = p.cls;
                if (c == FPROF_DEV) {
                    const int mono = il >> 1;
                    if (mono < FPROF_HIST) atomicAdd(&hist[mono], 1);
                    else atomicAdd(&a.sum[mono], 1);
                    atomicMax(&qmax_s, p.len);
                } else if (c == FPROF_HOST) {
                    atomicAdd(&nh_s, 1);
                }
            }
        }
        a.cls[m] = c;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += FPROF_T)
        if (hist[i]) atomicAdd(&a.sum[i], hist[i]);
    if (threadIdx.x == 0) {
        if (qmax_s) atomicMax(&a.sum[a.M], qmax_s);
        if (nh_s) atomicAdd(&a.sum[a.M + 1], nh_s);
    }
}

// one lane: M is the number of monomers of the set, tens to hundreds
__global__ void sd_fprof_scan(const int32_t* __restrict__ sum, int M, int32_t* __restrict__ base, int32_t* __restrict__ cursor) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int at = 0;
    for (int m = 0; m < M; ++m) {
        base[m] = at;
        cursor[m] = at;
        at += sum[m];
    }
    base[M] = at;
    cursor[M] = 0;
}

// the pairs of a plan as group_scatter reads them (sd_group_dev.hpp): kernel pairs by forward monomer, host pairs aside
struct FProfSrc {
    const uint8_t* cls;
    const int32_t* pair_il;
    const int64_t* seg_start;
    const int32_t* seg_len;
    FProfHostPair* hlist;
    __device__ int kind(int64_t m) const { return cls[m] == FPROF_DEV ? GROUP_IN : cls[m] == FPROF_HOST ? GROUP_ASIDE : GROUP_OUT; }
    __device__ int group(int64_t m) const { return pair_il[m] >> 1; }
    __device__ void aside(int64_t m, int64_t pos) const {
        FProfHostPair h;
        h.start = seg_start[m];
        h.len = seg_len[m];
        h.il = pair_il[m];
        hlist[pos] = h;
    }
};

__global__ __launch_bounds__(FPROF_T) void sd_fprof_scatter(const uint8_t* __restrict__ cls, const int32_t* __restrict__ pair_il,
                                                          const int64_t* __restrict__ seg_start, const int32_t* __restrict__ seg_len,
                                                          const int64_t* __restrict__ n_ptr, int64_t cap, int M,
                                                          int32_t* __restrict__ cursor, int32_t* __restrict__ order,
                                                          FProfHostPair* __restrict__ hlist) {
    static_assert(FPROF_T == GROUP_T && FPROF_HIST == GROUP_HIST, "group_scatter's workgroup");
    const int64_t n = *n_ptr < cap ? *n_ptr : cap;
    group_scatter(FProfSrc{cls, pair_il, seg_start, seg_len, hlist}, n, cap, M, cursor, order);
}

// workgroup m: the items of monomer m, behind those of the monomers before it
__global__ __launch_bounds__(64) void sd_fprof_items(const int32_t* __restrict__ base, int M, int per, int4* __restrict__ items, int n_items) {
    __shared__ int before;
    const int m = blockIdx.x;
    if (threadIdx.x == 0) before = 0;
    __syncthreads();
    int part = 0;
    for (int j = threadIdx.x; j < m; j += 64) part += (base[j + 1] - base[j] + per - 1) / per;
    if (part) atomicAdd(&before, part);
    __syncthreads();
    const int a = base[m], e = base[m + 1];
    for (int64_t k = threadIdx.x; a + k * per < e; k += 64) {
        const int64_t idx = before + k, first = a + k * per;
        if (idx < n_items) items[idx] = make_int4(m, (int)first, (int)(first + per < e ? first + per : e), 0);
    }
}

__global__ __launch_bounds__(FPROF_T) void sd_fprof_add(unsigned long long* __restrict__ dst, const unsigned long long* __restrict__ add, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * FPROF_T + threadIdx.x;
    if (i < n) dst[i] += add[i];
}

}  // namespace sd

namespace sdi {

static inline unsigned fprof_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + sd::FPROF_T - 1) / sd::FPROF_T); }

void ProfDev::setup(const std::vector<std::string>& il, const std::vector<int32_t>& own, hipStream_t st) {
    M = (int)il.size() / 2;
    tmax = 1;
    for (const std::string& t : il) tmax = std::max(tmax, (int)t.size());
    std::vector<int32_t> fl((size_t)M);
    for (int m = 0; m < M; ++m) fl[(size_t)m] = (int32_t)il[(size_t)(2 * m)].size();
    std::vector<int64_t> off;
    total = sd::profile_offsets(fl, off);
    int dev = 0;
    SD_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    SD_HIP(hipGetDeviceProperties(&prop, dev));
    n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    std::vector<int32_t> tl;
    std::vector<unsigned long long> masks;
    if (tmax <= sd::FPROF_TMAX) {   // (a longer set has no kernel pairs: the fold never runs)
        K = (tmax + 63) / 64;
        if (K == 5) K = 6;
        if (K == 7) K = 8;
        sd::nw_build_masks(il, K, masks, tl);
    } else {
        K = 8;
        for (const std::string& t : il) tl.push_back((int32_t)t.size());
        masks.assign(8, 0ull);
    }
    peq.alloc(masks.size());
    tlen.alloc(tl.size());
    own_il.alloc(own.size());
    poff.alloc(off.size());
    counts.alloc((size_t)total + 8);
    ckpos.alloc(64);
    SD_HIP(hipMemcpyAsync(peq.p, masks.data(), masks.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    SD_HIP(hipMemcpyAsync(tlen.p, tl.data(), tl.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (!own.empty()) SD_HIP(hipMemcpyAsync(own_il.p, own.data(), own.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SD_HIP(hipMemcpyAsync(poff.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    SD_HIP(hipMemsetAsync(counts.p, 0, ((size_t)total + 8) * sizeof(unsigned long long), st));
    SD_HIP(hipStreamSynchronize(st));   // (the vectors above leave)
}

void group_scan(hipStream_t st, const int32_t* sum, int M, int32_t* base, int32_t* cursor) {
    hipLaunchKernelGGL(sd::sd_fprof_scan, dim3(1), dim3(64), 0, st, sum, M, base, cursor);
}

void prof_group(ProfWS& w, int M, hipStream_t st, int64_t cap, const int64_t* n_ptr) {
    group_scan(st, w.sum.p, M, w.base.p, w.cursor.p);
    if (cap > 0)
        hipLaunchKernelGGL(sd::sd_fprof_scatter, dim3(fprof_grid(cap)), dim3(sd::FPROF_T), 0, st, w.cls.p, w.pair_il.p, w.seg_start.p,
                           w.seg_len.p, n_ptr, cap, M, w.cursor.p, w.order.p, w.hlist.p);
    SD_HIP(hipGetLastError());
}

void prof_items(ProfWS& w, int M, int per, int64_t n_items, hipStream_t st, bool clear) {
    w.items.alloc((size_t)n_items);
    if (clear) SD_HIP(hipMemsetAsync(w.items.p, 0, (size_t)std::max<int64_t>(n_items, 1) * sizeof(int4), st));
    hipLaunchKernelGGL(sd::sd_fprof_items, dim3((unsigned)M), dim3(64), 0, st, w.base.p, M, per, w.items.p, (int)n_items);
    SD_HIP(hipGetLastError());
}

void prof_plan(ProfWS& w, const ProfDev& d, hipStream_t st, const sd::DevRec* recs, const int64_t* src, const uint8_t* keep,
               const int64_t* moff, const int64_t* rlen, int32_t n_reads, int64_t cap_rows, const int64_t* n_ptr) {
    const int64_t cap = std::max<int64_t>(cap_rows, 0);
    const int M = d.M;
    w.seg_start.alloc((size_t)cap);
    w.seg_len.alloc((size_t)cap);
    w.pair_il.alloc((size_t)cap);
    w.order.alloc((size_t)cap);
    w.cls.alloc((size_t)cap);
    w.hlist.alloc((size_t)cap);
    w.sum.alloc((size_t)M + 2);
    w.base.alloc((size_t)M + 1);
    w.cursor.alloc((size_t)M + 1);
    w.h_sum.alloc((size_t)M + 2);
    SD_HIP(hipMemsetAsync(w.sum.p, 0, ((size_t)M + 2) * sizeof(int32_t), st));
    const bool rows = cap > 0 && n_reads > 0;
    if (rows) {
        sd::FProfArgs a{recs, src, keep, moff, rlen, w.text_off.p, (int)n_reads, n_ptr, cap, d.own_il.p, d.tlen.p,
                        (int)d.own_il.n, d.tmax, M, w.seg_start.p, w.seg_len.p, w.pair_il.p, w.cls.p, w.sum.p};
        hipLaunchKernelGGL(sd::sd_fprof_plan, dim3(fprof_grid(cap)), dim3(sd::FPROF_T), 0, st, a);
    }
    prof_group(w, M, st, rows ? cap : 0, n_ptr);
    SD_HIP(hipMemcpyAsync(w.h_sum.p, w.sum.p, ((size_t)M + 2) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    w.planned = true;
}

int64_t prof_fold(ProfWS& w, ProfDev& d, hipStream_t st, const uint8_t* text) {
    const int M = d.M;
    const int32_t* hs = w.h_sum.p;
    int64_t nd = 0;
    for (int m = 0; m < M; ++m) nd += hs[m];
    if (nd == 0) return 0;
    // (the sizes of nw_profile_device, from the summary instead of its host vectors)
    const int K = d.K, S = sd::nw_block_cols(K);
    const int qmax = std::max(1, (int)hs[M]);
    const int cap = std::max(1, (qmax + S - 1) / S);
    const int64_t R = std::max<int64_t>(1, std::min<int64_t>(64, nd / ((int64_t)d.n_cu * 12 * 64)));
    const int per = (int)(64 * R);
    int64_t n_items = 0;
    for (int m = 0; m < M; ++m) n_items += (hs[m] + per - 1) / per;
    const size_t lane_bytes = (size_t)cap * K * 16;
    int grid = (int)std::min<int64_t>(n_items, (int64_t)d.n_cu * 12);
    grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(((size_t)1 << 30) / (lane_bytes * 64))));
    const size_t lds = (size_t)10 * K * 8 + (size_t)(d.tmax + 1) * 12 * 4;
    const size_t need = lane_bytes * 64 * (size_t)grid;
    if (need > d.ck.cap) {   // the fold in flight reads the old block
        SD_HIP(hipStreamSynchronize(st));
        d.ck.alloc(need);
    }
    prof_items(w, M, per, n_items, st, false);
    sd::launch_nw_profile(K, st, grid, lds, text, w.seg_start.p, w.seg_len.p, w.order.p, w.pair_il.p, w.items.p, (int)n_items,
                          d.peq.p, d.tlen.p, d.poff.p, cap, d.ck.p, d.ckpos.p, d.counts.p, d.fails());
    SD_HIP(hipGetLastError());
    return nd;
}

void prof_add(hipStream_t st, unsigned long long* dst, const unsigned long long* add, int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sd::sd_fprof_add, dim3(fprof_grid(n)), dim3(sd::FPROF_T), 0, st, dst, add, n);
    SD_HIP(hipGetLastError());
}

// the checked arguments of the two test entries: il, own and the rows' bounds
static int fprof_entry_args(const char* text, const int64_t* read_off, int32_t n_reads, const sd_rec* rows, const int64_t* row_off,
                            const uint8_t* keep, const char* const* templates, const int32_t* tlen, int32_t T, uint64_t* counts,
                            std::vector<std::string>& il, std::vector<int32_t>& own, std::vector<int64_t>& poff) {
    if (n_reads < 0 || !read_off || !row_off || T < 1 || !templates || !tlen || !counts) return SD_ERR_PARAM;
    if (read_off[0] < 0 || row_off[0] != 0) return SD_ERR_PARAM;
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_off[r + 1] < read_off[r] || row_off[r + 1] < row_off[r]) return SD_ERR_PARAM;
    const int64_t nB = row_off[n_reads];
    if (nB >= ((int64_t)1 << 31) || (nB > 0 && (!rows || !keep)) || (read_off[n_reads] > 0 && !text)) return SD_ERR_PARAM;
    for (int64_t b = 0; b < nB; ++b)
        if (rows[b].tmpl < 0 || rows[b].tmpl >= 2 * T) return SD_ERR_PARAM;
    il.clear();
    for (int32_t t = 0; t < T; ++t) {
        if (!templates[t] || tlen[t] <= 0) return SD_ERR_PARAM;
        std::string f(templates[t], (size_t)tlen[t]), rc;
        if (!sd::reverse_complement(f, rc)) return SD_ERR_SYMBOL;
        il.push_back(f);
        il.push_back(rc);
    }
    own.resize((size_t)2 * T);   // the DP's order: the monomers, then their reverse complements
    for (int32_t t = 0; t < T; ++t) { own[(size_t)t] = 2 * t; own[(size_t)(T + t)] = 2 * t + 1; }
    std::vector<int32_t> fl((size_t)T);
    for (int32_t t = 0; t < T; ++t) fl[(size_t)t] = tlen[t];
    std::memset(counts, 0, sizeof(uint64_t) * (size_t)sd::profile_offsets(fl, poff));
    return SD_OK;
}

}  // namespace sdi

extern "C" {

int sd_final_profile_host(const char* text, const int64_t* read_off, int32_t n_reads, const sd_rec* rows, const int64_t* row_off,
                          const uint8_t* keep, const char* const* templates, const int32_t* tlen, int32_t T, int32_t device,
                          int32_t threads, uint64_t* counts, int64_t pairs[2]) try {
    std::vector<std::string> il;
    std::vector<int32_t> own;
    std::vector<int64_t> poff;
    const int rc = fprof_entry_args(text, read_off, n_reads, rows, row_off, keep, templates, tlen, T, counts, il, own, poff);
    if (rc) return rc;
    int tmax = 1;
    for (const std::string& t : il) tmax = std::max(tmax, (int)t.size());
    std::vector<const char*> q;
    std::vector<int32_t> ql, pil;
    int64_t n_dev = 0, n_host = 0;
    for (int32_t r = 0; r < n_reads; ++r)
        for (int64_t b = row_off[r]; b < row_off[r + 1]; ++b) {
            if (!keep[b]) continue;
            const int32_t x = own[(size_t)rows[b].tmpl];
            const sd::FProfPair p = sd::final_prof_pair(rows[b].start, rows[b].end, read_off[r + 1] - read_off[r], read_off[r], x,
                                                        (int32_t)il[(size_t)x].size(), tmax);
            if (p.cls == sd::FPROF_NONE) continue;
            (p.cls == sd::FPROF_DEV ? n_dev : n_host) += 1;
            q.push_back(text + p.start);
            ql.push_back(p.len);
            pil.push_back(p.il);
        }
    if (pairs) { pairs[0] = n_dev; pairs[1] = n_host; }
    return sd::profile_host(q.data(), ql.data(), pil.data(), (int64_t)q.size(), il, std::max(1, (int)threads), counts);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_final_profile_dev(const char* text, const int64_t* read_off, int32_t n_reads, const sd_rec* rows, const int64_t* row_off,
                         const uint8_t* keep, const char* const* templates, const int32_t* tlen, int32_t T, int32_t device,
                         int32_t threads, uint64_t* counts, int64_t pairs[2]) try {
    static_assert(sizeof(sd_rec) == sizeof(sd::DevRec), "record layout");
    std::vector<std::string> il;
    std::vector<int32_t> own;
    std::vector<int64_t> poff;
    int rc = fprof_entry_args(text, read_off, n_reads, rows, row_off, keep, templates, tlen, T, counts, il, own, poff);
    if (rc) return rc;
    if (device < 0) return SD_ERR_PARAM;
    if ((rc = device_check(device, nullptr, 0))) return rc;   // (device < 0: refused above)
    hipStream_t st = nullptr;
    try {
        SD_HIP(hipSetDevice(device));
        SD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        const size_t nr = (size_t)n_reads, nB = (size_t)row_off[n_reads];
        const size_t nt = (size_t)read_off[n_reads];
        ProfDev d;
        d.setup(il, own, st);
        ProfWS w;
        DevBuf<uint8_t> d_text, d_keep;
        DevBuf<sd::DevRec> d_rows;
        DevBuf<int64_t> d_moff, d_rlen;
        std::vector<int64_t> rlen(nr + 1, 0);
        for (size_t r = 0; r < nr; ++r) rlen[r] = read_off[r + 1] - read_off[r];
        d_text.alloc(nt + 8);
        d_keep.alloc(nB);
        d_rows.alloc(nB);
        d_moff.alloc(nr + 1);
        d_rlen.alloc(nr + 1);
        w.text_off.alloc(nr + 1);
        if (nt) SD_HIP(hipMemcpyAsync(d_text.p, text, nt, hipMemcpyHostToDevice, st));
        if (nB) SD_HIP(hipMemcpyAsync(d_keep.p, keep, nB, hipMemcpyHostToDevice, st));
        if (nB) SD_HIP(hipMemcpyAsync(d_rows.p, rows, nB * sizeof(sd_rec), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(d_moff.p, row_off, (nr + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(d_rlen.p, rlen.data(), (nr + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemcpyAsync(w.text_off.p, read_off, (nr + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        prof_plan(w, d, st, d_rows.p, nullptr, d_keep.p, d_moff.p, d_rlen.p, n_reads, (int64_t)nB, d_moff.p + nr);
        SD_HIP(hipStreamSynchronize(st));
        const int64_t nd = prof_fold(w, d, st, d_text.p);
        const int64_t nh = w.h_sum.p[d.M + 1];
        if (pairs) { pairs[0] = nd; pairs[1] = nh; }
        // the host's pairs, under the kernel: 16 bytes each come down, their text is the caller's
        if (nh > 0) {
            std::vector<sd::FProfHostPair> hp((size_t)nh);
            SD_HIP(hipMemcpyAsync(hp.data(), w.hlist.p, (size_t)nh * sizeof(sd::FProfHostPair), hipMemcpyDeviceToHost, st));
            SD_HIP(hipStreamSynchronize(st));
            std::vector<const char*> q((size_t)nh);
            std::vector<int32_t> ql((size_t)nh), pil((size_t)nh);
            for (size_t x = 0; x < (size_t)nh; ++x) { q[x] = text + hp[x].start; ql[x] = hp[x].len; pil[x] = hp[x].il; }
            rc = sd::profile_host(q.data(), ql.data(), pil.data(), nh, il, std::max(1, (int)threads), counts);
        }
        std::vector<unsigned long long> dc((size_t)d.total + 8);
        SD_HIP(hipMemcpyAsync(dc.data(), d.counts.p, dc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        SD_HIP(hipStreamSynchronize(st));   // (the buffers go back with nothing in flight on them)
        int fails = 0;
        std::memcpy(&fails, dc.data() + d.total, sizeof fails);
        if (rc == SD_OK && fails) rc = SD_ERR_INTERNAL;
        for (int64_t i = 0; i < d.total; ++i) counts[i] += dc[(size_t)i];
    } catch (const HipFail&) {
        rc = SD_ERR_HIP;
    }
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    return rc;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
