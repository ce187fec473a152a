// sd_msa.hip -- the rows of --msa on the device: the walk of sd_nw_profile (sd_nw.hip) with a second sink.  Where the profile
// adds every step of a pair into its monomer's counters, NwMsa writes it into the pair's own row (sd_msa.hpp: the forward
// monomer's L columns, then its L + 1 insertion slots), so the rows of a job summed per monomer are its profile.
//
// Work items, grouping and checkpoints are the profile kernel's: one-wave workgroups, an item is up to `per` pairs of ONE
// forward monomer, the masks of m and rc(m) in LDS, a lane owns a pair.  A pass of 64 pairs stages its rows in LDS in the
// counters' place and the wave streams them out with 16-byte stores (the pitch is a multiple of 16, so is every row's
// offset); where 64 rows of the set's longest monomer do not fit the launch's 64 KB (monomers of 496 bp and more)
// the lane writes through to its row in HBM instead (stage = 0).
#include <algorithm>
#include <cstring>
#include <mutex>

#include "sd_final_ws.hpp"
#include "sd_job_dev.hpp"
#include "sd_msa.hpp"
#include "sd_nw_kernel.hpp"
#include "sd_scan_dev.hpp"

namespace sd {

struct NwMsa : MsaRow {};

__device__ __forceinline__ uint4 msa_clear16(int b, int L) {
    return make_uint4(msa_clear_word(b, L), msa_clear_word(b + 4, L), msa_clear_word(b + 8, L), msa_clear_word(b + 12, L));
}

template <int K>
__global__ __launch_bounds__(64) void sd_nw_msa(const uint8_t* __restrict__ seq, const int64_t* __restrict__ seg_start,
                                                const int32_t* __restrict__ seg_len, const int32_t* __restrict__ order,
                                                const int32_t* __restrict__ pair_il, const int4* __restrict__ items, int n_items,
                                                const unsigned long long* __restrict__ peq, const int32_t* __restrict__ tlen,
                                                int cap, uint4* __restrict__ ck, int* __restrict__ ckpos, int stage,
                                                uint8_t* __restrict__ out, const int64_t* __restrict__ row_at,
                                                uint8_t* __restrict__ status, int* __restrict__ fails) {
    extern __shared__ __align__(16) unsigned long long smem[];   // [2][5][K] masks of m and rc(m), [64] row offsets, then (stage) 64 rows
    int64_t* dst = reinterpret_cast<int64_t*>(smem + 10 * K);
    uint8_t* rows = reinterpret_cast<uint8_t*>(smem + 10 * K + 64);
    uint32_t* ckl = reinterpret_cast<uint32_t*>(ck) + (size_t)blockIdx.x * (size_t)cap * K * 4 * 64 + threadIdx.x;
    int* ckp = ckpos + threadIdx.x;   // (not written: no homopolymer compression)
    for (int w = blockIdx.x; w < n_items; w += gridDim.x) {
        const int4 it = items[w];
        const int m = it.x;
        const int L = tlen[2 * m];
        const int pitch = SD_MSA_PITCH(L), chunks = pitch >> 4;
        __syncthreads();   // the previous item's walks have read their masks
        for (int i = threadIdx.x; i < 10 * K; i += blockDim.x) smem[i] = peq[(size_t)2 * m * 5 * K + i];
        __syncthreads();
        for (int p0 = it.y; p0 < it.z; p0 += 64) {
            const int p = p0 + (int)threadIdx.x;
            const bool have = p < it.z;
            const int n = min(64, it.z - p0);
            const int sg = have ? order[p] : 0;
            uint8_t* row = nullptr;
            if (stage) {
                __syncthreads();   // the previous pass has streamed its rows out
                for (int idx = threadIdx.x; idx < n * chunks; idx += 64) {
                    const int r = idx / chunks, c = idx - r * chunks;
                    *reinterpret_cast<uint4*>(rows + (size_t)r * pitch + 16 * c) = msa_clear16(16 * c, L);
                }
                if (have) dst[threadIdx.x] = row_at[sg];
                __syncthreads();
                row = rows + (size_t)threadIdx.x * pitch;
            } else if (have) {
                row = out + row_at[sg];
                for (int c = 0; c < chunks; ++c) *reinterpret_cast<uint4*>(row + 16 * c) = msa_clear16(16 * c, L);
            }
            if (have) {
                const int rc = pair_il[sg] & 1;
                NwQueryAscii q{seq, seg_start[sg]};
                NwMsa sink{{row, L, rc != 0}};
                int d = 0, mm = 0;
                if (nw_pair<K, NwQueryAscii, NwMsa>(q, seg_len[sg], reinterpret_cast<const uint2*>(smem + rc * 5 * K), L, false, ckl,
                                                    ckp, (size_t)64, cap, d, mm, &sink))
                    status[sg] = MSA_ST_DONE;
                else
                    atomicAdd(fails, 1);
            }
            if (stage) {
                __syncthreads();
                for (int idx = threadIdx.x; idx < n * chunks; idx += 64) {
                    const int r = idx / chunks, c = idx - r * chunks;
                    *reinterpret_cast<uint4*>(out + dst[r] + 16 * c) = *reinterpret_cast<const uint4*>(rows + (size_t)r * pitch + 16 * c);
                }
            }
        }
    }
}

size_t nw_msa_lds_bytes(int K, int tmax, int* stage) {
    const size_t fixed = (size_t)10 * K * 8 + 64 * 8, staged = fixed + (size_t)64 * SD_MSA_PITCH(tmax);
    const bool st = staged <= (size_t)64 * 1024;
    if (stage) *stage = st ? 1 : 0;
    return st ? staged : fixed;
}

void launch_nw_msa(int K, hipStream_t st, int grid, int tmax, const uint8_t* seq, const int64_t* seg_start, const int32_t* seg_len,
                   const int32_t* order, const int32_t* pair_il, const int4* items, int n_items, const unsigned long long* peq,
                   const int32_t* tlen, int cap, void* ck, int* ckpos, uint8_t* out, const int64_t* row_at, uint8_t* status,
                   int* fails) {
    int stage = 0;
    const size_t lds = nw_msa_lds_bytes(K, tmax, &stage);
#define SD_NWM(KK)                                                                                                            \
    hipLaunchKernelGGL(sd_nw_msa<KK>, dim3(grid), dim3(64), lds, st, seq, seg_start, seg_len, order, pair_il, items, n_items, \
                       peq, tlen, cap, reinterpret_cast<uint4*>(ck), ckpos, stage, out, row_at, status, fails)
    switch (K) {
        case 1: SD_NWM(1); break;
        case 2: SD_NWM(2); break;
        case 3: SD_NWM(3); break;
        case 4: SD_NWM(4); break;
        case 6: SD_NWM(6); break;
        default: SD_NWM(8); break;
    }
#undef SD_NWM
}

int64_t msa_row_offsets(const int32_t* tlen, int32_t T, const int32_t* pair_il, int64_t n, int64_t* row_at) {
    int64_t at = 0;
    for (int64_t s = 0; s < n; ++s) {
        row_at[s] = at;
        const int il = pair_il[s];
        if (il < 0 || il >= 2 * T || tlen[il >> 1] < 0) return -1;
        at += SD_MSA_PITCH((int64_t)tlen[il >> 1]);
    }
    row_at[n] = at;
    return at;
}

namespace {
// device buffers of sd_msa_segments_dev, kept between calls (the command line calls once per read; calls serialise)
struct MsaCtx {
    int dev = -1;
    DevBuf<uint8_t> seq, ck, out, status;
    DevBuf<int64_t> starts, row_at;
    DevBuf<int32_t> lens, pair, order, tlen, items;
    DevBuf<unsigned long long> peq;
    DevBuf<int> ckpos, fails;
};
std::mutex g_msa_m;
MsaCtx* g_msa = nullptr;
inline bool msa_sym_ok(char ch) { return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == 'N'; }
}  // namespace

// Rows of segments of a text on the device: pairs of monomers up to 512 bp and segments up to 1024 bp that edlib aligns by
// its block traceback go to sd_nw_msa, the others -- and every pair when the text or a monomer holds a symbol outside
// ACGTN -- to the host fold (msa_host) under the kernel: the split of nw_profile_device.
int nw_msa_device(const char* seq, int64_t seqlen, const int64_t* seg_start, const int32_t* seg_len, int64_t n_seg,
                  const std::vector<std::string>& il, const int32_t* pair_il, int device, int threads, uint8_t* rows,
                  const int64_t* row_at, uint8_t* status, const MsaBench* bench) try {
    constexpr int NWM_QMAX = 1024;
    const int M = (int)il.size() / 2;
    if (n_seg == 0 || M == 0) return SD_OK;
    if (n_seg > 0x7fffffff) return SD_ERR_UNSUPPORTED;
    if (const int rc = sdi::device_check(device, nullptr, 0)) return rc;
    int tmax = 1;
    bool dev_ok = true;
    for (const std::string& t : il) {
        tmax = std::max(tmax, (int)t.size());
        for (char ch : t) dev_ok = dev_ok && msa_sym_ok(ch);
    }
    dev_ok = dev_ok && tmax <= 512;
    if (dev_ok) {   // the alphabet of the text (pieces of 1 MB over all threads)
        const int64_t np = (seqlen + (1 << 20) - 1) >> 20;
        std::vector<uint8_t> bad((size_t)std::max<int64_t>(np, 1), 0);
        sd::parallel_for(np, threads, 1, [&](int64_t x) {
            const int64_t e = std::min<int64_t>(seqlen, (x + 1) << 20);
            uint8_t b = 0;
            for (int64_t i = x << 20; i < e; ++i) b |= (uint8_t)!msa_sym_ok(seq[i]);
            bad[(size_t)x] = b;
        });
        for (uint8_t b : bad) dev_ok = dev_ok && !b;
    }
    // the kernel's pairs grouped by forward monomer (counting sort), the host's pairs as a list
    auto takes = [&](int64_t s) {
        const int64_t L = (int64_t)il[(size_t)pair_il[s]].size();
        return dev_ok && seg_len[s] <= NWM_QMAX && !sd::edlib_splits(seg_len[s], L);
    };
    std::vector<int32_t> order, per_m((size_t)M + 1, 0);
    std::vector<const char*> hq;
    std::vector<int32_t> hl, hp;
    std::vector<int64_t> hs, dev_at((size_t)n_seg, 0);
    int qmax = 1;
    int64_t dev_bytes = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        const int64_t L = (int64_t)il[(size_t)pair_il[s]].size();
        if (seg_len[s] <= 0 || L == 0) continue;   // no alignment: not an instance
        if (takes(s)) {
            ++per_m[(size_t)(pair_il[s] >> 1) + 1];
            qmax = std::max(qmax, (int)seg_len[s]);
            dev_at[(size_t)s] = dev_bytes;
            dev_bytes += SD_MSA_PITCH(L);
        } else {
            hq.push_back(seq + seg_start[s]);
            hl.push_back(seg_len[s]);
            hp.push_back(pair_il[s]);
            hs.push_back(s);
        }
    }
    for (int m = 0; m < M; ++m) per_m[(size_t)m + 1] += per_m[(size_t)m];
    const int64_t nd = per_m[(size_t)M];
    order.resize((size_t)nd);
    {
        std::vector<int32_t> at(per_m.begin(), per_m.end() - 1);
        for (int64_t s = 0; s < n_seg; ++s) {
            if (seg_len[s] <= 0 || il[(size_t)pair_il[s]].empty()) continue;
            if (takes(s)) order[(size_t)at[(size_t)(pair_il[s] >> 1)]++] = (int32_t)s;
        }
    }
    std::lock_guard<std::mutex> g(g_msa_m);
    if (nd > 0) {
        SD_HIP(hipSetDevice(device));
        if (!g_msa || g_msa->dev != device) {
            delete g_msa;   // (its blocks go to the pools)
            g_msa = new MsaCtx;
            g_msa->dev = device;
        }
        MsaCtx& c = *g_msa;
        hipDeviceProp_t prop;
        SD_HIP(hipGetDeviceProperties(&prop, device));
        const int n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        int K = (tmax + 63) / 64;
        if (K == 5) K = 6;
        if (K == 7) K = 8;
        const int S = sd::nw_block_cols(K);
        const int cap = std::max(1, (qmax + S - 1) / S);
        // (the items and the grid of nw_profile_device)
        const int64_t R = std::max<int64_t>(1, std::min<int64_t>(64, nd / ((int64_t)n_cu * 12 * 64)));
        const int64_t per = 64 * R;
        std::vector<int4> items;
        for (int m = 0; m < M; ++m)
            for (int64_t a = per_m[(size_t)m]; a < per_m[(size_t)m + 1]; a += per)
                items.push_back(make_int4(m, (int)a, (int)std::min<int64_t>(a + per, per_m[(size_t)m + 1]), 0));
        const int n_items = (int)items.size();
        const size_t lane_bytes = (size_t)cap * K * 16;
        int grid = (int)std::min<int64_t>(n_items, (int64_t)n_cu * 12);
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(((size_t)1 << 30) / (lane_bytes * 64))));
        std::vector<unsigned long long> peq;
        std::vector<int32_t> tl;
        sd::nw_build_masks(il, K, peq, tl);
        c.seq.alloc((size_t)seqlen + 8);
        c.starts.alloc((size_t)n_seg);
        c.lens.alloc((size_t)n_seg);
        c.pair.alloc((size_t)n_seg);
        c.row_at.alloc((size_t)n_seg);
        c.status.alloc((size_t)n_seg);
        c.order.alloc((size_t)nd);
        c.items.alloc(items.size() * 4);
        c.peq.alloc(peq.size());
        c.tlen.alloc(tl.size());
        c.ck.alloc(lane_bytes * 64 * (size_t)grid);
        c.ckpos.alloc(64);
        c.fails.alloc(16);
        c.out.alloc((size_t)dev_bytes);
        SD_HIP(hipMemcpy(c.seq.p, seq, (size_t)seqlen, hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(c.starts.p, seg_start, sizeof(int64_t) * (size_t)n_seg, hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(c.lens.p, seg_len, sizeof(int32_t) * (size_t)n_seg, hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(c.pair.p, pair_il, sizeof(int32_t) * (size_t)n_seg, hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(c.row_at.p, dev_at.data(), sizeof(int64_t) * (size_t)n_seg, hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(c.order.p, order.data(), sizeof(int32_t) * (size_t)nd, hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(c.items.p, items.data(), sizeof(int4) * items.size(), hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(c.peq.p, peq.data(), sizeof(unsigned long long) * peq.size(), hipMemcpyHostToDevice));
        SD_HIP(hipMemcpy(c.tlen.p, tl.data(), sizeof(int32_t) * tl.size(), hipMemcpyHostToDevice));
        SD_HIP(hipMemset(c.status.p, 0, (size_t)n_seg));
        SD_HIP(hipMemset(c.fails.p, 0, sizeof(int) * 16));
        auto walk = [&]() {
            launch_nw_msa(K, nullptr, grid, tmax, c.seq.p, c.starts.p, c.lens.p, c.order.p, c.pair.p,
                          reinterpret_cast<const int4*>(c.items.p), n_items, c.peq.p, c.tlen.p, cap, c.ck.p, c.ckpos.p, c.out.p,
                          c.row_at.p, c.status.p, c.fails.p);
            SD_HIP(hipGetLastError());
        };
        if (bench) {   // (tools/msa_bench.py) the row kernel and the profile kernel in turn on these pairs, each between two events
            std::vector<int32_t> fl((size_t)M);
            for (int m = 0; m < M; ++m) fl[(size_t)m] = (int32_t)il[(size_t)(2 * m)].size();
            std::vector<int64_t> off;
            const int64_t total = profile_offsets(fl, off);
            DevBuf<int64_t> poff;
            DevBuf<unsigned long long> pcnt;
            poff.upload(off);
            pcnt.alloc((size_t)total + 8);
            SD_HIP(hipMemset(pcnt.p, 0, ((size_t)total + 8) * sizeof(unsigned long long)));
            const size_t plds = (size_t)10 * K * 8 + (size_t)(tmax + 1) * 12 * 4;
            hipEvent_t e0 = nullptr, e1 = nullptr;
            SD_HIP(hipEventCreate(&e0));
            SD_HIP(hipEventCreate(&e1));
            for (int it = 0; it < bench->warmup + bench->reps; ++it)
                for (int which = 0; which < 2; ++which) {
                    SD_HIP(hipEventRecord(e0, nullptr));
                    if (which == 0) walk();
                    else launch_nw_profile(K, nullptr, grid, plds, c.seq.p, c.starts.p, c.lens.p, c.order.p, c.pair.p,
                                           reinterpret_cast<const int4*>(c.items.p), n_items, c.peq.p, c.tlen.p, poff.p, cap, c.ck.p,
                                           c.ckpos.p, pcnt.p, reinterpret_cast<int*>(pcnt.p + total));
                    SD_HIP(hipEventRecord(e1, nullptr));
                    SD_HIP(hipEventSynchronize(e1));
                    float ms = 0;
                    SD_HIP(hipEventElapsedTime(&ms, e0, e1));
                    if (it >= bench->warmup) (which == 0 ? bench->ms_msa : bench->ms_profile)[it - bench->warmup] = ms;
                }
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            bench->info[0] = K; bench->info[1] = grid; bench->info[2] = n_items; bench->info[3] = (int64_t)nd;
            int stage = 0;
            bench->info[4] = (int64_t)nw_msa_lds_bytes(K, tmax, &stage);
            bench->info[5] = stage;
            bench->info[6] = (int64_t)plds;
            bench->info[7] = cap;
        }
        walk();
    }
    // the host's pairs, under the kernel
    int hrc = SD_OK;
    if (!hq.empty()) {
        std::vector<int64_t> hat(hq.size());
        std::vector<uint8_t> hst(hq.size(), 0);
        for (size_t x = 0; x < hq.size(); ++x) hat[x] = row_at[hs[x]];
        hrc = msa_host(hq.data(), hl.data(), hp.data(), (int64_t)hq.size(), il, threads, rows, hat.data(), hst.data());
        for (size_t x = 0; x < hq.size(); ++x) status[hs[x]] = hst[x];
    }
    if (nd > 0) {
        MsaCtx& c = *g_msa;
        std::vector<uint8_t> dr((size_t)dev_bytes), ds((size_t)n_seg);
        int fails = 0;
        SD_HIP(hipMemcpy(dr.data(), c.out.p, (size_t)dev_bytes, hipMemcpyDeviceToHost));
        SD_HIP(hipMemcpy(ds.data(), c.status.p, (size_t)n_seg, hipMemcpyDeviceToHost));
        SD_HIP(hipMemcpy(&fails, c.fails.p, sizeof fails, hipMemcpyDeviceToHost));
        if (fails) return SD_ERR_INTERNAL;   // cannot happen: the checkpoints are sized by the longest segment
        for (int64_t x = 0; x < nd; ++x) {
            const int64_t s = order[(size_t)x];
            std::memcpy(rows + row_at[s], dr.data() + dev_at[(size_t)s], (size_t)(row_at[s + 1] - row_at[s]));
            status[s] = ds[(size_t)s];
        }
    }
    return hrc;
} catch (const HipFail&) {
    return SD_ERR_HIP;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // namespace sd

// ---- the device-resident form: final rows in HBM + the reads' text in HBM -> rows of --msa in the caller's buffers ----
//   sd_msa_gather   the reads' bytes, wherever they lie in the caller's buffer, back to back into the object's own text
//                   (the walk reads aligned dwords up to the next multiple of 4 past a segment's end)
//   sd_msa_plan     one lane per final row: its pair (final_prof_pair: the segment the selection measured, the row's own
//                   interleaved template), its class, its pitch; per forward monomer the number of kernel pairs, the
//                   longest such segment, the class counts; its first lane writes the row count the grouping reads
//   exclusive_scan_dev   (sd_scan_dev.hpp) exclusive prefix of the pitches, in place: the rows' places
//   sd_msa_fill     status of every row; the rows of pairs the kernel does not take, cleared
// Grouping and work items are those of the device profile (prof_group / prof_items), the walk is sd_nw_msa.
namespace sd {

constexpr int MSA_T = 256;
enum { MSA_SUM_QMAX = 0, MSA_SUM_HOST = 1, MSA_SUM_NONE = 2, MSA_SUM_BAD = 3 };   // w.sum[M + ...] (the first two: sd_fprof's)

__global__ __launch_bounds__(MSA_T) void sd_msa_gather(const uint8_t* __restrict__ src, const int64_t* __restrict__ roff,
                                                       const int64_t* __restrict__ toff, int n_reads, uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * MSA_T + threadIdx.x;
    if (i >= toff[n_reads]) return;
    int lo = 0, hi = n_reads - 1;   // the read that owns byte i: the first r with toff[r + 1] > i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (toff[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    dst[i] = src[roff[lo] + (i - toff[lo])];
}

void launch_text_gather(hipStream_t st, const uint8_t* src, const int64_t* roff, const int64_t* toff, int n_reads, int64_t text,
                        uint8_t* dst) {
    if (text <= 0) return;
    hipLaunchKernelGGL(sd_msa_gather, dim3((unsigned)((text + MSA_T - 1) / MSA_T)), dim3(MSA_T), 0, st, src, roff, toff, n_reads, dst);
}

struct MsaPlanArgs {
    const sd_final_row* rows;
    int64_t n;
    const int32_t* key_il;
    int n_keys;
    const int32_t* tlen;       // interleaved
    int tmax, M;
    const int64_t* rlen;
    const int64_t* text_off;
    int n_reads;
    int64_t* seg_start;
    int32_t* seg_len;
    int32_t* pair_il;
    uint8_t* cls;
    int32_t* sum;              // M + 4
    int64_t* row_at;           // the row's pitch, scanned afterwards
    int64_t* n_ptr;            // = n (prof_group's n_ptr)
};

__global__ __launch_bounds__(MSA_T) void sd_msa_plan(MsaPlanArgs a) {
    const int64_t i = (int64_t)blockIdx.x * MSA_T + threadIdx.x;
    if (i >= a.n) return;
    if (i == 0) *a.n_ptr = a.n;
    const sd_final_row x = a.rows[i];
    uint8_t c = FPROF_NONE;
    int32_t il = -1, len = 0;
    int64_t start = 0, pitch = 0;
    if (x.best < 0 || x.best >= a.n_keys || x.read < 0 || x.read >= a.n_reads) {
        atomicAdd(&a.sum[a.M + MSA_SUM_BAD], 1);
    } else {
        il = a.key_il[x.best];
        const FProfPair p = final_prof_pair(x.start, x.end, a.rlen[x.read], a.text_off[x.read], il, a.tlen[il], a.tmax);
        start = p.start;
        len = p.len;
        c = p.cls;
        pitch = SD_MSA_PITCH((int64_t)a.tlen[il]);
        if (c == FPROF_DEV) {
            atomicAdd(&a.sum[il >> 1], 1);
            atomicMax(&a.sum[a.M + MSA_SUM_QMAX], len);
        } else {
            atomicAdd(&a.sum[a.M + (c == FPROF_HOST ? MSA_SUM_HOST : MSA_SUM_NONE)], 1);
        }
    }
    a.seg_start[i] = start;
    a.seg_len[i] = len;
    a.pair_il[i] = il;
    a.cls[i] = c;
    a.row_at[i] = pitch;
}

__global__ __launch_bounds__(MSA_T) void sd_msa_fill(const uint8_t* __restrict__ cls, const int32_t* __restrict__ pair_il,
                                                     const int32_t* __restrict__ tlen, const int64_t* __restrict__ row_at, int64_t n,
                                                     uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * MSA_T + threadIdx.x;
    if (i >= n) return;
    const uint8_t c = cls[i];
    status[i] = c == FPROF_HOST ? MSA_ST_LEFT : MSA_ST_NONE;   // (a kernel pair: 1 once sd_nw_msa has walked it)
    if (c == FPROF_DEV || pair_il[i] < 0) return;
    const int L = tlen[pair_il[i]];
    uint8_t* row = out + row_at[i];
    const int chunks = (int)((row_at[i + 1] - row_at[i]) >> 4);
    for (int k = 0; k < chunks; ++k) *reinterpret_cast<uint4*>(row + 16 * k) = msa_clear16(16 * k, L);
}

}  // namespace sd

struct sd_msa_tables {
    std::vector<std::string> il;             // m0, rc(m0), m1, ...
    std::vector<int32_t> key_il;
    std::mutex m;
    int device = -1;                         // where the templates were uploaded (-1: not yet)
    ProfDev d;
    ProfWS w;
    DevBuf<uint8_t> text;
    DevBuf<int64_t> reads, n_ptr;            // [roff | rlen | text_off] (n_reads + 1 each); the rows of the last size pass
    DevBuf<int64_t> tsum, tbase;             // the tiles of the scan of row_at
    PinBuf<int64_t> h_reads, h_tot;
    PinBuf<int32_t> h_sum;                   // qmax, host pairs, no instance, bad rows, failed walks
    hipEvent_t ev_size = nullptr, ev_use = nullptr;
    hipStream_t use_stream = nullptr;
    bool used = false;                       // ev_use has been recorded: a kernel may still read the buffers
    // the last size pass
    const void* rows_of = nullptr;
    int64_t n_rows = -1, total = 0, nd = 0;
    int qmax = 1;
};

namespace sdi {
static inline unsigned msa_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + sd::MSA_T - 1) / sd::MSA_T); }
static void msa_used(sd_msa_tables* t, hipStream_t st) {
    if (t->used && t->use_stream != st) SD_HIP(hipEventSynchronize(t->ev_use));   // (an event remembers one stream)
    SD_HIP(hipEventRecord(t->ev_use, st));
    t->use_stream = st;
    t->used = true;
}
static int msa_dev_check(sd_msa_tables* t, int32_t device, hipStream_t st, char* eb, size_t el) {
    if (const int rc = device_check(device, eb, el)) return rc;
    if (t->device >= 0 && t->device != device) {
        set_err(eb, el, "the templates lie on device " + std::to_string(t->device) + ", the call names device " + std::to_string(device));
        return SD_ERR_PARAM;
    }
    return SD_OK;
}
}  // namespace sdi

extern "C" {

int sd_msa_tables_create(sd_msa_tables** out, const int32_t* key_il, int32_t n_keys, const char* const* mono_seqs,
                         const int32_t* mono_lens, int32_t n_mono, char* errbuf, size_t errlen) try {
    if (!out || n_keys < 0 || n_mono < 1 || (n_keys > 0 && !key_il) || !mono_seqs || !mono_lens) {
        set_err(errbuf, errlen, "sd_msa_tables_create: missing argument");
        return SD_ERR_PARAM;
    }
    std::unique_ptr<sd_msa_tables> t(new sd_msa_tables);
    for (int32_t m = 0; m < n_mono; ++m) {
        if (!mono_seqs[m] || mono_lens[m] <= 0) { set_err(errbuf, errlen, "sd_msa_tables_create: empty monomer"); return SD_ERR_PARAM; }
        std::string f(mono_seqs[m], (size_t)mono_lens[m]), rc;
        if (!sd::reverse_complement(f, rc)) { set_err(errbuf, errlen, "sd_msa_tables_create: a monomer holds a symbol outside ACGTN"); return SD_ERR_SYMBOL; }
        t->il.push_back(f);
        t->il.push_back(rc);
    }
    for (int32_t k = 0; k < n_keys; ++k) {
        if (key_il[k] < 0 || key_il[k] >= 2 * n_mono) { set_err(errbuf, errlen, "sd_msa_tables_create: a key names no template"); return SD_ERR_PARAM; }
        t->key_il.push_back(key_il[k]);
    }
    *out = t.release();
    return SD_OK;
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

void sd_msa_tables_destroy(sd_msa_tables* t) {
    if (!t) return;
    if (t->used && hipEventSynchronize(t->ev_use) != hipSuccess) (void)hipGetLastError();   // (the buffers go to a pool below)
    if (t->ev_size) (void)hipEventDestroy(t->ev_size);
    if (t->ev_use) (void)hipEventDestroy(t->ev_use);
    delete t;
}

int sd_msa_final_size_dev(sd_msa_tables* t, const sd_final_row* d_rows, int64_t n_rows, const void* d_text, const int64_t* read_off,
                          const int64_t* read_lens, int32_t n_reads, int32_t device, void* hip_stream, int64_t* d_row_at,
                          int64_t* total_bytes, int64_t classes[3], char* errbuf, size_t errlen) try {
    static const char* who = "sd_msa_final_size_dev";
    if (!t || n_rows < 0 || n_rows >= ((int64_t)1 << 31) || n_reads < 0 || !d_row_at || !total_bytes || (n_rows > 0 && !d_rows) ||
        (n_reads > 0 && (!read_off || !read_lens))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    int64_t text = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_off[r] < 0 || read_lens[r] < 0) { set_err(errbuf, errlen, std::string(who) + ": negative read offset or length"); return SD_ERR_PARAM; }
        text += read_lens[r];
    }
    if (text > 0 && !d_text) { set_err(errbuf, errlen, std::string(who) + ": missing text"); return SD_ERR_PARAM; }
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    int rc = msa_dev_check(t, device, st, errbuf, errlen);
    if (rc) return rc;
    try {
        std::lock_guard<std::mutex> g(t->m);
        DeviceScope on(device);
        if ((rc = buffer_on_device(d_row_at, device, who, "row offset", errbuf, errlen))) return rc;
        if (n_rows > 0 && (rc = buffer_on_device(d_rows, device, who, "row", errbuf, errlen))) return rc;
        if (text > 0 && (rc = buffer_on_device(d_text, device, who, "text", errbuf, errlen))) return rc;
        if (t->device < 0) {
            t->d.setup(t->il, t->key_il, st);
            ensure_event(t->ev_size, hipEventDisableTiming);
            ensure_event(t->ev_use, hipEventDisableTiming);
            t->device = device;
        }
        if (t->used) SD_HIP(hipEventSynchronize(t->ev_use));   // a write pass in flight reads the plan this one overwrites
        t->n_rows = -1;
        const int M = t->d.M;
        const size_t nr = (size_t)n_reads + 1, cap = (size_t)n_rows;
        ProfWS& w = t->w;
        t->h_reads.alloc(3 * nr);
        t->reads.alloc(3 * nr);
        t->text.alloc((size_t)text + 8);
        t->n_ptr.alloc(1);
        t->tsum.alloc((size_t)sd::scan_tiles_of(n_rows));
        t->tbase.alloc((size_t)sd::scan_tiles_of(n_rows) + 1);
        t->h_tot.alloc(1);
        t->h_sum.alloc(8);
        w.seg_start.alloc(cap);
        w.seg_len.alloc(cap);
        w.pair_il.alloc(cap);
        w.order.alloc(cap);
        w.cls.alloc(cap);
        w.hlist.alloc(cap);
        w.sum.alloc((size_t)M + 4);
        w.base.alloc((size_t)M + 1);
        w.cursor.alloc((size_t)M + 1);
        int64_t* roff = t->h_reads.p, *rlen = roff + nr, *toff = rlen + nr;
        int64_t at = 0;
        for (int32_t r = 0; r < n_reads; ++r) { roff[r] = read_off[r]; rlen[r] = read_lens[r]; toff[r] = at; at += read_lens[r]; }
        roff[n_reads] = 0; rlen[n_reads] = 0; toff[n_reads] = at;
        SD_HIP(hipMemcpyAsync(t->reads.p, t->h_reads.p, 3 * nr * sizeof(int64_t), hipMemcpyHostToDevice, st));
        SD_HIP(hipMemsetAsync(w.sum.p, 0, ((size_t)M + 4) * sizeof(int32_t), st));
        sd::launch_text_gather(st, static_cast<const uint8_t*>(d_text), t->reads.p, t->reads.p + 2 * nr, (int)n_reads, text, t->text.p);
        if (n_rows > 0) {
            sd::MsaPlanArgs a{d_rows, n_rows, t->d.own_il.p, (int)t->key_il.size(), t->d.tlen.p, t->d.tmax, M, t->reads.p + nr,
                              t->reads.p + 2 * nr, (int)n_reads, w.seg_start.p, w.seg_len.p, w.pair_il.p, w.cls.p, w.sum.p, d_row_at, t->n_ptr.p};
            hipLaunchKernelGGL(sd::sd_msa_plan, dim3(msa_grid(n_rows)), dim3(sd::MSA_T), 0, st, a);
        }
        sd::exclusive_scan_dev(st, sd::ScanArray<int64_t>{d_row_at}, n_rows, d_row_at, t->tsum.p, t->tbase.p);
        SD_HIP(hipGetLastError());
        SD_HIP(hipMemcpyAsync(t->h_tot.p, d_row_at + n_rows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        SD_HIP(hipMemcpyAsync(t->h_sum.p, w.sum.p + M, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SD_HIP(hipMemcpyAsync(t->h_sum.p + 4, t->d.fails(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SD_HIP(hipEventRecord(t->ev_size, st));
        SD_HIP(hipEventSynchronize(t->ev_size));   // the only wait: the bytes and the class counts
        const int32_t* hs = t->h_sum.p;
        if (hs[4]) { set_err(errbuf, errlen, std::string(who) + ": a walk of the previous write pass ran out of checkpoints"); return SD_ERR_INTERNAL; }
        if (hs[sd::MSA_SUM_BAD]) {
            set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(hs[sd::MSA_SUM_BAD]) + " rows with a read or key index outside its table");
            return SD_ERR_PARAM;
        }
        t->rows_of = d_rows;
        t->n_rows = n_rows;
        t->total = t->h_tot.p[0];
        t->qmax = std::max(1, (int)hs[sd::MSA_SUM_QMAX]);
        t->nd = n_rows - hs[sd::MSA_SUM_HOST] - hs[sd::MSA_SUM_NONE];
        *total_bytes = t->total;
        if (classes) { classes[0] = hs[sd::MSA_SUM_NONE]; classes[1] = t->nd; classes[2] = hs[sd::MSA_SUM_HOST]; }
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_msa_final_write_dev(sd_msa_tables* t, const sd_final_row* d_rows, int64_t n_rows, int32_t device, void* hip_stream,
                           const int64_t* d_row_at, uint8_t* d_out, int64_t cap, uint8_t* d_status, char* errbuf, size_t errlen) try {
    static const char* who = "sd_msa_final_write_dev";
    if (!t || n_rows < 0 || cap < 0 || !d_row_at || (n_rows > 0 && (!d_rows || !d_status))) {
        set_err(errbuf, errlen, std::string(who) + ": missing argument");
        return SD_ERR_PARAM;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    int rc = msa_dev_check(t, device, st, errbuf, errlen);
    if (rc) return rc;
    try {
        std::lock_guard<std::mutex> g(t->m);
        DeviceScope on(device);
        if (t->n_rows != n_rows || t->rows_of != d_rows) {
            set_err(errbuf, errlen, std::string(who) + ": no size pass over these rows precedes the call");
            return SD_ERR_PARAM;
        }
        if (cap < t->total) {
            set_err(errbuf, errlen, std::string(who) + ": the rows take " + std::to_string(t->total) + " bytes, the buffer holds " + std::to_string(cap));
            return SD_ERR_PARAM;
        }
        if ((rc = buffer_on_device(d_row_at, device, who, "row offset", errbuf, errlen))) return rc;
        if (n_rows > 0 && (rc = buffer_on_device(d_status, device, who, "status", errbuf, errlen))) return rc;
        if (t->total > 0 && (rc = buffer_on_device(d_out, device, who, "row", errbuf, errlen))) return rc;
        if (t->total > 0 && (reinterpret_cast<uintptr_t>(d_out) & 15)) {
            set_err(errbuf, errlen, std::string(who) + ": the row buffer must be 16-byte aligned");
            return SD_ERR_PARAM;
        }
        if (n_rows == 0) return SD_OK;
        ProfWS& w = t->w;
        ProfDev& d = t->d;
        const int M = d.M;
        hipLaunchKernelGGL(sd::sd_msa_fill, dim3(msa_grid(n_rows)), dim3(sd::MSA_T), 0, st, w.cls.p, w.pair_il.p, d.tlen.p, d_row_at, n_rows,
                           d_out, d_status);
        SD_HIP(hipGetLastError());
        if (t->nd > 0) {
            prof_group(w, M, st, n_rows, t->n_ptr.p);
            // (the sizes of nw_profile_device; the items from the pair count alone: at most nd / per + M of them)
            const int K = d.K, S = sd::nw_block_cols(K);
            const int ckcap = std::max(1, (t->qmax + S - 1) / S);
            const int64_t R = std::max<int64_t>(1, std::min<int64_t>(64, t->nd / ((int64_t)d.n_cu * 12 * 64)));
            const int per = (int)(64 * R);
            const int64_t n_items = t->nd / per + M;
            const size_t lane_bytes = (size_t)ckcap * K * 16;
            int grid = (int)std::min<int64_t>(n_items, (int64_t)d.n_cu * 12);
            grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(((size_t)1 << 30) / (lane_bytes * 64))));
            const size_t need = lane_bytes * 64 * (size_t)grid;
            if (need > d.ck.cap) {   // a walk in flight reads the old block
                if (t->used) SD_HIP(hipEventSynchronize(t->ev_use));
                d.ck.alloc(need);
            }
            prof_items(w, M, per, n_items, st, true);
            sd::launch_nw_msa(K, st, grid, d.tmax, t->text.p, w.seg_start.p, w.seg_len.p, w.order.p, w.pair_il.p, w.items.p, (int)n_items,
                              d.peq.p, d.tlen.p, ckcap, d.ck.p, d.ckpos.p, d_out, d_row_at, d_status, d.fails());
            SD_HIP(hipGetLastError());
        }
        msa_used(t, st);
        return SD_OK;
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

}  // extern "C"
