// sd_nw.hpp -- launch wrapper of the batched NW identity kernel (sd_nw.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace sd {

// columns per register-resident block of the identity kernel (sd_nw_kernel.hpp): S * K * 4 history registers;
// a pair of q columns needs ceil(q / S) - 1 checkpoint slots
__host__ __device__ constexpr int nw_block_cols(int K) { return K <= 1 ? 16 : K == 2 ? 12 : K == 3 ? 9 : K == 4 ? 6 : K <= 6 ? 4 : 3; }

// One lane per (segment, template) pair; K = 64-bit words per template (ceil(max tlen / 64): 1, 2, 3, 4, 6, 8).
// ck / ckpos: grid * 256 lanes x cap checkpoint slots x (K x 16 B + 4 B); peq: [T][5][K], top-aligned
// (nw_build_masks); seg_idx (optional): the segments of this launch.
void launch_nw_pairs(int K, hipStream_t st, int grid, const uint8_t* seq, const int64_t* seg_start,
                     const int32_t* seg_len, const int32_t* seg_idx, int64_t n_seg, int T, const int32_t* pair_tmpl,
                     const unsigned long long* peq, const int32_t* tlen, int homo, int cap, void* ck, int* ckpos,
                     int32_t* dist, int32_t* matches);
// templates of 513 .. 2048 bp (sd_nw_long.hip): a pair across K lanes, systolic over the columns.  plist: the pair ids of
// the launch; ck: grid * (block_threads / 64) * (64 / lpp) pair slots x cap x 5 x lpp dwords, lpp = 16 (K <= 16) or 32
void launch_nw_long(int K, hipStream_t st, int grid, int block_threads, const uint8_t* seq, const int64_t* seg_start,
                    const int32_t* seg_len, const int64_t* plist, int64_t n_pairs, int T, const int32_t* pair_tmpl,
                    const unsigned long long* peq, const int32_t* tlen, int homo, int qcap, int cap, void* ck,
                    int32_t* dist, int32_t* matches);
size_t nw_long_lds_bytes(int lpp, int qcap, int block_threads);
int nw_long_slots(int qmax, int K);
void nw_build_masks(const std::vector<std::string>& ts, int K, std::vector<unsigned long long>& peq,
                    std::vector<int32_t>& tl);

// Host driver (sd_nw.hip): identity of segments of a text (the concatenation of `spans`) against templates on
// the device; see the definition.
int nw_identity_device(const std::vector<std::pair<const char*, int64_t>>& spans, const int64_t* seg_start,
                       const int32_t* seg_len, int64_t n_seg, const std::vector<std::string>& tmpl,
                       const int32_t* pair_tmpl, bool homo, int device, int threads, int32_t* dist,
                       int32_t* matches);
// Column profiles (include/sd_hip.h: SD_FLAG_PROFILE).  il: the interleaved templates m0, rc(m0), m1, ...; pair_il[s]:
// segment s's template; counts: the forward monomers' blocks (profile_offsets), ADDED to.  nw_profile_device takes the
// pairs of its kernel and gives the rest to profile_host (q[x], qlen[x]: pair x's query).
int nw_profile_device(const std::vector<std::pair<const char*, int64_t>>& spans, const int64_t* seg_start,
                      const int32_t* seg_len, int64_t n_seg, const std::vector<std::string>& il, const int32_t* pair_il,
                      int device, int threads, uint64_t* counts);
int profile_host(const char* const* q, const int32_t* qlen, const int32_t* pair_il, int64_t n,
                 const std::vector<std::string>& il, int threads, uint64_t* counts);
int64_t profile_offsets(const std::vector<int32_t>& fwd_len, std::vector<int64_t>& off);   // -> total counters
// The fold kernel alone (sd_nw_profile<K>): one-wave workgroups over items[0 .. n_items) = {monomer, first, end} into
// order[], whose entries index seg_start / seg_len / pair_il; lds = 80 K + 48 (tmax + 1) bytes; ck: grid x 64 lanes x
// cap slots x K x 16 B; counts: the forward monomers' blocks at off[m], ADDED to; *fails counts pairs beyond `cap`.
void launch_nw_profile(int K, hipStream_t st, int grid, size_t lds, const uint8_t* seq, const int64_t* seg_start,
                       const int32_t* seg_len, const int32_t* order, const int32_t* pair_il, const int4* items, int n_items,
                       const unsigned long long* peq, const int32_t* tlen, const int64_t* off, int cap, void* ck, int* ckpos,
                       unsigned long long* counts, int* fails);
// Rows of --msa (include/sd_hip.h: SD_MSA_PITCH; sd_msa.hpp).  msa_row_offsets: row_at[0 .. n] for pairs of interleaved
// templates pair_il over forward lengths tlen[0 .. T) -> total bytes, -1 for a template out of range.  msa_host
// (sd_post.hip): pair x's row at rows + at[x], status[x] 0 / 1.  nw_msa_device (sd_msa.hip): the split of
// nw_profile_device; rows and status of every segment cleared by the caller, row_at holds n_seg + 1 offsets.
int64_t msa_row_offsets(const int32_t* tlen, int32_t T, const int32_t* pair_il, int64_t n, int64_t* row_at);
int msa_host(const char* const* q, const int32_t* qlen, const int32_t* pair_il, int64_t n, const std::vector<std::string>& il,
             int threads, uint8_t* rows, const int64_t* at, uint8_t* status);
// bench (sd_msa_kernel_bench): before the rows are made, the row kernel and the profile kernel run warmup + reps times
// in turn on the kernel's pairs, each between two HIP events; info = K, grid, items, pairs, LDS bytes of the row kernel,
// rows staged (1) or written through (0), LDS bytes of the profile kernel, checkpoint slots.
struct MsaBench {
    int warmup, reps;
    float* ms_msa;
    float* ms_profile;
    int64_t* info;
};
int nw_msa_device(const char* seq, int64_t seqlen, const int64_t* seg_start, const int32_t* seg_len, int64_t n_seg,
                  const std::vector<std::string>& il, const int32_t* pair_il, int device, int threads, uint8_t* rows,
                  const int64_t* row_at, uint8_t* status, const MsaBench* bench = nullptr);
// The row kernel alone (sd_nw_msa<K>): the items, order[] and checkpoints of launch_nw_profile; tmax sizes the LDS
// (nw_msa_lds_bytes; *stage = rows staged in LDS); a pair's row goes to out + row_at[segment], its status byte becomes 1.
size_t nw_msa_lds_bytes(int K, int tmax, int* stage);
void launch_nw_msa(int K, hipStream_t st, int grid, int tmax, const uint8_t* seq, const int64_t* seg_start, const int32_t* seg_len,
                   const int32_t* order, const int32_t* pair_il, const int4* items, int n_items, const unsigned long long* peq,
                   const int32_t* tlen, int cap, void* ck, int* ckpos, uint8_t* out, const int64_t* row_at, uint8_t* status,
                   int* fails);
// The reads of a caller's device buffer (read r at src + roff[r]; roff and toff device arrays), copied back to back into dst:
// read r at dst + toff[r], toff[n_reads] = text bytes.  The walks read aligned dwords up to the next multiple of 4 past a
// segment's end, so they work on such a copy of their own (sd_msa.hip, sd_lags.hip), 8 bytes longer than the text.
void launch_text_gather(hipStream_t st, const uint8_t* src, const int64_t* roff, const int64_t* toff, int n_reads, int64_t text,
                        uint8_t* dst);
// accumulated over the device identity calls of the process: preparation + staging, uploads, kernel, downloads
void nw_stage_seconds(double out[4]);

}  // namespace sd
