// sd_kernels.hpp -- launch wrappers of the HIP kernels (defined in sd_generic.hip / sd_fast.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "sd_device.hpp"

namespace sd {

// generic int32 workgroup-per-chunk family (sd_generic.hip)
int generic_pick_q(int64_t sum_len);
void launch_generic_fill(int Q, int threads, int grid, hipStream_t st, const ChunkDesc* chunks,
                         int chunk_begin, const uint32_t* bases2, const uint32_t* nmask,
                         const uint8_t* tmeta, const int32_t* tend_kd, const int32_t* tend_j,
                         ScoreArgs sc, int rowBytes, uint8_t* ptr, uint64_t row0_base, int32_t* B,
                         int32_t* argB, const uint16_t* grank, int T, int n_tiles, int32_t* Estate);
void launch_generic_trace(int n_sub, hipStream_t st, const ChunkDesc* chunks, int chunk_begin,
                          const uint8_t* ptr, uint64_t row0_base, int rowBytes, const int32_t* B,
                          const int32_t* argB, const int32_t* toff, const int32_t* tlen,
                          DevRec* recs, int32_t* rec_cnt);
void launch_compact(hipStream_t st, const ChunkDesc* chunks, int n_chunks, const int32_t* cnt,
                    int64_t* roff, const DevRec* recs, DevRec* out, int64_t out_cap, bool scan,
                    int32_t* out_chunk = nullptr,
                    long long* scan_ws = nullptr,   // 520 zeroed words that persist between launches: offsets + compaction in
                    long long epoch = 0,            // one launch (sd_scan_compact); a value no earlier launch on scan_ws has used
                    long long* tickets = nullptr);  // host: tickets drawn from scan_ws so far (advanced by the launch)

// device packer (sd_pack_dev.hip): chunk c = the n bytes at device address src[c] -> bases2 at chunks[c].woff and, if it
// holds an N, nmask at chunks[c].noff (else chunks[c].noff = -1 is stored); a byte outside A C G T N lowers *bad to
// ((gpos[c] + index) << 8) | byte (*bad starts as all ones)
struct PackDevArgs {
    ChunkDesc* chunks;
    const unsigned long long* src;
    const long long* gpos;
    int n_chunks;
    uint32_t* bases2;
    uint32_t* nmask;
    unsigned long long* bad;
};
void launch_pack_dev(hipStream_t st, const PackDevArgs& a);

// lenient normalisation of read text in device memory (sd_normalize_dev.hip): piece x = the len bytes at src + off, the
// rule of sd_normalize.hpp applied, written at dst + off (dst == src: in place); a piece lies inside one read and holds
// at most kNormPiece bytes.  stats (may be null): four counters the kernel adds to (sd_normalize_dev in sd_hip.h).
constexpr int32_t kNormPiece = 16384;
struct NormPiece {
    long long off;
    int32_t len, pad;
};
struct NormDevArgs {
    unsigned long long src, dst;
    const NormPiece* pieces;
    long long n_pieces;
    unsigned long long* stats;
    unsigned long long total;   // bytes of all pieces: what stats[3] grows by, added once
};
void launch_normalize_dev(hipStream_t st, const NormDevArgs& a);

}  // namespace sd
