// sd_pack_dev.hip -- the device packer: read text that already lies in device memory -> the 2-bit words and N masks
// of a batch, in the layout load_chunks_impl (sd_engine.hip) gives a batch packed on the host.
//
// One workgroup per chunk, one lane per 32 bases: a lane owns two whole words of bases2 and one whole mask word, so
// every store is a plain vector store.  A chunk's source is an arbitrary byte address (reads are concatenated, chunk
// starts are multiples of part_size): the text is read with 16-byte loads through an align-1 type, which gfx950 does
// in one global_load_dwordx4 whatever the address; the last, partial 16 bytes of a chunk are read byte by byte, so
// nothing past src[c] + n is ever touched.
//
// N masks: the host cannot know which chunks hold an N without reading the text, so it gives every chunk the mask
// offset it would have if every chunk had one (the buffer is sized for that anyway).  The workgroup ORs its lanes' mask
// words; with an N in the chunk the lanes store them (in a second pass, which re-reads the chunk from L2), without one
// lane 0 stores noff = -1 into the chunk's device descriptor and the mask words stay untouched: the chunk runs maskless,
// as from the host.
//
// Alphabet: a byte outside A C G T N still gets the masked code ((c >> 1) ^ (c >> 2)) & 3 -- nothing downstream can
// leave its tables -- and the wave that saw it posts (position << 8 | byte), position = gpos[c] + index, with ONE
// 64-bit atomic minimum: the flag ends as the smallest offending position of the batch.
#include "sd_kernels.hpp"

namespace sd {
namespace {

typedef uint32_t Bytes16 __attribute__((ext_vector_type(4), aligned(1)));   // 16 bytes at any address
// (the source addresses arrive as integers: said to be global memory, the loads are global_load, not flat_load)
typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;
typedef const __attribute__((address_space(1))) Bytes16* GlobalBytes16;

// 0x80 in every byte of y that is zero (exact: no borrow between bytes)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t y) {
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
}
// bits 7, 15, 23, 31 -> bits 0..3
__device__ __forceinline__ uint32_t gather4(uint32_t z) {
    const uint32_t m = z >> 7;
    return (m | (m >> 7) | (m >> 14) | (m >> 21)) & 0xFu;
}

// Bases [16 * h, 16 * h + 16) of the chunk s[0 .. n), h = half-unit index: *w = their 2-bit word, the returns' low 16
// bits = which are 'N', *inv = which are outside the alphabet.  Bytes past n count as 0: code 0, neither N nor invalid.
__device__ __forceinline__ uint32_t pack16(GlobalBytes s, int32_t n, int32_t off, uint32_t* w, uint32_t* inv) {
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    const int32_t rem = n - off;
    if (rem >= 16) {
        const uint32_t __attribute__((ext_vector_type(4))) t = *(GlobalBytes16)(s + off);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
        for (int32_t i = 0; i < rem; ++i) x[i >> 2] |= (uint32_t)s[off + i] << (8 * (i & 3));
    }
    uint32_t word = 0, nm = 0, ok = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t t = ((x[k] >> 1) ^ (x[k] >> 2)) & 0x03030303u;
        t = (t | (t >> 6)) & 0x000F000Fu;
        t = (t | (t >> 12)) & 0xFFu;
        word |= t << (8 * k);
        const uint32_t zn = zero_bytes(x[k] ^ 0x4E4E4E4Eu);
        const uint32_t zv = zn | zero_bytes(x[k] ^ 0x41414141u) | zero_bytes(x[k] ^ 0x43434343u) |
                            zero_bytes(x[k] ^ 0x47474747u) | zero_bytes(x[k] ^ 0x54545454u);
        nm |= gather4(zn) << (4 * k);
        ok |= gather4(zv) << (4 * k);
    }
    const uint32_t live = rem >= 16 ? 0xFFFFu : ((1u << (rem > 0 ? rem : 0)) - 1u);
    *w = word;
    *inv = ~ok & live;
    return nm & live;
}

__global__ __launch_bounds__(256) void sd_pack_dev_kernel(PackDevArgs a) {
    const int c = (int)blockIdx.x;
    if (c >= a.n_chunks) return;
    const ChunkDesc cd = a.chunks[c];
    GlobalBytes s = (GlobalBytes)a.src[c];
    const int32_t n = cd.n;
    const int32_t units = (n + 31) >> 5;            // 32 bases each: two words of bases, one mask word
    const int32_t words = (n + 15) >> 4;
    uint32_t any_n = 0;
    unsigned long long bad = ~0ull;
    for (int32_t u = (int32_t)threadIdx.x; u < units; u += (int32_t)blockDim.x) {
        uint32_t w0, w1, i0, i1;
        const uint32_t m0 = pack16(s, n, 32 * u, &w0, &i0);
        const uint32_t m1 = pack16(s, n, 32 * u + 16, &w1, &i1);
        a.bases2[(size_t)cd.woff + 2 * (size_t)u] = w0;
        if (2 * u + 1 < words) a.bases2[(size_t)cd.woff + 2 * (size_t)u + 1] = w1;
        any_n |= m0 | m1;
        const uint32_t inv = i0 | (i1 << 16);
        if (inv && bad == ~0ull) {                  // (units ascend: the lane's first offending byte)
            const int32_t i = 32 * u + __builtin_ctz(inv);
            bad = ((unsigned long long)(a.gpos[c] + i) << 8) | s[i];
        }
    }
    // the smallest offending position of the wave, posted once
    if (__ballot(bad != ~0ull)) {
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(bad, d);
            bad = o < bad ? o : bad;
        }
        if ((threadIdx.x & 63) == 0) atomicMin(a.bad, bad);
    }
    if (!__syncthreads_or(any_n != 0)) {
        if (threadIdx.x == 0) a.chunks[c].noff = -1;
        return;
    }
    for (int32_t u = (int32_t)threadIdx.x; u < units; u += (int32_t)blockDim.x) {
        uint32_t w0, w1, i0, i1;
        const uint32_t m0 = pack16(s, n, 32 * u, &w0, &i0);
        const uint32_t m1 = pack16(s, n, 32 * u + 16, &w1, &i1);
        a.nmask[(size_t)cd.noff + (size_t)u] = m0 | (m1 << 16);
    }
}

}  // namespace

void launch_pack_dev(hipStream_t st, const PackDevArgs& a) {
    if (a.n_chunks <= 0) return;
    hipLaunchKernelGGL(sd_pack_dev_kernel, dim3((unsigned)a.n_chunks), dim3(256), 0, st, a);
}

}  // namespace sd
