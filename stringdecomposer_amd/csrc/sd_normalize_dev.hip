// sd_normalize_dev.hip -- the lenient mode's rule (sd_normalize.hpp) applied to read text that lies in device memory: a
// pass of its own in front of everything that reads the text (the packer's 2-bit words are one reader of a job's text
// in HBM, the identity, profile and MSA kernels are others).
//
// The host cuts the reads into pieces of <= kNormPiece bytes (a piece never leaves its read); one wave per piece, four
// pieces per workgroup.  A piece is three parts: the head, up to the first 16-byte boundary of its source address; the
// body, whole 16-byte units, loaded and stored through align-1 16-byte types (aligned loads by the head's choice; the
// destination has the same offsets but maybe another base, so its stores may be unaligned, which gfx950 does in one
// global_store_dwordx4 all the same); the tail, what is left.  Head and tail go byte by byte, so no byte outside
// [off, off + len) is read or written, and every lane stores exactly the bytes it loaded -- with dst == src no lane
// ever reads a byte another lane has written.
//
// Counters: every lane counts in registers, the wave sums by shuffles, lane 0 adds each counter with one 64-bit vector
// atomic (none for a zero).  Adds to one cache line serialise: measured on 50 MB (3 200 waves), a launch took 55 us with
// one add per wave and 101 us with two, against 27 us with none (profiles/lenient_timing.md, section 3; ~17 ns per add
// is derived from those times).  So the one counter the host can compute -- the bytes examined -- is added once per
// launch, and canonical text costs no atomic at all.
//
// The call waits for nothing: the piece table goes up from a pinned staging block by an asynchronous copy on the
// caller's stream.  Staging block and device table form a slot that is taken from a small process-wide list when the
// event of its last use has completed (a new slot is made otherwise, never resized) -- 16 bytes per 16 KB of text;
// the slots stay for the life of the process.
#include "sd_pipeline.hpp"
#include "sd_normalize.hpp"

namespace sd {
namespace {

typedef uint32_t NBytes16 __attribute__((ext_vector_type(4), aligned(1)));   // 16 bytes at any address
typedef const __attribute__((address_space(1))) uint8_t* NSrcBytes;
typedef __attribute__((address_space(1))) uint8_t* NDstBytes;
typedef const __attribute__((address_space(1))) NBytes16* NSrc16;
typedef __attribute__((address_space(1))) NBytes16* NDst16;

__global__ __launch_bounds__(256) void sd_normalize_dev_kernel(NormDevArgs a) {
    const int lane = (int)(threadIdx.x & 63);
    const long long pc = (long long)blockIdx.x * 4 + (long long)(threadIdx.x >> 6);
    if (pc >= a.n_pieces) return;                  // (whole waves leave: the shuffles below see full waves)
    const NormPiece p = a.pieces[pc];
    NSrcBytes s = (NSrcBytes)(a.src + (unsigned long long)p.off);
    NDstBytes d = (NDstBytes)(a.dst + (unsigned long long)p.off);
    const int32_t n = p.len;
    int32_t head = (int32_t)((16u - (uint32_t)((a.src + (unsigned long long)p.off) & 15u)) & 15u);
    if (head > n) head = n;
    const int32_t units = (n - head) >> 4;
    const int32_t tail0 = head + (units << 4);     // tail = [tail0, n), < 16 bytes
    NormCount k;
    if (lane < head) d[lane] = normalize_byte(s[lane], k);
    if (lane >= 32 && tail0 + (lane - 32) < n) d[tail0 + (lane - 32)] = normalize_byte(s[tail0 + (lane - 32)], k);
    // four units per lane in flight: all four loads are issued before the first store (with dst == src the compiler
    // must keep a later load behind an earlier store, so the order is spelled out)
    for (int32_t u0 = lane; u0 < units; u0 += 256) {
        uint32_t __attribute__((ext_vector_type(4))) t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (u0 + 64 * j < units) t[j] = *(NSrc16)(s + head + ((u0 + 64 * j) << 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (u0 + 64 * j >= units) break;
            uint32_t x[4] = {t[j].x, t[j].y, t[j].z, t[j].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint32_t lo, am, bd;
                x[i] = normalize_word(x[i], &lo, &am, &bd);
                k.lower += norm_popc(lo);
                k.amb += norm_popc(am);
                k.bad += norm_popc(bd);
            }
            uint32_t __attribute__((ext_vector_type(4))) o;
            o.x = x[0]; o.y = x[1]; o.z = x[2]; o.w = x[3];
            *(NDst16)(d + head + ((u0 + 64 * j) << 4)) = o;
        }
    }
    if (!a.stats) return;
    for (int sh = 32; sh > 0; sh >>= 1) {
        k.lower += __shfl_xor(k.lower, sh);
        k.amb += __shfl_xor(k.amb, sh);
        k.bad += __shfl_xor(k.bad, sh);
    }
    if (lane == 0) {
        if (k.lower) atomicAdd(a.stats + 0, (unsigned long long)k.lower);
        if (k.amb) atomicAdd(a.stats + 1, (unsigned long long)k.amb);
        if (k.bad) atomicAdd(a.stats + 2, (unsigned long long)k.bad);
        if (pc == 0) atomicAdd(a.stats + 3, a.total);   // (the host knows the bytes examined: one add per launch)
    }
}

}  // namespace

void launch_normalize_dev(hipStream_t st, const NormDevArgs& a) {
    if (a.n_pieces <= 0) return;
    hipLaunchKernelGGL(sd_normalize_dev_kernel, dim3((unsigned)((a.n_pieces + 3) / 4)), dim3(256), 0, st, a);
}

}  // namespace sd

namespace sdi {
namespace {

// piece table of one call: pinned staging + device copy + the event of its last use
struct NormSlot {
    int dev = -1;
    sd::NormPiece* h = nullptr;
    sd::NormPiece* d = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool busy = false;    // handed to a call that has not recorded `ev` yet
};
std::mutex g_norm_m;
std::vector<NormSlot*>& norm_slots() { static std::vector<NormSlot*>* v = new std::vector<NormSlot*>; return *v; }

// A slot of `dev` with room for n pieces whose last use is over, marked busy; the caller holds a DeviceScope of dev.
// No slot is ever resized or freed on this path: a job that needs more room than any idle slot has gets a new slot, and
// the smaller ones stay for smaller jobs.  A slot enters the list only when its event and both blocks exist.
NormSlot* norm_slot_take(int dev, size_t n) {
    std::lock_guard<std::mutex> g(g_norm_m);
    NormSlot* s = nullptr;
    for (NormSlot* x : norm_slots())
        if (x->dev == dev && !x->busy && x->cap >= n && hipEventQuery(x->ev) == hipSuccess && (!s || x->cap < s->cap)) s = x;
    (void)hipGetLastError();   // (hipErrorNotReady of a slot still in use)
    if (s) { s->busy = true; return s; }
    std::unique_ptr<NormSlot> f(new NormSlot);
    f->dev = dev;
    f->cap = std::max<size_t>(n, 4096);
    hipError_t e = hipEventCreateWithFlags(&f->ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&f->h), f->cap * sizeof(sd::NormPiece), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&f->d), f->cap * sizeof(sd::NormPiece));
    if (e != hipSuccess) {   // nothing half-made is kept
        (void)hipGetLastError();
        if (f->d) (void)hipFree(f->d);
        if (f->h) (void)hipHostFree(f->h);
        if (f->ev) (void)hipEventDestroy(f->ev);
        throw HipFail{std::string("sd_normalize_dev: piece table of ") + std::to_string(f->cap) + " entries: " + hipGetErrorString(e)};
    }
    f->busy = true;
    norm_slots().push_back(f.get());
    return f.release();
}
void norm_slot_give(NormSlot* s) {
    std::lock_guard<std::mutex> g(g_norm_m);
    s->busy = false;
}

}  // namespace
}  // namespace sdi

extern "C" int sd_normalize_dev(const void* d_in, void* d_out, const int64_t* read_off, const int64_t* read_lens,
                                int32_t n_reads, int32_t device, void* hip_stream, uint64_t* d_stats, char* errbuf,
                                size_t errlen) {
    using namespace sdi;
    if (n_reads < 0 || (n_reads > 0 && (!d_in || !d_out || !read_off || !read_lens))) {
        set_err(errbuf, errlen, "sd_normalize_dev: a NULL argument or n_reads < 0");
        return SD_ERR_PARAM;
    }
    int64_t n_pieces = 0, hi = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] < 0 || read_off[r] < 0 || read_off[r] > INT64_MAX - read_lens[r]) {
            set_err(errbuf, errlen, "sd_normalize_dev: read " + std::to_string(r) + " has a negative offset or length");
            return SD_ERR_PARAM;
        }
        n_pieces += (read_lens[r] + sd::kNormPiece - 1) / sd::kNormPiece;
        hi = std::max(hi, read_off[r] + read_lens[r]);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_err(errbuf, errlen, "no usable HIP device");
        return SD_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_err(errbuf, errlen, "device " + std::to_string(device) + " does not exist");
        return SD_ERR_PARAM;
    }
    if (n_reads == 0) return SD_OK;
    int rc = buffer_on_device(d_in, device, "sd_normalize_dev", "input", errbuf, errlen);
    if (rc == SD_OK && d_out != d_in) rc = buffer_on_device(d_out, device, "sd_normalize_dev", "output", errbuf, errlen);
    if (rc == SD_OK && d_stats) rc = buffer_on_device(d_stats, device, "sd_normalize_dev", "counter", errbuf, errlen);
    if (rc) return rc;
    // the reads must lie inside the allocations the two addresses belong to (where the runtime tells their extent)
    for (const void* q : {d_in, static_cast<const void*>(d_out)}) {
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, const_cast<void*>(q)) != hipSuccess) { (void)hipGetLastError(); continue; }
        const uint64_t room = (uint64_t)size - (uint64_t)(static_cast<const char*>(q) - static_cast<const char*>(base));
        if ((uint64_t)hi > room) {
            set_err(errbuf, errlen, "sd_normalize_dev: the reads end " + std::to_string(hi) + " bytes into a buffer that holds " +
                                        std::to_string(room));
            return SD_ERR_PARAM;
        }
    }
    if (n_pieces == 0) return SD_OK;
    if (n_pieces > 4ll * 0x7fffffff) {
        set_err(errbuf, errlen, "sd_normalize_dev: more pieces than one launch takes");
        return SD_ERR_UNSUPPORTED;
    }
    NormSlot* slot = nullptr;
    try {
        DeviceScope scope(device);
        hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
        slot = norm_slot_take(device, (size_t)n_pieces);
        size_t k = 0;
        for (int32_t r = 0; r < n_reads; ++r)
            for (int64_t o = 0; o < read_lens[r]; o += sd::kNormPiece)
                slot->h[k++] = sd::NormPiece{(long long)(read_off[r] + o),
                                             (int32_t)std::min<int64_t>(sd::kNormPiece, read_lens[r] - o), 0};
        SD_HIP(hipMemcpyAsync(slot->d, slot->h, k * sizeof(sd::NormPiece), hipMemcpyHostToDevice, st));
        sd::NormDevArgs a{};
        a.src = (unsigned long long)reinterpret_cast<uintptr_t>(d_in);
        a.dst = (unsigned long long)reinterpret_cast<uintptr_t>(d_out);
        a.pieces = slot->d;
        a.n_pieces = (long long)k;
        for (size_t x = 0; x < k; ++x) a.total += (unsigned long long)slot->h[x].len;
        a.stats = reinterpret_cast<unsigned long long*>(d_stats);
        sd::launch_normalize_dev(st, a);
        SD_HIP(hipGetLastError());
        SD_HIP(hipEventRecord(slot->ev, st));
        norm_slot_give(slot);
    } catch (const HipFail& f) {
        if (slot) {
            // the copy from the slot's staging block may be queued: the slot is reusable once the stream has passed it
            hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
            if (hipEventRecord(slot->ev, st) != hipSuccess) (void)hipStreamSynchronize(st);
            (void)hipGetLastError();
            norm_slot_give(slot);
        }
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}
