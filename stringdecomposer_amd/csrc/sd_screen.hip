// sd_screen.hip -- the screen: which chunks of a read can hold a monomer at all.
//
// key[c] = (min over templates j of dist(j, c)) << 16 | first j that attains it, dist = the infix ("HW") unit-cost edit
// distance of template j against chunk c -- the distance of the --ed_thr prefilter (sd_filter.hip), computed by the same
// kernels with another sink (KeyMin): no [chunk][T] matrix, one uint32 per chunk.  A chunk passes a threshold when
// key >> 16 <= thr; a region is a maximal run of passing chunks of one read (sd_screen_regions).  The DP, traceback and
// everything behind them then see only the regions: the caller decomposes the regions' substrings as reads of their own.
//
//   sd_screen_create / destroy   templates (monomers, then reverse complements), match masks and scratch on one device
//   sd_screen_chunks             reads in host memory: packed on host threads, one launch, the keys copied back
//   sd_screen_chunks_dev         reads in device memory: packed by sd_pack_dev.hip, ordered with the caller's stream by events
//   sd_screen_chunks_host        the same keys by a plain DP on the host (tests; exact, not fast)
//   sd_screen_regions            host: keys -> regions
#include "sd_pipeline.hpp"

using namespace sdi;

struct sd_screen {
    int device = 0;
    int T = 0, Lmax = 0;
    int uniform = -1;          // FilterArgs::uniform_half of the set
    bool general = false;      // sd_screen_set_general: the general kernel where the uniform one would run (A/B, tests)
    std::vector<std::string> tseq;
    std::vector<int32_t> tlen;
    DevBuf<unsigned long long> d_peq;
    DevBuf<int32_t> d_tlen;
    DevBuf<uint8_t> d_in;      // [chunk table][chunk addresses][chunk positions][alphabet flag][bases2][nmask]
    PinBuf<uint8_t> h_in;
    DevBuf<uint32_t> d_key;
    PinBuf<uint32_t> h_key;
    hipStream_t st = nullptr;
    hipEvent_t ev_ready = nullptr, ev_done = nullptr, ev_in = nullptr;
    bool in_pending = false;   // the last batch's upload may still read h_in
    hipEvent_t ev_k[4] = {nullptr, nullptr, nullptr, nullptr};   // around the kernels of a batch (timing), two batches in flight
    int slot = 0, fetch_slot = 0;
    double kernel_ms = 0;      // summed over the batches fetched so far
    int threads = 0;           // host threads of the packer (0: up to 16)
    sd::FilterArgs last{};     // the operands of the last batch (sd_screen_kernel_bench runs on them again)
    DevBuf<int32_t> d_dist;    // sd_screen_kernel_bench: the [chunk][T] matrix of the --ed_thr form
    std::mutex m;              // calls on one handle serialise
};

namespace {

int screen_templates(const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, std::vector<std::string>& tseq,
                     std::string& err) {
    if (n_mono <= 0 || !mono_seqs || !mono_lens) { err = "no monomers"; return SD_ERR_PARAM; }
    if (2 * (int64_t)n_mono > 65535) { err = "the screen's key holds a template index of 16 bits: at most 32 767 monomers"; return SD_ERR_UNSUPPORTED; }
    tseq.resize(2 * (size_t)n_mono);
    for (int j = 0; j < n_mono; ++j) {
        if (mono_lens[j] <= 0) { err = "ERROR: empty monomer sequence"; return SD_ERR_EMPTY; }
        if (mono_lens[j] > 2048) { err = "the screen takes monomers of up to 2048 bp"; return SD_ERR_UNSUPPORTED; }
        tseq[(size_t)j].assign(mono_seqs[j], (size_t)mono_lens[j]);
        const int rc = sd::check_alphabet("<monomer>", mono_seqs[j], mono_lens[j], err);
        if (rc) return rc;
        if (!sd::reverse_complement(tseq[(size_t)j], tseq[(size_t)n_mono + (size_t)j])) { err = "map::at"; return SD_ERR_SYMBOL; }
    }
    return SD_OK;
}

int screen_plan_params(int32_t part, int32_t overlap, std::string& err) {
    if (part <= 0) { err = "part_size must be > 0"; return SD_ERR_PARAM; }
    if (overlap < 0) { err = "overlap must be >= 0"; return SD_ERR_PARAM; }
    return SD_OK;
}

inline int code_of(char ch) {
    switch (ch) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return 4;
    }
}

// min over all columns of the bottom row of the unit-cost DP with a free first row (the pattern may start anywhere in
// the text) -- Sellers 1980; the value the bit-vector kernels compute
int hw_distance(const uint8_t* pat, int m, const char* text, int64_t n, std::vector<int>& col) {
    col.resize((size_t)m + 1);
    for (int i = 0; i <= m; ++i) col[(size_t)i] = i;
    int best = m;
    for (int64_t x = 0; x < n; ++x) {
        const int r = code_of(text[x]);
        int diag = 0;   // D[0][x - 1]
        for (int i = 1; i <= m; ++i) {
            const int up = col[(size_t)i - 1], left = col[(size_t)i];
            const int v = std::min(std::min(up, left) + 1, diag + (pat[i - 1] == r ? 0 : 1));
            diag = left;
            col[(size_t)i] = v;
        }
        best = std::min(best, col[(size_t)m]);
    }
    return best;
}

struct ChunkRef { int32_t read; int64_t off; int32_t len; };

int chunk_refs(const int64_t* read_lens, int32_t n_reads, int32_t part, int32_t overlap, std::vector<ChunkRef>& out, std::string& err) {
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] <= 0) { err = "ERROR: Sequence #" + std::to_string(r) + " is empty"; return SD_ERR_EMPTY; }
        sd::chunk_plan(read_lens[r], part, overlap, [&](int64_t off, int32_t l) { out.push_back(ChunkRef{r, off, l}); });
    }
    return SD_OK;
}

int host_threads(const sd_screen* h) {
    if (h && h->threads > 0) return h->threads;
    const int hw = (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(16, hw > 0 ? hw : 1));
}

// One batch: table and (host reads) packed bases up, (device reads) the packer, the distance kernels with the key sink.
// key_dev: the caller's device buffer or null (then the handle's, copied to h_key).  Throws HipFail.
struct ScreenIn {
    const char* const* host_seqs = nullptr;   // reads in host memory, or
    const char* dev_bases = nullptr;          // reads in device memory with
    const int64_t* dev_off = nullptr;         //   their offsets
};

int screen_launch(sd_screen* h, const ScreenIn& in, const ChunkRef* ck, size_t C, uint32_t* key_dev, std::string& err) {
    std::vector<sd::ChunkDesc> tab(C);
    size_t words = 0, nwords_max = 0;
    for (size_t c = 0; c < C; ++c) {
        tab[c] = sd::ChunkDesc{};
        tab[c].woff = (uint32_t)words;
        tab[c].n = ck[c].len;
        tab[c].noff = -1;
        words += ((size_t)ck[c].len + 15) / 16;
        nwords_max += ((size_t)ck[c].len + 31) / 32;
    }
    if (words >= (1ull << 31) || C * (size_t)h->T >= (1ull << 31) * 256) {
        err = "batch too large: split the reads into smaller groups";
        return SD_ERR_UNSUPPORTED;
    }
    const bool dev = in.dev_bases != nullptr;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_tab = 0;
    const size_t o_src = al(o_tab + C * sizeof(sd::ChunkDesc));
    const size_t o_gpos = o_src + (dev ? C * sizeof(uint64_t) : 0);
    const size_t o_bad = o_gpos + (dev ? C * sizeof(int64_t) : 0);
    const size_t o_bases = dev ? al(o_bad + sizeof(uint64_t)) : o_src;
    const size_t o_nmask = al(o_bases + words * sizeof(uint32_t));
    const size_t total = o_nmask + nwords_max * sizeof(uint32_t) + 256;
    if (h->in_pending) {   // the previous batch's upload still reads the staging buffer
        SD_HIP(hipEventSynchronize(h->ev_in));
        h->in_pending = false;
    }
    // (a block a buffer gives up goes to a pool any engine of the process may take it from: nothing of this handle may
    // still be running on it)
    if (total > h->d_in.cap || (!key_dev && C > h->d_key.cap)) SD_HIP(hipStreamSynchronize(h->st));
    h->h_in.alloc(dev ? o_bases : total);
    h->d_in.alloc(total);
    size_t nwords = 0;
    if (dev) {
        uint64_t* src = reinterpret_cast<uint64_t*>(h->h_in.p + o_src);
        int64_t* gpos = reinterpret_cast<int64_t*>(h->h_in.p + o_gpos);
        for (size_t c = 0; c < C; ++c) {
            tab[c].noff = (int32_t)nwords;   // (the packer stores -1 for a chunk without N)
            nwords += ((size_t)ck[c].len + 31) / 32;
            src[c] = (uint64_t)reinterpret_cast<uintptr_t>(in.dev_bases + in.dev_off[ck[c].read] + ck[c].off);
            gpos[c] = (int64_t)c;
        }
        *reinterpret_cast<uint64_t*>(h->h_in.p + o_bad) = ~0ull;
    } else {
        uint32_t* bases2 = reinterpret_cast<uint32_t*>(h->h_in.p + o_bases);
        uint32_t* nmask = reinterpret_cast<uint32_t*>(h->h_in.p + o_nmask);
        std::vector<uint8_t> hasn(C, 0);
        sd::parallel_for((int64_t)C, host_threads(h), 16, [&](int64_t c) {
            const ChunkRef& r = ck[(size_t)c];
            hasn[(size_t)c] = sd::pack_chunk(in.host_seqs[r.read] + r.off, r.len, bases2 + tab[(size_t)c].woff) ? 1 : 0;
        });
        for (size_t c = 0; c < C; ++c)
            if (hasn[c]) {
                tab[c].noff = (int32_t)nwords;
                nwords += ((size_t)ck[c].len + 31) / 32;
            }
        if (nwords) {
            std::memset(nmask, 0, nwords * sizeof(uint32_t));
            sd::parallel_for((int64_t)C, host_threads(h), 16, [&](int64_t c) {
                const sd::ChunkDesc& cd = tab[(size_t)c];
                if (cd.noff < 0) return;
                const char* s = in.host_seqs[ck[(size_t)c].read] + ck[(size_t)c].off;
                for (int32_t i = 0; i < cd.n; ++i)
                    if (s[i] == 'N') nmask[(size_t)cd.noff + (size_t)(i >> 5)] |= 1u << (i & 31);
            });
        }
    }
    if (C) std::memcpy(h->h_in.p + o_tab, tab.data(), C * sizeof(sd::ChunkDesc));
    const size_t up = dev ? o_bad + sizeof(uint64_t) : o_nmask + nwords * sizeof(uint32_t);
    SD_HIP(hipMemcpyAsync(h->d_in.p, h->h_in.p, up, hipMemcpyHostToDevice, h->st));
    SD_HIP(hipEventRecord(h->ev_in, h->st));
    h->in_pending = true;
    sd::ChunkDesc* d_tab = reinterpret_cast<sd::ChunkDesc*>(h->d_in.p + o_tab);
    uint32_t* d_bases2 = reinterpret_cast<uint32_t*>(h->d_in.p + o_bases);
    uint32_t* d_nmask = reinterpret_cast<uint32_t*>(h->d_in.p + o_nmask);
    h->slot ^= 1;
    SD_HIP(hipEventRecord(h->ev_k[2 * h->slot], h->st));
    if (dev) {
        sd::PackDevArgs pa{};
        pa.chunks = d_tab; pa.n_chunks = (int)C; pa.bases2 = d_bases2; pa.nmask = d_nmask;
        pa.src = reinterpret_cast<const unsigned long long*>(h->d_in.p + o_src);
        pa.gpos = reinterpret_cast<const long long*>(h->d_in.p + o_gpos);
        pa.bad = reinterpret_cast<unsigned long long*>(h->d_in.p + o_bad);
        sd::launch_pack_dev(h->st, pa);
        SD_HIP(hipGetLastError());
    }
    sd::FilterArgs a{};
    a.chunks = d_tab; a.n_chunks = (int)C; a.T = h->T; a.Lmax = h->Lmax; a.ed_thr = 0;
    a.bases2 = d_bases2; a.nmask = d_nmask; a.peq = h->d_peq.p; a.tlen = h->d_tlen.p;
    a.uniform_half = h->general ? -1 : h->uniform;
    if (!key_dev) { h->d_key.alloc(C); key_dev = h->d_key.p; }
    a.screen_key = key_dev;
    h->last = a;
    sd::launch_edthr_filter(h->st, a);
    SD_HIP(hipGetLastError());
    SD_HIP(hipEventRecord(h->ev_k[2 * h->slot + 1], h->st));
    return SD_OK;
}

// keys of the handle's buffer to key_out (host memory), through the pinned copy: the copy enqueued behind the batch
// (the previous batch's keys have left h_key), then the wait for it
void screen_fetch_begin(sd_screen* h, size_t C) {
    h->h_key.alloc(C);
    SD_HIP(hipMemcpyAsync(h->h_key.p, h->d_key.p, C * sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
    SD_HIP(hipEventRecord(h->ev_done, h->st));
    h->fetch_slot = h->slot;
}
void screen_fetch_end(sd_screen* h, size_t C, uint32_t* key_out) {
    SD_HIP(hipEventSynchronize(h->ev_done));
    std::memcpy(key_out, h->h_key.p, C * sizeof(uint32_t));
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev_k[2 * h->fetch_slot], h->ev_k[2 * h->fetch_slot + 1]) == hipSuccess) h->kernel_ms += ms; else (void)hipGetLastError();
}
void screen_fetch(sd_screen* h, size_t C, uint32_t* key_out) {
    screen_fetch_begin(h, C);
    screen_fetch_end(h, C, key_out);
}

}  // namespace

extern "C" {

int sd_screen_create(const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, int32_t device, sd_screen** out,
                     char* errbuf, size_t errlen) {
    if (!out) return SD_ERR_PARAM;
    *out = nullptr;
    std::unique_ptr<sd_screen> h(new sd_screen);
    std::string err;
    int rc = screen_templates(mono_seqs, mono_lens, n_mono, h->tseq, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    h->T = (int)h->tseq.size();
    for (const std::string& t : h->tseq) {
        h->tlen.push_back((int32_t)t.size());
        h->Lmax = std::max(h->Lmax, (int)t.size());
    }
    {
        const int w0 = (h->tlen[0] - 1) >> 6, h0 = ((h->tlen[0] - 1) >> 5) & 1;
        bool same = true;
        for (int j = 1; j < h->T; ++j) same = same && ((h->tlen[(size_t)j] - 1) >> 6) == w0 && (((h->tlen[(size_t)j] - 1) >> 5) & 1) == h0;
        h->uniform = same && w0 == ((h->Lmax + 63) / 64) - 1 ? h0 : -1;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        set_err(errbuf, errlen, "no HIP device available (libsd_hip has no CPU fallback)");
        return SD_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n_dev) { set_err(errbuf, errlen, "no such device: " + std::to_string(device)); return SD_ERR_PARAM; }
    try {
        DeviceScope on(device);
        h->device = device;
        std::vector<unsigned long long> peq;
        sd::build_peq(h->tseq, peq);
        h->d_peq.upload(peq);
        h->d_tlen.upload(h->tlen);
        SD_HIP(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
        SD_HIP(hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming));
        SD_HIP(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming | hipEventBlockingSync));
        SD_HIP(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming | hipEventBlockingSync));
        for (hipEvent_t& ev : h->ev_k) SD_HIP(hipEventCreate(&ev));
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    *out = h.release();
    return SD_OK;
}

void sd_screen_destroy(sd_screen* h) {
    if (!h) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(h->device);
    if (h->st) { (void)hipStreamSynchronize(h->st); (void)hipStreamDestroy(h->st); }
    if (h->ev_ready) (void)hipEventDestroy(h->ev_ready);
    if (h->ev_done) (void)hipEventDestroy(h->ev_done);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    for (hipEvent_t ev : h->ev_k)
        if (ev) (void)hipEventDestroy(ev);
    delete h;   // (the buffers go to the pools: no hipFree here)
    if (prev >= 0) (void)hipSetDevice(prev);
}

int sd_screen_set_general(sd_screen* h, int32_t on) {
    if (!h) return SD_ERR_PARAM;
    std::lock_guard<std::mutex> g(h->m);
    h->general = on != 0;
    return SD_OK;
}

/* 0: sd_hw_dist<W>, 1: sd_hw_dist_u<W, lo>, 2: sd_hw_dist_u<W, hi>; *words = W */
int sd_screen_kernel(sd_screen* h, int32_t* words) {
    if (!h) return -1;
    const int W = std::max(1, (h->Lmax + 63) / 64);
    const bool uni = !h->general && h->uniform >= 0 && W <= 4;
    if (words) *words = uni || W <= 4 ? W : W <= 8 ? 8 : W <= 16 ? 16 : 32;
    return uni ? 1 + h->uniform : 0;
}

/* device time of the kernels (packer included for reads in device memory) of the calls so far whose keys came back to
 * the host, in ms; reset != 0 zeroes the sum */
double sd_screen_kernel_ms(sd_screen* h, int32_t reset) {
    if (!h) return 0;
    std::lock_guard<std::mutex> g(h->m);
    const double v = h->kernel_ms;
    if (reset) h->kernel_ms = 0;
    return v;
}

/* The screen's launch (key fill + distance kernel with the key sink) beside the distance kernel of --ed_thr alone (the
 * same instantiation with the matrix sink) on the batch of the last sd_screen_chunks call, in turn in one process, each
 * launch between two HIP events: warmup untimed rounds, then reps timed ones into screen_ms[reps] and dist_ms[reps]. */
int sd_screen_kernel_bench(sd_screen* h, int32_t warmup, int32_t reps, float* screen_ms, float* dist_ms, char* errbuf, size_t errlen) {
    if (!h || reps < 1 || warmup < 0 || !screen_ms || !dist_ms) return SD_ERR_PARAM;
    std::lock_guard<std::mutex> g(h->m);
    if (!h->last.chunks || h->last.screen_key != h->d_key.p) { set_err(errbuf, errlen, "sd_screen_kernel_bench: no batch (call sd_screen_chunks first)"); return SD_ERR_PARAM; }
    try {
        DeviceScope on(h->device);
        SD_HIP(hipStreamSynchronize(h->st));
        h->d_dist.alloc((size_t)h->last.n_chunks * (size_t)h->last.T);
        sd::FilterArgs ks = h->last, kd = h->last;
        kd.screen_key = nullptr;
        kd.dist = h->d_dist.p;
        kd.dist_only = true;
        for (int r = -warmup; r < reps; ++r) {
            SD_HIP(hipEventRecord(h->ev_k[0], h->st));
            sd::launch_edthr_filter(h->st, ks);
            SD_HIP(hipEventRecord(h->ev_k[1], h->st));
            sd::launch_edthr_filter(h->st, kd);
            SD_HIP(hipEventRecord(h->ev_k[2], h->st));
            SD_HIP(hipGetLastError());
            SD_HIP(hipStreamSynchronize(h->st));
            if (r < 0) continue;
            SD_HIP(hipEventElapsedTime(&screen_ms[r], h->ev_k[0], h->ev_k[1]));
            SD_HIP(hipEventElapsedTime(&dist_ms[r], h->ev_k[1], h->ev_k[2]));
        }
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

int sd_screen_chunks(sd_screen* h, const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads, int32_t part,
                     int32_t overlap, uint32_t* key_out, int64_t cap, int64_t* n_chunks, char* errbuf, size_t errlen) {
    if (!h || n_reads < 0 || (n_reads > 0 && (!read_seqs || !read_lens))) return SD_ERR_PARAM;
    std::string err;
    int rc = screen_plan_params(part, overlap, err);
    std::vector<ChunkRef> ck;
    if (!rc) rc = chunk_refs(read_lens, n_reads, part, overlap, ck, err);
    for (int32_t r = 0; !rc && r < n_reads; ++r) rc = sd::check_alphabet("<read>", read_seqs[r], read_lens[r], err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_chunks) *n_chunks = (int64_t)ck.size();
    if (ck.empty()) return SD_OK;
    if (!key_out || cap < (int64_t)ck.size()) { set_err(errbuf, errlen, "sd_screen_chunks: key_out is too small"); return SD_ERR_PARAM; }
    std::lock_guard<std::mutex> g(h->m);
    try {
        DeviceScope on(h->device);
        ScreenIn in;
        in.host_seqs = read_seqs;
        rc = screen_launch(h, in, ck.data(), ck.size(), nullptr, err);
        if (rc) { set_err(errbuf, errlen, err); return rc; }
        screen_fetch(h, ck.size(), key_out);
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

int sd_screen_chunks_dev(sd_screen* h, const void* d_bases, const int64_t* read_off, const int64_t* read_lens, int32_t n_reads,
                         int32_t part, int32_t overlap, void* hip_stream, uint32_t* key_out, int64_t cap, int64_t* n_chunks,
                         char* errbuf, size_t errlen) {
    if (!h || n_reads < 0 || (n_reads > 0 && (!d_bases || !read_off || !read_lens))) return SD_ERR_PARAM;
    std::string err;
    int rc = screen_plan_params(part, overlap, err);
    std::vector<ChunkRef> ck;
    if (!rc) rc = chunk_refs(read_lens, n_reads, part, overlap, ck, err);
    for (int32_t r = 0; !rc && r < n_reads; ++r)
        if (read_off[r] < 0) { err = "negative read offset"; rc = SD_ERR_PARAM; }
    int dev = -1;
    if (!rc && n_reads > 0) {
        rc = device_pointer(d_bases, dev, err);
        if (!rc && dev != h->device) {
            err = "the reads lie in the memory of device " + std::to_string(dev) + ", the screen runs on device " + std::to_string(h->device);
            rc = SD_ERR_UNSUPPORTED;
        }
    }
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_chunks) *n_chunks = (int64_t)ck.size();
    if (ck.empty()) return SD_OK;
    if (!key_out || cap < (int64_t)ck.size()) { set_err(errbuf, errlen, "sd_screen_chunks_dev: key_out is too small"); return SD_ERR_PARAM; }
    // device or host memory for the keys: whichever the pointer is
    bool key_on_dev = false;
    {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, key_out) == hipSuccess && at.type == hipMemoryTypeDevice) {
            if (at.device != h->device) {
                set_err(errbuf, errlen, "the key buffer lies in the memory of device " + std::to_string(at.device) +
                                            ", the screen runs on device " + std::to_string(h->device));
                return SD_ERR_UNSUPPORTED;
            }
            key_on_dev = true;
        } else {
            (void)hipGetLastError();
        }
    }
    std::lock_guard<std::mutex> g(h->m);
    try {
        DeviceScope on(h->device);
        hipStream_t user = reinterpret_cast<hipStream_t>(hip_stream);
        // behind whatever produced the text (and last touched the key buffer) on the caller's stream
        SD_HIP(hipEventRecord(h->ev_ready, user));
        SD_HIP(hipStreamWaitEvent(h->st, h->ev_ready, 0));
        ScreenIn in;
        in.dev_bases = static_cast<const char*>(d_bases);
        in.dev_off = read_off;
        rc = screen_launch(h, in, ck.data(), ck.size(), key_on_dev ? key_out : nullptr, err);
        if (rc) { set_err(errbuf, errlen, err); return rc; }
        if (key_on_dev) {
            // the caller's stream goes on behind the kernels: the keys are there, and the text may be overwritten or freed
            SD_HIP(hipEventRecord(h->ev_done, h->st));
            SD_HIP(hipStreamWaitEvent(user, h->ev_done, 0));
        } else {
            screen_fetch(h, ck.size(), key_out);
            SD_HIP(hipStreamWaitEvent(user, h->ev_done, 0));
        }
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

int sd_screen_chunks_host(const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, const char* const* read_seqs,
                          const int64_t* read_lens, int32_t n_reads, int32_t part, int32_t overlap, uint32_t* key_out,
                          int64_t cap, int64_t* n_chunks, char* errbuf, size_t errlen) {
    if (n_reads < 0 || (n_reads > 0 && (!read_seqs || !read_lens))) return SD_ERR_PARAM;
    std::string err;
    std::vector<std::string> tseq;
    int rc = screen_templates(mono_seqs, mono_lens, n_mono, tseq, err);
    if (!rc) rc = screen_plan_params(part, overlap, err);
    std::vector<ChunkRef> ck;
    if (!rc) rc = chunk_refs(read_lens, n_reads, part, overlap, ck, err);
    for (int32_t r = 0; !rc && r < n_reads; ++r) rc = sd::check_alphabet("<read>", read_seqs[r], read_lens[r], err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_chunks) *n_chunks = (int64_t)ck.size();
    if (ck.empty()) return SD_OK;
    if (!key_out || cap < (int64_t)ck.size()) { set_err(errbuf, errlen, "sd_screen_chunks_host: key_out is too small"); return SD_ERR_PARAM; }
    std::vector<std::vector<uint8_t>> pat(tseq.size());
    for (size_t j = 0; j < tseq.size(); ++j)
        for (char ch : tseq[j]) pat[j].push_back((uint8_t)code_of(ch));
    sd::parallel_for((int64_t)ck.size(), host_threads(nullptr), 1, [&](int64_t c) {
        const ChunkRef& r = ck[(size_t)c];
        std::vector<int> col;
        uint32_t key = 0xffffffffu;
        for (size_t j = 0; j < pat.size(); ++j) {
            const int d = hw_distance(pat[j].data(), (int)pat[j].size(), read_seqs[r.read] + r.off, r.len, col);
            key = std::min(key, ((uint32_t)d << 16) | (uint32_t)j);
        }
        key_out[c] = key;
    });
    return SD_OK;
}

int sd_screen_regions(const uint32_t* keys, const int32_t* chunk_read, int64_t n_chunks, const int64_t* read_lens, int32_t n_reads,
                      int32_t part, int32_t overlap, int32_t thr, sd_screen_region* regions_out, int64_t cap, int64_t* n_regions,
                      char* errbuf, size_t errlen) {
    if (n_chunks < 0 || (n_chunks > 0 && (!keys || !chunk_read || !read_lens)) || !n_regions) return SD_ERR_PARAM;
    *n_regions = 0;
    std::string err;
    int rc = screen_plan_params(part, overlap, err);
    if (!rc && thr < 0) { err = "the screen's threshold must be >= 0"; rc = SD_ERR_PARAM; }
    if (!rc && overlap >= part) { err = "the screen needs overlap < part_size (the regions of a read must not overlap)"; rc = SD_ERR_PARAM; }
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    int64_t n = 0;
    for (int64_t c = 0; c < n_chunks;) {
        const int32_t r = chunk_read[c];
        if (r < 0 || r >= n_reads || (c > 0 && r < chunk_read[c - 1])) { set_err(errbuf, errlen, "sd_screen_regions: chunk_read is not a chunk table"); return SD_ERR_PARAM; }
        int64_t e = c;
        while (e < n_chunks && chunk_read[e] == r) ++e;   // the chunks of read r: c .. e - 1, chunk k at k * part
        for (int64_t a = c; a < e;) {
            if ((int32_t)(keys[a] >> 16) > thr) { ++a; continue; }
            int64_t b = a;
            uint32_t best = keys[a];
            while (b + 1 < e && (int32_t)(keys[b + 1] >> 16) <= thr) { ++b; best = std::min(best, keys[b]); }
            if (n < cap && regions_out) {
                sd_screen_region& g = regions_out[n];
                g.read = r;
                g.start = (a - c) * (int64_t)part;
                g.end_incl = std::min(read_lens[r], (b - c + 1) * (int64_t)part + overlap) - 1;
                g.n_chunks = (int32_t)(b - a + 1);
                g.best_key = best;
            }
            ++n;
            a = b + 1;
        }
        c = e;
    }
    *n_regions = n;
    if (n > cap) { set_err(errbuf, errlen, "sd_screen_regions: regions_out is too small"); return SD_ERR_PARAM; }
    return SD_OK;
}

}  // extern "C"

// Phase 1 of sd_run_files_screen: the keys of every chunk of the reads (host memory: the mapped FASTA), in chunk-table
// order.  The chunks are cut into batches that the device entries take in turn, one handle and one thread per entry; an
// entry packs batch k + 1 on host threads while the device screens its batch k.
namespace sdi {
int screen_file_reads(const char* const* seqs, const int64_t* lens, size_t n_reads, const char* const* mono_seqs,
                      const int32_t* mono_lens, int32_t n_mono, const sd_params* p, const std::vector<int32_t>& devs,
                      std::vector<uint32_t>& keys, double* kernel_ms, std::string& err) {
    std::vector<ChunkRef> ck;
    int rc = chunk_refs(lens, (int32_t)n_reads, p->part_size, p->overlap, ck, err);
    if (rc) return rc;
    keys.assign(ck.size(), 0xffffffffu);
    if (kernel_ms) *kernel_ms = 0;
    if (ck.empty()) return SD_OK;
    const size_t B = 8192;   // chunks per batch: 45 MB of bases at the default plan
    const size_t nb = (ck.size() + B - 1) / B;
    std::atomic<size_t> next{0};
    std::atomic<int> first_rc{SD_OK};
    std::mutex em;
    std::vector<double> ms(devs.size(), 0);
    auto entry = [&](size_t i) {
        sd_screen* h = nullptr;
        char eb[512] = {0};
        int r = sd_screen_create(mono_seqs, mono_lens, n_mono, devs[i], &h, eb, sizeof eb);
        std::string e2 = eb;
        if (r == SD_OK) {
            h->threads = std::max(1, p->threads / (int)devs.size());
            try {
                DeviceScope on(h->device);
                ScreenIn in;
                in.host_seqs = seqs;
                size_t prev = SIZE_MAX, prev_n = 0;   // the batch whose keys are on their way
                for (;;) {
                    const size_t b = first_rc.load() == SD_OK ? next.fetch_add(1) : nb;
                    if (b < nb) {
                        const size_t c0 = b * B, n = std::min(B, ck.size() - c0);
                        r = screen_launch(h, in, ck.data() + c0, n, nullptr, e2);
                        if (r) break;
                        if (prev != SIZE_MAX) screen_fetch_end(h, prev_n, keys.data() + prev * B);
                        screen_fetch_begin(h, n);
                        prev = b;
                        prev_n = n;
                    } else {
                        if (prev != SIZE_MAX) screen_fetch_end(h, prev_n, keys.data() + prev * B);
                        break;
                    }
                }
                ms[i] = h->kernel_ms;
            } catch (const HipFail& f) {
                r = SD_ERR_HIP;
                e2 = f.msg;
            }
        }
        if (h) sd_screen_destroy(h);
        if (r) {
            std::lock_guard<std::mutex> g(em);
            if (first_rc.load() == SD_OK) { first_rc.store(r); err = e2; }
        }
    };
    std::vector<std::thread> th;
    for (size_t i = 1; i < devs.size(); ++i) th.emplace_back(entry, i);
    entry(0);
    for (std::thread& t : th) t.join();
    if (kernel_ms)
        for (double v : ms) *kernel_ms += v;
    return first_rc.load();
}
}  // namespace sdi
