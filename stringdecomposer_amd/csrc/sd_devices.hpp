// sd_devices.hpp -- internal to libsd_hip.so: what a job on one or several devices of one process is made of, shared by
// sd_run_files.hip (sd_run_files*), sd_engine.hip (the raw calls) and sd_stream.hip (the streams): the device-list check,
// the batch plan of several pipelines and the budget rule of entries that share a device, the batch-ordered hand-over of
// their records (BatchTurns), the per-entry drivers (on_entries, drive_entry) and the owner of a job's pipelines (JobPipes).
#pragma once

#include "sd_pipeline.hpp"

namespace sdi {

static constexpr int kMaxDevices = 16;   // entries of a device list

// The device list of a multi-device call, checked completely before anything is started on any of its devices: 1 to
// kMaxDevices entries, each an existing gfx950 device (repeats allowed).  who names the call in the message of a bad
// count (devices == nullptr counts as one).
inline int check_device_list(const char* who, const int32_t* devices, int32_t n_devices, char* errbuf, size_t errlen) {
    if (!devices || n_devices < 1 || n_devices > kMaxDevices) {
        set_err(errbuf, errlen, std::string(who) + ": 1 to " + std::to_string(kMaxDevices) + " device entries");
        return SD_ERR_PARAM;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    static std::atomic<int> arch_ok[64];   // per ordinal: 0 not looked at, 1 gfx950, 2 another chip
    for (int32_t i = 0; i < n_devices; ++i) {
        const int32_t d = devices[i];
        if (d < 0 || d >= count) {
            set_err(errbuf, errlen, "device " + std::to_string(d) + " does not exist (" + std::to_string(count) + " HIP devices visible)");
            return d < 0 ? SD_ERR_PARAM : SD_ERR_NO_DEVICE;
        }
        int known = d < 64 ? arch_ok[d].load() : 0;
        if (known == 0) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, d) != hipSuccess) { (void)hipGetLastError(); known = 2; }
            else known = std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 2;
            if (d < 64) arch_ok[d].store(known);
        }
        if (known != 1) {
            set_err(errbuf, errlen, "device " + std::to_string(d) + " is not a gfx950 device");
            return SD_ERR_NO_DEVICE;
        }
    }
    return SD_OK;
}

// The rows per batch of a job on the entries devs whose pipelines hold entry_budget rows: every entry's budget, its
// device's free HBM shared with the other entries on that device (an explicit cap stays as it is); the job takes the
// smallest.  One entry: its budget as it is.
inline int64_t shared_row_budget(const std::vector<int64_t>& entry_budget, const std::vector<int32_t>& devs, const sd_params* p) {
    int64_t budget = INT64_MAX;
    for (size_t i = 0; i < devs.size(); ++i) {
        int64_t b = entry_budget[i];
        const int same = (int)std::count(devs.begin(), devs.end(), devs[i]);
        if (same > 1 && p->max_batch_rows <= 0 && !getenv("SD_BATCH_ROWS")) b = std::max<int64_t>(b / same, (int64_t)p->part_size + p->overlap);
        budget = std::min(budget, b);
    }
    return budget;
}

// The pipelines of a job (one per device entry, several with sd_run_files_devices) hand their batches to the assembler
// from their own driver threads, and this makes them take turns in batch order -- batch b's records (every slice of them) reach the
// assembler only after all of batch b - 1's have.  A pipeline pops its batches in the order it was dealt them, and it is
// always dealt the lowest batch nobody has, so the thread that holds the batch whose turn it is never waits for another.
// abort() (a failed pipeline) releases every waiter; their records are dropped.
struct BatchTurns {
    std::mutex m;
    std::condition_variable cv;
    size_t turn = 0;
    bool aborted = false;
    bool wait(size_t b) {   // false: the job was aborted
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return aborted || turn == b; });
        return !aborted;
    }
    void done(size_t b) {   // the last slice of batch b was consumed
        {
            std::lock_guard<std::mutex> g(m);
            if (turn == b) turn = b + 1;
        }
        cv.notify_all();
    }
    void abort() {
        {
            std::lock_guard<std::mutex> g(m);
            aborted = true;
        }
        cv.notify_all();
    }
    bool is_aborted() {
        std::lock_guard<std::mutex> g(m);
        return aborted;
    }
};

// The driver of one device entry of a job (every job that runs to its end, one entry or several; not the streams):
// push(b) deals batch b to the entry's pipeline (whose sinks take their turns in `turns`) until the batches run out, the
// job has failed somewhere (turns aborted, a sink failed: sink_rc) or this pipeline fails; then busy() runs -- once, while
// the device works on what was dealt, unless a push failed -- and the pipeline is drained.  A pop that fails drops its
// batch before the batch's last slice reaches the assembler, so every batch behind it -- in this pipeline and in the
// others -- would wait for that turn forever: the turns are aborted at once, and the rest is drained with sinks that
// return at once.  (Pipe: Pipeline, or the host-only model of sd_multi_device_selftest.)  Returns the first error of
// this entry; dealt counts the batches it took.
template <class Pipe, class Push, class Busy>
int drive_entry(Pipe& pq, BatchTurns& turns, std::atomic<size_t>& next_batch, size_t n_batches,
                const std::atomic<int>& sink_rc, Push&& push, int64_t& dealt, Busy&& busy) {
    int r = SD_OK;
    while (r == SD_OK && sink_rc.load() == SD_OK && !turns.is_aborted()) {
        const size_t b = next_batch.fetch_add(1);
        if (b >= n_batches) break;
        r = push(b);
        if (r == SD_OK) ++dealt;
        else turns.abort();   // (this batch, or the one a full pipeline popped for it, never reaches its sink)
    }
    if (r == SD_OK) busy();
    while (pq.inflight() > 0) {
        const int e = pq.pop();
        if (e) {
            if (r == SD_OK) r = e;
            turns.abort();
        }
    }
    return r;
}

// The batches of a job on n_dev pipelines: at least min_batches and 2 * n_dev of them (as far as the chunks go), so that
// every pipeline gets work and the last batch to finish is short, cut where the cumulative rows cross k / nb of the
// total -- equal shares up to one chunk -- and none of several chunks above the budget.
inline void plan_device_batches(const std::vector<CRef>& table, int64_t budget, int min_batches, int n_dev,
                                std::vector<std::pair<size_t, size_t>>& out) {
    out.clear();
    const size_t n = table.size();
    if (n == 0) return;
    std::vector<int64_t> cum(n + 1, 0);
    int64_t lmax = 1;
    for (size_t c = 0; c < n; ++c) { cum[c + 1] = cum[c] + table[c].len; lmax = std::max<int64_t>(lmax, table[c].len); }
    budget = std::max<int64_t>(budget, 1);
    const int64_t holds = std::max<int64_t>(1, budget - (lmax - 1));
    size_t nb = std::max<size_t>({(size_t)std::max(min_batches, 1), (size_t)2 * (size_t)std::max(n_dev, 1),
                                  (size_t)((cum[n] + holds - 1) / holds)});
    for (nb = std::min(nb, n);; nb = std::min(nb + 1, n)) {
        out.clear();
        bool fits = true;
        size_t c0 = 0;
        for (size_t k = 1; k <= nb; ++k) {
            const int64_t want = (int64_t)((__int128)cum[n] * (int64_t)k / (int64_t)nb);
            size_t c1 = k == nb ? n : (size_t)(std::lower_bound(cum.begin(), cum.end(), want) - cum.begin());
            c1 = std::min(std::max(c1, c0 + 1), n - (nb - k));
            if (c1 - c0 > 1 && cum[c1] - cum[c0] > budget) fits = false;
            out.emplace_back(c0, c1);
            c0 = c1;
        }
        if (fits || nb == n) return;
    }
}

// The planner of a job: plan_batches for one device entry (a job that fits one batch stays one batch), plan_device_batches
// for several (at least two batches per entry, so that every pipeline gets work).
inline void cut_batches(const std::vector<CRef>& table, int64_t budget, int min_batches, int n_dev,
                        std::vector<std::pair<size_t, size_t>>& out) {
    if (n_dev == 1) plan_batches(table, 0, table.size(), budget, min_batches, out);
    else plan_device_batches(table, budget, min_batches, n_dev, out);
}

// fn(i) for every device entry of a job.  One entry: inline, on the calling thread and its current device (as every
// single-device call).  Several: side by side, each on a thread bound to devs[i] (hipSetDevice is per host thread); a
// failed hipSetDevice or a std::bad_alloc there is the entry's result, with its message in msg[i], and calls on_fail().
// Returns the first failed entry's result; its message (err) names the device when there are several.
template <class Fn, class OnFail>
int on_entries(const std::vector<int32_t>& devs, std::vector<std::string>& msg, std::string& err, Fn&& fn, OnFail&& on_fail) {
    std::vector<int> rc(devs.size(), SD_OK);
    if (devs.size() == 1) rc[0] = fn(0);
    else {
        struct Joined { std::vector<std::thread> t; ~Joined() { for (std::thread& x : t) x.join(); } } th;
        for (size_t i = 0; i < devs.size(); ++i)
            th.t.emplace_back([&, i]() {
                try {
                    if (hipSetDevice(devs[i]) == hipSuccess) { rc[i] = fn((int)i); return; }
                    (void)hipGetLastError();
                    rc[i] = SD_ERR_HIP;
                    msg[i] = "hipSetDevice failed";
                } catch (const std::bad_alloc&) {
                    rc[i] = SD_ERR_INTERNAL;
                    msg[i] = "out of host memory";
                }
                on_fail();
            });
    }
    for (size_t i = 0; i < rc.size(); ++i)
        if (rc[i]) {
            err = devs.size() > 1 ? "device " + std::to_string(devs[i]) + ": " + msg[i] : msg[i];
            return rc[i];
        }
    return SD_OK;
}

// The pipelines of a job that runs to its end, one per device entry: sd_run_files* ('1', or '2' with --second-best) and
// the raw calls of sd_engine.hip ('C', the one entry {p->device}).  This is the only place that takes pipelines from the
// cache and gives them back.  The cache key of an entry is the job's kind, parameters (with the entry's device) and
// monomers, and beyond the first entry its index.
struct JobPipes {
    const std::vector<int32_t> devs;
    std::vector<std::unique_ptr<Pipeline>> pipes;   // after open: one per entry (empty if its device could not be opened)
    std::vector<std::string> keys, msg;             // per entry: cache key, message of its first error
    std::vector<int64_t> budget, dealt;             // per entry: rows per batch (row_budget), batches it took
    std::vector<char> cached;                       // per entry: the pipeline came from the cache

    explicit JobPipes(const std::vector<int32_t>& d)
        : devs(d), pipes(d.size()), keys(d.size()), msg(d.size()), budget(d.size(), 0), dealt(d.size(), 0), cached(d.size(), 0) {}
    bool reused() const { return std::count(cached.begin(), cached.end(), 1) == (std::ptrdiff_t)cached.size(); }

    // Every entry's pipeline, from the cache or new, on the entry's thread (on_entries); on_engine (may be empty) is
    // called for every engine the pipelines create.  Returns the first error, its message in err.
    int open(const sd_params* p, char kind, const TemplateSet& ts, const std::function<void(sd_engine*)>& on_engine, std::string& err) {
        const int rc = on_entries(devs, msg, err, [&](int i) -> int {
            sd_params pi = *p, pe = *p;
            pi.device = pe.device = devs[(size_t)i];
            apply_env_overrides(pe);   // (host threads do not shape an engine; pipe_cache_key leaves them out)
            keys[(size_t)i] = pipe_cache_key(pe, kind, ts.mseq, ts.mlen) + (i > 0 ? "#entry " + std::to_string(i) : std::string());
            std::unique_ptr<Pipeline>& h = pipes[(size_t)i];
            if (!getenv("SD_PIPE_CACHE_OFF")) h = pipe_cache_take(keys[(size_t)i]);
            cached[(size_t)i] = h != nullptr;
            if (!h) h.reset(new Pipeline);
            h->restart_idle = true;
            h->on_engine = on_engine;
            if (cached[(size_t)i]) h->begin_job(&pi, ts.mseq.data(), ts.mlen.data(), (int32_t)ts.mseq.size());
            else if (const int r = h->create(&pi, ts.mseq.data(), ts.mlen.data(), (int32_t)ts.mseq.size())) {
                msg[(size_t)i] = h->eb;
                return r;
            }
            budget[(size_t)i] = h->row_budget();   // (hipMemGetInfo of the entry's device)
            return SD_OK;
        }, [] {});
        for (std::unique_ptr<Pipeline>& h : pipes)
            if (!h) h.reset(new Pipeline);   // (an entry whose device could not be selected)
        return rc;
    }

    // Deals the batches -- the chunks [c0, c1) of `table`, their identities cut into slices by slices(c0, c1, slice_end)
    // -- to the entries' pipelines and drains them (drive_entry on every entry, through on_entries); every slice of
    // records goes to sink(pq, c0', c1', recs, rec_off) in batch order (BatchTurns).  busy() runs in entry 0's driver,
    // i.e. on the calling thread of a one-entry job.  Returns the first error, its message in err.
    template <class Reads, class Slices, class Sink, class Busy>
    int drive(const Reads& reads, const std::vector<CRef>& table, const std::vector<std::pair<size_t, size_t>>& batches,
              const std::atomic<int>& sink_rc, Slices&& slices, Sink&& sink, Busy&& busy, std::string& err) {
        BatchTurns turns;
        std::atomic<size_t> next_batch{0};
        return on_entries(devs, msg, err, [&](int i) {
            Pipeline& pq = *pipes[(size_t)i];
            std::string& m = msg[(size_t)i];
            std::vector<const char*> cptr;
            std::vector<int32_t> clen;
            std::vector<int> slice_end;
            const int r = drive_entry(pq, turns, next_batch, batches.size(), sink_rc, [&](size_t b) {
                const size_t c0 = batches[b].first, c1 = batches[b].second;
                batch_chunks(reads, table, c0, c1, cptr, clen);
                slice_end.clear();
                slices(c0, c1, slice_end);
                const int rp = pq.push(cptr, clen, [&turns, &pq, &sink, b, c0, c1](const sd_rec* rr, const int64_t* ro, size_t first, size_t n) {
                    if (turns.wait(b)) sink(pq, c0 + first, c0 + first + n, rr, ro);
                    if (c0 + first + n == c1) turns.done(b);
                }, slice_end);
                if (rp) m = pq.eb;   // (what failed first, not a pop while the pipeline drains)
                return rp;
            }, dealt[(size_t)i], [&] { if (i == 0) busy(); });
            if (r && m.empty()) m = pq.eb;
            return r;
        }, [&turns] { turns.abort(); });
    }

    // The pipelines of a job that succeeded go back to the cache (unless SD_PIPE_CACHE_OFF); on_engine, which refers to
    // the caller's locals, is cleared in any case.
    void give_back(bool ok) {
        const bool keep = ok && !getenv("SD_PIPE_CACHE_OFF");
        for (size_t i = 0; i < pipes.size(); ++i) {
            pipes[i]->on_engine = nullptr;
            if (keep) pipe_cache_give(keys[i], std::move(pipes[i]), (int)i);
        }
    }
};

}  // namespace sdi
