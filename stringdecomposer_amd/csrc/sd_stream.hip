// sd_stream.hip -- sd_stream_*: the streaming form of the job (sequences in host memory -> rows in host memory,
// AlignReadsSet of main.cpp:67-122 without the text), jobs pipelined through the device in sub-batches; in final mode
// (sd_stream_create_final) the rows of final_decomposition.tsv / _alt.tsv as typed rows instead of the raw ones; with a
// device list (sd_stream_create_devices, sd_stream_create_final_devices) one pipeline per entry, each driven by a thread
// of its own.
#include "sd_devices.hpp"

// (lib.py's numpy dtype of the rows mirrors this layout)
static_assert(sizeof(sd_final_row) == 80 && offsetof(sd_final_row, start) == 8 && offsetof(sd_final_row, ident) == 40 &&
              offsetof(sd_final_row, reliable) == 72, "sd_final_row layout");

namespace sdi {
// The final mode of a stream (sd_stream_create_final): the post-processor of the file path -- its selection rules, and its
// fallback for pairs the in-stream kernels do not take -- and whether the engines compute the identities in-stream.
struct FinalMode {
    sd::PostProcessor pp;
    bool second_best = false;
    std::atomic<bool> ident{true};   // every engine so far took the identity tables (engine_set_identity)
    int64_t kept = 0;        // rows handed to callers
};

// A submitted job: its rows as they are assembled and, in final mode, its own copy of the reads and its kept rows.
struct StreamJob : RowJob {
    std::vector<std::string> seq;
    sd::HeapArray<sd_final_row> fin;   // handed to the caller by collect
    sd::HeapArray<double> alt;
    int rc = SD_OK;          // first failure of the job's post-processing
    std::string err;
    // several entries: where the entries pack the job's batches from (the caller's buffers in raw mode, seq in final
    // mode) and, in raw mode, its batches no entry has packed yet (submit returns when they are 0)
    const char* const* reads = nullptr;
    std::vector<const char*> own;
    int to_pack = 0;
};

// Final mode: the records of the chunks [c0, c1) are assembled into the rows of the reads they complete, which go through
// the post-processor at once with the identity words that came with them (sd_run_files' assemble without the hand-over:
// the words stay in the pipeline's pinned blocks until the sink returns).  Rows of a read that began in an earlier batch
// carry their words by value (RowJob::xid / xidh).
static void final_sink(FinalMode& fm, const Pipeline& pipe, StreamJob& j, size_t c0, size_t c1, const sd_rec* recs, const int64_t* roff) {
    const size_t r0 = j.next_read;
    j.n_rows = 0;
    j.row_off[r0] = 0;
    j.bid = pipe.cur_ident.id;
    j.bidh = pipe.cur_ident.idh;
    j.add(c0, c1, recs, roff);
    if (j.oom && j.rc == SD_OK) { j.rc = SD_ERR_INTERNAL; j.err = "out of host memory"; }
    const size_t r1 = j.next_read;
    if (r1 == r0) return;
    if (j.rc == SD_OK) {
        std::vector<sd::PostRead> pr;
        for (size_t r = r0; r < r1; ++r) pr.push_back(sd::PostRead{"", 0, j.seq[r].data(), (int64_t)j.seq[r].size()});
        // a batch without identities (more records than the outputs had room for) sends these rows to the fallback
        const sd::IdentRef iref{j.bid, fm.second_best ? j.bidh : nullptr, j.rsrc, j.xid.data(), j.xidh.data()};
        try {
            j.rc = fm.pp.process_rows(pr.data(), r1 - r0, (int32_t)r0, j.rows, j.row_off + r0, j.fin, j.alt, j.err,
                                      j.per && j.ident_ok ? &iref : nullptr);
        } catch (const std::bad_alloc&) {
            j.rc = SD_ERR_INTERNAL;
            j.err = "out of host memory";
        }
    }
    j.xid.clear();
    j.xidh.clear();
    j.ident_ok = j.carry.empty() || j.bid != nullptr;
}

// The pipelines of a stream made with several device entries (sd_stream_create_devices), one per entry, each driven for
// the life of the stream by a thread of its own that is bound to the entry's device and makes every HIP call of its
// pipeline.  submit appends a job's batches to one queue; their numbers run on across jobs, and an entry always takes
// the one at the front -- the lowest batch no entry has.  The sinks take their turns in batch order (BatchTurns), so the
// rows are assembled as by one pipeline.  An entry with nothing to take pops its oldest batch (without that, a batch
// whose turn has come could sit in an idle pipeline while the others wait for it).  (drive_entry does not fit here: it
// drains its pipeline when a job's batches run out, and a stream keeps batches in flight across job boundaries.)
// The first failure of any entry aborts the turns and drops the queued batches; every entry drains what it has in
// flight, and the caller's next wait (settle) reports the failure, drops the jobs and starts the numbering anew.
struct StreamEntries {
    // an entry's pipeline counters, copied under the lock after every push and pop (stats read them while it runs)
    struct Counters {
        double fill_ms = 0, trace_ms = 0, compact_ms = 0, run_ms = 0, ident_ms = 0, pack_s = 0, wait_s = 0, sink_s = 0;
        int64_t launches = 0, batches = 0, rows = 0, ident_pairs = 0;
    };
    struct Queued { StreamJob* job; size_t c0, c1, b; };
    std::vector<int32_t> devs;
    std::vector<std::unique_ptr<Pipeline>> pipes;
    FinalMode* fm = nullptr;
    std::mutex m;
    std::condition_variable cv;
    std::deque<Queued> queue;
    size_t next_b = 0;            // number of the next batch submitted
    BatchTurns turns;
    bool stop = false, failed = false;
    uint64_t gen = 0;             // failures so far; an entry has drained for failure `gen` when its seen == gen
    int drained = 0;              // entries that have drained for the current failure
    int fail_rc = SD_OK;
    std::string fail_msg;
    std::vector<int> inflight;
    std::vector<int64_t> dealt;
    std::vector<Counters> cnt;
    int64_t fallback_blocks = 0;  // fm->pp.fallback_blocks as the last sink left it
    int64_t info0[8] = {0};       // sd_engine_info of entry 0's first engine, as of its last push or pop
    std::vector<std::thread> th;

    ~StreamEntries() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        turns.abort();   // (sinks of batches still in flight return at once)
        cv.notify_all();
        for (std::thread& t : th) t.join();
    }

    // The pipelines, each created on a thread bound to its device (on_entries), and the rows per batch of the stream.
    int open(const sd_params* p, const std::vector<const char*>& ms, const int32_t* mono_lens, int32_t n_mono,
             int64_t& budget, std::string& err) {
        const size_t nd = devs.size();
        pipes.resize(nd);
        inflight.assign(nd, 0);
        dealt.assign(nd, 0);
        cnt.assign(nd, Counters{});
        std::vector<int64_t> entry_budget(nd, 0);
        std::vector<std::string> msg(nd);
        auto open_pipe = [&](int i) -> int {
            sd_params pi = *p;
            pi.device = devs[(size_t)i];
            pipes[(size_t)i].reset(new Pipeline);
            Pipeline* q = pipes[(size_t)i].get();
            if (fm) {
                FinalMode* f = fm;
                q->on_engine = [f, q](sd_engine* e) {
                    if (q->p.reserved[1] & SD_FLAG_NO_STREAM_IDENT) f->ident = false;
                    if (f->ident && !engine_set_identity(e, f->pp.interleaved_seqs(), f->pp.own_interleaved(), f->second_best)) f->ident = false;
                };
            }
            if (const int r = q->create(&pi, ms.data(), mono_lens, n_mono)) { msg[(size_t)i] = q->eb; return r; }
            entry_budget[(size_t)i] = q->row_budget();
            return SD_OK;
        };
        int rc = on_entries(devs, msg, err, open_pipe, [] {});
        if (rc) {   // what was created goes on its own device's thread
            std::string e2;
            (void)on_entries(devs, msg, e2, [&](int i) { pipes[(size_t)i].reset(); return SD_OK; }, [] {});
            return rc;
        }
        budget = shared_row_budget(entry_budget, devs, p);
        (void)sd_engine_info(pipes[0]->eng[0], info0);
        for (size_t i = 0; i < nd; ++i) th.emplace_back([this, i] { drive((int)i); });
        return SD_OK;
    }

    // The first failure of the stream (under the lock): the turns are aborted, the queued batches dropped.
    void fail_locked(size_t i, int rc, const std::string& msg) {
        if (failed) return;
        failed = true;
        ++gen;
        drained = 0;
        fail_rc = rc;
        fail_msg = "device " + std::to_string(devs[i]) + ": " + msg;
        queue.clear();
        turns.abort();
    }

    // Batch q on entry i's pipeline: its sink assembles the records in q's turn (final mode: with the identities of this
    // pipeline's engine) and counts the batch off its job when the last slice is through.
    int push(size_t i, const Queued& q, std::vector<const char*>& cptr, std::vector<int32_t>& clen, std::vector<int>& slice_end) {
        Pipeline& pq = *pipes[i];
        StreamJob* jp = q.job;
        batch_chunks(jp->reads, jp->table, q.c0, q.c1, cptr, clen);
        slice_end.clear();
        if (fm && fm->second_best && jp->per) ident_slices(jp->table, q.c0, q.c1, slice_end);
        const int32_t dev = devs[i];
        const size_t c0 = q.c0, c1 = q.c1, b = q.b;
        return pq.push(cptr, clen, [this, &pq, jp, dev, b, c0, c1](const sd_rec* r, const int64_t* ro, size_t first, size_t n) {
            const bool mine = turns.wait(b);   // (false: the stream failed; the batch is dropped)
            if (mine) {
                if (fm) {
                    final_sink(*fm, pq, *jp, c0 + first, c0 + first + n, r, ro);
                    if (dev != devs[0]) (void)hipSetDevice(dev);   // (the fallback identities run on devs[0], sd_nw.hip)
                } else {
                    jp->add(c0 + first, c0 + first + n, r, ro);
                }
            }
            if (c0 + first + n == c1) {
                if (mine) {
                    std::lock_guard<std::mutex> g(m);
                    --jp->batches_left;   // (the last use of jp: collect may hand the job over from here on)
                    if (fm) fallback_blocks = fm->pp.fallback_blocks;
                }
                cv.notify_all();
                turns.done(b);
            }
        }, slice_end);
    }

    // The driver of entry i: push what the queue holds, pop when it holds nothing, drain after a failure and at the end.
    void drive(int ii) {
        const size_t i = (size_t)ii;
        Pipeline& pq = *pipes[i];
        const bool bound = hipSetDevice(devs[i]) == hipSuccess;
        if (!bound) (void)hipGetLastError();
        uint64_t seen = 0;
        std::vector<const char*> cptr;
        std::vector<int32_t> clen;
        std::vector<int> slice_end;
        enum { PUSH, POP, DRAIN, EXIT };
        for (;;) {
            Queued q{};
            int act;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || (failed ? seen != gen : (!queue.empty() || inflight[i] > 0)); });
                if (stop) act = EXIT;
                else if (failed) act = DRAIN;
                else if (!queue.empty()) { q = queue.front(); queue.pop_front(); act = PUSH; }
                else act = POP;
            }
            int r = SD_OK;
            std::string msg;
            try {
                if (act == PUSH && !bound) { r = SD_ERR_HIP; msg = "hipSetDevice failed"; }
                else if (act == PUSH) r = push(i, q, cptr, clen, slice_end);
                else if (act == POP) r = pq.pop();
                else
                    while (pq.inflight() > 0) (void)pq.pop();   // (turns aborted: the sinks return at once)
                if (r && msg.empty()) msg = pq.eb;
            } catch (const std::bad_alloc&) {
                r = SD_ERR_INTERNAL;
                msg = "out of host memory";
            }
            {
                std::lock_guard<std::mutex> g(m);
                inflight[i] = pq.inflight();
                Counters& c = cnt[i];
                c.fill_ms = pq.fill_ms; c.trace_ms = pq.trace_ms; c.compact_ms = pq.compact_ms; c.run_ms = pq.run_ms;
                c.ident_ms = pq.ident_ms; c.pack_s = pq.pack_s; c.wait_s = pq.wait_s; c.sink_s = pq.sink_s;
                c.launches = pq.launches; c.batches = pq.batches; c.rows = pq.rows; c.ident_pairs = pq.ident_pairs;
                if (i == 0) (void)sd_engine_info(pq.eng[0], info0);
                if (act == PUSH) {
                    if (r == SD_OK) ++dealt[i];
                    if (q.job->to_pack > 0) --q.job->to_pack;
                }
                if (r) fail_locked(i, r, msg);
                if (act == DRAIN) { seen = gen; ++drained; }
            }
            cv.notify_all();
            if (act == EXIT) break;
        }
        pipes[i].reset();   // its streams, events and engines, on its device's thread
    }

    // Caller side, after a failure: waits until every entry has drained, then reports the failure and clears it (the next
    // batch submitted has the next turn).  The caller drops every job.
    int settle(std::unique_lock<std::mutex>& lk, std::string& err) {
        cv.wait(lk, [&] { return drained == (int)devs.size(); });
        const int rc = fail_rc;
        err = fail_msg;
        failed = false;
        drained = 0;
        fail_rc = SD_OK;
        {
            std::lock_guard<std::mutex> g(turns.m);
            turns.turn = next_b;
            turns.aborted = false;
        }
        return rc;
    }
};
}  // namespace sdi

struct sd_stream {
    sd_params p{};
    std::vector<std::string> mono;       // owned copies
    std::unique_ptr<FinalMode> fin;      // final mode only
    Pipeline pipe;
    int sub_batches = 1;
    std::vector<std::unique_ptr<StreamJob>> jobs;   // FIFO: submitted, not collected yet
    int64_t budget = 0;
    double submit_s = 0, collect_s = 0;
    int64_t n_jobs = 0;
    std::unique_ptr<StreamEntries> multi;   // several device entries (then `pipe` is not used); destroyed first
};

// devs (several entries): one pipeline per entry (StreamEntries) instead of `pipe`
static int stream_open(sd_stream* s, const sd_params* p, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                int32_t sub_batches, char* errbuf, size_t errlen, const std::vector<int32_t>* devs = nullptr) {
    s->p = *p;
    s->sub_batches = std::max(1, (int)sub_batches);
    std::vector<const char*> ms;
    for (int32_t m = 0; m < n_mono; ++m) {
        if (mono_lens[m] <= 0) { set_err(errbuf, errlen, "ERROR: empty monomer sequence"); return SD_ERR_EMPTY; }
        s->mono.emplace_back(mono_seqs[m], (size_t)mono_lens[m]);
    }
    for (const std::string& m : s->mono) ms.push_back(m.data());
    if (devs && devs->size() > 1) {
        s->multi.reset(new StreamEntries);
        s->multi->devs = *devs;
        s->multi->fm = s->fin.get();
        std::string err;
        const int rc = s->multi->open(p, ms, mono_lens, n_mono, s->budget, err);
        if (rc) { set_err(errbuf, errlen, err); s->multi.reset(); }
        return rc;
    }
    const int rc = s->pipe.create(p, ms.data(), mono_lens, n_mono);
    if (rc) { set_err(errbuf, errlen, s->pipe.eb); return rc; }
    s->budget = s->pipe.row_budget();
    return SD_OK;
}

// Waits for every batch of the oldest job.  On failure every job is dropped (batches of this or a later job may still
// be in flight and their sinks hold pointers to the jobs: all of them are waited for first, as sd_stream_submit's error
// path does).
static int stream_wait_oldest(sd_stream* s, char* errbuf, size_t errlen) {
    StreamJob* job = s->jobs.front().get();
    int rc = SD_OK;
    if (StreamEntries* me = s->multi.get()) {   // its batches consumed, or the stream failed before that
        std::unique_lock<std::mutex> lk(me->m);
        me->cv.wait(lk, [&] { return job->batches_left == 0 || me->failed; });
        if (job->batches_left == 0) return SD_OK;
        std::string err;
        rc = me->settle(lk, err);
        lk.unlock();
        set_err(errbuf, errlen, err);
        s->jobs.clear();
        return rc;
    }
    while (job->batches_left > 0 && rc == SD_OK) {
        if (s->pipe.inflight() == 0) { set_err(errbuf, errlen, "stream lost a batch"); rc = SD_ERR_INTERNAL; break; }
        rc = s->pipe.pop();
        if (rc) set_err(errbuf, errlen, s->pipe.eb);
    }
    if (rc != SD_OK) {
        (void)s->pipe.drain();
        s->jobs.clear();
    }
    return rc;
}

extern "C" {

int sd_stream_create(sd_stream** out, const sd_params* p, const char* const* mono_seqs,
                     const int32_t* mono_lens, int32_t n_mono, int32_t sub_batches, char* errbuf, size_t errlen) {
    if (!out) return SD_ERR_PARAM;
    *out = nullptr;
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_mono <= 0 || !mono_seqs || !mono_lens) { set_err(errbuf, errlen, "no monomers"); return SD_ERR_PARAM; }
    if (p->reserved[1] & SD_FLAG_PROFILE) { set_err(errbuf, errlen, "SD_FLAG_PROFILE needs a final-mode stream"); return SD_ERR_PARAM; }
    std::unique_ptr<sd_stream> s(new sd_stream);
    rc = stream_open(s.get(), p, mono_seqs, mono_lens, n_mono, sub_batches, errbuf, errlen);
    if (rc) return rc;
    *out = s.release();
    return SD_OK;
}

}  // extern "C"

// sd_stream_create_final, and with devs (several entries) sd_stream_create_final_devices
static int stream_create_final(sd_stream** out, const sd_params* p, const char* const* mono_names,
                               const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                               int32_t sub_batches, int32_t min_identity, int32_t second_best,
                               const double* lr_coef, char* errbuf, size_t errlen, const std::vector<int32_t>* devs) try {
    if (!out) return SD_ERR_PARAM;
    *out = nullptr;
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (n_mono <= 0 || !mono_seqs || !mono_lens) { set_err(errbuf, errlen, "no monomers"); return SD_ERR_PARAM; }
    if (!mono_names) { set_err(errbuf, errlen, "no monomer names"); return SD_ERR_PARAM; }
    if (!lr_coef) { set_err(errbuf, errlen, "no logistic-regression coefficients"); return SD_ERR_PARAM; }
    std::vector<sd::Seq> monos;
    for (int32_t m = 0; m < n_mono; ++m) {
        if (!mono_names[m]) { set_err(errbuf, errlen, "monomer " + std::to_string(m) + " has no name"); return SD_ERR_PARAM; }
        if (!mono_seqs[m] || mono_lens[m] <= 0) { set_err(errbuf, errlen, "ERROR: empty monomer sequence"); return SD_ERR_EMPTY; }
        monos.push_back(sd::Seq{mono_names[m], std::string(mono_seqs[m], (size_t)mono_lens[m])});
    }
    std::unique_ptr<sd_stream> s(new sd_stream);
    s->fin.reset(new FinalMode);
    FinalMode& fm = *s->fin;
    fm.second_best = second_best != 0;
    rc = fm.pp.init(monos, min_identity, fm.second_best, lr_coef, p->device, p->threads, err);
    if (rc == SD_OK && (p->reserved[1] & SD_FLAG_PROFILE)) rc = fm.pp.enable_profile(err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    sd_params q = *p;   // (the flag shapes the post-processing only)
    q.reserved[1] &= ~SD_FLAG_PROFILE;
    // every engine of the pipeline (the first now, the others as the pipeline creates them) computes the identities of
    // its batches in-stream; a template set the kernels do not take, or SD_FLAG_NO_STREAM_IDENT, leaves them all to
    // the fallback
    sd_stream* sp = s.get();
    s->pipe.on_engine = [sp](sd_engine* e) {
        FinalMode& f = *sp->fin;
        if (sp->pipe.p.reserved[1] & SD_FLAG_NO_STREAM_IDENT) f.ident = false;
        if (f.ident && !engine_set_identity(e, f.pp.interleaved_seqs(), f.pp.own_interleaved(), f.second_best)) f.ident = false;
    };
    rc = stream_open(s.get(), &q, mono_seqs, mono_lens, n_mono, sub_batches, errbuf, errlen, devs);
    if (rc) return rc;
    *out = s.release();
    return SD_OK;
} catch (const std::bad_alloc&) {
    set_err(errbuf, errlen, "out of host memory");
    return SD_ERR_INTERNAL;
}

extern "C" {

int sd_stream_create_final(sd_stream** out, const sd_params* p, const char* const* mono_names,
                           const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                           int32_t sub_batches, int32_t min_identity, int32_t second_best,
                           const double* lr_coef, char* errbuf, size_t errlen) {
    return stream_create_final(out, p, mono_names, mono_seqs, mono_lens, n_mono, sub_batches, min_identity, second_best,
                               lr_coef, errbuf, errlen, nullptr);
}

int sd_stream_create_devices(sd_stream** out, const sd_params* p, const int32_t* devices, int32_t n_devices,
                             const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, int32_t sub_batches,
                             char* errbuf, size_t errlen) try {
    if (!out) return SD_ERR_PARAM;
    *out = nullptr;
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    rc = check_device_list("sd_stream_create_devices", devices, n_devices, errbuf, errlen);
    if (rc) return rc;
    sd_params q = *p;
    q.device = devices[0];
    if (n_devices == 1) return sd_stream_create(out, &q, mono_seqs, mono_lens, n_mono, sub_batches, errbuf, errlen);
    if (n_mono <= 0 || !mono_seqs || !mono_lens) { set_err(errbuf, errlen, "no monomers"); return SD_ERR_PARAM; }
    if (p->reserved[1] & SD_FLAG_PROFILE) { set_err(errbuf, errlen, "SD_FLAG_PROFILE needs a final-mode stream"); return SD_ERR_PARAM; }
    const std::vector<int32_t> devs(devices, devices + n_devices);
    std::unique_ptr<sd_stream> s(new sd_stream);
    rc = stream_open(s.get(), &q, mono_seqs, mono_lens, n_mono, sub_batches, errbuf, errlen, &devs);
    if (rc) return rc;
    *out = s.release();
    return SD_OK;
} catch (const std::bad_alloc&) {
    set_err(errbuf, errlen, "out of host memory");
    return SD_ERR_INTERNAL;
}

int sd_stream_create_final_devices(sd_stream** out, const sd_params* p, const int32_t* devices, int32_t n_devices,
                                   const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens,
                                   int32_t n_mono, int32_t sub_batches, int32_t min_identity, int32_t second_best,
                                   const double* lr_coef, char* errbuf, size_t errlen) try {
    if (!out) return SD_ERR_PARAM;
    *out = nullptr;
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    rc = check_device_list("sd_stream_create_final_devices", devices, n_devices, errbuf, errlen);
    if (rc) return rc;
    sd_params q = *p;
    q.device = devices[0];   // (also the device of the fallback identities)
    const std::vector<int32_t> devs(devices, devices + n_devices);
    return stream_create_final(out, &q, mono_names, mono_seqs, mono_lens, n_mono, sub_batches, min_identity, second_best,
                               lr_coef, errbuf, errlen, n_devices > 1 ? &devs : nullptr);
} catch (const std::bad_alloc&) {
    set_err(errbuf, errlen, "out of host memory");
    return SD_ERR_INTERNAL;
}

void sd_stream_destroy(sd_stream* s) { delete s; }

}  // extern "C"

// A submitted job before its batches: the chunk table, the rows' offsets and, in final mode, the copy of the reads
// (own: pointers to it).  Returns the job's batches' source: the caller's buffers or the copy.
static int stream_job(sd_stream* s, const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads, StreamJob* job,
                      std::vector<const char*>& own, const char* const*& reads, char* errbuf, size_t errlen) {
    job->n_reads = n_reads;
    job->threads = s->p.threads;
    job->nch.assign((size_t)n_reads, 0);
    for (int32_t r = 0; r < n_reads; ++r) {
        if (read_lens[r] <= 0) { set_err(errbuf, errlen, "ERROR: Sequence #" + std::to_string(r) + " is empty"); return SD_ERR_EMPTY; }
        job->nch[(size_t)r] = sd::chunk_plan(read_lens[r], s->p.part_size, s->p.overlap,
                                             [&](int64_t off, int32_t l) { job->table.push_back(CRef{r, off, l}); });
    }
    job->row_off = static_cast<int64_t*>(std::calloc((size_t)n_reads + 1, sizeof(int64_t)));
    if (!job->row_off) { set_err(errbuf, errlen, "out of host memory"); return SD_ERR_INTERNAL; }
    FinalMode* fm = s->fin.get();
    reads = read_seqs;
    if (fm) {   // the fallback identities read the text when the rows come back: the job keeps a copy (sd_hip.h)
        job->seq.resize((size_t)n_reads);
        sd::parallel_for(n_reads, s->p.threads, 1, [&](int64_t r) { job->seq[(size_t)r].assign(read_seqs[r], (size_t)read_lens[r]); });
        for (const std::string& q : job->seq) own.push_back(q.data());
        reads = own.data();
        if (fm->ident) job->per = fm->second_best ? (int)fm->pp.interleaved_seqs().size() : 1;
    }
    return SD_OK;
}

// sd_stream_submit with several entries: the job's batches (plan_device_batches: at least two per entry) join the queue
// and the job the FIFO.  A raw-mode submit returns once every batch of the job has been packed by its entry, so that
// the caller's read buffers are free (the entries pack from them; a final-mode job packs from its own copy and submit
// returns at once).  A failure of the stream that this call meets is reported here and drops every job, this one too.
static int entries_submit(sd_stream* s, StreamEntries& me, std::unique_ptr<StreamJob> job, std::vector<const char*>& own,
                          const char* const* reads, char* errbuf, size_t errlen) try {
    const bool raw = !s->fin;
    std::vector<std::pair<size_t, size_t>> batches;
    cut_batches(job->table, s->budget, s->sub_batches, (int)me.devs.size(), batches);
    job->batches_left = (int)batches.size();
    job->own.swap(own);   // (the pointers stay valid: the vector's buffer moves with it)
    job->reads = raw ? reads : job->own.data();
    job->to_pack = raw ? (int)batches.size() : 0;
    StreamJob* jp = job.get();
    std::unique_lock<std::mutex> lk(me.m);
    if (!me.failed) {
        s->jobs.push_back(std::move(job));
        ++s->n_jobs;
        for (const auto& b : batches) me.queue.push_back(StreamEntries::Queued{jp, b.first, b.second, me.next_b++});
        me.cv.notify_all();
        if (raw) me.cv.wait(lk, [&] { return jp->to_pack == 0 || me.failed; });
        if (!me.failed) return SD_OK;
    }
    std::string err;
    const int rc = me.settle(lk, err);
    lk.unlock();
    set_err(errbuf, errlen, err);
    s->jobs.clear();
    return rc;
} catch (const std::bad_alloc&) {
    set_err(errbuf, errlen, "out of host memory");
    return SD_ERR_INTERNAL;
}

extern "C" {

int sd_stream_submit(sd_stream* s, const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads,
                     char* errbuf, size_t errlen) {
    if (!s || n_reads < 0 || (n_reads && (!read_seqs || !read_lens))) return SD_ERR_PARAM;
    const double t0 = now_s();
    std::unique_ptr<StreamJob> job(new StreamJob);
    std::vector<const char*> own;
    const char* const* reads = nullptr;
    if (s->multi) {
        int rc;
        try {
            rc = stream_job(s, read_seqs, read_lens, n_reads, job.get(), own, reads, errbuf, errlen);
        } catch (const std::bad_alloc&) {
            set_err(errbuf, errlen, "out of host memory");
            rc = SD_ERR_INTERNAL;
        }
        if (rc == SD_OK) rc = entries_submit(s, *s->multi, std::move(job), own, reads, errbuf, errlen);
        s->submit_s += now_s() - t0;
        return rc;
    }
    const int jrc = stream_job(s, read_seqs, read_lens, n_reads, job.get(), own, reads, errbuf, errlen);
    if (jrc) return jrc;
    FinalMode* fm = s->fin.get();
    std::vector<std::pair<size_t, size_t>> batches;
    plan_batches(job->table, 0, job->table.size(), s->budget, s->sub_batches, batches);
    job->batches_left = (int)batches.size();
    StreamJob* jp = job.get();
    s->jobs.push_back(std::move(job));
    ++s->n_jobs;
    std::vector<const char*> cptr;
    std::vector<int32_t> clen;
    std::vector<int> slice_end;
    int rc = SD_OK;
    for (size_t b = 0; b < batches.size() && rc == SD_OK; ++b) {
        const size_t c0 = batches[b].first, c1 = batches[b].second;
        batch_chunks(reads, jp->table, c0, c1, cptr, clen);
        slice_end.clear();
        RecSink sink;
        if (fm) {
            // --second-best: the identities of a batch in slices of whole reads, each handed over as the device finishes it
            // (sd_engine::slice_end), so that the host selects slice s while the device computes slice s + 1
            if (fm->second_best && jp->per) ident_slices(jp->table, c0, c1, slice_end);
            sink = [s, fm, jp, c0, c1](const sd_rec* r, const int64_t* ro, size_t first, size_t n) {
                final_sink(*fm, s->pipe, *jp, c0 + first, c0 + first + n, r, ro);
                if (c0 + first + n == c1) --jp->batches_left;
            };
        } else {
            sink = [jp, c0, c1](const sd_rec* r, const int64_t* ro, size_t first, size_t n) {
                jp->add(c0 + first, c0 + first + n, r, ro);
                if (c0 + first + n == c1) --jp->batches_left;
            };
        }
        rc = s->pipe.push(cptr, clen, std::move(sink), slice_end);
    }
    if (rc) {
        set_err(errbuf, errlen, s->pipe.eb);
        (void)s->pipe.drain();   // sinks of older jobs still run; this job is dropped
        for (size_t j = 0; j < s->jobs.size(); ++j)
            if (s->jobs[j].get() == jp) { s->jobs.erase(s->jobs.begin() + (long)j); break; }
    }
    s->submit_s += now_s() - t0;
    return rc;
}

int sd_stream_collect(sd_stream* s, sd_rec** rows, int64_t** row_off, int64_t* n_rows, char* errbuf, size_t errlen) {
    if (!s || !rows || !row_off) return SD_ERR_PARAM;
    *rows = nullptr;
    *row_off = nullptr;
    if (n_rows) *n_rows = 0;
    if (s->fin) { set_err(errbuf, errlen, "a final-mode stream is collected with sd_stream_collect_final"); return SD_ERR_PARAM; }
    if (s->jobs.empty()) { set_err(errbuf, errlen, "sd_stream_collect without a submitted job"); return SD_ERR_PARAM; }
    const double t0 = now_s();
    int rc = stream_wait_oldest(s, errbuf, errlen);
    if (rc != SD_OK) {
        s->collect_s += now_s() - t0;
        return rc;
    }
    RowJob* job = s->jobs.front().get();
    if (rc == SD_OK && job->oom) { set_err(errbuf, errlen, "out of host memory"); rc = SD_ERR_INTERNAL; }
    if (rc == SD_OK) {
        if (!job->rows) job->rows = static_cast<sd_rec*>(std::malloc(sizeof(sd_rec)));
        *rows = job->rows;
        *row_off = job->row_off;
        if (n_rows) *n_rows = (int64_t)job->n_rows;
        job->rows = nullptr;      // ownership moves to the caller (sd_free)
        job->row_off = nullptr;
    }
    s->jobs.erase(s->jobs.begin());
    s->collect_s += now_s() - t0;
    return rc;
}

int sd_stream_collect_final(sd_stream* s, sd_final_row** rows, int64_t** row_off, int64_t* n_rows, double** alt,
                            char* errbuf, size_t errlen) {
    if (!s || !rows || !row_off) return SD_ERR_PARAM;
    *rows = nullptr;
    *row_off = nullptr;
    if (n_rows) *n_rows = 0;
    if (alt) *alt = nullptr;
    if (!s->fin) { set_err(errbuf, errlen, "sd_stream_collect_final on a stream made by sd_stream_create"); return SD_ERR_PARAM; }
    if (s->jobs.empty()) { set_err(errbuf, errlen, "sd_stream_collect_final without a submitted job"); return SD_ERR_PARAM; }
    const double t0 = now_s();
    int rc = stream_wait_oldest(s, errbuf, errlen);
    if (rc != SD_OK) {
        s->collect_s += now_s() - t0;
        return rc;
    }
    StreamJob& job = *s->jobs.front();
    rc = job.rc;
    if (rc) set_err(errbuf, errlen, job.err);
    const size_t n = job.fin.n;
    int64_t* off = nullptr;
    if (rc == SD_OK) {
        off = static_cast<int64_t*>(std::calloc((size_t)job.n_reads + 1, sizeof(int64_t)));
        if (!off || !job.fin.resize(std::max<size_t>(n, 1)) || !job.alt.resize(std::max<size_t>(job.alt.n, 1))) {
            set_err(errbuf, errlen, "out of host memory");
            rc = SD_ERR_INTERNAL;
        }
    }
    if (rc == SD_OK) {
        for (size_t i = 0; i < n; ++i) ++off[(size_t)job.fin.p[i].read + 1];   // rows come in read order
        for (int32_t r = 0; r < job.n_reads; ++r) off[r + 1] += off[r];
        *rows = job.fin.release();   // ownership moves to the caller (sd_free)
        *row_off = off;
        if (n_rows) *n_rows = (int64_t)n;
        if (alt && s->fin->second_best) *alt = job.alt.release();
        s->fin->kept += (int64_t)n;
    } else {
        std::free(off);
    }
    s->jobs.erase(s->jobs.begin());
    s->collect_s += now_s() - t0;
    return rc;
}

int sd_stream_keys(sd_stream* s, const char** keys, int32_t cap, int32_t* n_keys) {
    if (!s || !s->fin || (cap > 0 && !keys)) return SD_ERR_PARAM;
    const std::vector<std::string>& k = s->fin->pp.key_names();
    for (int32_t i = 0; i < cap && i < (int32_t)k.size(); ++i) keys[i] = k[(size_t)i].c_str();
    if (n_keys) *n_keys = (int32_t)k.size();
    return SD_OK;
}

int sd_stream_profile(sd_stream* s, int32_t reset, int32_t* n_monomers, int64_t* n_counts, int64_t* text_bytes,
                      char* text, uint64_t* counts) {
    if (!s || !s->fin || !s->fin->pp.profiling()) return SD_ERR_PARAM;
    sd::PostProcessor& pp = s->fin->pp;
    const std::vector<uint64_t> v = pp.profile(reset && counts);
    const std::string t = pp.profile_text();
    if (n_monomers) *n_monomers = (int32_t)(pp.interleaved_seqs().size() / 2);
    if (n_counts) *n_counts = (int64_t)v.size();
    if (text_bytes) *text_bytes = (int64_t)t.size() + 1;
    if (text) std::memcpy(text, t.c_str(), t.size() + 1);
    if (counts) std::memcpy(counts, v.data(), sizeof(uint64_t) * v.size());
    return SD_OK;
}

int sd_stream_final_stats(sd_stream* s, double out[4]) {
    if (!s || !out) return SD_ERR_PARAM;
    const FinalMode* fm = s->fin.get();
    if (StreamEntries* me = s->multi.get()) {   // summed over the entries
        std::lock_guard<std::mutex> g(me->m);
        double ms = 0, pairs = 0;
        for (const StreamEntries::Counters& c : me->cnt) { ms += c.ident_ms; pairs += (double)c.ident_pairs; }
        out[0] = fm ? ms : 0.0;
        out[1] = fm ? pairs : 0.0;
        out[2] = fm ? (double)me->fallback_blocks : 0.0;
        out[3] = fm ? (double)fm->kept : 0.0;
        return SD_OK;
    }
    out[0] = fm ? s->pipe.ident_ms : 0.0;
    out[1] = fm ? (double)s->pipe.ident_pairs : 0.0;
    out[2] = fm ? (double)fm->pp.fallback_blocks : 0.0;
    out[3] = fm ? (double)fm->kept : 0.0;
    return SD_OK;
}

int sd_stream_stats(sd_stream* s, double out[16]) {
    if (!s || !out) return SD_ERR_PARAM;
    if (StreamEntries* me = s->multi.get()) {   // summed over the entries
        StreamEntries::Counters t;
        {
            std::lock_guard<std::mutex> g(me->m);
            for (const StreamEntries::Counters& c : me->cnt) {
                t.fill_ms += c.fill_ms; t.trace_ms += c.trace_ms; t.compact_ms += c.compact_ms; t.run_ms += c.run_ms;
                t.launches += c.launches; t.batches += c.batches; t.rows += c.rows;
                t.pack_s += c.pack_s; t.wait_s += c.wait_s; t.sink_s += c.sink_s;
            }
        }
        const double v[16] = {t.fill_ms, t.trace_ms, t.compact_ms, t.run_ms, (double)t.launches, (double)t.batches,
                              (double)t.rows, t.pack_s * 1e3, t.wait_s * 1e3, t.sink_s * 1e3, s->submit_s * 1e3,
                              s->collect_s * 1e3, (double)s->n_jobs, (double)s->sub_batches, (double)s->budget, 0.0};
        std::memcpy(out, v, sizeof v);
        return SD_OK;
    }
    const Pipeline& q = s->pipe;
    const double v[16] = {q.fill_ms, q.trace_ms, q.compact_ms, q.run_ms, (double)q.launches, (double)q.batches,
                          (double)q.rows, q.pack_s * 1e3, q.wait_s * 1e3, q.sink_s * 1e3, s->submit_s * 1e3,
                          s->collect_s * 1e3, (double)s->n_jobs, (double)s->sub_batches, (double)s->budget, 0.0};
    std::memcpy(out, v, sizeof v);
    return SD_OK;
}

int sd_stream_info(sd_stream* s, int64_t info[8]) {
    if (!s) return SD_ERR_PARAM;
    if (StreamEntries* me = s->multi.get()) {   // entry 0's first engine
        std::lock_guard<std::mutex> g(me->m);
        std::memcpy(info, me->info0, sizeof me->info0);
        return SD_OK;
    }
    return sd_engine_info(s->pipe.eng[0], info);
}

int sd_stream_device_stats(sd_stream* s, int64_t* batches, double* busy_ms, int32_t cap) {
    if (!s) return 0;
    if (StreamEntries* me = s->multi.get()) {
        std::lock_guard<std::mutex> g(me->m);
        for (size_t i = 0; i < me->devs.size() && (int32_t)i < cap; ++i) {
            if (batches) batches[i] = me->dealt[i];
            if (busy_ms) busy_ms[i] = me->cnt[i].run_ms;
        }
        return (int)me->devs.size();
    }
    if (cap > 0 && batches) batches[0] = (int64_t)s->pipe.pushed;
    if (cap > 0 && busy_ms) busy_ms[0] = s->pipe.run_ms;
    return 1;
}

}  // extern "C"
