// sd_stream.hip -- sd_stream_*: the streaming form of the job (sequences -> rows, AlignReadsSet of main.cpp:67-122
// without the text), jobs pipelined through the device in sub-batches; in final mode (sd_stream_create_final) the rows
// of final_decomposition.tsv / _alt.tsv as typed rows instead of the raw ones; with a device list
// (sd_stream_create_devices, sd_stream_create_final_devices) one pipeline per entry, several of them each driven by a
// thread of its own.  The reads of a job lie in host memory (sd_stream_submit) or in device memory
// (sd_stream_submit_dev).  Where its rows end up is the stream's mode (StreamMode): in host memory (sd_stream_collect,
// _collect_final), or, on one device, in the caller's device buffers -- the raw rows assembled there
// (SD_FLAG_DEVICE_ROWS: _peek_dev, _collect_dev), the final rows selected there (SD_FLAG_DEVICE_FINAL: _peek_final_dev,
// _collect_final_dev) and with SD_FLAG_DEVICE_PROFILE their column profiles folded there (_profile_dev).  The six
// collect and peek entries share one frame (on_oldest_job).
#include <optional>

#include "sd_devices.hpp"
#include "sd_final_ws.hpp"

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
    // SD_FLAG_DEVICE_FINAL: the selection runs on the device (sd_final_dev.hip) from these copies of the tables, uploaded
    // when the first job's rows are assembled
    bool dtab_up = false;
    FinalDevTables dtab;
    // SD_FLAG_DEVICE_PROFILE: the stream's templates and counters on the device; the pairs of every selected job are
    // planned behind its selection (sd_final_prof_dev.hip)
    ProfDev* pd = nullptr;
};

// Something on loan from a list of spares (a stream's): it goes back to the list with the lease.
template <class T>
struct Lease {
    std::unique_ptr<T> p;
    std::vector<std::unique_ptr<T>>* home = nullptr;
    Lease() = default;
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    void take(std::unique_ptr<T> q, std::vector<std::unique_ptr<T>>& from) { p = std::move(q); home = &from; }
    ~Lease() { if (p) home->push_back(std::move(p)); }
    T* get() const { return p.get(); }
    T* operator->() const { return p.get(); }
    T& operator*() const { return *p; }
    explicit operator bool() const { return (bool)p; }
};

// A submitted job: its rows as they are assembled and, in final mode, its own copy of the reads and its kept rows.
struct StreamJob : RowJob {
    std::vector<std::string> seq;
    sd::HeapArray<sd_final_row> fin;   // handed to the caller by collect
    sd::HeapArray<double> alt;
    int rc = SD_OK;          // first failure of the job's post-processing
    std::string err;
    // where the entries pack the job's batches from (the caller's buffers in raw mode, seq through own in final mode),
    // and its batches no entry has packed yet
    const char* const* reads = nullptr;
    std::vector<const char*> own;
    int to_pack = 0;
    // A job whose reads lie in device memory (sd_stream_submit_dev): `own` holds DEVICE addresses, which the entries
    // hand to the device packer with `ds`; gpos = per chunk of the table, where it starts in the job (DevSrc::gpos).  In
    // final mode the packers read the job's own device copy of the reads (text, read r at text_off[r], made on the
    // caller's stream), from which the post-processor's fallback fetches the reads it asks for into seq; rlen = the
    // read lengths.  The copy goes back to the stream's spare list with the job.  (A device-profile job submitted from
    // host memory has text and text_off too: stream_prof_upload.)
    struct DevInput {
        bool dev = false;
        DevSrc ds;
        std::vector<int64_t> gpos, rlen, text_off;
        Lease<DevBuf<uint8_t>> text;
    } din;
    // A job of a device-rows stream (SD_FLAG_DEVICE_ROWS): ws = its record store and merge workspace (RowsWS), taken
    // from and given back to the stream's list.  Layout of the store: the compact records of the job's chunks in
    // chunk-table order, back to back across its batches, already in read coordinates and the caller's score scale;
    // appended = records in it, rec_at[c] = first record of chunk c (from the batches' host-side record offsets).
    // rows_batch appends a batch and, behind the last one, enqueues the merge.
    struct Store {
        Lease<RowsWS> ws;
        std::vector<int64_t> rec_at;
        int64_t appended = 0;
        bool ws_begun = false, assembled = false;
    } store;
    // A job of a device-final stream (SD_FLAG_DEVICE_FINAL) has a record store too, and fws: the identity words of the
    // store's records and the selection's workspace.  selected: the selection kernels were enqueued behind the merge.
    // A job that takes the text-based path (final_dev_slow) leaves its rows in fin / alt / fin_off on the host.
    struct DevFinal {
        Lease<FinalWS> fws;
        bool selected = false, slow_done = false;
        std::vector<int64_t> fin_off;
    } dfin;
    // The one rule of order among the three leases (which go home with the members above, last to first): a fold or an
    // upload that is still recorded on the text reads it, so the text waits in the final workspace, under the
    // workspace's event, before that workspace goes home.
    ~StreamJob() {
        if (din.text && dfin.fws && dfin.fws->prof_recorded) dfin.fws->held_text = std::move(din.text.p);
    }
};

// read r's text, from the job's device copy of the reads into job.seq[r]
static hipError_t fetch_read_text(StreamJob& job, size_t r) {
    const StreamJob::DevInput& in = job.din;
    job.seq[r].resize((size_t)in.rlen[r]);
    return hipMemcpy(&job.seq[r][0], in.text->p + in.text_off[r], (size_t)in.rlen[r], hipMemcpyDeviceToHost);
}

// Device rows: the records of the batch [c0, c1) of job j, still in engine e's buffers after fetch_begin (total of them,
// offsets in e->h_roff), are appended to the job's store on `st`; behind the job's last batch the merge is enqueued.
// A device-final job (fm given) also keeps the batch's identity words at the records' indices -- zeroes, which decide
// nothing, for a batch whose identity outputs are not valid -- and behind the merge enqueues the selection, a
// device-profile job behind that the plan of its pairs.  The steps, in the order rows_batch takes them:
struct RowsBatch {
    StreamJob& j;
    sd_engine* e;
    const int64_t total;
    hipStream_t st;
    const size_t c0, c1;
    FinalMode* fm;
    RowsWS& ws = *j.store.ws;
    FinalWS* fw = j.dfin.fws.get();
    const size_t per = fw ? (size_t)j.per : 0;   // identity words kept per record (0: a job without in-stream identities)
    const bool homo = fm && fm->second_best;
    const size_t C = c1 - c0, CJ = j.table.size();

    // The first batch of the job.  The workspace's last user: its scatter ran on ITS caller's stream and reads these
    // buffers; every alloc below may give a block up to the pool, so the HOST has to have seen that scatter end
    // (stream_take_ws hands out idle workspaces: this returns at once).  A job that was dropped never settled.
    void begin_store() {
        j.store.ws_begun = true;
        ws.wait_idle();
        bool settled = ws.settled;
        if (fw) { fw->wait_idle(); settled = settled && fw->settled; }
        if (!settled) { SD_HIP(hipStreamSynchronize(st)); ws.settled = true; if (fw) fw->settled = true; }
        ws.h_add.alloc(CJ);
        for (size_t c = 0; c < CJ; ++c) ws.h_add.p[c] = (int32_t)j.table[c].off;   // (main.cpp:109-111)
        ws.add.alloc(CJ);
        ws.settled = false;
        SD_HIP(hipMemcpyAsync(ws.add.p, ws.h_add.p, CJ * sizeof(int32_t), hipMemcpyHostToDevice, st));
        j.store.rec_at.assign(1, 0);
        j.store.rec_at.reserve(CJ + 1);
    }

    // Room for the batch, records and words together.
    void reserve() {
        const size_t need = (size_t)(j.store.appended + total);
        if (j.store.appended == 0) size_first(need);
        else if (need > ws.recs.cap) regrow(need);
    }
    // the first batch sizes the store for the whole job by its share of the chunks, with a quarter to spare (short
    // chunks first: the store grows below); the words' room follows the store's (a store kept from an earlier job may
    // be larger)
    void size_first(size_t need) {
        if (need > ws.recs.cap) {
            const double share = C < CJ ? 1.25 * (double)CJ / (double)std::max<size_t>(C, 1) : 1.0;
            ws.recs.alloc((size_t)((double)need * share) + (C < CJ ? 64 : 0));
        }
        if (!per) return;
        fw->words.alloc(ws.recs.cap * per);
        if (homo) fw->hwords.alloc(ws.recs.cap * per);
    }
    // a later batch outgrew it: larger blocks, what was appended so far copied over; the old blocks leave with nothing
    // in flight on them.  (An allocation that fails leaves the store half swapped: the job fails with it, and the next
    // job sizes the store anew.)
    template <class T>
    void grow(DevBuf<T>& buf, DevBuf<T>& old, size_t count, size_t keep) {
        old.swap(buf);
        buf.alloc(count);
        SD_HIP(hipMemcpyAsync(buf.p, old.p, keep * sizeof(T), hipMemcpyDeviceToDevice, st));
    }
    void regrow(size_t need) {
        DevBuf<sd::DevRec> old;
        DevBuf<uint32_t> old_w, old_h;
        const size_t have = (size_t)j.store.appended;
        grow(ws.recs, old, std::max<size_t>(need, 2 * ws.recs.cap), have);
        if (per) {
            grow(fw->words, old_w, ws.recs.cap * per, have * per);
            if (homo) grow(fw->hwords, old_h, ws.recs.cap * per, have * per);
        }
        SD_HIP(hipStreamSynchronize(st));
    }

    // The batch's identity words behind those of the records so far (a device-final job with in-stream identities; the
    // run is through -- fetch_begin waited for it -- so they are complete in the engine's outputs).
    void append_words() {
        fw->settled = false;
        const size_t nb = (size_t)total * per * sizeof(uint32_t), at = (size_t)j.store.appended * per;
        const bool valid = e->ident_valid && (size_t)e->ident_words() == per && (!homo || e->ident_mode == 2);
        auto put = [&](uint32_t* w, const uint32_t* from) {
            if (valid) SD_HIP(hipMemcpyAsync(w, from, nb, hipMemcpyDeviceToDevice, st));
            else SD_HIP(hipMemsetAsync(w, 0, nb, st));
        };
        put(fw->words.p + at, e->d_ident.p);
        if (homo) put(fw->hwords.p + at, e->d_identh.p);
    }

    void append_records() {
        rows_append(ws, st, e->d_dense.p, e->d_roff.p, (int)C, ws.add.p + c0, j.store.appended, e->score_scale);
        for (size_t c = 0; c < C; ++c) j.store.rec_at.push_back(j.store.appended + e->h_roff.p[c + 1]);
        j.store.appended += total;
    }

    // Behind the last batch: the merge,
    void merge() {
        std::vector<int64_t> read_off((size_t)j.n_reads + 1, 0);
        size_t c = 0;
        for (int32_t r = 0; r < j.n_reads; ++r) {
            c += (size_t)j.nch[(size_t)r];
            read_off[(size_t)r + 1] = j.store.rec_at[c];
        }
        rows_assemble(ws, st, ws.recs.p, read_off.data(), j.n_reads, ROWS_PIECE);
        j.store.assembled = true;
    }
    // the selection (a device-final job with in-stream identities),
    void select() {
        if (!fm->dtab_up) { fm->dtab.upload(fm->pp.final_tables()); fm->dtab_up = true; }
        const size_t nr = (size_t)j.n_reads;
        fw->h_rlen.alloc(nr);
        for (size_t r = 0; r < nr; ++r) fw->h_rlen.p[r] = j.din.dev ? j.din.rlen[r] : (int64_t)j.seq[r].size();
        fw->rlen.alloc(nr);
        fw->settled = false;
        SD_HIP(hipMemcpyAsync(fw->rlen.p, fw->h_rlen.p, nr * sizeof(int64_t), hipMemcpyHostToDevice, st));
        final_sources(*fw, ws, st);
        final_select(*fw, st, fm->dtab.tb, ws.recs.p, fw->src.p, fw->src.p, fw->words.p, fw->hwords.p, fw->moff.p,
                     fw->rlen.p, j.n_reads, ws.n_recs, ws.bbase.p + ws.n_tiles);
    }
    // and (a device-profile stream) the pairs of the kept rows, planned and grouped behind the selection; their summary
    // travels with the selection's counts, ahead of ev_sel (recorded anew behind it).
    void plan_profile() {
        const size_t nr = (size_t)j.n_reads;
        ProfWS& pw = fw->prof;
        pw.h_text_off.alloc(nr + 1);
        for (size_t r = 0; r < nr; ++r) pw.h_text_off.p[r] = j.din.text_off[r];
        pw.h_text_off.p[nr] = 0;
        pw.text_off.alloc(nr + 1);
        SD_HIP(hipMemcpyAsync(pw.text_off.p, pw.h_text_off.p, (nr + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        prof_plan(pw, *fm->pd, st, ws.recs.p, fw->src.p, fw->keep.p, fw->moff.p, fw->rlen.p, j.n_reads, ws.n_recs,
                  ws.bbase.p + ws.n_tiles);
        SD_HIP(hipEventRecord(fw->ev_sel, st));
    }
};

static int rows_batch(StreamJob& j, sd_engine* e, int64_t total, hipStream_t st, size_t c0, size_t c1, char* eb, size_t eblen,
                      FinalMode* fm = nullptr) {
    RowsBatch b{j, e, total, st, c0, c1, fm};
    try {
        if (!j.store.ws_begun) b.begin_store();
        b.reserve();
        if (b.per && total > 0) b.append_words();
        b.append_records();
        if (c1 == b.CJ) {
            b.merge();
            if (b.per) {
                b.select();
                if (fm->pd) b.plan_profile();
                j.dfin.selected = true;
            }
        }
    } catch (const HipFail& f) {
        std::snprintf(eb, eblen, "%s", f.msg.c_str());
        return SD_ERR_HIP;
    }
    return SD_OK;
}

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
        for (size_t r = r0; r < r1; ++r)
            pr.push_back(sd::PostRead{"", 0, j.din.dev ? nullptr : j.seq[r].data(), j.din.dev ? j.din.rlen[r] : (int64_t)j.seq[r].size()});
        // reads in device memory: the text of these reads comes to the host only if the post-processor asks for it
        // (its fallback identities, the profiles); the rows have come back, so the job's copy is complete
        if (j.din.dev)
            fm.pp.fetch_text = [&j, &pr, r0, r1](std::string& e) -> int {
                for (size_t r = r0; r < r1; ++r) {
                    if (fetch_read_text(j, r) != hipSuccess) {
                        (void)hipGetLastError();
                        e = "cannot fetch the text of read " + std::to_string(r) + " from the device";
                        return SD_ERR_HIP;
                    }
                    pr[r - r0].seq = j.seq[r].data();
                }
                return SD_OK;
            };
        // a batch without identities (more records than the outputs had room for) sends these rows to the fallback
        const sd::IdentRef iref{j.bid, fm.second_best ? j.bidh : nullptr, j.rsrc, j.xid.data(), j.xidh.data()};
        try {
            j.rc = fm.pp.process_rows(pr.data(), r1 - r0, (int32_t)r0, j.rows, j.row_off + r0, j.fin, j.alt, j.err,
                                      j.per && j.ident_ok ? &iref : nullptr);
        } catch (const std::bad_alloc&) {
            j.rc = SD_ERR_INTERNAL;
            j.err = "out of host memory";
        }
        if (j.din.dev) {
            fm.pp.fetch_text = nullptr;
            for (size_t r = r0; r < r1; ++r) std::string().swap(j.seq[r]);
        }
    }
    j.xid.clear();
    j.xidh.clear();
    j.ident_ok = j.carry.empty() || j.bid != nullptr;
}

// The pipelines of a stream, one per entry of its device list ({p->device} without one).  submit appends a job's batches
// to one queue; their numbers run on across jobs, and an entry always takes the one at the front -- the lowest batch no
// entry has.  The sinks take their turns in batch order (BatchTurns), so the rows are assembled as by one pipeline.  An
// entry with nothing to take pops its oldest batch (without that, a batch whose turn has come could sit in an idle
// pipeline while the others wait for it).  (drive_entry does not fit here: it drains its pipeline when a job's batches
// run out, and a stream keeps batches in flight across job boundaries.)
// Only who drives the pipelines depends on the entry count, and both drivers run `step`: one entry is driven on the
// calling thread, inside submit and collect (wait), with no thread of its own and no hipSetDevice; several are driven
// each by a thread of its own (drive), bound to the entry's device for the life of the stream, which makes every HIP
// call of its pipeline.  The first failure of any entry aborts the turns and drops the queued batches; every entry
// drains what it has in flight, and the caller's submit or collect that meets the failure reports it (wait), drops
// every job and starts the numbering anew.
struct StreamEntries {
    enum Act { PUSH, POP, DRAIN, EXIT };
    struct Queued { StreamJob* job; size_t c0, c1, b; };
    // An entry: its pipeline and the scratch of its pushes, used by its driver; then, under the lock, what the others
    // read of it, copied after every push and pop (stats read them while it runs).
    struct Entry {
        std::unique_ptr<Pipeline> pipe;
        bool bound = true;           // the driver thread is on the entry's device
        std::vector<const char*> cptr;
        std::vector<int32_t> clen;
        std::vector<int> slice_end;
        std::vector<int64_t> gpos;
        uint64_t seen = 0;           // it has drained for failure `gen` when seen == gen
        int inflight = 0;
        int64_t dealt = 0;
        PipeCounters cnt;
    };
    std::vector<int32_t> devs;
    std::vector<Entry> ent;
    FinalMode* fm = nullptr;
    std::mutex m;
    std::condition_variable cv;
    std::deque<Queued> queue;
    size_t next_b = 0;            // number of the next batch submitted
    BatchTurns turns;
    bool stop = false, failed = false;
    uint64_t gen = 0;             // failures so far
    int drained = 0;              // entries that have drained for the current failure
    int fail_rc = SD_OK;
    std::string fail_msg;
    int64_t fallback_blocks = 0;  // fm->pp.fallback_blocks as the last sink left it
    int64_t info0[8] = {0};       // sd_engine_info of entry 0's first engine, as of its last push or pop
    std::vector<std::thread> th;  // the drivers of several entries

    ~StreamEntries() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        turns.abort();   // (sinks of batches still in flight return at once)
        cv.notify_all();
        for (std::thread& t : th) t.join();
    }

    // The pipelines, each created on its entry's driver thread (on_entries), and the rows per batch of the stream.  In
    // final mode every engine of every pipeline (the first now, the others as the pipeline creates them) computes the
    // identities of its batches in-stream; a template set the kernels do not take, or SD_FLAG_NO_STREAM_IDENT, leaves
    // them all to the fallback.
    int open(const sd_params* p, const std::vector<const char*>& ms, const int32_t* mono_lens, int32_t n_mono,
             int64_t& budget, std::string& err) {
        const size_t nd = devs.size();
        ent.resize(nd);
        std::vector<int64_t> entry_budget(nd, 0);
        std::vector<std::string> msg(nd);
        auto open_pipe = [&](int i) -> int {
            sd_params pi = *p;
            pi.device = devs[(size_t)i];
            ent[(size_t)i].pipe.reset(new Pipeline);
            Pipeline* q = ent[(size_t)i].pipe.get();
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
            (void)on_entries(devs, msg, e2, [&](int i) { ent[(size_t)i].pipe.reset(); return SD_OK; }, [] {});
            return rc;
        }
        budget = shared_row_budget(entry_budget, devs, p);
        (void)sd_engine_info(ent[0].pipe->eng[0], info0);
        if (nd > 1)
            for (size_t i = 0; i < nd; ++i) th.emplace_back([this, i] { drive(i); });
        return SD_OK;
    }

    // The first failure of the stream (under the lock): the turns are aborted, the queued batches dropped.
    void fail_locked(size_t i, int rc, const std::string& msg) {
        if (failed) return;
        failed = true;
        ++gen;
        drained = 0;
        fail_rc = rc;
        fail_msg = devs.size() > 1 ? "device " + std::to_string(devs[i]) + ": " + msg : msg;
        queue.clear();
        turns.abort();
    }

    // What an entry does next (under the lock): exit, drain for a failure, push the front of the queue, or pop.
    Act next_locked(Queued& q) {
        if (stop) return EXIT;
        if (failed) return DRAIN;
        if (queue.empty()) return POP;
        q = queue.front();
        queue.pop_front();
        return PUSH;
    }

    // Batch q on entry i's pipeline: its sink assembles the records in q's turn (final mode: with the identities of this
    // pipeline's engine) and counts the batch off its job when the last slice is through.
    int push(size_t i, const Queued& q) {
        Entry& e = ent[i];
        Pipeline& pq = *e.pipe;
        StreamJob* jp = q.job;
        batch_chunks(jp->reads, jp->table, q.c0, q.c1, e.cptr, e.clen);
        e.slice_end.clear();
        // --second-best: the identities of a batch in slices of whole reads, each handed over as the device finishes it
        // (sd_engine::slice_end), so that the host selects slice s while the device computes slice s + 1
        // (a device-final job's words stay on the device: nothing to hand over in slices)
        if (fm && fm->second_best && jp->per && !jp->store.ws) ident_slices(jp->table, q.c0, q.c1, e.slice_end);
        DevSrc ds;
        if (jp->din.dev) {
            ds = jp->din.ds;
            ds.gpos = jp->din.gpos.data() + q.c0;
        }
        const int32_t dev = devs[i];
        const size_t c0 = q.c0, c1 = q.c1, b = q.b;
        // device rows: the records stay in HBM (rows_batch, called when the batch is popped: one entry, so in batch
        // order); the sink below then only takes its turn and counts the batch off its job
        DevSink dsink;
        FinalMode* const fmq = fm;
        if (jp->store.ws) dsink = [&pq, jp, c0, c1, fmq](sd_engine* en, int64_t total, hipStream_t st) { return rows_batch(*jp, en, total, st, c0, c1, pq.eb, sizeof pq.eb, fmq); };
        return pq.push(e.cptr, e.clen, [this, &pq, jp, dev, b, c0, c1](const sd_rec* r, const int64_t* ro, size_t first, size_t n) {
            const bool mine = turns.wait(b);   // (false: the stream failed; the batch is dropped)
            if (mine) {
                if (jp->store.ws) {
                    // (the records stayed on the device: rows_batch has them)
                } else if (fm) {
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
        }, e.slice_end, jp->din.dev ? &ds : nullptr, std::move(dsink));
    }

    // One action of entry i, on the thread that drives it: push q, pop, or drain (after a failure, and at exit); then the
    // entry's figures are copied under the lock, and a failure fails the stream.
    void step(size_t i, Act act, const Queued& q) {
        Entry& e = ent[i];
        Pipeline& pq = *e.pipe;
        int r = SD_OK;
        std::string msg;
        try {
            if (act == PUSH && !e.bound) { r = SD_ERR_HIP; msg = "hipSetDevice failed"; }
            else if (act == PUSH) r = push(i, q);
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
            e.inflight = pq.inflight();
            e.cnt = pq.cnt;
            if (i == 0) (void)sd_engine_info(pq.eng[0], info0);
            if (act == PUSH) {
                if (r == SD_OK) ++e.dealt;
                --q.job->to_pack;
            }
            if (r) fail_locked(i, r, msg);
            if (act == DRAIN) { e.seen = gen; ++drained; }
        }
        cv.notify_all();
    }

    // The driver thread of entry i (several entries): push what the queue holds, pop when it holds nothing, drain after
    // a failure and at the end.
    void drive(size_t i) {
        Entry& e = ent[i];
        e.bound = hipSetDevice(devs[i]) == hipSuccess;
        if (!e.bound) (void)hipGetLastError();
        for (Act act = POP; act != EXIT;) {
            Queued q{};
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || (failed ? e.seen != gen : (!queue.empty() || e.inflight > 0)); });
                act = next_locked(q);
            }
            step(i, act, q);
        }
        e.pipe.reset();   // its streams, events and engines, on its device's thread
    }

    // Caller side: returns once done() holds (read under the lock) or the stream has failed.  One entry: the caller
    // drives it meanwhile, as its thread would -- and with nothing queued and nothing in flight, done() waits for a batch
    // that is nowhere: that fails the stream.  After a failure, waits until every entry has drained, then returns the
    // failure in err and clears it (the next batch submitted has the next turn); the caller drops every job.
    template <class Done>
    int wait(Done&& done, std::string& err) {
        while (th.empty()) {
            Queued q{};
            Act act = POP;
            {
                std::lock_guard<std::mutex> g(m);
                if (failed ? ent[0].seen == gen : done()) break;
                act = next_locked(q);
                if (act == POP && ent[0].inflight == 0) {
                    fail_locked(0, SD_ERR_INTERNAL, "stream lost a batch");
                    act = DRAIN;
                }
            }
            step(0, act, q);
        }
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return failed || done(); });
        if (!failed) return SD_OK;
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

    PipeCounters counters() {   // summed over the entries
        std::lock_guard<std::mutex> g(m);
        PipeCounters t;
        for (const Entry& e : ent) t += e.cnt;
        return t;
    }
};
}  // namespace sdi

// Which rows a stream makes and where it leaves them, and so which collect and peek calls belong to it (wrong_call).
enum class StreamMode {
    RawHost,       // sd_stream_create: raw rows in host memory
    RawDevice,     // with SD_FLAG_DEVICE_ROWS: the jobs' rows are assembled and collected on the device
    FinalHost,     // sd_stream_create_final: final rows in host memory
    FinalDevice,   // with SD_FLAG_DEVICE_FINAL: the final rows are selected and collected on the device (dev_prof: and folded)
};

struct sd_stream {
    sd_params p{};
    std::vector<std::string> mono;       // owned copies
    StreamMode mode = StreamMode::RawHost;
    bool device_store() const { return mode == StreamMode::RawDevice || mode == StreamMode::FinalDevice; }   // the jobs have a record store
    std::unique_ptr<FinalMode> fin;      // the final modes only
    int sub_batches = 1;
    std::vector<std::unique_ptr<DevBuf<uint8_t>>> spare;   // device copies of reads (StreamJob::din.text) between jobs
    std::vector<std::unique_ptr<RowsWS>> ws_spare;         // record stores (StreamJob::store.ws) between jobs
    std::vector<std::unique_ptr<FinalWS>> fws_spare;       // selection workspaces (StreamJob::dfin.fws) between jobs
    hipEvent_t ev_src = nullptr;         // sd_stream_submit_dev: the caller's stream has produced the job's reads
    int ev_src_dev = -1;
    std::vector<std::unique_ptr<StreamJob>> jobs;   // FIFO: submitted, not collected yet
    hipStream_t slow_st = nullptr;       // device-final streams: the text-based path's copies to the host (final_dev_slow)
    // SD_FLAG_DEVICE_PROFILE: the profiles of the selected jobs are folded on the device, on prof_st, into pd.counts;
    // what the host folds (pairs the kernel does not take, jobs of the text-based path) is in the post-processor
    bool dev_prof = false;
    ProfDev pd;
    hipStream_t prof_st = nullptr;
    double prof_ms = 0;                  // fold kernels, HIP events
    int64_t prof_pairs_dev = 0, prof_pairs_host = 0, prof_text_to_host = 0;
    PinBuf<unsigned long long> h_up;     // sd_stream_profile_dev: the host's counters on their way to the device
    DevBuf<unsigned long long> d_up;
    hipEvent_t ev_up = nullptr, ev_pd = nullptr;
    bool up_recorded = false;
    int64_t budget = 0;
    double submit_s = 0, collect_s = 0;
    int64_t n_jobs = 0;
    StreamEntries me;                    // destroyed first: its sinks hold pointers to the jobs
    ~sd_stream() {
        if (prof_st) {   // the folds of collected jobs read pd and the jobs' workspaces
            (void)hipStreamSynchronize(prof_st);
            (void)hipStreamDestroy(prof_st);
        }
        if (up_recorded) (void)hipEventSynchronize(ev_up);
        if (ev_up) (void)hipEventDestroy(ev_up);
        if (ev_pd) (void)hipEventDestroy(ev_pd);
        if (ev_src) (void)hipEventDestroy(ev_src);
        if (slow_st) (void)hipStreamDestroy(slow_st);
    }
};

// The refusals of a combination of modes and flags: the first test that holds gives the text, null: none does.
// (several: a device list of more than one entry.)  Most stand before the device list is checked (mode_refusal), three
// behind that check and the one for monomers (mode_refusal_behind_list).
struct ModeFlags {
    bool dev_rows, dev_final, dev_prof, profile;
    explicit ModeFlags(int32_t f) : dev_rows(f & SD_FLAG_DEVICE_ROWS), dev_final(f & SD_FLAG_DEVICE_FINAL),
                                    dev_prof(f & SD_FLAG_DEVICE_PROFILE), profile(f & SD_FLAG_PROFILE) {}
};

// SD_FLAG_DEVICE_ROWS on a final-mode stream; with SD_FLAG_DEVICE_FINAL it is refused before the device list, without behind it
static const char* device_rows_on_final(bool dev_final) {
    return dev_final ? "SD_FLAG_DEVICE_ROWS needs a raw-mode stream: the rows of a final-mode stream are selected on the host (or, with SD_FLAG_DEVICE_FINAL alone, on the device)"
                     : "SD_FLAG_DEVICE_ROWS needs a raw-mode stream: the rows of a final-mode stream are selected on the host";
}

static const char* mode_refusal(bool final, ModeFlags f, bool several) {
    if (f.dev_prof && !final)
        return "SD_FLAG_DEVICE_PROFILE needs a final-mode stream made with SD_FLAG_DEVICE_FINAL (sd_stream_create_final): a raw-mode stream selects no rows to profile";
    if (f.dev_prof && !f.dev_final)
        return "SD_FLAG_DEVICE_PROFILE needs SD_FLAG_DEVICE_FINAL: it folds the rows the device selects; the rows of a host final stream are profiled with SD_FLAG_PROFILE";
    if (f.dev_prof && several)
        return "SD_FLAG_DEVICE_PROFILE needs SD_FLAG_DEVICE_FINAL and so a device list of one entry: the batches of a job would lie on several devices";
    if (f.dev_prof && f.profile)
        return "SD_FLAG_DEVICE_PROFILE and SD_FLAG_PROFILE do not go together: a SD_FLAG_DEVICE_FINAL stream folds its profiles on the device, the host pass of SD_FLAG_PROFILE has no rows there";
    if (f.dev_final && final && f.dev_rows) return device_rows_on_final(true);
    if (f.dev_final && !final)
        return "SD_FLAG_DEVICE_FINAL needs a final-mode stream (sd_stream_create_final): a raw-mode stream keeps its rows on the device with SD_FLAG_DEVICE_ROWS";
    if (f.dev_final && several)
        return "SD_FLAG_DEVICE_FINAL needs a device list of one entry: the batches of a job would lie on several devices";
    if (f.dev_final && f.profile)
        return "SD_FLAG_DEVICE_FINAL and SD_FLAG_PROFILE do not go together: the profile pass reads the kept rows and the read text on the host";
    return nullptr;
}

static const char* mode_refusal_behind_list(bool final, ModeFlags f, bool several) {
    if (!final && f.profile) return "SD_FLAG_PROFILE needs a final-mode stream";
    if (f.dev_rows && final) return device_rows_on_final(false);   // (mode_refusal has taken those with SD_FLAG_DEVICE_FINAL)
    if (f.dev_rows && several)
        return "SD_FLAG_DEVICE_ROWS needs a device list of one entry: the batches of a job would lie on several devices";
    return nullptr;
}

// The four creates.  who: the name of a call with a device list, which is checked as by sd_run_files_devices; without
// one (who == nullptr) the stream has the one entry p->device.  final: the final mode, with mono_names .. lr_coef.
static int stream_create(sd_stream** out, const sd_params* p, const char* who, const int32_t* devices, int32_t n_devices,
                         bool final, const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens,
                         int32_t n_mono, int32_t sub_batches, int32_t min_identity, int32_t second_best,
                         const double* lr_coef, char* errbuf, size_t errlen) try {
    if (!out) return SD_ERR_PARAM;
    *out = nullptr;
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    sd_params q = *p;
    const ModeFlags flags(p->reserved[1]);
    const bool several = who && n_devices > 1;
    if (const char* no = mode_refusal(final, flags, several)) { set_err(errbuf, errlen, no); return SD_ERR_PARAM; }
    if (who) {
        rc = check_device_list(who, devices, n_devices, errbuf, errlen);
        if (rc) return rc;
        q.device = devices[0];   // (also the device of the fallback identities)
    }
    if (n_mono <= 0 || !mono_seqs || !mono_lens) { set_err(errbuf, errlen, "no monomers"); return SD_ERR_PARAM; }
    if (const char* no = mode_refusal_behind_list(final, flags, several)) { set_err(errbuf, errlen, no); return SD_ERR_PARAM; }
    const bool dev_prof = flags.dev_prof;
    q.reserved[1] &= ~(SD_FLAG_DEVICE_ROWS | SD_FLAG_DEVICE_FINAL | SD_FLAG_DEVICE_PROFILE);   // (the flags shape the stream, not its engines)
    if (final && !mono_names) { set_err(errbuf, errlen, "no monomer names"); return SD_ERR_PARAM; }
    if (final && !lr_coef) { set_err(errbuf, errlen, "no logistic-regression coefficients"); return SD_ERR_PARAM; }
    for (int32_t m = 0; m < n_mono; ++m) {
        if (final && !mono_names[m]) { set_err(errbuf, errlen, "monomer " + std::to_string(m) + " has no name"); return SD_ERR_PARAM; }
        if ((final && !mono_seqs[m]) || mono_lens[m] <= 0) { set_err(errbuf, errlen, "ERROR: empty monomer sequence"); return SD_ERR_EMPTY; }
    }
    std::unique_ptr<sd_stream> s(new sd_stream);
    for (int32_t m = 0; m < n_mono; ++m) s->mono.emplace_back(mono_seqs[m], (size_t)mono_lens[m]);
    if (final) {
        std::vector<sd::Seq> monos;
        for (int32_t m = 0; m < n_mono; ++m) monos.push_back(sd::Seq{mono_names[m], s->mono[(size_t)m]});
        s->fin.reset(new FinalMode);
        FinalMode& fm = *s->fin;
        fm.second_best = second_best != 0;
        rc = fm.pp.init(monos, min_identity, fm.second_best, lr_coef, q.device, q.threads, err);
        if (rc == SD_OK && (q.reserved[1] & SD_FLAG_PROFILE)) rc = fm.pp.enable_profile(err);
        if (rc == SD_OK && dev_prof) {   // (the host counters: pairs the kernel does not take, jobs of the text-based path)
            rc = fm.pp.enable_profile(err);
            if (rc) err = "SD_FLAG_DEVICE_PROFILE (with SD_FLAG_DEVICE_FINAL): " + err;
        }
        if (rc) { set_err(errbuf, errlen, err); return rc; }
        q.reserved[1] &= ~SD_FLAG_PROFILE;   // (the flag shapes the post-processing only)
    }
    s->p = q;
    s->mode = final ? (flags.dev_final ? StreamMode::FinalDevice : StreamMode::FinalHost)
                    : (flags.dev_rows ? StreamMode::RawDevice : StreamMode::RawHost);
    s->sub_batches = std::max(1, (int)sub_batches);
    std::vector<const char*> ms;
    for (const std::string& m : s->mono) ms.push_back(m.data());
    s->me.devs = who ? std::vector<int32_t>(devices, devices + n_devices) : std::vector<int32_t>{q.device};
    s->me.fm = s->fin.get();
    rc = s->me.open(&q, ms, mono_lens, n_mono, s->budget, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (dev_prof) {
        try {
            DeviceScope on(s->me.devs[0]);
            SD_HIP(hipStreamCreateWithFlags(&s->prof_st, hipStreamNonBlocking));
            s->pd.setup(s->fin->pp.interleaved_seqs(), s->fin->pp.own_interleaved(), s->prof_st);
        } catch (const HipFail& f) {
            set_err(errbuf, errlen, f.msg);
            return SD_ERR_HIP;   // (s is destroyed with the guard's device restored)
        }
        s->dev_prof = true;
        s->fin->pd = &s->pd;
    }
    *out = s.release();
    return SD_OK;
} catch (const std::bad_alloc&) {
    set_err(errbuf, errlen, "out of host memory");
    return SD_ERR_INTERNAL;
}

// Waits for every batch of the oldest job.  On failure every job is dropped.
static int stream_wait_oldest(sd_stream* s, char* errbuf, size_t errlen) {
    StreamJob* job = s->jobs.front().get();
    std::string err;
    const int rc = s->me.wait([job] { return job->batches_left == 0; }, err);
    if (rc) {
        set_err(errbuf, errlen, err);
        s->jobs.clear();
    }
    return rc;
}

// sd_stream_submit: the job's chunk table, the rows' offsets and, in final mode, the copy of the reads; then its batches
// (cut_batches: with several entries at least two per entry) join the queue and the job the FIFO.  One entry: submit
// pushes them all.  Several: a raw-mode submit returns once every batch of the job has been packed by its entry, so that
// the caller's read buffers are free (the entries pack from them); a final-mode job packs from its own copy and submit
// returns at once.  A failure of the stream that this call meets is reported here and drops every job, this one too.
// Reads in device memory (sd_stream_submit_dev): read r = base[off[r] .. off[r] + read_lens[r]) on device `device`,
// produced on the stream `user`.
struct DevIn { const char* base; const int64_t* off; hipStream_t user; int device; };

// A buffer of `bytes` for the job's device copy of its reads, from the stream's spare list where that has one.
static void take_text(sd_stream* s, StreamJob& job, size_t bytes) {
    std::unique_ptr<DevBuf<uint8_t>> t;
    if (!s->spare.empty()) { t = std::move(s->spare.back()); s->spare.pop_back(); }
    else t.reset(new DevBuf<uint8_t>);
    job.din.text.take(std::move(t), s->spare);
    job.din.text->alloc(bytes);
}

// The device half of a submit: the job's device addresses and chunk positions; in final mode its own device copy of the
// reads, made on the caller's stream (so it follows what produced them and precedes what overwrites them); the event
// on that stream the packers wait for.  Runs with the data's device current.
static int stream_dev_job(sd_stream* s, StreamJob& job, const DevIn& dv, const int64_t* read_lens, std::string& err) {
    const size_t n = (size_t)job.n_reads;
    StreamJob::DevInput& in = job.din;
    in.dev = true;
    auto cum = std::make_shared<std::vector<int64_t>>(n + 1, 0);
    for (size_t r = 0; r < n; ++r) (*cum)[r + 1] = (*cum)[r] + read_lens[r];
    in.gpos.reserve(job.table.size());
    for (const CRef& c : job.table) in.gpos.push_back((*cum)[(size_t)c.read] + c.off);
    in.ds.user = dv.user;
    in.ds.cum = cum;
    job.own.resize(n);
    try {
        if (s->fin && n > 0) {
            // one copy of the span the reads lie in where that is not much more than the reads, else read by read
            int64_t lo = INT64_MAX, hi = 0;
            for (size_t r = 0; r < n; ++r) { lo = std::min(lo, dv.off[r]); hi = std::max(hi, dv.off[r] + read_lens[r]); }
            const bool span = hi - lo <= 2 * (*cum)[n] + ((int64_t)1 << 20);
            take_text(s, job, (size_t)(span ? hi - lo : (*cum)[n]) + (s->dev_prof ? 8 : 0));   // (the fold reads whole dwords)
            in.rlen.assign(read_lens, read_lens + n);
            in.text_off.resize(n);
            for (size_t r = 0; r < n; ++r) in.text_off[r] = span ? dv.off[r] - lo : (*cum)[r];
            if (span) SD_HIP(hipMemcpyAsync(in.text->p, dv.base + lo, (size_t)(hi - lo), hipMemcpyDeviceToDevice, dv.user));
            else
                for (size_t r = 0; r < n; ++r)
                    SD_HIP(hipMemcpyAsync(in.text->p + in.text_off[r], dv.base + dv.off[r], (size_t)read_lens[r], hipMemcpyDeviceToDevice, dv.user));
            for (size_t r = 0; r < n; ++r) job.own[r] = reinterpret_cast<const char*>(in.text->p) + in.text_off[r];
            in.ds.release = false;   // (the packers read the job's copy: the caller's stream need not wait for them)
        } else {
            for (size_t r = 0; r < n; ++r) job.own[r] = dv.base + dv.off[r];
        }
        if (s->ev_src && s->ev_src_dev != dv.device) { (void)hipEventDestroy(s->ev_src); s->ev_src = nullptr; }
        ensure_event(s->ev_src, hipEventDisableTiming);
        s->ev_src_dev = dv.device;
        // (every batch of the job is packed -- its wait for this event enqueued -- before the submit returns, so the
        // next submit may record the event anew)
        SD_HIP(hipEventRecord(s->ev_src, dv.user));
        in.ds.ready = s->ev_src;
    } catch (const HipFail& f) {
        err = f.msg;
        return SD_ERR_HIP;
    }
    job.reads = job.own.data();
    return SD_OK;
}

// The fold time of a workspace's last job, once its fold has completed.
static void prof_harvest(sd_stream* s, FinalWS& fw) {
    if (!fw.fold_timed) return;
    if (hipEventQuery(fw.ev_prof) != hipSuccess) { (void)hipGetLastError(); return; }
    float ms = 0;
    if (hipEventElapsedTime(&ms, fw.ev_f0, fw.ev_prof) == hipSuccess) s->prof_ms += ms;
    else (void)hipGetLastError();
    fw.fold_timed = false;
}

// SD_FLAG_DEVICE_PROFILE, a job submitted from host memory: its reads go up once, back to back, into a buffer of the
// kind a DeviceReads job has (StreamJob::din.text), through the workspace's pinned staging, on the stream's own stream.
static void stream_prof_upload(sd_stream* s, StreamJob& job) {
    const size_t n = (size_t)job.n_reads;
    FinalWS& fw = *job.dfin.fws;
    std::vector<int64_t>& text_off = job.din.text_off;
    text_off.assign(n + 1, 0);
    for (size_t r = 0; r < n; ++r) text_off[r + 1] = text_off[r] + (int64_t)job.seq[r].size();
    const size_t total = (size_t)text_off[n];
    text_off.resize(n);
    if (n == 0) return;
    take_text(s, job, total + 8);
    fw.prof.h_text.alloc(total);
    uint8_t* stage = fw.prof.h_text.p;
    sd::parallel_for((int64_t)n, s->p.threads, 1, [&](int64_t r) {
        std::memcpy(stage + text_off[(size_t)r], job.seq[(size_t)r].data(), job.seq[(size_t)r].size());
    });
    SD_HIP(hipMemcpyAsync(job.din.text->p, stage, total, hipMemcpyHostToDevice, s->prof_st));
    ensure_event(fw.ev_prof);
    SD_HIP(hipEventRecord(fw.ev_prof, s->prof_st));
    fw.prof_recorded = true;
}

// A record store (or a selection workspace) for a new job of a device-rows or device-final stream: a spare one whose
// last scatter -- enqueued on that job's caller's stream, which may be far behind -- has completed; else a new one, so
// that a slow consumer never stalls the pipeline and no buffer a pending scatter reads is ever reallocated.  Beyond
// eight spares the oldest is waited for instead.
template <class WS>
static std::unique_ptr<WS> stream_take_ws(std::vector<std::unique_ptr<WS>>& sp) {
    for (size_t i = sp.size(); i-- > 0;)
        if (sp[i]->idle()) {
            std::unique_ptr<WS> ws = std::move(sp[i]);
            sp.erase(sp.begin() + (long)i);
            return ws;
        }
    if (sp.size() >= 8) {
        std::unique_ptr<WS> ws = std::move(sp.front());
        sp.erase(sp.begin());
        ws->wait_idle();
        return ws;
    }
    return std::unique_ptr<WS>(new WS);
}

// identity words per record of a job whose engines compute the identities in-stream
static int job_ident_words(const FinalMode& fm) { return fm.second_best ? (int)fm.pp.interleaved_seqs().size() : 1; }

static int stream_submit(sd_stream* s, const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads,
                         char* errbuf, size_t errlen, const DevIn* dv = nullptr) {
    std::unique_ptr<StreamJob> job(new StreamJob);
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
    job->reads = read_seqs;
    if (s->device_store()) job->store.ws.take(stream_take_ws(s->ws_spare), s->ws_spare);
    if (s->mode == StreamMode::FinalDevice) {
        job->dfin.fws.take(stream_take_ws(s->fws_spare), s->fws_spare);
        if (s->dev_prof) {   // (the workspace is idle: its last fold is through, the text that waited for it is free)
            prof_harvest(s, *job->dfin.fws);
            if (job->dfin.fws->held_text) s->spare.push_back(std::move(job->dfin.fws->held_text));
            job->dfin.fws->prof.planned = false;
        }
    }
    if (fm && fm->ident) job->per = job_ident_words(*fm);
    if (dv) {
        // the data's device is current while the job's events and copies are made (the entries all run on it)
        try {
            DeviceScope on(dv->device);
            std::string err;
            if (fm) job->seq.resize((size_t)n_reads);
            int rd = stream_dev_job(s, *job, *dv, read_lens, err);
            // (the folds of this job and of later ones run behind the copy of its text)
            if (rd == SD_OK && s->dev_prof && n_reads > 0 && hipStreamWaitEvent(s->prof_st, s->ev_src, 0) != hipSuccess) {
                (void)hipGetLastError();
                err = "hipStreamWaitEvent failed";
                rd = SD_ERR_HIP;
            }
            if (rd) { set_err(errbuf, errlen, err); return rd; }
        } catch (const HipFail&) {   // (the guard's; stream_dev_job reports its own)
            (void)hipGetLastError();
            set_err(errbuf, errlen, "hipSetDevice failed");
            return SD_ERR_HIP;
        }
    } else if (fm) {   // the fallback identities read the text when the rows come back: the job keeps a copy (sd_hip.h)
        job->seq.resize((size_t)n_reads);
        sd::parallel_for(n_reads, s->p.threads, 1, [&](int64_t r) { job->seq[(size_t)r].assign(read_seqs[r], (size_t)read_lens[r]); });
        for (const std::string& q : job->seq) job->own.push_back(q.data());
        job->reads = job->own.data();
        if (s->dev_prof) {
            try {
                DeviceScope on(s->me.devs[0]);
                stream_prof_upload(s, *job);
            } catch (const HipFail& f) {
                set_err(errbuf, errlen, f.msg);
                return SD_ERR_HIP;
            }
        }
    }
    StreamEntries& me = s->me;
    std::vector<std::pair<size_t, size_t>> batches;
    cut_batches(job->table, s->budget, s->sub_batches, (int)me.devs.size(), batches);
    job->batches_left = job->to_pack = (int)batches.size();
    StreamJob* jp = job.get();
    {
        std::lock_guard<std::mutex> g(me.m);
        if (!me.failed) {
            s->jobs.push_back(std::move(job));
            ++s->n_jobs;
            for (const auto& b : batches) me.queue.push_back(StreamEntries::Queued{jp, b.first, b.second, me.next_b++});
        }
    }
    me.cv.notify_all();
    const bool at_once = fm && !me.th.empty() && !dv;   // (a device job's packers wait for an event of THIS submit)
    std::string err;
    const int rc = me.wait([&] { return at_once || jp->to_pack == 0; }, err);
    if (rc) {
        set_err(errbuf, errlen, err);
        s->jobs.clear();
    }
    return rc;
}

extern "C" {

int sd_stream_create(sd_stream** out, const sd_params* p, const char* const* mono_seqs,
                     const int32_t* mono_lens, int32_t n_mono, int32_t sub_batches, char* errbuf, size_t errlen) {
    return stream_create(out, p, nullptr, nullptr, 0, false, nullptr, mono_seqs, mono_lens, n_mono, sub_batches, 0, 0,
                         nullptr, errbuf, errlen);
}

int sd_stream_create_final(sd_stream** out, const sd_params* p, const char* const* mono_names,
                           const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                           int32_t sub_batches, int32_t min_identity, int32_t second_best,
                           const double* lr_coef, char* errbuf, size_t errlen) {
    return stream_create(out, p, nullptr, nullptr, 0, true, mono_names, mono_seqs, mono_lens, n_mono, sub_batches,
                         min_identity, second_best, lr_coef, errbuf, errlen);
}

int sd_stream_create_devices(sd_stream** out, const sd_params* p, const int32_t* devices, int32_t n_devices,
                             const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono, int32_t sub_batches,
                             char* errbuf, size_t errlen) {
    return stream_create(out, p, "sd_stream_create_devices", devices, n_devices, false, nullptr, mono_seqs, mono_lens,
                         n_mono, sub_batches, 0, 0, nullptr, errbuf, errlen);
}

int sd_stream_create_final_devices(sd_stream** out, const sd_params* p, const int32_t* devices, int32_t n_devices,
                                   const char* const* mono_names, const char* const* mono_seqs, const int32_t* mono_lens,
                                   int32_t n_mono, int32_t sub_batches, int32_t min_identity, int32_t second_best,
                                   const double* lr_coef, char* errbuf, size_t errlen) {
    return stream_create(out, p, "sd_stream_create_final_devices", devices, n_devices, true, mono_names, mono_seqs,
                         mono_lens, n_mono, sub_batches, min_identity, second_best, lr_coef, errbuf, errlen);
}

void sd_stream_destroy(sd_stream* s) { delete s; }

int sd_stream_submit(sd_stream* s, const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads,
                     char* errbuf, size_t errlen) {
    if (!s || n_reads < 0 || (n_reads && (!read_seqs || !read_lens))) return SD_ERR_PARAM;
    const double t0 = now_s();
    int rc;
    try {
        rc = stream_submit(s, read_seqs, read_lens, n_reads, errbuf, errlen);
    } catch (const std::bad_alloc&) {
        set_err(errbuf, errlen, "out of host memory");
        rc = SD_ERR_INTERNAL;
    }
    s->submit_s += now_s() - t0;
    return rc;
}

int sd_stream_submit_dev(sd_stream* s, const void* d_bases, const int64_t* read_off, const int64_t* read_lens,
                         int32_t n_reads, void* hip_stream, char* errbuf, size_t errlen) {
    if (!s || n_reads < 0 || (n_reads > 0 && (!d_bases || !read_off || !read_lens))) return SD_ERR_PARAM;
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_lens[r] <= 0) { set_err(errbuf, errlen, "ERROR: Sequence #" + std::to_string(r) + " is empty"); return SD_ERR_EMPTY; }
    const double t0 = now_s();
    int rc = SD_OK;
    try {
        std::string err;
        DevIn dv{static_cast<const char*>(d_bases), read_off, reinterpret_cast<hipStream_t>(hip_stream), s->me.devs[0]};
        if (n_reads > 0) {
            rc = device_pointer(d_bases, dv.device, err);
            for (size_t i = 0; rc == SD_OK && i < s->me.devs.size(); ++i)
                if (s->me.devs[i] != dv.device) {
                    err = "the reads lie in the memory of device " + std::to_string(dv.device) + ", the stream runs on device " +
                          std::to_string(s->me.devs[i]) + ": copies between devices are not made";
                    rc = SD_ERR_UNSUPPORTED;
                }
            if (rc) set_err(errbuf, errlen, err);
        }
        if (rc == SD_OK) rc = stream_submit(s, nullptr, read_lens, n_reads, errbuf, errlen, &dv);
    } catch (const std::bad_alloc&) {
        set_err(errbuf, errlen, "out of host memory");
        rc = SD_ERR_INTERNAL;
    }
    s->submit_s += now_s() - t0;
    return rc;
}

}  // extern "C"

// The six collect and peek calls: their names, and whether their work needs the stream's device current.
enum StreamCall { CALL_COLLECT, CALL_COLLECT_FINAL, CALL_PEEK_DEV, CALL_COLLECT_DEV, CALL_PEEK_FINAL_DEV, CALL_COLLECT_FINAL_DEV };
static const struct { const char* name; bool on_device; } kStreamCalls[] = {
    {"sd_stream_collect", false},  {"sd_stream_collect_final", false},  {"sd_stream_peek_dev", false},
    {"sd_stream_collect_dev", true}, {"sd_stream_peek_final_dev", true}, {"sd_stream_collect_final_dev", true}};

// Why a call does not belong to a stream of this mode, or null: it does.
static const char* wrong_call(StreamMode m, StreamCall c) {
    const bool raw = m == StreamMode::RawHost || m == StreamMode::RawDevice, fdev = m == StreamMode::FinalDevice;
    switch (c) {
    case CALL_COLLECT:
        if (fdev) return "a device-final stream (SD_FLAG_DEVICE_FINAL) is collected with sd_stream_collect_final_dev: its rows are not on the host";
        if (!raw) return "a final-mode stream is collected with sd_stream_collect_final";
        if (m == StreamMode::RawDevice) return "a device-rows stream (SD_FLAG_DEVICE_ROWS) is collected with sd_stream_collect_dev: its rows are not on the host";
        return nullptr;
    case CALL_COLLECT_FINAL:
        if (raw) return "sd_stream_collect_final on a stream made by sd_stream_create";
        if (fdev) return "a device-final stream (SD_FLAG_DEVICE_FINAL) is collected with sd_stream_collect_final_dev: its rows are not on the host";
        return nullptr;
    case CALL_PEEK_DEV:
        if (fdev) return "a device-final stream (SD_FLAG_DEVICE_FINAL) is peeked with sd_stream_peek_final_dev";
        if (m != StreamMode::RawDevice) return "sd_stream_peek_dev on a stream made without SD_FLAG_DEVICE_ROWS";
        return nullptr;
    case CALL_COLLECT_DEV:
        if (fdev) return "a device-final stream (SD_FLAG_DEVICE_FINAL) is collected with sd_stream_collect_final_dev: it has final rows, not raw ones";
        if (m != StreamMode::RawDevice) return "sd_stream_collect_dev on a stream made without SD_FLAG_DEVICE_ROWS: its rows are on the host (sd_stream_collect)";
        return nullptr;
    case CALL_PEEK_FINAL_DEV:
        return fdev ? nullptr : "sd_stream_peek_final_dev on a stream made without SD_FLAG_DEVICE_FINAL";
    case CALL_COLLECT_FINAL_DEV:
        return fdev ? nullptr : "sd_stream_collect_final_dev on a stream made without SD_FLAG_DEVICE_FINAL";
    }
    return nullptr;
}

// The frame of the six collect and peek calls, behind the check of their arguments: the refusals (a call that does not
// belong to the stream's mode, no job, and `also_refused`, one of the call's own that ranks behind them), the wait for
// the oldest job, the body -- with the stream's device current where the call needs it, a guard that ends before the
// job may be destroyed -- and the time of it all.  (The bodies' refusals of a misplaced buffer run under that guard.)
// The body returns the call's result, its message set, and says whether the job stays; a HipFail or std::bad_alloc it
// throws becomes the call's result.  What becomes of the oldest job:
//   kept      a refusal (wrong call for the mode, no job, a buffer in the wrong place, a buffer too small) and a
//             successful peek: the bodies say keep = true for these;
//   dropped   a collect that succeeded, or failed on the device, on memory or in the job's post-processing, and a failed
//             sd_stream_peek_final_dev (a job whose rows cannot be made is dropped, as collect drops it);
//   a stream-wide failure met in the wait drops every job (stream_wait_oldest).
template <class Body>
static int on_oldest_job(sd_stream* s, StreamCall call, char* errbuf, size_t errlen, Body&& body, const char* also_refused = nullptr) {
    if (const char* wrong = wrong_call(s->mode, call)) { set_err(errbuf, errlen, wrong); return SD_ERR_PARAM; }
    if (s->jobs.empty()) { set_err(errbuf, errlen, std::string(kStreamCalls[call].name) + " without a submitted job"); return SD_ERR_PARAM; }
    if (also_refused) { set_err(errbuf, errlen, also_refused); return SD_ERR_PARAM; }
    const double t0 = now_s();
    int rc = stream_wait_oldest(s, errbuf, errlen);
    if (rc == SD_OK) {
        bool keep = false;
        try {
            std::optional<DeviceScope> on;
            if (kStreamCalls[call].on_device) on.emplace(s->me.devs[0]);
            rc = body(*s->jobs.front(), keep);
        } catch (const HipFail& f) {
            set_err(errbuf, errlen, f.msg);
            rc = SD_ERR_HIP;
        } catch (const std::bad_alloc&) {
            set_err(errbuf, errlen, "out of host memory");
            rc = SD_ERR_INTERNAL;
        }
        if (!keep) s->jobs.erase(s->jobs.begin());
    }
    s->collect_s += now_s() - t0;
    return rc;
}

extern "C" {

int sd_stream_collect(sd_stream* s, sd_rec** rows, int64_t** row_off, int64_t* n_rows, char* errbuf, size_t errlen) {
    if (!s || !rows || !row_off) return SD_ERR_PARAM;
    *rows = nullptr;
    *row_off = nullptr;
    if (n_rows) *n_rows = 0;
    return on_oldest_job(s, CALL_COLLECT, errbuf, errlen, [&](StreamJob& job, bool&) -> int {
        if (job.oom) { set_err(errbuf, errlen, "out of host memory"); return SD_ERR_INTERNAL; }
        if (!job.rows) job.rows = static_cast<sd_rec*>(std::malloc(sizeof(sd_rec)));
        *rows = job.rows;
        *row_off = job.row_off;
        if (n_rows) *n_rows = (int64_t)job.n_rows;
        job.rows = nullptr;      // ownership moves to the caller (sd_free)
        job.row_off = nullptr;
        return SD_OK;
    });
}

int sd_stream_collect_final(sd_stream* s, sd_final_row** rows, int64_t** row_off, int64_t* n_rows, double** alt,
                            char* errbuf, size_t errlen) {
    if (!s || !rows || !row_off) return SD_ERR_PARAM;
    *rows = nullptr;
    *row_off = nullptr;
    if (n_rows) *n_rows = 0;
    if (alt) *alt = nullptr;
    return on_oldest_job(s, CALL_COLLECT_FINAL, errbuf, errlen, [&](StreamJob& job, bool&) -> int {
        if (job.rc) { set_err(errbuf, errlen, job.err); return job.rc; }
        const size_t n = job.fin.n;
        int64_t* off = static_cast<int64_t*>(std::calloc((size_t)job.n_reads + 1, sizeof(int64_t)));
        if (!off || !job.fin.resize(std::max<size_t>(n, 1)) || !job.alt.resize(std::max<size_t>(job.alt.n, 1))) {
            std::free(off);
            set_err(errbuf, errlen, "out of host memory");
            return SD_ERR_INTERNAL;
        }
        for (size_t i = 0; i < n; ++i) ++off[(size_t)job.fin.p[i].read + 1];   // rows come in read order
        for (int32_t r = 0; r < job.n_reads; ++r) off[r + 1] += off[r];
        *rows = job.fin.release();   // ownership moves to the caller (sd_free)
        *row_off = off;
        if (n_rows) *n_rows = (int64_t)n;
        if (alt && s->fin->second_best) *alt = job.alt.release();
        s->fin->kept += (int64_t)n;
        return SD_OK;
    });
}

int sd_stream_peek_dev(sd_stream* s, int32_t* n_reads, int64_t* max_rows, char* errbuf, size_t errlen) {
    if (!s) return SD_ERR_PARAM;
    return on_oldest_job(s, CALL_PEEK_DEV, errbuf, errlen, [&](StreamJob& job, bool& keep) -> int {
        keep = true;
        if (n_reads) *n_reads = job.n_reads;
        if (max_rows) *max_rows = job.store.appended;
        return SD_OK;
    });
}

int sd_stream_collect_dev(sd_stream* s, sd_rec* d_rows, int64_t cap_rows, int64_t* d_row_off, void* hip_stream,
                          int64_t* n_rows, char* errbuf, size_t errlen) {
    if (!s || !d_row_off || cap_rows < 0 || (cap_rows > 0 && !d_rows)) return SD_ERR_PARAM;
    if (n_rows) *n_rows = 0;
    return on_oldest_job(s, CALL_COLLECT_DEV, errbuf, errlen, [&](StreamJob& job, bool& keep) -> int {
        if (cap_rows > 0)
            if (const int rc = buffer_on_device(d_rows, s->me.devs[0], "sd_stream_collect_dev", "row", errbuf, errlen)) { keep = true; return rc; }
        hipStream_t user = reinterpret_cast<hipStream_t>(hip_stream);
        RowsWS& ws = *job.store.ws;
        int64_t n = 0;
        if (job.store.assembled) {
            SD_HIP(hipEventSynchronize(ws.ev_asm));   // (the row count is on the host)
            ws.settled = true;
            n = ws.h_total.p[0];
        }
        if (n_rows) *n_rows = n;
        if (cap_rows < n) {
            set_err(errbuf, errlen, "sd_stream_collect_dev: the job has " + std::to_string(n) + " rows, the buffer room for " + std::to_string(cap_rows));
            keep = true;
            return SD_ERR_PARAM;
        }
        if (job.store.assembled) {
            SD_HIP(hipStreamWaitEvent(user, ws.ev_asm, 0));
            rows_scatter(ws, user, ws.recs.p, reinterpret_cast<sd::DevRec*>(d_rows), cap_rows, d_row_off);
        } else {   // (a job without chunks: no reads)
            SD_HIP(hipMemsetAsync(d_row_off, 0, sizeof(int64_t) * ((size_t)job.n_reads + 1), user));
        }
        return SD_OK;
    });
}

// ---- SD_FLAG_DEVICE_FINAL: the final rows of a job, selected on the device ---------------------------------------

// The text-based path of a device-final job, once per job: a job without in-stream identities (SD_FLAG_NO_STREAM_IDENT, a
// template set the kernels do not take) or with rows the words do not decide.  The merged raw rows come to the host, the
// reads too where they lie on the device, and the post-processor of the file path computes every identity from the
// text; the rows stay in job.fin / alt / fin_off.  Correct and slow.
static int final_dev_slow(sd_stream* s, StreamJob& job, std::string& err) {
    if (job.dfin.slow_done) { err = job.err; return job.rc; }
    job.dfin.slow_done = true;
    FinalMode& fm = *s->fin;
    RowsWS& ws = *job.store.ws;
    FinalWS& fw = *job.dfin.fws;
    const size_t nr = (size_t)job.n_reads;
    const int64_t n = ws.h_total.p[0];
    std::vector<sd_rec> rows((size_t)std::max<int64_t>(n, 1));
    std::vector<int64_t> off(nr + 1, 0);
    // a stream of the stream's own: the pipeline's rows stream may already hold later jobs' appends, merges and
    // selections, which this job need not wait for (the merge it reads from is through: ev_asm has been waited for)
    if (!s->slow_st) SD_HIP(hipStreamCreateWithFlags(&s->slow_st, hipStreamNonBlocking));
    hipStream_t st = s->slow_st;
    fw.mrows.alloc((size_t)std::max<int64_t>(n, 1));
    fw.moff.alloc(nr + 1);
    fw.settled = false;
    rows_scatter(ws, st, ws.recs.p, fw.mrows.p, n, fw.moff.p);
    if (n > 0) SD_HIP(hipMemcpyAsync(rows.data(), fw.mrows.p, (size_t)n * sizeof(sd_rec), hipMemcpyDeviceToHost, st));
    SD_HIP(hipMemcpyAsync(off.data(), fw.moff.p, (nr + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SD_HIP(hipStreamSynchronize(st));
    fw.settled = true;
    std::vector<sd::PostRead> pr;
    for (size_t r = 0; r < nr; ++r) {
        if (job.din.dev) SD_HIP(fetch_read_text(job, r));   // (stream_dev_job made the copy)
        pr.push_back(sd::PostRead{"", 0, job.seq[r].data(), (int64_t)job.seq[r].size()});
    }
    job.rc = fm.pp.process_rows(pr.data(), nr, 0, rows.data(), off.data(), job.fin, job.alt, job.err, nullptr);
    if (job.din.dev)
        for (size_t r = 0; r < nr; ++r) std::string().swap(job.seq[r]);
    if (job.rc) { err = job.err; return job.rc; }
    if (s->dev_prof)   // (process_rows folded the kept rows on the host: profile_kept)
        for (size_t i = 0; i < job.fin.n; ++i) {
            const sd_final_row& f = job.fin.p[i];
            const int64_t rl = job.din.dev ? job.din.rlen[(size_t)f.read] : (int64_t)job.seq[(size_t)f.read].size();
            if (sd::final_seg_len(f.start, f.end, rl) > 0) ++s->prof_pairs_host;
        }
    std::vector<int64_t>& fin_off = job.dfin.fin_off;
    fin_off.assign(nr + 1, 0);
    for (size_t i = 0; i < job.fin.n; ++i) ++fin_off[(size_t)job.fin.p[i].read + 1];   // rows come in read order
    for (size_t r = 0; r < nr; ++r) fin_off[r + 1] += fin_off[r];
    return SD_OK;
}

// The kept-row count of the oldest job, which has been waited for: 16 bytes from the selection, or the text-based path.
static int final_dev_count(sd_stream* s, StreamJob& job, int64_t& n, std::string& err) {
    n = 0;
    if (!job.store.assembled) return SD_OK;   // (a job without chunks: no reads)
    RowsWS& ws = *job.store.ws;
    FinalWS& fw = *job.dfin.fws;
    SD_HIP(hipEventSynchronize(ws.ev_asm));
    ws.settled = true;
    bool slow = !job.dfin.selected;
    if (job.dfin.selected) {
        SD_HIP(hipEventSynchronize(fw.ev_sel));
        fw.settled = true;
        slow = fw.h_counts.p[1] != 0;
    }
    if (slow) {
        const int rc = final_dev_slow(s, job, err);
        if (rc) return rc;
        n = (int64_t)job.fin.n;
    } else {
        n = fw.h_counts.p[0];
    }
    return SD_OK;
}

// SD_FLAG_DEVICE_PROFILE: the fold of a selected job, enqueued on the stream's own stream once the host has its summary
// (ev_sel has been waited for), and the pairs the kernel does not take: their list comes down at 16 bytes a pair, the
// text of those segments alone is fetched (read from job.seq for a job submitted from host memory), and profile_host
// folds them into the post-processor's counters under the kernel.
static int stream_prof_fold(sd_stream* s, StreamJob& job, std::string& err) {
    FinalWS& fw = *job.dfin.fws;
    ProfWS& pw = fw.prof;
    const StreamJob::DevInput& in = job.din;
    if (!pw.planned || !in.text) return SD_OK;
    pw.planned = false;
    ensure_event(fw.ev_f0);
    ensure_event(fw.ev_prof);
    prof_harvest(s, fw);
    SD_HIP(hipEventRecord(fw.ev_f0, s->prof_st));
    const int64_t nd = prof_fold(pw, s->pd, s->prof_st, in.text->p);
    SD_HIP(hipEventRecord(fw.ev_prof, s->prof_st));
    fw.prof_recorded = true;
    fw.fold_timed = nd > 0;
    s->prof_pairs_dev += nd;
    const int64_t nh = pw.h_sum.p[s->pd.M + 1];
    if (nh <= 0) return SD_OK;
    // (the list was written ahead of ev_sel; the text of a DeviceReads job was read by its batches: both are complete)
    if (!s->slow_st) SD_HIP(hipStreamCreateWithFlags(&s->slow_st, hipStreamNonBlocking));
    pw.h_hlist.alloc((size_t)nh);
    SD_HIP(hipMemcpyAsync(pw.h_hlist.p, pw.hlist.p, (size_t)nh * sizeof(sd::FProfHostPair), hipMemcpyDeviceToHost, s->slow_st));
    SD_HIP(hipStreamSynchronize(s->slow_st));
    const sd::FProfHostPair* hp = pw.h_hlist.p;
    std::vector<const char*> q((size_t)nh);
    std::vector<int32_t> ql((size_t)nh), pil((size_t)nh);
    std::vector<char> fetched;
    if (in.dev) {
        size_t bytes = 0;
        for (int64_t x = 0; x < nh; ++x) bytes += (size_t)hp[x].len;
        fetched.resize(std::max<size_t>(bytes, 1));
        size_t at = 0;
        for (int64_t x = 0; x < nh; ++x) {
            SD_HIP(hipMemcpyAsync(fetched.data() + at, in.text->p + hp[x].start, (size_t)hp[x].len, hipMemcpyDeviceToHost, s->slow_st));
            q[(size_t)x] = fetched.data() + at;
            at += (size_t)hp[x].len;
        }
        SD_HIP(hipStreamSynchronize(s->slow_st));
        s->prof_text_to_host += (int64_t)bytes;
    } else {
        for (int64_t x = 0; x < nh; ++x) {
            const size_t r = (size_t)(std::upper_bound(in.text_off.begin(), in.text_off.end(), hp[x].start) - in.text_off.begin()) - 1;
            q[(size_t)x] = job.seq[r].data() + (hp[x].start - in.text_off[r]);
        }
    }
    for (int64_t x = 0; x < nh; ++x) { ql[(size_t)x] = hp[x].len; pil[(size_t)x] = hp[x].il; }
    s->prof_pairs_host += nh;
    return s->fin->pp.profile_pairs(q.data(), ql.data(), pil.data(), nh, err);
}

int sd_stream_peek_final_dev(sd_stream* s, int32_t* n_reads, int64_t* n_rows, int32_t* n_keys, char* errbuf, size_t errlen) {
    if (!s) return SD_ERR_PARAM;
    return on_oldest_job(s, CALL_PEEK_FINAL_DEV, errbuf, errlen, [&](StreamJob& job, bool& keep) -> int {
        int64_t n = 0;
        std::string err;
        if (const int rc = final_dev_count(s, job, n, err)) { set_err(errbuf, errlen, err); return rc; }
        keep = true;
        if (n_reads) *n_reads = job.n_reads;
        if (n_rows) *n_rows = n;
        if (n_keys) *n_keys = (int32_t)s->fin->pp.key_names().size();
        return SD_OK;
    });
}

int sd_stream_collect_final_dev(sd_stream* s, sd_final_row* d_rows, int64_t cap_rows, int64_t* d_row_off, double* d_alt,
                                void* hip_stream, int64_t* n_rows, char* errbuf, size_t errlen) {
    if (!s || !d_row_off || cap_rows < 0 || (cap_rows > 0 && !d_rows)) return SD_ERR_PARAM;
    if (n_rows) *n_rows = 0;
    const bool sb = s->fin && s->fin->second_best;
    const char* no_alt = sb && cap_rows > 0 && !d_alt ? "sd_stream_collect_final_dev: a second_best stream needs the alt buffer" : nullptr;
    return on_oldest_job(s, CALL_COLLECT_FINAL_DEV, errbuf, errlen, [&](StreamJob& job, bool& keep) -> int {
        const void* const bufs[3] = {cap_rows > 0 ? d_rows : nullptr, d_row_off, sb && cap_rows > 0 ? d_alt : nullptr};
        const char* const what[3] = {"row", "row-offset", "alt"};
        for (int b = 0; b < 3; ++b)
            if (bufs[b])
                if (const int rc = buffer_on_device(bufs[b], s->me.devs[0], "sd_stream_collect_final_dev", what[b], errbuf, errlen)) { keep = true; return rc; }
        hipStream_t user = reinterpret_cast<hipStream_t>(hip_stream);
        int64_t n = 0;
        std::string err;
        int rc = final_dev_count(s, job, n, err);
        if (rc) { set_err(errbuf, errlen, err); return rc; }
        const size_t nk = s->fin->pp.key_names().size();
        if (n_rows) *n_rows = n;
        if (cap_rows < n) {
            set_err(errbuf, errlen, "sd_stream_collect_final_dev: the job has " + std::to_string(n) + " rows, the buffers room for " + std::to_string(cap_rows));
            keep = true;
            return SD_ERR_PARAM;
        }
        if (!job.store.assembled) {
            SD_HIP(hipMemsetAsync(d_row_off, 0, sizeof(int64_t) * ((size_t)job.n_reads + 1), user));
        } else if (job.dfin.slow_done) {
            // the rows of the text-based path: pageable memory of the job's, so the host waits for the copies
            const std::vector<int64_t>& fin_off = job.dfin.fin_off;
            if (n > 0) SD_HIP(hipMemcpyAsync(d_rows, job.fin.p, (size_t)n * sizeof(sd_final_row), hipMemcpyHostToDevice, user));
            SD_HIP(hipMemcpyAsync(d_row_off, fin_off.data(), fin_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, user));
            if (sb && n > 0) SD_HIP(hipMemcpyAsync(d_alt, job.alt.p, (size_t)n * nk * sizeof(double), hipMemcpyHostToDevice, user));
            SD_HIP(hipStreamSynchronize(user));
        } else {
            FinalWS& fw = *job.dfin.fws;
            SD_HIP(hipStreamWaitEvent(user, fw.ev_sel, 0));
            final_scatter(fw, user, d_rows, cap_rows, d_row_off, sb ? d_alt : nullptr);
            // (the scatter reads the merged-row count in the record store's workspace: the store waits for it too)
            RowsWS& ws = *job.store.ws;
            ensure_event(ws.ev_free, hipEventDisableTiming);
            SD_HIP(hipEventRecord(ws.ev_free, user));
            ws.free_recorded = true;
            if (s->dev_prof) {
                rc = stream_prof_fold(s, job, err);
                if (rc) set_err(errbuf, errlen, err);
            }
        }
        if (rc == SD_OK) s->fin->kept += n;
        return rc;
    }, no_alt);
}

int sd_stream_keys(sd_stream* s, const char** keys, int32_t cap, int32_t* n_keys) {
    if (!s || !s->fin || (cap > 0 && !keys)) return SD_ERR_PARAM;
    const std::vector<std::string>& k = s->fin->pp.key_names();
    for (int32_t i = 0; i < cap && i < (int32_t)k.size(); ++i) keys[i] = k[(size_t)i].c_str();
    if (n_keys) *n_keys = (int32_t)k.size();
    return SD_OK;
}

// SD_FLAG_DEVICE_PROFILE: waits for the folds enqueued so far and brings the fold's failure count (and, with dc given,
// the counters) to the host on the stream's own stream; reset zeroes the device counters behind the copy.  The stream's
// device is current.
static int stream_prof_down(sd_stream* s, std::vector<unsigned long long>* dc, bool reset) {
    const size_t total = (size_t)s->pd.total;
    std::vector<unsigned long long> tail(8, 0);
    if (dc) {
        dc->assign(total + 8, 0);
        SD_HIP(hipMemcpyAsync(dc->data(), s->pd.counts.p, (total + 8) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->prof_st));
    } else {
        SD_HIP(hipMemcpyAsync(tail.data(), s->pd.counts.p + total, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->prof_st));
    }
    if (reset) SD_HIP(hipMemsetAsync(s->pd.counts.p, 0, total * sizeof(unsigned long long), s->prof_st));
    SD_HIP(hipStreamSynchronize(s->prof_st));
    int fails = 0;
    std::memcpy(&fails, dc ? dc->data() + total : tail.data(), sizeof fails);
    return fails ? SD_ERR_INTERNAL : SD_OK;   // cannot happen: the checkpoints are sized by the longest segment
}

int sd_stream_profile(sd_stream* s, int32_t reset, int32_t* n_monomers, int64_t* n_counts, int64_t* text_bytes,
                      char* text, uint64_t* counts) {
    if (!s || !s->fin || !s->fin->pp.profiling()) return SD_ERR_PARAM;
    sd::PostProcessor& pp = s->fin->pp;
    std::vector<unsigned long long> dc;
    if (s->dev_prof && counts) {   // device counters + host counters
        try {
            DeviceScope on(s->me.devs[0]);
            if (const int rc = stream_prof_down(s, &dc, reset != 0)) return rc;
        } catch (const HipFail&) {
            return SD_ERR_HIP;
        } catch (const std::bad_alloc&) {
            return SD_ERR_INTERNAL;
        }
    }
    std::vector<uint64_t> v = pp.profile(reset && counts);
    for (size_t i = 0; i < v.size() && i < dc.size(); ++i) v[i] += dc[i];
    const std::string t = pp.profile_text();
    if (n_monomers) *n_monomers = (int32_t)(pp.interleaved_seqs().size() / 2);
    if (n_counts) *n_counts = (int64_t)v.size();
    if (text_bytes) *text_bytes = (int64_t)t.size() + 1;
    if (text) std::memcpy(text, t.c_str(), t.size() + 1);
    if (counts) std::memcpy(counts, v.data(), sizeof(uint64_t) * v.size());
    return SD_OK;
}

int sd_stream_profile_dev(sd_stream* s, int32_t reset, uint64_t* d_counts, int64_t cap_counts, void* hip_stream,
                          int64_t* n_counts, char* errbuf, size_t errlen) {
    if (!s) return SD_ERR_PARAM;
    if (n_counts) *n_counts = 0;
    if (!s->dev_prof) { set_err(errbuf, errlen, "sd_stream_profile_dev on a stream made without SD_FLAG_DEVICE_PROFILE"); return SD_ERR_PARAM; }
    const int64_t total = s->pd.total;
    if (n_counts) *n_counts = total;
    if (!d_counts || cap_counts < total) {
        set_err(errbuf, errlen, "sd_stream_profile_dev: the profile has " + std::to_string(total) + " counters, the buffer room for " +
                                    std::to_string(std::max<int64_t>(cap_counts, 0)));
        return SD_ERR_PARAM;
    }
    int rc = buffer_on_device(d_counts, s->me.devs[0], "sd_stream_profile_dev", "count", errbuf, errlen);
    if (rc) return rc;
    try {
        DeviceScope on(s->me.devs[0]);
        hipStream_t user = reinterpret_cast<hipStream_t>(hip_stream);
        rc = stream_prof_down(s, nullptr, false);   // (the folds so far are through)
        if (rc) set_err(errbuf, errlen, "a profile fold ran out of checkpoints");
        if (rc == SD_OK) {
            const size_t nb = (size_t)total * sizeof(unsigned long long);
            SD_HIP(hipMemcpyAsync(d_counts, s->pd.counts.p, nb, hipMemcpyDeviceToDevice, user));
            // the host's counters (pairs the kernel does not take, jobs of the text-based path), added on the caller's stream
            const std::vector<uint64_t> hv = s->fin->pp.profile(reset != 0);
            bool any = false;
            for (uint64_t x : hv) any = any || x != 0;
            if (any) {
                if (s->up_recorded) { SD_HIP(hipEventSynchronize(s->ev_up)); s->up_recorded = false; }
                s->h_up.alloc((size_t)total);
                s->d_up.alloc((size_t)total);
                for (int64_t i = 0; i < total; ++i) s->h_up.p[i] = hv[(size_t)i];
                SD_HIP(hipMemcpyAsync(s->d_up.p, s->h_up.p, nb, hipMemcpyHostToDevice, user));
                prof_add(user, reinterpret_cast<unsigned long long*>(d_counts), s->d_up.p, total);
                ensure_event(s->ev_up, hipEventDisableTiming);
                SD_HIP(hipEventRecord(s->ev_up, user));
                s->up_recorded = true;
            }
            // later folds, and the zeroing, follow the caller's copy on the stream's own stream
            ensure_event(s->ev_pd, hipEventDisableTiming);
            SD_HIP(hipEventRecord(s->ev_pd, user));
            SD_HIP(hipStreamWaitEvent(s->prof_st, s->ev_pd, 0));
            if (reset) SD_HIP(hipMemsetAsync(s->pd.counts.p, 0, nb, s->prof_st));
        }
    } catch (const HipFail& f) {
        set_err(errbuf, errlen, f.msg);
        rc = SD_ERR_HIP;
    } catch (const std::bad_alloc&) {
        set_err(errbuf, errlen, "out of host memory");
        rc = SD_ERR_INTERNAL;
    }
    return rc;
}

int sd_stream_profile_stats(sd_stream* s, double out[4]) {
    if (!s || !out) return SD_ERR_PARAM;
    if (s->dev_prof) {   // (the folds that have completed; a fold in flight is counted by a later call)
        for (std::unique_ptr<FinalWS>& f : s->fws_spare) prof_harvest(s, *f);
        for (std::unique_ptr<StreamJob>& j : s->jobs)
            if (j->dfin.fws) prof_harvest(s, *j->dfin.fws);
    }
    out[0] = (double)s->prof_pairs_dev;
    out[1] = (double)s->prof_pairs_host;
    out[2] = (double)s->prof_text_to_host;
    out[3] = s->prof_ms;
    return SD_OK;
}

int sd_stream_final_stats(sd_stream* s, double out[4]) {
    if (!s || !out) return SD_ERR_PARAM;
    const FinalMode* fm = s->fin.get();
    const PipeCounters t = s->me.counters();
    std::lock_guard<std::mutex> g(s->me.m);
    out[0] = fm ? t.ident_ms : 0.0;
    out[1] = fm ? (double)t.ident_pairs : 0.0;
    // (a device-final stream runs the text-based path inside peek / collect, on the caller's thread)
    out[2] = fm ? (double)(s->mode == StreamMode::FinalDevice ? fm->pp.fallback_blocks : s->me.fallback_blocks) : 0.0;
    out[3] = fm ? (double)fm->kept : 0.0;
    return SD_OK;
}

int sd_stream_stats(sd_stream* s, double out[16]) {
    if (!s || !out) return SD_ERR_PARAM;
    const PipeCounters t = s->me.counters();
    const double v[16] = {t.fill_ms, t.trace_ms, t.compact_ms, t.run_ms, (double)t.launches, (double)t.batches,
                          (double)t.rows, t.pack_s * 1e3, t.wait_s * 1e3, t.sink_s * 1e3, s->submit_s * 1e3,
                          s->collect_s * 1e3, (double)s->n_jobs, (double)s->sub_batches, (double)s->budget, 0.0};
    std::memcpy(out, v, sizeof v);
    return SD_OK;
}

int sd_stream_info(sd_stream* s, int64_t info[8]) {   // entry 0's first engine
    if (!s) return SD_ERR_PARAM;
    std::lock_guard<std::mutex> g(s->me.m);
    std::memcpy(info, s->me.info0, sizeof s->me.info0);
    return SD_OK;
}

int sd_stream_device_stats(sd_stream* s, int64_t* batches, double* busy_ms, int32_t cap) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(s->me.m);
    const std::vector<StreamEntries::Entry>& ent = s->me.ent;
    for (size_t i = 0; i < ent.size() && (int32_t)i < cap; ++i) {
        if (batches) batches[i] = ent[i].dealt;
        if (busy_ms) busy_ms[i] = ent[i].cnt.run_ms;
    }
    return (int)ent.size();
}

}  // extern "C"
