// sd_stream.hip -- sd_stream_*: the streaming form of the job (sequences in host memory -> rows in host memory,
// AlignReadsSet of main.cpp:67-122 without the text), jobs pipelined through the device in sub-batches; in final mode
// (sd_stream_create_final) the rows of final_decomposition.tsv / _alt.tsv as typed rows instead of the raw ones.
#include "sd_pipeline.hpp"

// (lib.py's numpy dtype of the rows mirrors this layout)
static_assert(sizeof(sd_final_row) == 80 && offsetof(sd_final_row, start) == 8 && offsetof(sd_final_row, ident) == 40 &&
              offsetof(sd_final_row, reliable) == 72, "sd_final_row layout");

namespace sdi {
// The final mode of a stream (sd_stream_create_final): the post-processor of the file path -- its selection rules, and its
// fallback for pairs the in-stream kernels do not take -- and whether the engines compute the identities in-stream.
struct FinalMode {
    sd::PostProcessor pp;
    bool second_best = false;
    bool ident = true;       // every engine so far took the identity tables (engine_set_identity)
    int64_t kept = 0;        // rows handed to callers
};

// A submitted job: its rows as they are assembled and, in final mode, its own copy of the reads and its kept rows.
struct StreamJob : RowJob {
    std::vector<std::string> seq;
    sd::HeapArray<sd_final_row> fin;   // handed to the caller by collect
    sd::HeapArray<double> alt;
    int rc = SD_OK;          // first failure of the job's post-processing
    std::string err;
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
};

static int stream_open(sd_stream* s, const sd_params* p, const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                int32_t sub_batches, char* errbuf, size_t errlen) {
    s->p = *p;
    s->sub_batches = std::max(1, (int)sub_batches);
    std::vector<const char*> ms;
    for (int32_t m = 0; m < n_mono; ++m) {
        if (mono_lens[m] <= 0) { set_err(errbuf, errlen, "ERROR: empty monomer sequence"); return SD_ERR_EMPTY; }
        s->mono.emplace_back(mono_seqs[m], (size_t)mono_lens[m]);
    }
    for (const std::string& m : s->mono) ms.push_back(m.data());
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
    std::unique_ptr<sd_stream> s(new sd_stream);
    rc = stream_open(s.get(), p, mono_seqs, mono_lens, n_mono, sub_batches, errbuf, errlen);
    if (rc) return rc;
    *out = s.release();
    return SD_OK;
}

int sd_stream_create_final(sd_stream** out, const sd_params* p, const char* const* mono_names,
                           const char* const* mono_seqs, const int32_t* mono_lens, int32_t n_mono,
                           int32_t sub_batches, int32_t min_identity, int32_t second_best,
                           const double* lr_coef, char* errbuf, size_t errlen) try {
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
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    // every engine of the pipeline (the first now, the others as the pipeline creates them) computes the identities of
    // its batches in-stream; a template set the kernels do not take, or SD_FLAG_NO_STREAM_IDENT, leaves them all to
    // the fallback
    sd_stream* sp = s.get();
    s->pipe.on_engine = [sp](sd_engine* e) {
        FinalMode& f = *sp->fin;
        if (sp->pipe.p.reserved[1] & SD_FLAG_NO_STREAM_IDENT) f.ident = false;
        if (f.ident && !engine_set_identity(e, f.pp.interleaved_seqs(), f.pp.own_interleaved(), f.second_best)) f.ident = false;
    };
    rc = stream_open(s.get(), p, mono_seqs, mono_lens, n_mono, sub_batches, errbuf, errlen);
    if (rc) return rc;
    *out = s.release();
    return SD_OK;
} catch (const std::bad_alloc&) {
    set_err(errbuf, errlen, "out of host memory");
    return SD_ERR_INTERNAL;
}

void sd_stream_destroy(sd_stream* s) { delete s; }

int sd_stream_submit(sd_stream* s, const char* const* read_seqs, const int64_t* read_lens, int32_t n_reads,
                     char* errbuf, size_t errlen) {
    if (!s || n_reads < 0 || (n_reads && (!read_seqs || !read_lens))) return SD_ERR_PARAM;
    const double t0 = now_s();
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
    const char* const* reads = read_seqs;
    std::vector<const char*> own;
    if (fm) {   // the fallback identities read the text when the rows come back: the job keeps a copy (sd_hip.h)
        job->seq.resize((size_t)n_reads);
        sd::parallel_for(n_reads, s->p.threads, 1, [&](int64_t r) { job->seq[(size_t)r].assign(read_seqs[r], (size_t)read_lens[r]); });
        for (const std::string& q : job->seq) own.push_back(q.data());
        reads = own.data();
        if (fm->ident) job->per = fm->second_best ? (int)fm->pp.interleaved_seqs().size() : 1;
    }
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

int sd_stream_final_stats(sd_stream* s, double out[4]) {
    if (!s || !out) return SD_ERR_PARAM;
    const FinalMode* fm = s->fin.get();
    out[0] = fm ? s->pipe.ident_ms : 0.0;
    out[1] = fm ? (double)s->pipe.ident_pairs : 0.0;
    out[2] = fm ? (double)fm->pp.fallback_blocks : 0.0;
    out[3] = fm ? (double)fm->kept : 0.0;
    return SD_OK;
}

int sd_stream_stats(sd_stream* s, double out[16]) {
    if (!s || !out) return SD_ERR_PARAM;
    const Pipeline& q = s->pipe;
    const double v[16] = {q.fill_ms, q.trace_ms, q.compact_ms, q.run_ms, (double)q.launches, (double)q.batches,
                          (double)q.rows, q.pack_s * 1e3, q.wait_s * 1e3, q.sink_s * 1e3, s->submit_s * 1e3,
                          s->collect_s * 1e3, (double)s->n_jobs, (double)s->sub_batches, (double)s->budget, 0.0};
    std::memcpy(out, v, sizeof v);
    return SD_OK;
}

int sd_stream_info(sd_stream* s, int64_t info[8]) {
    if (!s) return SD_ERR_PARAM;
    return sd_engine_info(s->pipe.eng[0], info);
}

}  // extern "C"
