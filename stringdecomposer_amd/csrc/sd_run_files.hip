// sd_run_files.hip -- sd_run_files*: FASTA files on disk -> final_decomposition{_raw,,_alt}.tsv in one native call
// (main.py:186-197 run() + :168-184 convert_tsv), streamed through the device batch by batch.
// Split from sd_engine.hip in round 6; the C-ABI is unchanged.
#include <sys/mman.h>
#include <sys/vfs.h>

#include "sd_devices.hpp"

extern "C" {

// stage times of the last sd_run_files / sd_run_files_range call of this process (sd_last_run_stats)
static std::mutex g_last_m;
static double g_last_run[24] = {0};

// The three texts of one hand-over of sd_run_files (raw / final / _alt parts), and the process-wide pool their buffers
// return to (at most four; sd_release_cache() frees them).  Never destroyed at exit (as the other pools).
struct TextJob { std::vector<std::string> raw, fin; std::vector<sd::TextBuf> alt; };
struct TextPool {
    std::mutex m;
    std::deque<TextJob> free_;
    TextJob take() {
        std::lock_guard<std::mutex> g(m);
        TextJob j;
        if (!free_.empty()) { j = std::move(free_.front()); free_.pop_front(); }
        return j;
    }
    void give(TextJob&& j) {
        TextJob drop;   // freed outside the lock
        std::lock_guard<std::mutex> g(m);
        if (free_.size() < 4) free_.push_back(std::move(j)); else drop = std::move(j);
    }
    void clear() {
        std::deque<TextJob> drop;
        std::lock_guard<std::mutex> g(m);
        drop.swap(free_);
    }
};
static TextPool& g_textpool_ref() { static TextPool* p = new TextPool; return *p; }
#define g_textpool g_textpool_ref()
extern "C++" void text_pool_clear() { g_textpool.clear(); }

// per device entry of the last call (sd_last_run_device_stats): batches dealt to it, device busy ms
// the profile of the last sd_run_files* call (SD_FLAG_PROFILE; sd_last_run_profile)
static bool g_last_prof_on = false;
static std::vector<uint64_t> g_last_prof;
static std::string g_last_prof_text;
static int32_t g_last_prof_n = 0;
static int g_last_ndev = 0;
static int64_t g_last_screen[2] = {0, 0};   // reads, reads with a region of the last screened job
static int64_t g_last_dev_batches[kMaxDevices] = {0};
static double g_last_dev_busy[kMaxDevices] = {0};

// The FASTA side of a job: both files indexed and checked, the monomers, and this rank's reads -- the reads [lo, hi) of a
// split of the read set into `world` contiguous groups of about equal chunk counts (world == 1: everything).
struct JobInput {
    sd::FastaFile rf, mf;
    std::vector<sd::Seq> monos;
    std::vector<ReadView> reads;
    int load(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank, int32_t world, bool progress,
             int64_t* info, std::string& err) {
        if (progress)   // main.cpp:393
            std::fprintf(stderr, "Scores: insertion=%d deletion=%d mismatch=%d match=%d\n", p->ins, p->del, p->mismatch, p->match);
        const bool lenient = lenient_of(p);
        int rc = rf.open(reads_fa, p->threads, err, lenient);                     // main.cpp:394
        if (rc == SD_OK && world == 1) rc = rf.validate(0, rf.recs.size(), p->threads, err);   // reads are checked first, as there
        if (rc == SD_OK) rc = mf.open(monomers_fa, p->threads, err, lenient);     // main.cpp:395
        if (rc == SD_OK) rc = mf.validate(0, mf.recs.size(), p->threads, err);
        if (rc) return rc;
        sd_note_input_stats(rf, mf, lenient);
        for (const auto& r : mf.recs) monos.push_back(sd::Seq{std::string(r.name, r.name_len), std::string(r.seq, (size_t)r.len)});
        if (monos.empty()) { err = "no monomers"; return SD_ERR_PARAM; }
        std::vector<ReadView> all_reads;
        all_reads.reserve(rf.recs.size());
        for (const auto& r : rf.recs) {
            if (r.len <= 0) { err = "ERROR: Sequence " + std::string(r.name, r.name_len) + " is empty"; return SD_ERR_EMPTY; }
            all_reads.push_back(ReadView{r.name, r.name_len, r.seq, r.len});
        }
        {
            // SeqIO.to_dict (main.py:65) refuses repeated read ids
            std::vector<std::pair<std::string, size_t>> nm;
            nm.reserve(all_reads.size());
            for (size_t r = 0; r < all_reads.size(); ++r) nm.emplace_back(std::string(all_reads[r].name, all_reads[r].name_len), r);
            std::sort(nm.begin(), nm.end());
            for (size_t i = 1; i < nm.size(); ++i)
                if (nm[i].first == nm[i - 1].first) { err = "Duplicate key '" + nm[i].first + "'"; return SD_ERR_FORMAT; }
        }
        // this rank's reads: contiguous groups of about equal chunk counts
        size_t r_lo = 0, r_hi = all_reads.size();
        if (world > 1) {
            std::vector<int64_t> cum(all_reads.size() + 1, 0);
            int64_t biggest = 0;
            for (size_t r = 0; r < all_reads.size(); ++r) {
                const int64_t k = sd::chunk_plan(all_reads[r].len, p->part_size, p->overlap, [](int64_t, int32_t) {});
                cum[r + 1] = cum[r] + k;
                biggest = std::max(biggest, k);
            }
            const int64_t total = cum[all_reads.size()];
            if (biggest * 2 * world > total) {
                err = "read set cannot be split by reads (one read holds more than half a rank's share)";
                return SD_ERR_UNSUPPORTED;
            }
            auto bound = [&](int g) {
                const int64_t want = total * g / world;
                return (size_t)(std::lower_bound(cum.begin(), cum.end(), want) - cum.begin());
            };
            r_lo = std::min(bound(rank), all_reads.size());
            r_hi = rank + 1 == world ? all_reads.size() : std::min(bound(rank + 1), all_reads.size());
            if (r_hi < r_lo) r_hi = r_lo;
            rc = rf.validate(r_lo, r_hi, p->threads, err);   // a rank checks the reads it touches (the launcher exchanges failures)
            if (rc) return rc;
        }
        // main.cpp:343 (load_fasta): the N warning, once per file, on stderr
        for (const auto& ff : {std::make_pair(&rf, reads_fa), std::make_pair(&mf, monomers_fa)})
            if (ff.first->has_n && rank == 0)
                std::fprintf(stderr, "WARNING: sequences in %s contain N symbol. It will be counted as a separate symbol in scoring!\n", ff.second);
        reads.assign(all_reads.begin() + (long)r_lo, all_reads.begin() + (long)r_hi);
        if (info) { info[0] = (int64_t)r_lo; info[1] = (int64_t)r_hi; info[2] = (int64_t)all_reads.size(); info[3] = 0; }
        return SD_OK;
    }
};

// Bytes of a job's _alt TSV, known closely from the reads alone: every base ends up in a block (main.cpp:217-269), a
// block prints one row per template.
static int64_t alt_size_estimate(const std::vector<sd::Seq>& monos, const std::vector<ReadView>& reads) {
    double lmean = 0, nmean = 0;
    for (const sd::Seq& m : monos) { lmean += (double)m.seq.size(); nmean += (double)m.name.size() + 0.5; }   // (half of the templates carry the "'")
    lmean /= std::max<size_t>(1, monos.size());
    nmean /= std::max<size_t>(1, monos.size());
    double est = 0;
    auto digits = [](int64_t v) { int d = 1; while (v >= 10) { v /= 10; ++d; } return d; };
    for (const ReadView& r : reads)
        est += ((double)r.len / std::max(1.0, lmean) + 1.0) * (2.0 * (double)monos.size()) *
               ((double)r.name_len + nmean + 2.0 * digits(r.len) + 5 + 1 + 6);
    return (int64_t)est;
}

// The three outputs of a job as plain descriptors: every hand-over's text is written by all host threads with pwrite at
// its offset (sd::write_parts) -- the copy into the page cache is what a 300-MB _alt batch costs.  close() -- or the
// destructor, on a path that did not reach it -- ends the _alt reservation, cuts that file to what was written and
// closes all three.
struct OutFiles {
    int fr = -1, ff = -1, fa = -1;
    int64_t off_r = 0, off_f = 0, off_a = 0;
    int threads = 1;
    // Round 6: the pages of the _alt file are reserved WHILE THE DEVICE RUNS THE DP.  A --second-best job writes 2T rows of
    // text per block (280 MB at BASELINE config 4) and the page-cache copy of that text bounded the job: on tmpfs the pages
    // of a new range are zeroed by ONE thread inside fallocate (36-49 ms per 280 MB, sd::write_parts), and that could only
    // begin when the first identities arrived, 20 ms into the job.  The size of the file is known closely from the reads
    // alone (alt_size_estimate), so a helper thread reserves that much in steps of 16 MB from the start of the job (short
    // steps: write_parts' own fallocate of a range that already has its pages, and the page faults of the copying threads,
    // take the inode's lock in between); the file is cut to its real size at the end.  Only with -i 0 (a higher threshold
    // drops rows, main.py:152), only on tmpfs / ramfs (where write_parts copies through a mapping), only for texts of at
    // least 32 MB.
    // The reserved range is mapped ONCE for the job and the helper also fills its page tables (MADV_POPULATE_WRITE on pages
    // that exist is a walk, not an allocation): a hand-over's _alt text is then a plain parallel copy -- the per-hand-over
    // fallocate / mmap / 8 000 minor faults / munmap of write_parts made eight 34-MB writes take 5.5-7 ms each, back to
    // back on the writer thread from the first identities to 30 ms after the last (profiles/r06_c4_second_best_timeline.txt).
    std::thread prealloc;
    std::atomic<bool> pre_stop{false};
    std::atomic<int64_t> pre_done{0};
    char* alt_map = nullptr;
    int64_t alt_map_len = 0;
    int64_t alt_unmapped = 0;   // the mapping below this (page-aligned) offset is gone again

    bool open(const char* raw, const char* fin, const char* alt, int n_threads) {
        threads = n_threads;
        fr = ::open(raw, O_RDWR | O_CREAT | O_TRUNC, 0666);   // O_RDWR: write_parts maps the new range
        ff = fr >= 0 ? ::open(fin, O_RDWR | O_CREAT | O_TRUNC, 0666) : -1;
        fa = ff >= 0 ? ::open(alt, O_RDWR | O_CREAT | O_TRUNC, 0666) : -1;
        return fa >= 0;
    }
    // the _alt text of a job is expected to take `want` bytes
    void reserve_alt(int64_t want, double t_begin) {
        struct statfs fs;
        const bool ram = ::fstatfs(fa, &fs) == 0 && ((unsigned long)fs.f_type == 0x01021994ul || (unsigned long)fs.f_type == 0x858458f6ul);
        if (!ram || want < (32 << 20) || !sd::write_parts_fallocate_ok() || getenv("SD_ALT_PREALLOC_OFF")) return;
        void* mp = getenv("SD_ALT_MAP_OFF") ? MAP_FAILED : ::mmap(nullptr, (size_t)want, PROT_READ | PROT_WRITE, MAP_SHARED, fa, 0);
        if (mp != MAP_FAILED) { alt_map = static_cast<char*>(mp); alt_map_len = want; }
        prealloc = std::thread([this, want, t_begin]() {
            const double tp0 = now_s();
            const int64_t step = 16 << 20;
            for (int64_t at = 0; at < want && !pre_stop.load(std::memory_order_relaxed); at += step) {
                const int64_t n = std::min(step, want - at);
                if (::fallocate(fa, 0, (off_t)at, (off_t)n) != 0) break;   // (no space: write_parts reports it)
                // (page tables first, then the range is handed to the writer: write_alt unmaps what it has written, and
                // an madvise still walking a range that has left the mapping could meet somebody else's pages there)
#ifdef MADV_POPULATE_WRITE
                if (alt_map) (void)::madvise(alt_map + at, (size_t)n, MADV_POPULATE_WRITE);
#endif
                pre_done.store(at + n, std::memory_order_release);
            }
            if (getenv("SD_TIMING"))
                std::fprintf(stderr, "[sd timing] _alt pages reserved ahead: %lld of %lld bytes in %.1f ms (from %.1f ms into the job)\n",
                             (long long)pre_done.load(), (long long)want, (now_s() - tp0) * 1e3, (tp0 - t_begin) * 1e3);
        });
    }
    bool write(const TextJob& j) {
        return sd::write_parts(fr, off_r, j.raw, threads) && sd::write_parts(ff, off_f, j.fin, threads) && write_alt(j.alt);
    }
    // a hand-over's _alt text: into the job's mapping where its pages are reserved, else as every other text
    bool write_alt(const std::vector<sd::TextBuf>& parts) {
        std::vector<int64_t> at(parts.size() + 1, off_a);
        for (size_t i = 0; i < parts.size(); ++i) at[i + 1] = at[i] + (int64_t)parts[i].size();
        if (alt_map && at[parts.size()] <= pre_done.load(std::memory_order_acquire)) {
            sd::parallel_for((int64_t)parts.size(), threads, 1, [&](int64_t i) {
                const sd::TextBuf& q = parts[(size_t)i];
                if (q.size()) std::memcpy(alt_map + at[(size_t)i], q.data(), q.size());
            });
            off_a = at[parts.size()];
            // The pages behind the text just written leave the mapping at once, on this (the writer's) thread: taking all
            // 70 000 page-table entries of a 280-MB file down at the end of the job was 10-13 ms on the job's critical
            // path -- or, from a detached thread, on the mmap lock of whatever the process did next.
            const int64_t pg = (int64_t)::sysconf(_SC_PAGESIZE);
            const int64_t upto = off_a / pg * pg;
            if (upto > alt_unmapped) {
                ::munmap(alt_map + alt_unmapped, (size_t)(upto - alt_unmapped));
                alt_unmapped = upto;
            }
            return true;
        }
        return sd::write_parts(fa, off_a, parts, threads);
    }
    bool close() {   // false: a file did not close cleanly
        pre_stop.store(true);
        if (prealloc.joinable()) prealloc.join();
        if (fa >= 0 && pre_done.load() > off_a) (void)!::ftruncate(fa, (off_t)off_a);
        if (alt_map) {   // (what write_alt has not unmapped yet: the page of the file's end and the unused rest of the estimate)
            if (alt_unmapped < alt_map_len) ::munmap(alt_map + alt_unmapped, (size_t)(alt_map_len - alt_unmapped));
            alt_map = nullptr;
        }
        bool ok = true;
        for (int* f : {&fr, &ff, &fa}) {
            if (*f >= 0 && ::close(*f) != 0) ok = false;
            *f = -1;
        }
        return ok;
    }
    ~OutFiles() { close(); }
};

// The rows of the reads [r0, r1) as a driver hands them over, with their identities: the batch's pinned arrays (taken from
// the pipeline, given back to the pool when the text is made), where each row's words are (src), and the words of carried
// rows by value (xid / xidh).
struct Work {
    size_t r0, r1; sd_rec* rows; std::vector<int64_t> off;
    Pipeline::IdentOut ident; int64_t* src; std::vector<uint32_t> xid, xidh; bool have_ident;
};

// The host side of a job behind its drivers.  The rows of a batch are assembled on the driver's thread (they come out of
// the engine's pinned buffer, which the next load reuses) and handed to a sink thread that turns them into the three texts,
// while the driver packs and enqueues the next batch.  The texts go to a writer thread that copies them into the files
// (the page-cache copy of a --second-best job's _alt rows -- 280 MB at C4 -- takes twice as long as formatting them):
// formatting hand-over s + 1 and writing hand-over s run side by side.  At most two hand-overs wait for either thread.
// Text buffers circulate between the two threads and stay with the process between jobs (g_textpool: a fresh 35-MB vector
// is page faults, and giving 300 MB back to the kernel at the end of every job was 16 ms).  The first failure -- of
// either thread, or of a driver's assembly -- is the job's (rc, err); what is handed over after it is dropped.
struct TextStages {
    const std::vector<ReadView>& reads;
    const TemplateSet& ts;
    sd::PostProcessor& pp;
    sd::RecordsWriter* rec;   // the rows once more as the binary record stream, or null
    OutFiles& files;
    const char* raw_path;
    bool progress, second_best, timing;
    double t_begin;
    std::atomic<int> rc{SD_OK};
    std::string err;   // written under wq_m by whichever thread fails first
    double t_fmt = 0, t_post = 0, t_io = 0;
    std::mutex wq_m, io_m;
    std::condition_variable wq_cv, io_cv;
    std::deque<Work> wq;
    std::deque<TextJob> io_q;
    bool wq_done = false, io_done = false;
    std::thread sink_thread, io_thread;

    TextStages(const std::vector<ReadView>& reads_, const TemplateSet& ts_, sd::PostProcessor& pp_, sd::RecordsWriter* rec_,
               OutFiles& files_, const char* raw_path_, bool progress_, bool second_best_, bool timing_, double t_begin_)
        : reads(reads_), ts(ts_), pp(pp_), rec(rec_), files(files_), raw_path(raw_path_), progress(progress_),
          second_best(second_best_), timing(timing_), t_begin(t_begin_) {}
    ~TextStages() { finish(); }
    void start() {
        sink_thread = std::thread([this]() { sink_loop(); });
        io_thread = std::thread([this]() { io_loop(); });
    }
    bool failed() const { return rc.load() != SD_OK; }
    void fail(int code, const std::string& msg) {
        std::lock_guard<std::mutex> lk(wq_m);
        if (rc.load() == SD_OK) { err = msg; rc.store(code); }
    }
    void hand_over(Work&& w) {
        std::unique_lock<std::mutex> lk(wq_m);
        wq_cv.wait(lk, [&] { return wq.size() < 2; });
        wq.push_back(std::move(w));
        lk.unlock();
        wq_cv.notify_all();
    }
    // what was handed over is made and written; both threads end
    void finish() {
        {
            std::lock_guard<std::mutex> lk(wq_m);
            wq_done = true;
        }
        wq_cv.notify_all();
        if (sink_thread.joinable()) sink_thread.join();
        {
            std::lock_guard<std::mutex> lk(io_m);
            io_done = true;
        }
        io_cv.notify_all();
        if (io_thread.joinable()) io_thread.join();
    }

  private:
    void sink_loop() {
        sd::HostPool::lane() = 1;   // this thread's parallel loops run on the second pool, beside the driver's
        std::vector<sd::PostRead> preads;
        for (;;) {
            Work w;
            {
                std::unique_lock<std::mutex> lk(wq_m);
                wq_cv.wait(lk, [&] { return wq_done || !wq.empty(); });
                if (wq.empty()) return;
                w = std::move(wq.front());
                wq.pop_front();
            }
            wq_cv.notify_all();
            try {
                if (!failed()) make_text(w, preads);
            } catch (const std::bad_alloc&) {
                fail(SD_ERR_INTERNAL, "out of host memory");
            }
            std::free(w.rows);
            std::free(w.src);
            if (!w.ident.own_id) {   // (blocks of a slice go back when the last slice lets go of them)
                g_pinpool.give(w.ident.id, w.ident.id_bytes);
                g_pinpool.give(w.ident.idh, w.ident.idh_bytes);
            }
        }
    }
    // a hand-over's three texts (and its records), queued for the writer
    void make_text(const Work& w, std::vector<sd::PostRead>& preads) {
        if (progress) {   // main.cpp:115, one line per read, written per hand-over
            std::string pl;
            const size_t n_all = reads.size();
            for (size_t r = w.r0; r < w.r1; ++r) {
                sd::put_int(pl, (int64_t)((r + 1) * 100 / n_all));
                pl.append("%: Aligned ");
                pl.append(reads[r].name, reads[r].name_len);
                pl.push_back('\n');
            }
            (void)std::fwrite(pl.data(), 1, pl.size(), stderr);
        }
        double t0 = now_s();
        // raw TSV (SaveBatch, main.cpp:272-285): slices of <= 32 k rows, so that a chromosome-sized read is
        // formatted by all threads; a slice needs the end of the row before it
        struct Slice { size_t r; int64_t a, b; };
        std::vector<Slice> slices;
        const int64_t* off = w.off.data();   // off[r - r0] .. : rows of read r
        for (size_t r = w.r0; r < w.r1; ++r)
            for (int64_t a = off[r - w.r0]; a < off[r - w.r0 + 1]; a += 32768)
                slices.push_back(Slice{r, a, std::min<int64_t>(off[r - w.r0 + 1], a + 32768)});
        TextJob wj = g_textpool.take();
        wj.raw.resize(slices.size());
        for (std::string& q : wj.raw) q.clear();
        sd::parallel_for((int64_t)slices.size(), files.threads, 1, [&](int64_t x) {
            const Slice& sl = slices[(size_t)x];
            sd::format_rows(wj.raw[(size_t)x], reads[sl.r].name, reads[sl.r].name_len, ts.tnames, w.rows + sl.a,
                            (size_t)(sl.b - sl.a), sl.a > off[sl.r - w.r0] ? w.rows[sl.a - 1].end : 0, reads[sl.r].base);
        });
        if (rec)
            for (size_t r = w.r0; r < w.r1; ++r)
                rec->add_read(reads[r].name, reads[r].name_len, reads[r].len, w.rows + off[r - w.r0], off[r - w.r0 + 1] - off[r - w.r0]);
        t_fmt += now_s() - t0;
        t0 = now_s();
        preads.clear();
        for (size_t r = w.r0; r < w.r1; ++r)
            preads.push_back(sd::PostRead{reads[r].name, reads[r].name_len, reads[r].seq, reads[r].len, reads[r].base});
        std::string e2;
        sd::IdentRef iref;
        if (w.have_ident)
            iref = sd::IdentRef{w.ident.id, second_best ? w.ident.idh : nullptr, w.src, w.xid.data(), w.xidh.data()};
        const int r2 = pp.process_parts(preads.data(), preads.size(), w.rows, off, wj.fin, wj.alt, e2,
                                        w.have_ident ? &iref : nullptr);
        t_post += now_s() - t0;
        if (r2) { fail(r2, e2); return; }
        std::unique_lock<std::mutex> lk(io_m);
        io_cv.wait(lk, [&] { return io_q.size() < 2; });
        io_q.push_back(std::move(wj));
        lk.unlock();
        io_cv.notify_all();
    }
    void io_loop() {
        sd::HostPool::lane() = 2;
        for (;;) {
            TextJob j;
            {
                std::unique_lock<std::mutex> lk(io_m);
                io_cv.wait(lk, [&] { return io_done || !io_q.empty(); });
                if (io_q.empty()) return;
                j = std::move(io_q.front());
                io_q.pop_front();
            }
            io_cv.notify_all();
            try {
                const double t0 = now_s();
                const int64_t a0 = files.off_a;
                if (!failed() && !files.write(j)) fail(SD_ERR_IO, std::string("short write to ") + raw_path);
                t_io += now_s() - t0;
                if (timing)
                    std::fprintf(stderr, "[sd timing] write of a hand-over: %.1f MB of _alt rows in %.1f ms, at %.1f ms into the job\n",
                                 (double)(files.off_a - a0) / 1e6, (now_s() - t0) * 1e3, (now_s() - t_begin) * 1e3);
                g_textpool.give(std::move(j));
            } catch (const std::bad_alloc&) {
                fail(SD_ERR_INTERNAL, "out of host memory");
            }
        }
    }
};

// A driver's side of a hand-over: the records of the chunks [c0, c1) that pipeline pq just fetched are assembled into the
// rows of the reads they complete, which go to the text stages with their identities.
static void assemble(RowJob& job, Pipeline& pq, size_t c0, size_t c1, const sd_rec* recs, const int64_t* roff, TextStages& text) {
    if (text.failed()) return;
    const size_t r0 = job.next_read;
    job.n_rows = 0;
    job.row_off[r0] = 0;
    job.bid = pq.cur_ident.id;
    job.bidh = pq.cur_ident.idh;
    job.add(c0, c1, recs, roff);
    if (job.oom) { text.fail(SD_ERR_INTERNAL, "out of host memory"); return; }
    const size_t r1 = job.next_read;
    if (r1 == r0) return;
    Work w;
    w.r0 = r0;
    w.r1 = r1;
    w.rows = job.rows;
    w.off.assign(job.row_off + r0, job.row_off + r1 + 1);
    // identities that came with the batches of these rows; a batch without them (more records than the outputs
    // had room for) sends the whole hand-over through the text-based identities
    w.have_ident = job.per && job.ident_ok;
    w.src = job.rsrc;
    job.rsrc = nullptr;
    w.xid.swap(job.xid);
    w.xidh.swap(job.xidh);   // (w's are empty)
    if (w.have_ident && job.bid) w.ident = pq.take_ident();   // the rows point into the batch's pinned arrays
    job.ident_ok = job.carry.empty() || job.bid != nullptr;
    job.rows = nullptr;       // the next batch assembles into a fresh (or recycled) buffer
    job.cap_rows = 0;
    job.n_rows = 0;
    text.hand_over(std::move(w));
}

// The batches of a job whose pipelines hold entry_budget rows per batch.
static void plan_job(const RowJob& job, const std::vector<int64_t>& entry_budget, const std::vector<int32_t>& devs,
                     const sd_params* p, bool second_best, bool slice_ident, bool reused,
                     std::vector<std::pair<size_t, size_t>>& batches) {
    const size_t nc = job.table.size();
    // --second-best makes the host side of a batch (2T identities' worth of text per row) as long as its kernels.  Round 3
    // cut a job that fits ONE batch in up to four, so that the text of a part is written while the next is on the
    // device -- four under-filled fill launches (C4: 47.6 instead of 22.6 ms of fill).  Now the DP of a batch is one
    // launch and its IDENTITIES run in slices of whole reads (sd_engine::slice_end): the host fetches, assembles and
    // formats slice s while the device computes slice s + 1.
    int min_batches = 1;
    if (second_best && !slice_ident)
        min_batches = nc >= 2048 ? 4 : nc >= 1024 ? 2 : 1;   // C4 shape, 2 560 chunks: 170 / 159 / 149 / 140 / 134+ ms for 1 / 2 / 3 / 4 / 5+
    // A process's first job pays for every byte it allocates: the driver scrubs memory another process released before
    // it hands it out -- the 17 GB a 50-Mbp job takes as ONE batch cost 0.2-1.2 s, more than the job (0.3 s).  Such a
    // job is cut into eight batches (two run side by side, stream mode 2), so that its buffers are an eighth as large;
    // a pipeline that comes from the cache has its buffers, and a job of many batches allocates full-size ones once.
    if (!reused && !slice_ident) min_batches = std::max(min_batches, nc >= 4096 ? 8 : nc >= 1024 ? 4 : 1);
    if (const char* ev = getenv("SD_MIN_BATCHES")) min_batches = std::max(1, atoi(ev));   // developer A/B
    int64_t budget = shared_row_budget(entry_budget, devs, p);
    if (!reused) {
        int64_t rows = 0;
        for (const CRef& c : job.table) rows += c.len;
        if (rows > budget) budget = fresh_row_budget(budget, rows);   // many batches: smaller ones, smaller engines
    }
    cut_batches(job.table, budget, min_batches, (int)devs.size(), batches);
}

// Kernel times, batches and host stage times of a job, summed over its pipelines: sd_last_run_stats,
// sd_last_run_device_stats, and with SD_TIMING on stderr.
static void report_stats(const std::vector<std::unique_ptr<Pipeline>>& pipes, const std::vector<int64_t>& dealt,
                         const TextStages& text, const sd::PostProcessor& pp, size_t n_batches, double t_setup) {
    PipeCounters t;
    for (const auto& q : pipes) t += q->cnt;
    if (text.timing)
        std::fprintf(stderr, "[sd timing] %zu batches: pack+enqueue %.1f ms, wait %.1f ms, raw text %.1f ms, post-processing %.1f ms, "
                     "file writes %.1f ms, total %.1f ms\n", n_batches, t.pack_s * 1e3, t.wait_s * 1e3, text.t_fmt * 1e3,
                     text.t_post * 1e3, text.t_io * 1e3, (now_s() - text.t_begin) * 1e3);
    if (text.timing)
        std::fprintf(stderr, "[sd timing] of which device / pinned allocations (hipMalloc, hipHostMalloc): %.1f ms\n", (double)g_alloc_ns.load() / 1e6);
    if (text.timing)
        std::fprintf(stderr, "[sd timing] post-processing: segments %.1f ms, identities %.1f ms, text %.1f ms, concatenation %.1f ms\n",
                     pp.t_prepare * 1e3, pp.t_identity * 1e3, pp.t_format * 1e3, pp.t_concat * 1e3);
    {
        std::lock_guard<std::mutex> lk(g_last_m);
        const double v[24] = {t.fill_ms, t.trace_ms, t.compact_ms, t.ident_ms, (double)t.ident_pairs, (double)t.batches,
                              (double)t.rows, t.pack_s * 1e3, t.wait_s * 1e3, text.t_fmt * 1e3,
                              text.t_post * 1e3, text.t_io * 1e3, pp.t_identity * 1e3, pp.t_format * 1e3, (now_s() - text.t_begin) * 1e3,
                              (double)g_alloc_ns.load() / 1e6, t_setup * 1e3, t.sink_s * 1e3, (double)t.homo_pairs,
                              (double)t.homo_full_pairs, 0, 0, 0, 0};
        std::memcpy(g_last_run, v, sizeof v);
        g_last_ndev = std::min((int)pipes.size(), kMaxDevices);
        for (int i = 0; i < g_last_ndev; ++i) { g_last_dev_batches[i] = dealt[(size_t)i]; g_last_dev_busy[i] = pipes[(size_t)i]->cnt.run_ms; }
    }
    if (text.timing) {
        double nw[4];
        sd::nw_stage_seconds(nw);
        std::fprintf(stderr, "[sd timing] identities on the device: preparation + staging %.1f ms, uploads %.1f ms, launch %.1f ms, "
                     "kernel + downloads %.1f ms\n", nw[0] * 1e3, nw[1] * 1e3, nw[2] * 1e3, nw[3] * 1e3);
    }
}

// --screen (sd_run_files_screen): the threshold and where the region file goes
struct ScreenOpt { int32_t thr; const char* tsv_out; };

// Phase 1 of a screened job: the key of every chunk of the file (sd_screen.hip, the batches dealt over the device
// entries), the regions of the threshold, the region file; `reads` becomes the region list -- each region a ReadView into
// its parent's mapped bases, with the parent's name and its start as `base` -- which phase 2, the job as it always was,
// decomposes as reads of their own.  stats: [0] wall ms, [1] device ms of the distance kernels, [2] bases read, [3] bases
// of the regions, [4] reads, [5] reads with a region.
static int screen_phase(const JobInput& in, const TemplateSet& ts, const sd_params* p, const std::vector<int32_t>& devs,
                        const ScreenOpt& so, std::vector<ReadView>& reads, double stats[6], std::string& err) {
    const double t0 = now_s();
    const size_t n = reads.size();
    std::vector<const char*> seqs(n);
    std::vector<int64_t> lens(n);
    for (size_t r = 0; r < n; ++r) { seqs[r] = reads[r].seq; lens[r] = reads[r].len; }
    std::vector<uint32_t> keys;
    int rc = screen_file_reads(seqs.data(), lens.data(), n, ts.mseq.data(), ts.mlen.data(), (int32_t)ts.mseq.size(), p, devs, keys,
                               &stats[1], err);
    if (rc) return rc;
    std::vector<int32_t> chunk_read;
    chunk_read.reserve(keys.size());
    for (size_t r = 0; r < n; ++r)
        sd::chunk_plan(lens[r], p->part_size, p->overlap, [&](int64_t, int32_t) { chunk_read.push_back((int32_t)r); });
    std::vector<sd_screen_region> reg(keys.size() + 1);
    int64_t n_reg = 0;
    char eb[256] = {0};
    rc = sd_screen_regions(keys.data(), chunk_read.data(), (int64_t)keys.size(), lens.data(), (int32_t)n, p->part_size, p->overlap,
                           so.thr, reg.data(), (int64_t)reg.size(), &n_reg, eb, sizeof eb);
    if (rc) { err = eb; return rc; }
    std::string txt;
    std::vector<ReadView> out;
    out.reserve((size_t)n_reg);
    int64_t bases = 0, with_region = 0;
    for (int64_t g = 0; g < n_reg; ++g) {
        const sd_screen_region& x = reg[(size_t)g];
        const ReadView& rd = reads[(size_t)x.read];
        if (g == 0 || reg[(size_t)g - 1].read != x.read) ++with_region;
        bases += x.end_incl - x.start + 1;
        out.push_back(ReadView{rd.name, rd.name_len, rd.seq + x.start, x.end_incl - x.start + 1, x.start});
        txt.append(rd.name, rd.name_len); txt.push_back('\t');
        sd::put_int(txt, x.start); txt.push_back('\t');
        sd::put_int(txt, x.end_incl); txt.push_back('\t');
        sd::put_int(txt, x.n_chunks); txt.push_back('\t');
        sd::put_int(txt, (int64_t)(x.best_key >> 16)); txt.push_back('\t');
        txt.append(ts.tnames[(size_t)(x.best_key & 0xffffu)]); txt.push_back('\n');
    }
    if (so.tsv_out) {
        const int fd = ::open(so.tsv_out, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        bool ok = fd >= 0;
        for (size_t at = 0; ok && at < txt.size();) {
            const ssize_t w = ::write(fd, txt.data() + at, txt.size() - at);
            if (w <= 0) ok = false; else at += (size_t)w;
        }
        if (fd >= 0 && ::close(fd) != 0) ok = false;
        if (!ok) { err = std::string("cannot write ") + so.tsv_out; return SD_ERR_IO; }
    }
    int64_t read_bases = 0;
    for (int64_t l : lens) read_bases += l;
    stats[0] = (now_s() - t0) * 1e3;
    stats[2] = (double)read_bases; stats[3] = (double)bases; stats[4] = (double)n; stats[5] = (double)with_region;
    reads.swap(out);
    return SD_OK;
}

// The whole CLI job as one native call: FASTA files -> raw TSV + final TSV + _alt TSV, streamed per device batch
// (main.py:186-197 run + :168-184 convert_tsv without the round trip through the raw file).  devs: the device entries,
// one pipeline each ({p->device} for the single-device calls); their batches are dealt and consumed in order below.
// rank / world and *info (may be null): [0] first read, [1] one past the last read, [2] reads in the file, [3] chunks of
// this rank.  A read set that cannot be split by reads (one read holds more than half a rank's share, e.g. a single
// chromosome) gives SD_ERR_UNSUPPORTED before anything is written; the caller then shards by chunk range instead.
// Every thread the job starts is joined by its owner on every path, so running out of host memory is an error like any other.
static int run_files_impl(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank, int32_t world,
                          const char* raw_tsv_out, const char* final_tsv_out, const char* alt_tsv_out,
                          int32_t min_identity, int32_t second_best, const double* lr_coef, int64_t* info,
                          char* errbuf, size_t errlen, const char* records_out = nullptr,
                          const std::vector<int32_t>* dev_list = nullptr, const ScreenOpt* screen = nullptr) try {
    std::string err;
    int rc = validate_params(p, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    // SD_FLAG_PROFILE shapes the post-processing only: the pipelines (and their cache keys) never see it
    sd_params p_job = *p;
    const bool profile = (p_job.reserved[1] & SD_FLAG_PROFILE) != 0;
    p_job.reserved[1] &= ~SD_FLAG_PROFILE;
    p = &p_job;
    {
        std::lock_guard<std::mutex> lk(g_last_m);
        g_last_prof_on = false;
    }
    const std::vector<int32_t> devs = dev_list ? *dev_list : std::vector<int32_t>{p->device};
    const size_t nd = devs.size();
    if (!reads_fa || !monomers_fa || !raw_tsv_out || !final_tsv_out || !alt_tsv_out || !lr_coef || world < 1 || rank < 0 ||
        rank >= world)
        return SD_ERR_PARAM;
    if (records_out && world != 1) { set_err(errbuf, errlen, "the record stream is written by a single process"); return SD_ERR_PARAM; }
    if (nd > 1 && world != 1) return SD_ERR_PARAM;
    if (screen) {   // (checked before any device is touched)
        const char* why = records_out ? "--screen: the record stream holds whole reads" :
                          world != 1 ? "--screen: a screened job is not split over ranks" :
                          screen->thr < 0 ? "--screen: the threshold must be >= 0" :
                          p->overlap >= p->part_size ? "--screen needs overlap < part_size (the regions of a read must not overlap)" : nullptr;
        if (why) { set_err(errbuf, errlen, why); return SD_ERR_PARAM; }
    }
    const bool timing = getenv("SD_TIMING") != nullptr;
    const double t_begin = now_s();
    double t_prev = t_begin;
    auto lap = [&](const char* what) {
        if (!timing) return;
        const double t = now_s();
        std::fprintf(stderr, "[sd timing] %-34s %9.2f ms\n", what, (t - t_prev) * 1e3);
        t_prev = t;
    };
    const bool progress = (p->reserved[1] & SD_FLAG_PROGRESS) != 0 && rank == 0;
    JobInput in;
    rc = in.load(reads_fa, monomers_fa, p, rank, world, progress, info, err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    p_job.reserved[1] &= ~SD_FLAG_LENIENT;   // (the files are read: the pipelines and their cache keys never see the flag)
    lap("FASTA index + alphabet check");
    TemplateSet ts(in.monos);
    double screen_stats[6] = {0, 0, 0, 0, 0, 0};
    if (screen) {
        rc = screen_phase(in, ts, p, devs, *screen, in.reads, screen_stats, err);
        if (rc) { set_err(errbuf, errlen, err); return rc; }
        lap("screen: keys of every chunk, regions");
    }
    const std::vector<ReadView>& reads = in.reads;
    sd::PostProcessor pp;
    rc = pp.init(in.monos, min_identity, second_best != 0, lr_coef, devs[0], p->threads, err);
    if (rc == SD_OK && profile) rc = pp.enable_profile(err);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    OutFiles files;
    if (!files.open(raw_tsv_out, final_tsv_out, alt_tsv_out, p->threads)) {
        set_err(errbuf, errlen, std::string("cannot write ") + raw_tsv_out);
        return SD_ERR_IO;
    }
    if (screen && reads.empty()) {   // nothing passed: three empty files, an empty profile
        if (!files.close()) { set_err(errbuf, errlen, std::string("short write to ") + raw_tsv_out); return SD_ERR_IO; }
        std::lock_guard<std::mutex> lk(g_last_m);
        std::memset(g_last_run, 0, sizeof g_last_run);
        for (int i = 0; i < 4; ++i) g_last_run[20 + i] = screen_stats[i];
        g_last_screen[0] = (int64_t)screen_stats[4];
        g_last_screen[1] = 0;
        g_last_ndev = 0;
        if (profile) {
            g_last_prof = pp.profile();
            g_last_prof_text = pp.profile_text();
            g_last_prof_n = (int32_t)in.monos.size();
            g_last_prof_on = true;
        }
        return SD_OK;
    }
    sd::RecordsWriter rec_w;   // the rows once more as the binary record stream (sd_records.hpp), written as reads complete
    if (records_out) {
        rc = rec_w.open(records_out, *p, ts.tnames, err);
        if (rc) { set_err(errbuf, errlen, err); return rc; }
    }
    if (second_best && min_identity <= 0) files.reserve_alt(alt_size_estimate(in.monos, reads), t_begin);
    RowJob job;
    job.n_reads = (int32_t)reads.size();
    job.threads = p->threads;
    build_chunk_table(reads, p, job.table, job.nch);
    if (info) info[3] = (int64_t)job.table.size();
    lap("chunk table");
    job.row_off = static_cast<int64_t*>(std::calloc(reads.size() + 1, sizeof(int64_t)));
    if (!job.row_off) { set_err(errbuf, errlen, "out of host memory"); return SD_ERR_INTERNAL; }
    // identities of the final TSV in-stream, behind every batch's compaction (sd_ident.hip); template sets the kernel
    // does not take (and SD_IDENT_STREAM=0, developer A/B) leave them to the post-processing as in round 2
    sd_params pe = *p;
    apply_env_overrides(pe);
    std::atomic<bool> stream_ident{!(pe.reserved[1] & SD_FLAG_NO_STREAM_IDENT)};
    JobPipes jp(devs);
    rc = jp.open(p, second_best ? '2' : '1', ts, [&](sd_engine* e) {
        if (stream_ident && !engine_set_identity(e, pp.interleaved_seqs(), pp.own_interleaved(), second_best != 0)) stream_ident = false;
    }, err);
    for (size_t i = 0; i < nd; ++i)
        if (jp.cached[i] && !jp.pipes[i]->ident_ok) stream_ident = false;   // (its engines carry no identity tables)
    lap(jp.reused() ? "pipeline from the cache" : "engine (HIP runtime start, layout plan, tables, identity masks)");
    if (stream_ident) job.per = second_best ? (int)pp.interleaved_seqs().size() : 1;
    const bool slice_ident = second_best && !getenv("SD_IDENT_SLICES_OFF");
    std::vector<std::pair<size_t, size_t>> batches;
    if (rc == SD_OK) plan_job(job, jp.budget, devs, p, second_best != 0, slice_ident, jp.reused(), batches);
    lap("batch plan");
    const double t_setup = now_s() - t_begin;
    if (progress) std::fprintf(stderr, "Prepared reads\n");   // main.cpp:82
    TextStages text(reads, ts, pp, records_out ? &rec_w : nullptr, files, raw_tsv_out, progress, second_best != 0, timing, t_begin);
    text.start();
    // One driver per entry takes the lowest batch nobody has whenever its pipeline can take one (a pipeline pushes until
    // all its slots are busy, then waits for its oldest batch), and hands its batches' records to the assembler in batch
    // order (BatchTurns).  Every HIP call of a pipeline -- engines, streams, events, copies, identity slices -- is made on
    // its driver's thread; the text stages make none.
    if (rc == SD_OK)
        rc = jp.drive(reads, job.table, batches, text.rc, [&](size_t c0, size_t c1, std::vector<int>& slice_end) {
            if (slice_ident && stream_ident) ident_slices(job.table, c0, c1, slice_end);
        }, [&](Pipeline& pq, size_t c0, size_t c1, const sd_rec* recs, const int64_t* roff) {
            assemble(job, pq, c0, c1, recs, roff, text);
        }, [] {}, err);
    text.finish();
    if (rc == SD_OK && text.failed()) { rc = text.rc.load(); err = text.err; }
    if (!files.close() && rc == SD_OK) { rc = SD_ERR_IO; err = std::string("short write to ") + raw_tsv_out; }
    if (records_out && rc == SD_OK) rc = rec_w.close(err, records_out);
    report_stats(jp.pipes, jp.dealt, text, pp, batches.size(), t_setup);
    if (screen) {
        std::lock_guard<std::mutex> lk(g_last_m);
        for (int i = 0; i < 4; ++i) g_last_run[20 + i] = screen_stats[i];   // (sd_last_run_stats: screen wall ms, kernel ms, bases read, bases decomposed)
        g_last_screen[0] = (int64_t)screen_stats[4];
        g_last_screen[1] = (int64_t)screen_stats[5];
    }
    for (std::unique_ptr<Pipeline>& q : jp.pipes) q->ident_ok = stream_ident;
    jp.give_back(rc == SD_OK);
    if (rc) { set_err(errbuf, errlen, err); return rc; }
    if (profile) {
        if (timing) std::fprintf(stderr, "[sd timing] column profiles of the kept rows: %.1f ms\n", pp.t_profile * 1e3);
        std::lock_guard<std::mutex> lk(g_last_m);
        g_last_prof = pp.profile();
        g_last_prof_text = pp.profile_text();
        g_last_prof_n = (int32_t)in.monos.size();
        g_last_prof_on = true;
    }
    return SD_OK;
} catch (const std::bad_alloc&) {
    set_err(errbuf, errlen, "out of host memory");
    return SD_ERR_INTERNAL;
}


int sd_run_files_records(const char* reads_fa, const char* monomers_fa, const sd_params* p, const char* raw_tsv_out,
                         const char* final_tsv_out, const char* alt_tsv_out, const char* records_out, int32_t min_identity,
                         int32_t second_best, const double* lr_coef, char* errbuf, size_t errlen) {
    return run_files_impl(reads_fa, monomers_fa, p, 0, 1, raw_tsv_out, final_tsv_out, alt_tsv_out, min_identity, second_best,
                          lr_coef, nullptr, errbuf, errlen, records_out);
}

int sd_last_run_profile(int32_t* n_monomers, int64_t* n_counts, int64_t* text_bytes, char* text, uint64_t* counts) {
    std::lock_guard<std::mutex> lk(g_last_m);
    if (!g_last_prof_on) return SD_ERR_PARAM;
    if (n_monomers) *n_monomers = g_last_prof_n;
    if (n_counts) *n_counts = (int64_t)g_last_prof.size();
    if (text_bytes) *text_bytes = (int64_t)g_last_prof_text.size() + 1;
    if (text) std::memcpy(text, g_last_prof_text.c_str(), g_last_prof_text.size() + 1);
    if (counts) std::memcpy(counts, g_last_prof.data(), sizeof(uint64_t) * g_last_prof.size());
    return SD_OK;
}

void sd_last_run_stats(double out[24]) {
    std::lock_guard<std::mutex> lk(g_last_m);
    std::memcpy(out, g_last_run, sizeof g_last_run);
}

int sd_run_files(const char* reads_fa, const char* monomers_fa, const sd_params* p, const char* raw_tsv_out,
                 const char* final_tsv_out, const char* alt_tsv_out, int32_t min_identity, int32_t second_best,
                 const double* lr_coef, char* errbuf, size_t errlen) {
    return run_files_impl(reads_fa, monomers_fa, p, 0, 1, raw_tsv_out, final_tsv_out, alt_tsv_out, min_identity, second_best,
                          lr_coef, nullptr, errbuf, errlen);
}

int sd_run_files_range(const char* reads_fa, const char* monomers_fa, const sd_params* p, int32_t rank, int32_t world,
                       const char* raw_tsv_out, const char* final_tsv_out, const char* alt_tsv_out, int32_t min_identity,
                       int32_t second_best, const double* lr_coef, int64_t* info, char* errbuf, size_t errlen) {
    return run_files_impl(reads_fa, monomers_fa, p, rank, world, raw_tsv_out, final_tsv_out, alt_tsv_out, min_identity,
                          second_best, lr_coef, info, errbuf, errlen);
}

int sd_run_files_devices(const char* reads_fa, const char* monomers_fa, const sd_params* p, const int32_t* devices,
                         int32_t n_devices, const char* raw_tsv_out, const char* final_tsv_out, const char* alt_tsv_out,
                         const char* records_out, int32_t min_identity, int32_t second_best, const double* lr_coef,
                         char* errbuf, size_t errlen) {
    // the device list is checked completely before anything is started on any of its devices
    const int rc = check_device_list("sd_run_files_devices", p ? devices : nullptr, n_devices, errbuf, errlen);
    if (rc) return rc;
    sd_params q = *p;
    q.device = devices[0];
    const std::vector<int32_t> devs(devices, devices + n_devices);
    return run_files_impl(reads_fa, monomers_fa, &q, 0, 1, raw_tsv_out, final_tsv_out, alt_tsv_out, min_identity, second_best,
                          lr_coef, nullptr, errbuf, errlen, records_out, &devs);
}

int sd_run_files_screen(const char* reads_fa, const char* monomers_fa, const sd_params* p, const int32_t* devices,
                        int32_t n_devices, const char* raw_tsv_out, const char* final_tsv_out, const char* alt_tsv_out,
                        int32_t min_identity, int32_t second_best, const double* lr_coef, int32_t screen_thr,
                        const char* screen_tsv_out, const char* records_out, int64_t* counts, char* errbuf, size_t errlen) {
    if (!p) return SD_ERR_PARAM;
    const ScreenOpt so{screen_thr, screen_tsv_out};
    sd_params q = *p;
    std::vector<int32_t> devs{q.device};
    if (devices || n_devices > 0) {
        // parameter errors of the screen come before the device list is looked at (they need no device)
        if (records_out) { set_err(errbuf, errlen, "--screen: the record stream holds whole reads"); return SD_ERR_PARAM; }
        if (screen_thr < 0) { set_err(errbuf, errlen, "--screen: the threshold must be >= 0"); return SD_ERR_PARAM; }
        const int rc = check_device_list("sd_run_files_screen", devices, n_devices, errbuf, errlen);
        if (rc) return rc;
        devs.assign(devices, devices + n_devices);
        q.device = devices[0];
    }
    const int rc = run_files_impl(reads_fa, monomers_fa, &q, 0, 1, raw_tsv_out, final_tsv_out, alt_tsv_out, min_identity, second_best,
                                  lr_coef, nullptr, errbuf, errlen, records_out, &devs, &so);
    if (rc == SD_OK && counts) {
        std::lock_guard<std::mutex> lk(g_last_m);
        counts[0] = g_last_screen[0];
        counts[1] = g_last_screen[1];
        counts[2] = (int64_t)g_last_run[22];
        counts[3] = (int64_t)g_last_run[23];
    }
    return rc;
}

int sd_last_run_device_stats(int64_t* batches, double* busy_ms, int32_t cap) {
    std::lock_guard<std::mutex> lk(g_last_m);
    for (int i = 0; i < g_last_ndev && i < cap; ++i) {
        if (batches) batches[i] = g_last_dev_batches[i];
        if (busy_ms) busy_ms[i] = g_last_dev_busy[i];
    }
    return g_last_ndev;
}

// Host only (CPU test): the dealing of sd_run_files_devices against its contract -- plan_device_batches and BatchTurns
// as the job uses them, without a device.
int sd_multi_device_selftest(char* errbuf, size_t errlen) {
    auto fail = [&](const std::string& m) { set_err(errbuf, errlen, m); return SD_ERR_INTERNAL; };
    uint64_t rng = 0x2545F4914F6CDD1Dull;
    auto rnd = [&](uint64_t n) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint64_t)(rng % n); };
    // (1) plans: contiguous, covering, non-empty; at least 2N batches (and min_batches) where the chunks allow; no batch of
    // several chunks above the budget; equal chunks: batch sizes differ by at most one chunk
    for (int nd = 1; nd <= kMaxDevices; ++nd)
        for (int trial = 0; trial < 60; ++trial) {
            const size_t n = 1 + (size_t)rnd(trial < 20 ? 40 : 3000);
            const bool equal = rnd(2) == 0;
            std::vector<CRef> table(n);
            for (size_t c = 0; c < n; ++c) table[c] = CRef{(int32_t)(c / 7), 0, equal ? 5500 : (int32_t)(1 + rnd(5500))};
            const int64_t budget = rnd(3) == 0 ? (int64_t)1 << 40 : 5500 + (int64_t)rnd(2000000);
            const int minb = 1 + (int)rnd(9);
            std::vector<std::pair<size_t, size_t>> out;
            plan_device_batches(table, budget, minb, nd, out);
            size_t at = 0, lo = SIZE_MAX, hi = 0;
            for (const auto& b : out) {
                if (b.first != at || b.second <= b.first) return fail("device batches are not contiguous and non-empty");
                int64_t rows = 0;
                for (size_t c = b.first; c < b.second; ++c) rows += table[c].len;
                if (rows > budget && b.second - b.first > 1) return fail("a device batch of several chunks exceeds the budget");
                lo = std::min(lo, b.second - b.first);
                hi = std::max(hi, b.second - b.first);
                at = b.second;
            }
            if (at != n) return fail("device batches do not cover the table");
            if (out.size() < std::min(n, (size_t)std::max(2 * nd, minb)))
                return fail("fewer than 2 x " + std::to_string(nd) + " device batches although the chunks allow them");
            if (equal && budget >= (int64_t)5500 * (int64_t)n && hi > lo + 1) return fail("device batches of unequal share");
        }
    // (2) consumption: N threads deal batches dynamically (as the driver threads), each completes its batches in the order
    // it took them but after shuffled delays, in one or several slices; the consumer must see every slice in batch order
    for (int nd = 1; nd <= 6; ++nd)
        for (int trial = 0; trial < 4; ++trial) {
            const size_t nb = 2 * (size_t)nd + (size_t)rnd(40);
            std::vector<int> slices(nb), delay_us(nb);
            for (size_t b = 0; b < nb; ++b) { slices[b] = 1 + (int)rnd(3); delay_us[b] = (int)rnd(400); }
            BatchTurns turns;
            std::atomic<size_t> next{0};
            std::mutex seen_m;
            std::vector<std::pair<size_t, int>> seen;
            std::vector<std::thread> th;
            for (int i = 0; i < nd; ++i)
                th.emplace_back([&]() {
                    for (;;) {
                        const size_t b = next.fetch_add(1);
                        if (b >= nb) return;
                        std::this_thread::sleep_for(std::chrono::microseconds(delay_us[b]));
                        for (int sl = 0; sl < slices[b]; ++sl) {
                            if (turns.wait(b)) { std::lock_guard<std::mutex> g(seen_m); seen.emplace_back(b, sl); }
                            if (sl + 1 == slices[b]) turns.done(b);
                        }
                    }
                });
            for (std::thread& t : th) t.join();
            size_t k = 0;
            for (size_t b = 0; b < nb; ++b)
                for (int sl = 0; sl < slices[b]; ++sl, ++k)
                    if (k >= seen.size() || seen[k] != std::make_pair(b, sl)) return fail("batches consumed out of batch order");
            if (k != seen.size()) return fail("a batch slice was consumed twice");
        }
    // (3) a pipeline that fails on a batch that is not its last -- when it pops the batch to make room for the next, or
    // while it drains, or when it cannot take a batch at all -- ends the job: every driver returns (a driver that waited
    // for the failed batch's turn would hang the job; a watchdog aborts the turns after 20 s and reports it), the error is
    // returned, and what was consumed is a prefix of the batches in order that stops before the failed one.  A driver's
    // busy() runs once, after its last push and before its first drain pop, and not at all after a failed push.
    {
        struct ModelPipe {   // Pipeline's order of pops: FIFO, the oldest popped when a push finds all slots busy
            int slots = 3;
            size_t fail_pop = SIZE_MAX, fail_push = SIZE_MAX;
            std::deque<std::pair<size_t, std::function<void()>>> q;
            std::string log;   // 'p' a batch taken, 'x' a push failed, 'o' a pop of the driver's drain, 'b' busy()
            int inflight() const { return (int)q.size(); }
            int pop(bool drain = true) {
                if (drain) log += 'o';
                std::pair<size_t, std::function<void()>> x = std::move(q.front());
                q.pop_front();
                if (x.first == fail_pop) return SD_ERR_HIP;   // (its sink never runs)
                x.second();
                return SD_OK;
            }
            int push(size_t b, std::function<void()> sink) {
                if (b == fail_push) { log += 'x'; return SD_ERR_HIP; }
                if (inflight() == slots) {
                    const int e = pop(false);
                    if (e) { log += 'x'; return e; }
                }
                q.emplace_back(b, std::move(sink));
                log += 'p';
                return SD_OK;
            }
        };
        for (int trial = 0; trial < 120; ++trial) {
            const int nd = 1 + (int)rnd(6);
            const size_t nb = 2 * (size_t)nd + (size_t)rnd(30);
            const size_t bad = (size_t)rnd(nb - 1);   // never the last batch
            const bool on_push = rnd(4) == 0;
            BatchTurns turns;
            std::atomic<size_t> next{0};
            const std::atomic<int> sink_ok{SD_OK};
            std::mutex seen_m;
            std::vector<size_t> seen;
            std::vector<int> rcs((size_t)nd, SD_OK);
            std::vector<int64_t> dealt((size_t)nd, 0);
            std::vector<ModelPipe> pipes((size_t)nd);
            for (ModelPipe& mp : pipes) {
                mp.slots = 1 + (int)rnd(3);
                if (on_push) mp.fail_push = bad; else mp.fail_pop = bad;
            }
            std::mutex fin_m;
            std::condition_variable fin_cv;
            int finished = 0;
            std::vector<std::thread> th;
            for (int i = 0; i < nd; ++i)
                th.emplace_back([&, i]() {
                    ModelPipe& mp = pipes[(size_t)i];
                    auto push = [&](size_t b) {
                        if ((b * 2654435761u + (size_t)trial) & 4) std::this_thread::sleep_for(std::chrono::microseconds(50));
                        return mp.push(b, [&, b]() {
                            if (turns.wait(b)) { std::lock_guard<std::mutex> g(seen_m); seen.push_back(b); }
                            turns.done(b);
                        });
                    };
                    rcs[(size_t)i] = drive_entry(mp, turns, next, nb, sink_ok, push, dealt[(size_t)i], [&mp] { mp.log += 'b'; });
                    std::lock_guard<std::mutex> g(fin_m);
                    ++finished;
                    fin_cv.notify_all();
                });
            bool hung;
            {
                std::unique_lock<std::mutex> lk(fin_m);
                hung = !fin_cv.wait_for(lk, std::chrono::seconds(20), [&] { return finished == nd; });
            }
            if (hung) turns.abort();
            for (std::thread& t : th) t.join();
            if (hung) return fail("a driver waited forever for the turn of a batch its pipeline failed on");
            int failed = 0;
            for (int r : rcs) failed += r != SD_OK;
            if (failed != 1) return fail("a failed batch did not end the job with exactly that pipeline's error");
            for (size_t k = 0; k < seen.size(); ++k)
                if (seen[k] != k || k >= bad) return fail("after a failure, consumption was not an in-order prefix before the failed batch");
            for (const ModelPipe& mp : pipes) {
                const size_t at = mp.log.find('b'), npos = std::string::npos;
                if (mp.log.find('x') != npos ? at != npos : at == npos || mp.log.find('b', at + 1) != npos)
                    return fail("busy() did not run exactly once, or ran after a failed push");
                if (at != npos && (mp.log.find('p', at) != npos || mp.log.rfind('o', at) != npos))
                    return fail("busy() did not run between the last push and the first drain pop");
            }
        }
    }
    // (4) an aborted job: every waiter returns, nothing after the abort is consumed
    {
        BatchTurns turns;
        std::atomic<int> consumed{0};
        std::vector<std::thread> th;
        for (size_t b = 1; b <= 4; ++b)
            th.emplace_back([&, b]() { if (turns.wait(b)) ++consumed; });
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        turns.abort();
        for (std::thread& t : th) t.join();
        if (consumed.load() != 0) return fail("a batch was consumed after the job was aborted");
    }
    return SD_OK;
}

}  // extern "C"
