// sd_convert.hpp -- native post-processing (sd_convert.hip): raw monomer alignments of a batch of reads ->
// rows of final_decomposition.tsv / _alt.tsv (stringdecomposer/main.py:107-165).
#pragma once

#include <functional>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sd_hip.h"
#include "sd_final_dev.hpp"
#include "sd_host.hpp"

namespace sd {

struct PostRead {
    const char* name; size_t name_len;
    const char* seq; int64_t len;       // upper-case sequence (main.py:66-67)
    int64_t base = 0;                   // a region of a screened job: added to the starts and ends of the text
};

// Identities that came with the rows from the device (sd_ident.hip): one word (dist << 16) | matches per row (light
// mode: the row's own monomer) or per (row, interleaved monomer) pair, plain (id) / homopolymer-compressed (idh).
// src == nullptr: row b's words start at id + b * per.  Otherwise src[b] >= 0: record src[b] of id / idh; src[b] < 0:
// entry -1 - src[b] of xid / xidh (rows of a read that began in an earlier device batch).
struct IdentRef {
    const uint32_t* id = nullptr;
    const uint32_t* idh = nullptr;
    const int64_t* src = nullptr;
    const uint32_t* xid = nullptr;
    const uint32_t* xidh = nullptr;
};

// A malloc'ed array that grows by realloc (a large block moves by remapping its pages, not by a copy) and hands its block
// to a caller of the C-ABI, who frees it with sd_free.
template <class T>
struct HeapArray {
    T* p = nullptr;
    size_t n = 0, cap = 0;
    HeapArray() = default;
    HeapArray(const HeapArray&) = delete;
    HeapArray& operator=(const HeapArray&) = delete;
    ~HeapArray() { std::free(p); }
    bool resize(size_t m) {   // false: out of memory (the contents are kept)
        if (m > cap) {
            const size_t c = std::max(m, cap * 2);
            T* q = static_cast<T*>(std::realloc(p, std::max<size_t>(c, 1) * sizeof(T)));
            if (!q) return false;
            p = q;
            cap = c;
        }
        n = m;
        return true;
    }
    T* release() { T* q = p; p = nullptr; n = cap = 0; return q; }
};

class PostProcessor {
  public:
    // monomers in file order (names = first header token, sequences upper-case); device < 0: host identities
    int init(const std::vector<Seq>& monos, int min_identity, bool second_best, const double coef[3], int device,
             int threads, std::string& err);
    // rows[row_off[r] .. row_off[r+1]) = blocks of reads[r] (sd_rec.tmpl in the DP's template order: monomers,
    // then their reverse complements; read-global inclusive coordinates).  Appends the text of the final TSV
    // rows (main.py:157-160) and, with second_best, of the _alt rows (:161-165).
    // id / idh (optional): identities that came with the rows from the device (sd_ident.hip), one word
    // (dist << 16) | matches per row (light mode: the row's own monomer) or per (row, interleaved monomer) pair,
    // plain / homopolymer-compressed; rows without a computed word send the batch through the text-based path.
    int process(const PostRead* reads, size_t n_reads, const sd_rec* rows, const int64_t* row_off, TextBuf& fin,
                TextBuf& alt, std::string& err, const IdentRef* ident = nullptr);   // fin / alt are REPLACED
    // the same, as the slices the threads formatted (in order; the caller writes them without a gather copy)
    int process_parts(const PostRead* reads, size_t n_reads, const sd_rec* rows, const int64_t* row_off,
                      std::vector<std::string>& fin_parts, std::vector<TextBuf>& alt_parts, std::string& err,
                      const IdentRef* ident = nullptr);
    // the same selection as typed rows (the final mode of sd_stream): the kept blocks are APPENDED to `out` in block
    // order, their read = read0 + index into reads; with second_best their identities in key order to `alt` (nK each)
    int process_rows(const PostRead* reads, size_t n_reads, int32_t read0, const sd_rec* rows, const int64_t* row_off,
                     HeapArray<sd_final_row>& out, HeapArray<double>& alt, std::string& err,
                     const IdentRef* ident = nullptr);
    const std::vector<std::string>& key_names() const { return keys; }   // distinct names, first-occurrence order
    const std::vector<std::string>& interleaved_seqs() const { return il_seq; }   // m0, m0', m1, m1', ... (main.py:79-84)
    const std::vector<int32_t>& own_interleaved() const { return own_il32; }      // DP template -> interleaved index
    int tmpl_of_name(const std::string& nm) const;   // first template of that name in the DP's order, -1 if none
    std::vector<std::string> tname;                  // the DP's template names: m, ..., m', ...
    // The tables the selection reads, as pointers into this object (the device selection uploads them: sd_final_dev.hip).
    FinalTables final_tables() const;
    // The selection alone, on identity words (sd_final_select_host; what the kernels of sd_final_dev.hip must equal): read
    // r = rows[row_off[r] .. row_off[r + 1]); row b's words = id / idh + widx[b] * per (per = 1, the row's own monomer,
    // or with second_best every interleaved template, plain / homopolymer-compressed); read_len may be nullptr.  The
    // kept rows go to out in order, their offsets per read to out_off (n_reads + 1) and, with second_best, their key
    // identities to alt (room for every row).  A row the words do not decide -- a missing word, a segment edlib aligns by
    // Hirschberg's split -- is counted in *n_undecided and not kept.
    int select_words(const sd_rec* rows, const int64_t* row_off, int32_t n_reads, const int64_t* widx, const uint32_t* id,
                     const uint32_t* idh, const int64_t* read_len, sd_final_row* out, int64_t* out_off, double* alt,
                     int64_t* n_kept, int64_t* n_undecided) const;
    // Column profiles of the kept rows (SD_FLAG_PROFILE): SD_ERR_PARAM when a name repeats (a key must name one template).
    // prof: the forward monomers' counters (include/sd_hip.h), summed over every process* call since enable_profile.
    int enable_profile(std::string& err);
    bool profiling() const { return prof_on; }
    std::vector<uint64_t> profile(bool reset = false) {   // a copy (reset: and zero it, in one step)
        std::lock_guard<std::mutex> g(*prof_m);
        std::vector<uint64_t> v = prof;
        if (reset) std::fill(prof.begin(), prof.end(), 0);
        return v;
    }
    std::string profile_text() const;   // "name\tsequence\n" per monomer, file order
    // pairs a caller planned itself (a device-final stream's host pairs): query x against interleaved template il[x],
    // folded by profile_host into prof
    int profile_pairs(const char* const* q, const int32_t* qlen, const int32_t* il, int64_t n, std::string& err);
    double t_prepare = 0, t_identity = 0, t_format = 0, t_concat = 0, t_profile = 0;   // seconds spent in process(), by stage
    int64_t fallback_blocks = 0;     // blocks whose identities were computed here, not taken from the rows' words
    // set by a caller whose PostRead::seq are not filled in yet: called (once per process* call, before the text is
    // read) only when the text is needed -- fallback identities or profiles; returns SD_OK or an error with err set
    std::function<int(std::string&)> fetch_text;

  private:
    // a batch's identities as the selection reads them: the words that came with the rows (id) or the values
    // computed from the read text (vals: own / all interleaved templates, hvals: homopolymer-compressed)
    struct Batch {
        const IdentRef* ident = nullptr;
        bool id = false;
        int per = 1;
        RawVec<double> vals, hvals;
        std::vector<int32_t> read_of;    // block -> index into reads
        // the blocks as segments of the concatenated reads, and (profiling) which of them select kept
        std::vector<std::pair<const char*, int64_t>> spans;
        std::vector<int64_t> seg_start;
        std::vector<int32_t> seg_len;
        std::vector<uint8_t> kept;
        const uint32_t* words(int64_t b, bool homo) const {   // words of block b (plain / compressed)
            if (!ident->src) return (homo ? ident->idh : ident->id) + (size_t)b * (size_t)per;
            const int64_t sx = ident->src[b];
            return sx >= 0 ? (homo ? ident->idh : ident->id) + (size_t)sx * (size_t)per
                           : (homo ? ident->xidh : ident->xid) + (size_t)(-1 - sx) * (size_t)per;
        }
    };
    int prepare(const PostRead* reads, size_t n_reads, const sd_rec* rows, const int64_t* row_off, const IdentRef* ident,
                Batch& bt, std::string& err);
    // main.py:107-150 + classify (:95-104) for block b: false if the block is filtered out (main.py:156); f.read = the
    // block's index into reads.  kbuf (nK) receives the block's identities in key order with second_best; hbuf (T) is scratch
    bool select(const Batch& bt, const sd_rec* rows, int64_t b, double* kbuf, double* hbuf, sd_final_row& f) const;
    int profile_kept(const Batch& bt, const sd_rec* rows, std::string& err);   // the kept blocks into prof
    int identities(const std::vector<std::pair<const char*, int64_t>>& spans, const std::vector<int64_t>& seg_start,
                   const std::vector<int32_t>& seg_len, const int32_t* pair, bool homo, RawVec<double>& out,
                   std::string& err, bool host_only = false);
    std::vector<std::string> il_name, il_seq;        // interleaved m0, m0', m1, m1', ... (main.py:79-84)
    std::vector<std::string> keys;                   // distinct names in first-occurrence order
    std::vector<int> kcol;                           // key -> last interleaved index of that name
    std::vector<int> key_of_t, own_il_of_t, key_of_il;
    std::vector<int32_t> own_il32;
    int min_identity = 0;
    int tmax = 1;                                    // the longest template
    bool second_best = false;
    double coef[3] = {0, 0, 0};
    int device = -1;
    int threads = 1;
    bool prof_on = false;
    std::vector<uint64_t> prof;
    std::shared_ptr<std::mutex> prof_m = std::make_shared<std::mutex>();
};

}  // namespace sd
