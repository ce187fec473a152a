// sd_final_dev.hpp -- the parts of the final selection (stringdecomposer/main.py:107-165, classify :95-104) on identity
// WORDS that host and device must compute alike, as plain C++ that compiles for both: the identity of a word, the test
// for a missing word, the segment length and edlib's split test, the (value, index) order of the maximum searches, and
// the end of the rule -- threshold, logit, the bytes of the row.  PostProcessor::select (sd_convert.hip) and the kernels
// of sd_final_dev.hip call these; the searches themselves are a left-to-right scan on the host and reductions over
// lanes on the device, both in the order of final_better.  A word is (dist << 16) | matches of one (segment, template)
// alignment (sd_ident.hip).
//
// Everything here is IEEE double arithmetic with separately rounded operations.  The compiler contracts a * b + c into
// a fused multiply-add for the device (v_fmac_f64) and not for the host (mulsd / addsd), which would change the logit's
// last bit and with it, at logit == 0, the '+' / '?' of a row -- and no test at the level of a stream would notice.  So
// contraction is switched off for every function of this header (#pragma clang fp contract(off) in each body).
#pragma once

#include <cstdint>

#include "../../include/sd_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SD_HD __host__ __device__
#else
#define SD_HD
#endif

namespace sd {

constexpr uint32_t FINAL_WORD_NONE = 0xffffffffu;   // a pair the identity kernels left out (sd_ident.hip: IDENT_NONE)

// The tables of a PostProcessor as the selection reads them (host or device pointers).
struct FinalTables {
    const int32_t* key_of_t = nullptr;    // DP template (m.., m'..) -> key
    const int32_t* kcol = nullptr;        // key -> the LAST interleaved template of that name
    const int32_t* key_of_il = nullptr;   // interleaved template (m0, m0', m1, ...) -> key
    int32_t n_tmpl = 0;                   // DP templates = interleaved templates = words per row with second_best
    int32_t n_keys = 0;
    int32_t min_identity = 0;
    int32_t second_best = 0;
    int32_t tmax = 1;                     // the longest template
    double coef[3] = {0, 0, 0};
};

// identity in percent of m '=' columns among `cols` columns: the arithmetic of main.py:47-60 (both are integers a double holds)
SD_HD inline double final_ident_ratio(double m, double cols) {
#pragma clang fp contract(off)
    double a = 0.0;
    a += m;
    a /= cols;
    return a * 100;
}

// identity in percent of a word, on the same integers
SD_HD inline double final_ident_percent(uint32_t w) {
    const uint32_t d = w >> 16, m = w & 0xffffu;
    return final_ident_ratio((double)m, (double)(d + m));
}

// a word that decides nothing: left out by the kernels, or dist + matches == 0, which no alignment has
SD_HD inline bool final_word_missing(uint32_t w) { return w == FINAL_WORD_NONE || w == 0u; }

// the segment read.seq[start : end + 1] of a row, as Python's slicing clamps it (read_len < 0: not clamped)
SD_HD inline int64_t final_seg_len(int64_t start, int64_t end, int64_t read_len) {
    const int64_t lim = read_len < 0 ? INT64_MAX : read_len;
    int64_t s0 = start > 0 ? start : 0;
    if (s0 > lim) s0 = lim;
    int64_t e1 = end + 1 > s0 ? end + 1 : s0;
    if (e1 > lim) e1 = lim;
    const int64_t n = e1 - s0;
    return n < 0x7fffffff ? n : 0x7fffffff;
}

// edlib walks a long alignment by Hirschberg's split (edlib_splits of sd_host.hpp is this function): the in-stream words
// were computed by its block traceback, so such a row is decided from the read text only
SD_HD inline bool final_seg_splits(int64_t qlen, int64_t tlen) {
    return 20ll * ((qlen + 63) / 64) * tlen + 8ll * tlen >= 1024 * 1024;
}

// (value, index) order of every maximum search of the selection: the greater value, on equal values the smaller index
// -- what "the first maximum" of a left-to-right scan is.  index < 0: no candidate.
SD_HD inline bool final_better(double v, int i, double v2, int i2) {
    if (i2 < 0) return i >= 0;
    if (i < 0) return false;
    return v > v2 || (v == v2 && i < i2);
}

// The end of the rule, from the row's identities: false if the row is filtered out (main.py:156), else the whole
// 80-byte row, padding zeroed.  sb / h0 / h1 = -1 and sbs / h0s / h1s = -1 where there is none (light mode: all).
SD_HD inline bool final_fill_row(const FinalTables& tb, int32_t read, const sd_rec& x, int ko, double score, int sb, double sbs,
                                 int h0, double h0s, int h1, double h1s, sd_final_row* f) {
#pragma clang fp contract(off)
    if (!(score >= (double)tb.min_identity)) return false;
    // classify (main.py:95-104): intercept + c1 * identity + c2 * (identity - second best) > 0
    const double logit = (1.0 * tb.coef[0] + score * tb.coef[1]) + (score - sbs) * tb.coef[2];
    unsigned char* z = reinterpret_cast<unsigned char*>(f);
    for (unsigned i = 0; i < sizeof(sd_final_row); ++i) z[i] = 0;   // (padding too: the same bytes for the same rows)
    f->read = read;
    f->start = x.start;
    f->end = x.end;
    f->best = ko; f->second = sb; f->homo_best = h0; f->homo_second = h1;
    f->ident = score; f->second_ident = sbs; f->homo_ident = h0s; f->homo_second_ident = h1s;
    f->reliable = logit > 0 ? 1 : 0;
    return true;
}

}  // namespace sd
