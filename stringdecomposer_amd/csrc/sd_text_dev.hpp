// sd_text_dev.hpp -- the text of the three row kinds (<out>_raw.tsv, <out>.tsv, <out>_alt.tsv) as plain C++ that compiles
// for host and device: for each kind a length function and a write function, one text for the kernels of
// sd_text_dev.hip and their host twin (sd_text_final_host / sd_text_raw_host).  The bytes are those of the formatters
// that exist: sd::format_rows (sd_host.hpp) for a raw row, formats.format_final / format_alt of formats.final_rows for
// the other two.  Integers print as put_int does (the whole int64 range), identities as put_fixed2 does: "%.2f" of the
// exact binary value, ties to even, from m * 100 >> sh in 64-bit integers -- no printf, no floating point.  That holds
// for every finite |v| < 2^40; anything else (infinity, NaN, |v| >= 2^40) goes to snprintf on the host, as put_fixed2
// does, and is COUNTED on the device, which has no snprintf: the length functions report such values and the device
// calls refuse the job (SD_ERR_UNSUPPORTED) before a byte is written.  No row the library produces holds one.
//
// A write function does not take a pointer: it takes the text position of its row and a TextWindow, which keeps the
// bytes of positions [lo, hi) and drops the others.  The host writes through a window over the whole text; a workgroup
// writes through a window over the tile it has staged in LDS, so a row longer than a tile comes out piece by piece.
//
// Every position is int64: the text of one call may exceed 4 GB.  That case is NOT tested (the largest tested text is
// the 297 MB of the timing note).
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sd_hip.h"
#include "sd_final_dev.hpp"

namespace sd {

// n byte strings back to back: name i = bytes[off[i] .. off[i + 1]) (host or device pointers)
struct TextNames {
    const char* bytes = nullptr;
    const int64_t* off = nullptr;
    int32_t n = 0;
};
SD_HD inline int64_t text_name_len(const TextNames& t, int32_t i) { return t.off[i + 1] - t.off[i]; }

// the bytes of text positions [lo, hi); position p lies at base[p - org]
struct TextWindow {
    char* base;
    int64_t org, lo, hi;
    SD_HD void set(int64_t p, char c) const {
        if (p >= lo && p < hi) base[p - org] = c;
    }
    SD_HD void copy(int64_t p, const char* s, int64_t n) const {
        const int64_t a = p > lo ? p : lo, b = p + n < hi ? p + n : hi;
        if (a >= b) return;
#if defined(__HIP_DEVICE_COMPILE__)
        for (int64_t x = a; x < b; ++x) base[x - org] = s[x - p];
#else
        std::memcpy(base + (a - org), s + (a - p), (size_t)(b - a));
#endif
    }
};

// ---- integers (put_int of sd_host.hpp) ------------------------------------------------------------------------------
SD_HD inline uint64_t text_abs(int64_t v) { return v < 0 ? (uint64_t)(-(v + 1)) + 1u : (uint64_t)v; }
SD_HD inline int text_digits(uint64_t u) {
    int n = 1;
    while (u >= 10) { u /= 10; ++n; }
    return n;
}
SD_HD inline int text_int_len(int64_t v) { return text_digits(text_abs(v)) + (v < 0 ? 1 : 0); }
template <class W>
SD_HD inline int64_t text_put_int(const W& w, int64_t p, int64_t v) {
    const int n = text_int_len(v);
    uint64_t u = text_abs(v);
    int64_t q = p + n;
    do { w.set(--q, (char)('0' + u % 10)); u /= 10; } while (u);
    if (v < 0) w.set(p, '-');
    return p + n;
}

// ---- identities (put_fixed2 of sd_host.hpp) -------------------------------------------------------------------------
SD_HD inline uint64_t text_bits(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}
// finite and |v| < 2^40: the integer path
SD_HD inline bool text_fixed2_plain(double v) { return (int)((text_bits(v) >> 52) & 0x7ff) < 1023 + 40; }
// round(100 |v|), ties to even, of a plain value: |v| = m * 2^-sh exactly, 13 <= sh, m * 100 < 2^60
SD_HD inline uint64_t text_fixed2_q(double v) {
    const uint64_t bits = text_bits(v);
    const int ex = (int)((bits >> 52) & 0x7ff);
    uint64_t m = bits & ((1ull << 52) - 1);
    int sh;
    if (ex) { m |= 1ull << 52; sh = 1075 - ex; } else sh = 1074;
    if (sh >= 64) return 0;   // 100 |v| < 2^-4
    const uint64_t num = m * 100u;
    uint64_t q = num >> sh;
    const uint64_t rem = num & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    return q;
}
// bytes of "%.2f"; *odd is counted up for a value the integer path does not take (and the device cannot print)
SD_HD inline int text_fixed2_len(double v, int* odd) {
    if (text_fixed2_plain(v)) return text_digits(text_fixed2_q(v) / 100) + 3 + (int)(text_bits(v) >> 63);
    ++*odd;
#if defined(__HIP_DEVICE_COMPILE__)
    return 0;
#else
    return std::snprintf(nullptr, 0, "%.2f", v);
#endif
}
template <class W>
SD_HD inline int64_t text_put_fixed2(const W& w, int64_t p, double v) {
    if (text_fixed2_plain(v)) {
        uint64_t q = text_fixed2_q(v);
        const int neg = (int)(text_bits(v) >> 63);
        const int n = text_digits(q / 100) + 3 + neg;
        int64_t at = p + n;
        w.set(--at, (char)('0' + q % 10)); q /= 10;
        w.set(--at, (char)('0' + q % 10)); q /= 10;
        w.set(--at, '.');
        do { w.set(--at, (char)('0' + q % 10)); q /= 10; } while (q);
        if (neg) w.set(p, '-');
        return p + n;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    return p;   // (never reached by a job the size call accepted)
#else
    char b[400];
    const int n = std::snprintf(b, sizeof b, "%.2f", v);
    w.copy(p, b, n);
    return p + n;
#endif
}

template <class W>
SD_HD inline int64_t text_put_name(const W& w, int64_t p, const TextNames& t, int32_t i) {
    const int64_t n = text_name_len(t, i);
    w.copy(p, t.bytes + t.off[i], n);
    return p + n;
}

// ---- a raw row (sd::format_rows): read, template, start, end, score ".000000", start - prev_end, end - start ---------
SD_HD inline bool text_raw_ok(const TextNames& T, const sd_rec& r) { return r.tmpl >= 0 && r.tmpl < T.n; }
SD_HD inline int64_t text_raw_len(const TextNames& R, const TextNames& T, int32_t read, const sd_rec& r, int32_t prev_end) {
    return text_name_len(R, read) + text_name_len(T, r.tmpl) + text_int_len(r.start) + text_int_len(r.end) + text_int_len(r.score) +
           text_int_len((int64_t)r.start - prev_end) + text_int_len((int64_t)r.end - r.start) + 14;
}
template <class W>
SD_HD inline int64_t text_raw_put(const W& w, int64_t p, const TextNames& R, const TextNames& T, int32_t read, const sd_rec& r,
                                  int32_t prev_end) {
    p = text_put_name(w, p, R, read);
    w.set(p++, '\t');
    p = text_put_name(w, p, T, r.tmpl);
    w.set(p++, '\t');
    p = text_put_int(w, p, r.start);
    w.set(p++, '\t');
    p = text_put_int(w, p, r.end);
    w.set(p++, '\t');
    p = text_put_int(w, p, r.score);
    w.copy(p, ".000000\t", 8);
    p += 8;
    p = text_put_int(w, p, (int64_t)r.start - prev_end);
    w.set(p++, '\t');
    p = text_put_int(w, p, (int64_t)r.end - r.start);
    w.set(p++, '\n');
    return p;
}

// ---- a final row: twelve columns.  K = the key names with "None" behind them (K.n = n_keys + 1) ----------------------
SD_HD inline int32_t text_key(const TextNames& K, int32_t k) { return k >= 0 ? k : K.n - 1; }
SD_HD inline bool text_final_ok(const TextNames& R, const TextNames& K, const sd_final_row& f) {
    const int32_t nk = K.n - 1;
    return f.read >= 0 && f.read < R.n && f.best >= 0 && f.best < nk && f.second >= -1 && f.second < nk && f.homo_best >= -1 &&
           f.homo_best < nk && f.homo_second >= -1 && f.homo_second < nk;
}
SD_HD inline int64_t text_final_len(const TextNames& R, const TextNames& K, const sd_final_row& f, int* odd) {
    return text_name_len(R, f.read) + text_name_len(K, f.best) + text_name_len(K, text_key(K, f.second)) +
           text_name_len(K, text_key(K, f.homo_best)) + text_name_len(K, text_key(K, f.homo_second)) + text_int_len(f.start) +
           text_int_len(f.end) + text_fixed2_len(f.ident, odd) + text_fixed2_len(f.second_ident, odd) +
           text_fixed2_len(f.homo_ident, odd) + text_fixed2_len(f.homo_second_ident, odd) + 13;
}
template <class W>
SD_HD inline int64_t text_final_put(const W& w, int64_t p, const TextNames& R, const TextNames& K, const sd_final_row& f) {
    p = text_put_name(w, p, R, f.read);
    w.set(p++, '\t');
    p = text_put_name(w, p, K, f.best);
    w.set(p++, '\t');
    p = text_put_int(w, p, f.start);
    w.set(p++, '\t');
    p = text_put_int(w, p, f.end);
    w.set(p++, '\t');
    p = text_put_fixed2(w, p, f.ident);
    w.set(p++, '\t');
    p = text_put_name(w, p, K, text_key(K, f.second));
    w.set(p++, '\t');
    p = text_put_fixed2(w, p, f.second_ident);
    w.set(p++, '\t');
    p = text_put_name(w, p, K, text_key(K, f.homo_best));
    w.set(p++, '\t');
    p = text_put_fixed2(w, p, f.homo_ident);
    w.set(p++, '\t');
    p = text_put_name(w, p, K, text_key(K, f.homo_second));
    w.set(p++, '\t');
    p = text_put_fixed2(w, p, f.homo_second_ident);
    w.set(p++, '\t');
    w.set(p++, f.reliable ? '+' : '?');
    w.set(p++, '\n');
    return p;
}

// ---- an _alt line of a final row: read, key k, start, end, "%.2f" of alt[k], '*' for the row's own key else '-' -------
// what the n_keys lines of a row share: read name, start, end, five tabs, the mark, the newline
SD_HD inline int64_t text_alt_common(const TextNames& R, const sd_final_row& f) {
    return text_name_len(R, f.read) + text_int_len(f.start) + text_int_len(f.end) + 7;
}
SD_HD inline int64_t text_alt_line_len(int64_t common, const TextNames& K, int32_t k, double v, int* odd) {
    return common + text_name_len(K, k) + text_fixed2_len(v, odd);
}
template <class W>
SD_HD inline int64_t text_alt_put(const W& w, int64_t p, const TextNames& R, const TextNames& K, const sd_final_row& f, int32_t k,
                                  double v) {
    p = text_put_name(w, p, R, f.read);
    w.set(p++, '\t');
    p = text_put_name(w, p, K, k);
    w.set(p++, '\t');
    p = text_put_int(w, p, f.start);
    w.set(p++, '\t');
    p = text_put_int(w, p, f.end);
    w.set(p++, '\t');
    p = text_put_fixed2(w, p, v);
    w.set(p++, '\t');
    w.set(p++, k == f.best ? '*' : '-');
    w.set(p++, '\n');
    return p;
}

}  // namespace sd
