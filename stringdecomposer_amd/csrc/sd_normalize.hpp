// sd_normalize.hpp -- the lenient mode's rule for a sequence byte, as plain C++ that compiles for host and device: one
// text for the kernel of sd_normalize_dev.hip, for sd_normalize_host and for sd::FastaFile's lenient index.
//
//   a-z                      -> the upper-case letter
//   then R Y S W K M B D H V -> N        (the IUPAC codes of more than one base; N keeps the reference's meaning: an
//                                         ordinary symbol that matches itself only, main.cpp:190)
//   every other byte         stays: U, digits, '*', '-', a stray '\r' and bytes >= 0x80 are still reported by the checks
//                            that exist (FastaFile::validate, check_alphabet, the device packer), in their words.
//
// Four bytes per step, in one 32-bit word: a byte below 0x80 equals a constant iff (byte ^ constant) + 0x7f has its top
// bit clear, and with every byte below 0x80 no carry crosses a byte, so the sixteen comparisons of a word (a range for
// the case, ten codes, five bases) are a xor, an add and an and each.  The per-byte form is the same function on a word
// padded with 'A', which the rule leaves alone and no counter counts.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SD_NORM_HD __host__ __device__
#else
#define SD_NORM_HD
#endif

namespace sd {

// what a word (or a run of words) held: bytes folded from lower case, ambiguity codes turned into N, bytes that are
// still outside A C G T N afterwards
struct NormCount {
    uint32_t lower = 0, amb = 0, bad = 0;
};

// top bit of every byte of y7 (all bytes < 0x80) that differs from c
SD_NORM_HD inline uint32_t norm_ne(uint32_t y7, uint32_t c) { return (y7 ^ (c * 0x01010101u)) + 0x7F7F7F7Fu; }

SD_NORM_HD inline uint32_t norm_popc(uint32_t m) { return (uint32_t)__builtin_popcount(m); }

// the four bytes of x normalised; *lower, *amb, *bad: 0x80 in every byte that was folded / was a code / is still outside
// the alphabet
SD_NORM_HD inline uint32_t normalize_word(uint32_t x, uint32_t* lower, uint32_t* amb, uint32_t* bad) {
    const uint32_t H = 0x80808080u;
    const uint32_t hi = x & H, y = x & ~H;
    // 'a' <= byte <= 'z': 0x61 + 0x1f reaches the top bit, 0x7b + 0x05 does
    const uint32_t lo = (y + 0x1F1F1F1Fu) & ~(y + 0x05050505u) & ~hi & H;
    const uint32_t u = y ^ (lo >> 2);                       // a lower-case letter has bit 5 set: cleared
    const uint32_t ne_code = norm_ne(u, 'R') & norm_ne(u, 'Y') & norm_ne(u, 'S') & norm_ne(u, 'W') & norm_ne(u, 'K') &
                             norm_ne(u, 'M') & norm_ne(u, 'B') & norm_ne(u, 'D') & norm_ne(u, 'H') & norm_ne(u, 'V');
    const uint32_t ne_base = norm_ne(u, 'A') & norm_ne(u, 'C') & norm_ne(u, 'G') & norm_ne(u, 'T') & norm_ne(u, 'N');
    const uint32_t am = ~ne_code & ~hi & H;
    const uint32_t full = (am >> 7) * 0xFFu;                // 0xff in every byte that is a code
    *lower = lo;
    *amb = am;
    *bad = (ne_base | hi) & ~am & H;
    return ((u | hi) & ~full) | (0x4E4E4E4Eu & full);
}

SD_NORM_HD inline uint8_t normalize_byte(uint8_t c, NormCount& k) {
    uint32_t lo, am, bd;
    const uint32_t w = normalize_word(0x41414100u | c, &lo, &am, &bd);
    k.lower += lo >> 7;
    k.amb += am >> 7;
    k.bad += bd >> 7;
    return (uint8_t)w;
}

// would the rule change any of s[0, n)?  (the lenient index leaves a canonical single-line record in the mapping)
inline bool normalize_changes(const char* s, int64_t n) {
    int64_t i = 0;
    for (; i + 4 <= n; i += 4) {
        uint32_t x, lo, am, bd;
        std::memcpy(&x, s + i, 4);
        if (normalize_word(x, &lo, &am, &bd) != x) return true;
    }
    for (; i < n; ++i) {
        NormCount k;
        if (normalize_byte((uint8_t)s[i], k) != (uint8_t)s[i]) return true;
    }
    return false;
}

// out[0, n) = the rule applied to in[0, n) (out may equal in); the counts are added to k64[0..2]
inline void normalize_span(const char* in, char* out, int64_t n, uint64_t k64[3]) {
    int64_t i = 0;
    while (i + 4 <= n) {
        // (blocks of <= 2^20 words keep the 32-bit sums exact)
        const int64_t stop = i + ((n - i) / 4 < (1 << 20) ? (n - i) / 4 : (1 << 20)) * 4;
        uint32_t cl = 0, ca = 0, cb = 0;
        for (; i < stop; i += 4) {
            uint32_t x, lo, am, bd;
            std::memcpy(&x, in + i, 4);
            x = normalize_word(x, &lo, &am, &bd);
            std::memcpy(out + i, &x, 4);
            cl += norm_popc(lo);
            ca += norm_popc(am);
            cb += norm_popc(bd);
        }
        k64[0] += cl; k64[1] += ca; k64[2] += cb;
    }
    NormCount k;
    for (; i < n; ++i) out[i] = (char)normalize_byte((uint8_t)in[i], k);
    k64[0] += k.lower; k64[1] += k.amb; k64[2] += k.bad;
}

}  // namespace sd
