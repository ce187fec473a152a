// sd_motif.hpp -- IUPAC motif hits on both strands of every read (--motif), the parts host and device must compute alike,
// as plain C++ that compiles for both (in the manner of sd_autocorr.hpp): the IUPAC table, the compiled form of a request,
// the limits, and the word step.  sd_motif.hip holds the kernels, the host form and the C-ABI (sd_motif_*, include/sd_hip.h).
//
// A motif is a pattern P of L IUPAC codes, 1 <= L <= 64 (lower case folded).  N is unconstrained: it matches every text
// byte.  Every other code is a set of bases and matches a text byte only when the byte is an upper-case A C G T of the set
// (the byte rule of sd_autocorr.hpp: a byte outside ACGT matches nothing constrained).  With a budget of E mismatches,
// 0 <= E <= 7, position i of a read of n bases is a hit on strand + when i + L <= n and at most E constrained positions j
// have T[i + j] outside the set of P[j]; it is a hit on strand - by the same rule against the reverse complement of P.  A
// pattern equal to its reverse complement is scanned on + only.  Every hit is reported, overlapping ones included.
//
// The text is read as the bit planes lo | hi | valid of sd_autocorr.hpp (zeros behind the read's end, one zero word behind
// each read).  L <= 64, so the 64 starts of word t need word t and word t + 1 and nothing else.
#pragma once

#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "sd_autocorr.hpp"

namespace sd {

constexpr int MOTIF_LMAX = 64;                          // 1 <= L <= MOTIF_LMAX
constexpr int MOTIF_EMAX = 7;                           // 0 <= E <= MOTIF_EMAX
constexpr int MOTIF_MAX = 1024;                         // motifs of a request
constexpr int64_t MOTIF_ITEMS_MAX = (int64_t)1 << 24;   // (read-tile, pattern-strand) items of a call
constexpr int64_t MOTIF_HITS_MAX = (int64_t)1 << 28;    // hits of a call: 4 GB of records
constexpr int MOTIF_TILE_WORDS = 256;                   // a workgroup's stretch of a read: one word per lane
constexpr int64_t MOTIF_TILE = 64 * MOTIF_TILE_WORDS;   // = 16 384 starts
constexpr int MOTIF_PB = 16;                            // pattern-strands a workgroup takes with its words in registers
// Workgroups of one launch of the size or the write kernel.  A workgroup is at most MOTIF_TILE x MOTIF_PB start x
// pattern-strand products (of at most 64 positions each), so a launch is at most 2^30 of them -- well under a millisecond
// on an MI355X -- whatever the reads and the request are: a 200-Mb sequence with 2 048 pattern-strands becomes some 400
// short launches per pass, never one long one.  (The scan between the passes is one launch of one workgroup whose length
// grows with the items of the call: this bound does not cover it.)
constexpr int64_t MOTIF_LAUNCH_WG = 4096;
constexpr int64_t MOTIF_LAUNCH_WORK = MOTIF_LAUNCH_WG * MOTIF_TILE * MOTIF_PB;

// ---- the IUPAC table: a code as a set of bases, bit c for the base of plane code c (A = 0, C = 1, G = 2, T = 3) ----------
SD_HD inline int motif_set(uint8_t ch) {
    switch (ch >= 'a' && ch <= 'z' ? ch - 32 : ch) {
        case 'A': return 1;  case 'C': return 2;  case 'G': return 4;  case 'T': return 8;
        case 'R': return 5;  case 'Y': return 10; case 'S': return 6;  case 'W': return 9;
        case 'K': return 12; case 'M': return 3;  case 'B': return 14; case 'D': return 13;
        case 'H': return 11; case 'V': return 7;  case 'N': return 15;
        default: return 0;   // (U and everything else: refused)
    }
}
// the complement of a set: A <-> T, C <-> G, the four bits reversed
SD_HD inline int motif_set_complement(int s) { return ((s & 1) << 3) | ((s & 2) << 1) | ((s & 4) >> 1) | ((s & 8) >> 3); }

// A constrained position as the kernels take it: bits 0-5 j, 8-11 the set, 12-13 the kind, 16-18 the constants a b c of the
// kind's match word, a boolean function of lo, hi and valid:
//   ONE   (one base)     valid & (lo ^ a) & (hi ^ b)
//   TWO   (two bases)    valid & ((lo & a) ^ (hi & b) ^ c)      every pair of bases is a linear function of the code bits
//   THREE (three bases)  valid & ~((lo ^ a) & (hi ^ b))         all but one base
enum { MOTIF_ONE = 1, MOTIF_TWO = 2, MOTIF_THREE = 3 };
SD_HD inline uint32_t motif_pos(int j, int set) {
    int n = (set & 1) + ((set >> 1) & 1) + ((set >> 2) & 1) + ((set >> 3) & 1), kind, a, b, c = 0;
    if (n == 2) {
        kind = MOTIF_TWO;
        c = set & 1;
        a = c ^ ((set >> 1) & 1);
        b = c ^ ((set >> 2) & 1);
    } else {
        const int one = n == 1 ? set : 15 ^ set;                        // the base that is in (ONE) or out (THREE)
        const int code = one == 1 ? 0 : one == 2 ? 1 : one == 4 ? 2 : 3;
        kind = n == 1 ? MOTIF_ONE : MOTIF_THREE;
        a = !(code & 1);   // lo ^ a is set where lo equals the code's bit
        b = !(code & 2);
    }
    return (uint32_t)j | (uint32_t)set << 8 | (uint32_t)kind << 12 | (uint32_t)a << 16 | (uint32_t)b << 17 | (uint32_t)c << 18;
}
SD_HD inline uint64_t motif_match(uint32_t p, uint64_t lo, uint64_t hi, uint64_t v) {
    const uint64_t a = (uint64_t)0 - ((p >> 16) & 1), b = (uint64_t)0 - ((p >> 17) & 1), c = (uint64_t)0 - ((p >> 18) & 1);
    const int kind = (int)(p >> 12) & 3;
    if (kind == MOTIF_ONE) return v & (lo ^ a) & (hi ^ b);
    if (kind == MOTIF_TWO) return v & ((lo & a) ^ (hi & b) ^ c);
    return v & ~((lo ^ a) & (hi ^ b));
}

// bits j .. j + 63 of the 128 bits {next, cur}, 0 <= j <= 63.  On the device: v_alignbit on the 32-bit halves, the half
// index j >> 5 being uniform over the workgroup.
SD_HD inline uint64_t motif_shift(uint64_t cur, uint64_t next, int j) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t w0 = (uint32_t)cur, w1 = (uint32_t)(cur >> 32), w2 = (uint32_t)next, w3 = (uint32_t)(next >> 32);
    const uint32_t s = (uint32_t)j & 31;
    if (j & 32) return __builtin_amdgcn_alignbit(w2, w1, s) | (uint64_t)__builtin_amdgcn_alignbit(w3, w2, s) << 32;
    return __builtin_amdgcn_alignbit(w1, w0, s) | (uint64_t)__builtin_amdgcn_alignbit(w2, w1, s) << 32;
#else
    return j ? (cur >> j) | (next << (64 - j)) : cur;
#endif
}

// A word that the kernel reading it does not write (the request; in the write kernel also the counts and bases of the
// earlier passes): on the device read through the constant address space, so that the load
// is a scalar load wherever its address is uniform -- also behind the barriers and record stores of the write kernel, which
// the compiler would otherwise take for possible writers of it.
template <class T>
SD_HD inline T motif_request_word(const T* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const __attribute__((address_space(4))) T*)p;
#else
    return *p;
#endif
}

// planes of the mismatch counter: bit_length(E + 1)
SD_HD inline int motif_counter_planes(int E) { return E + 1 >= 8 ? 4 : E + 1 >= 4 ? 3 : E + 1 >= 2 ? 2 : 1; }

// The word step.  From the planes of word t (lo0 hi0 v0) and word t + 1 (lo1 hi1 v1) and the npos constrained positions of
// one pattern-strand: the hit word of the 64 starts of word t, and in cnt[0 .. B) the planes of their mismatch counts.  The
// count is a bit-sliced counter of B = bit_length(E + 1) planes that saturates at E1 = E + 1 -- a start that has reached
// E + 1 takes no further increment, so 64 mismatches at E = 7 are 8 and never wrap to 0 -- and a start is a hit when its
// count is not E + 1.  At E = 0 this is one plane and the step is cnt |= mismatch: one AND of the match words per position.
// The caller masks the starts with i + L <= n (autocorr_word_mask(t, 0, n - L + 1)).
template <int E1>
SD_HD inline uint64_t motif_word(const uint32_t* pos, int npos, uint64_t lo0, uint64_t hi0, uint64_t v0, uint64_t lo1, uint64_t hi1,
                                 uint64_t v1, uint64_t* cnt) {
    constexpr int B = E1 >= 8 ? 4 : E1 >= 4 ? 3 : E1 >= 2 ? 2 : 1;
    uint64_t c[B];
    for (int k = 0; k < B; ++k) c[k] = 0;
    for (int x = 0; x < npos; ++x) {
        const uint32_t p = motif_request_word(pos + x);
        const int j = (int)(p & 63);
        uint64_t carry = ~motif_match(p, motif_shift(lo0, lo1, j), motif_shift(hi0, hi1, j), motif_shift(v0, v1, j));
        if (E1 == 1) {
            c[0] |= carry;
        } else {
            uint64_t sat = ~(uint64_t)0;
            for (int k = 0; k < B; ++k) sat &= (E1 >> k) & 1 ? c[k] : ~c[k];
            carry &= ~sat;
            for (int k = 0; k < B; ++k) {
                const uint64_t t = c[k] & carry;
                c[k] ^= carry;
                carry = t;
            }
        }
    }
    uint64_t sat = ~(uint64_t)0;
    for (int k = 0; k < B; ++k) {
        sat &= (E1 >> k) & 1 ? c[k] : ~c[k];
        cnt[k] = c[k];
    }
    return ~sat;
}
// the mismatches of start `bit` from the counter planes
SD_HD inline int motif_count_at(const uint64_t* cnt, int B, int bit) {
    int m = 0;
    for (int k = 0; k < B; ++k) m |= (int)((cnt[k] >> bit) & 1) << k;
    return m;
}

// f(std::integral_constant<int, E + 1>) for the budget E
template <class F>
inline void motif_with_budget(int E, F&& f) {
    switch (E) {
        case 0: f(std::integral_constant<int, 1>{}); break;
        case 1: f(std::integral_constant<int, 2>{}); break;
        case 2: f(std::integral_constant<int, 3>{}); break;
        case 3: f(std::integral_constant<int, 4>{}); break;
        case 4: f(std::integral_constant<int, 5>{}); break;
        case 5: f(std::integral_constant<int, 6>{}); break;
        case 6: f(std::integral_constant<int, 7>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}

// tiles of a read of n bases: stretches of MOTIF_TILE_WORDS words; a read without bases has none
SD_HD inline int64_t motif_tiles(int64_t n) { return (autocorr_words(n) + MOTIF_TILE_WORDS - 1) / MOTIF_TILE_WORDS; }

// ---- the compiled form of a request (host) -----------------------------------------------------------------------------
// A pattern-strand: one pattern as it is laid against the text.  Motif m gives strand + and, unless it equals its reverse
// complement (palindrome), strand -, next to each other and in request order: the canonical order of the hits.
struct MotifStrand {
    int32_t L, motif, strand;   // strand: 0 = +, 1 = -
    int32_t pos_off, npos;      // its constrained positions in MotifSet::pos, j ascending
    int32_t palindrome;
};
struct MotifSet {
    int32_t E = 0, n_motifs = 0;
    std::vector<MotifStrand> ps;
    std::vector<uint32_t> pos;   // motif_pos
};

// patterns (and names, may be null: then not checked) -> set; false with the refusal in err
inline bool motif_compile(const char* const* names, const char* const* patterns, int64_t n_motifs, int64_t E, MotifSet& out, std::string& err) {
    out = MotifSet();
    if (E < 0 || E > MOTIF_EMAX) { err = "mismatches = " + std::to_string(E) + ", must be 0 .. " + std::to_string(MOTIF_EMAX); return false; }
    if (n_motifs < 1 || n_motifs > MOTIF_MAX) {
        err = std::to_string(n_motifs) + " motifs, must be 1 .. " + std::to_string(MOTIF_MAX) + " (MOTIF_MAX)";
        return false;
    }
    out.E = (int32_t)E;
    out.n_motifs = (int32_t)n_motifs;
    for (int64_t m = 0; m < n_motifs; ++m) {
        const std::string name = names && names[m] ? names[m] : "motif " + std::to_string(m);
        if (names) {
            bool ok = names[m] && names[m][0];
            for (const char* q = names[m]; ok && *q; ++q)
                ok = (*q >= 'A' && *q <= 'Z') || (*q >= 'a' && *q <= 'z') || (*q >= '0' && *q <= '9') || *q == '_' || *q == '.' || *q == '-';
            if (!ok) { err = "motif " + std::to_string(m) + ": a name must match [A-Za-z0-9_.-]+"; return false; }
            for (int64_t o = 0; o < m; ++o)
                if (name == names[o]) { err = "motif name '" + name + "' is given twice"; return false; }
        }
        const char* p = patterns ? patterns[m] : nullptr;
        int64_t L = 0;
        while (p && p[L]) ++L;
        if (L < 1 || L > MOTIF_LMAX) { err = "motif '" + name + "': " + std::to_string(L) + " codes, must be 1 .. " + std::to_string(MOTIF_LMAX); return false; }
        int fw[MOTIF_LMAX], rc[MOTIF_LMAX], constrained = 0;
        for (int64_t j = 0; j < L; ++j) {
            fw[j] = motif_set((uint8_t)p[j]);
            if (!fw[j]) { err = "motif '" + name + "': code '" + std::string(1, p[j]) + "' at position " + std::to_string(j) + " is not one of ACGTRYSWKMBDHVN"; return false; }
            constrained += fw[j] != 15;
        }
        if (constrained <= E) {
            err = "motif '" + name + "': " + std::to_string(constrained) + " constrained positions with " + std::to_string(E) +
                  " mismatches allowed: it would hit everywhere";
            return false;
        }
        bool pal = true;
        for (int64_t j = 0; j < L; ++j) {
            rc[j] = motif_set_complement(fw[L - 1 - j]);
            pal = pal && rc[j] == fw[j];
        }
        for (int s = 0; s < (pal ? 1 : 2); ++s) {
            MotifStrand q{(int32_t)L, (int32_t)m, s, (int32_t)out.pos.size(), constrained, pal ? 1 : 0};
            for (int64_t j = 0; j < L; ++j)
                if ((s ? rc : fw)[j] != 15) out.pos.push_back(motif_pos((int)j, (s ? rc : fw)[j]));
            out.ps.push_back(q);
        }
    }
    return true;
}

}  // namespace sd
