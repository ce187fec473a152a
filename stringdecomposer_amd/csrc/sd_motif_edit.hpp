// sd_motif_edit.hpp -- IUPAC motif hits with insertions and deletions (--motif-edits), the parts host and device must
// compute alike, as plain C++ that compiles for both (in the manner of sd_motif.hpp): the rule, the compiled form of a
// request, the limits, the bit-vector step and the start of a hit.  sd_motif_edit.hip holds the kernels, the host form and
// the C-ABI (sd_motif_edit_*, include/sd_hip.h).
//
// Pattern, strands and byte rule are those of sd_motif.hpp: P of L IUPAC codes, 1 <= L <= 64; strand - is the reverse
// complement of P laid on the forward text; a pattern equal to its reverse complement is scanned on + only; N matches every
// byte, any other code only an upper-case A C G T of its set.  With a budget of K edits, 0 <= K <= 7: a text byte the code
// does not match costs 1 (substitution), an inserted text byte costs 1, a deleted pattern code costs 1 (an N too).
//
// d(j), 1 <= j <= n, is the smallest edit distance of P to any substring of the read that ends just before position j
// (Sellers' bottom row); d(0) = L, d(n + 1) is infinite.  End j is a hit when
//     d(j) <= K   and   d(j) <= d(j + 1)   and   (d(j) < d(j - 1) or d(j) = 0):
// the first end of every valley, and every exact occurrence.  Its start is the largest s with ed(P, read[s .. j)) = d(j)
// -- the shortest such substring, of L - d .. L + d bases -- found by the recurrence anchored at j and run backwards
// (motif_edit_start).  Records are in the order read, motif in request order, + before -, end.
//
// Locality.  A column started fresh (D[i] = i) L + K bases before j gives a value >= d(j), and d(j) itself whenever
// d(j) <= K: an alignment of cost <= K spans at most L + K bases.  The hit rule compares only values saturated at K + 1, so
// a scan that warms up over the L + K bases before its first end decides exactly as a scan from the read's first base,
// where the fresh column is the true state.  MOTIF_EDIT_WARM_MAX = 64 + 7 bases at worst.
//
// The column is Myers' bit vector with the pattern along the bits (Hyyro's form of the step): one word of 32 bits for
// L <= 32, one of 64 bits above.  The request is one match word per text class (A, C, G, T, other) and pattern-strand:
// bit i is set where code i matches the class; and the same for the reversed pattern, which the start needs.
#pragma once

#include "sd_motif.hpp"

namespace sd {

constexpr int MOTIF_EDIT_KMAX = 7;                                  // 0 <= K <= MOTIF_EDIT_KMAX
constexpr int MOTIF_EDIT_WARM_MAX = MOTIF_LMAX + MOTIF_EDIT_KMAX;   // bases a scan warms up over, at most
// A lane's stretch of consecutive ends, in words of 64; a workgroup of 256 lanes takes a tile of 256 stretches.  The
// stretch trades the warm-up (L + K bases per lane and pattern-strand, 71 at worst) against lanes per read and against hits
// per lane in the write pass.  Measured with 1, 2 and 4 words (profiles/motif_edits_timing.md): one word is ahead by 7 to
// 30 % over size and write together, and makes the tile that of --motif.
#ifndef SD_MOTIF_EDIT_STRETCH_WORDS
#define SD_MOTIF_EDIT_STRETCH_WORDS 1
#endif
constexpr int MOTIF_EDIT_STRETCH_WORDS = SD_MOTIF_EDIT_STRETCH_WORDS;
constexpr int MOTIF_EDIT_STRETCH = 64 * MOTIF_EDIT_STRETCH_WORDS;
constexpr int MOTIF_EDIT_LANES = 256;
constexpr int MOTIF_EDIT_TILE_WORDS = MOTIF_EDIT_LANES * MOTIF_EDIT_STRETCH_WORDS;
constexpr int64_t MOTIF_EDIT_TILE = 64 * (int64_t)MOTIF_EDIT_TILE_WORDS;
constexpr int MOTIF_EDIT_PB = 16;                                   // pattern-strands a workgroup takes
// Workgroups of one launch of the size or the write kernel.  A workgroup is at most MOTIF_EDIT_TILE x MOTIF_EDIT_PB ends x
// pattern-strands, each one step of the column plus its share of the warm-up (at most 1 + 71 / MOTIF_EDIT_STRETCH).  A step
// is four to five times a Hamming start, so MOTIF_LAUNCH_WORK does not carry over.  Rate of the size kernel on an MI355X
// (profiles/motif_edits_timing.md): 4.2e11 to 5.2e11 steps per second, warm-up not counted, so a launch of 2^30 steps is
// about 2 ms (measured: 1.4 ms).  The bound must not be much smaller: the step is a dependent chain that needs many waves
// per SIMD, and launches of 2^28 steps -- four workgroups per compute unit -- took 1.6 to 1.9 times as long in all.
constexpr int64_t MOTIF_EDIT_LAUNCH_WG = ((int64_t)1 << 30) / (MOTIF_EDIT_TILE * MOTIF_EDIT_PB);
constexpr int64_t MOTIF_EDIT_LAUNCH_WORK = MOTIF_EDIT_LAUNCH_WG * MOTIF_EDIT_TILE * MOTIF_EDIT_PB;
constexpr int MOTIF_EDIT_CLASSES = 5;                               // A C G T other
constexpr int MOTIF_EDIT_WORDS = 2 * MOTIF_EDIT_CLASSES;            // match words of a pattern-strand: forward, then reversed

// The five match words of a pattern-strand (or of its reversal), by name so that they stay in registers -- on the device
// scalar ones: they are the same in every lane -- and the word of the class of a base given by its plane bits.
template <class W>
struct MotifEditEq {
    W a, c, g, t, other;
};
template <class W>
SD_HD inline MotifEditEq<W> motif_edit_words(const uint64_t* w) {
    return MotifEditEq<W>{(W)motif_request_word(w), (W)motif_request_word(w + 1), (W)motif_request_word(w + 2), (W)motif_request_word(w + 3),
                          (W)motif_request_word(w + 4)};
}
template <class W>
SD_HD inline W motif_edit_eq(const MotifEditEq<W>& eq, bool lo, bool hi, bool valid) {
    return valid ? (hi ? (lo ? eq.t : eq.g) : (lo ? eq.c : eq.a)) : eq.other;
}

// The column: vertical deltas of D[1 .. L] as two bit vectors and the bottom value.
template <class W>
struct MotifEditCol {
    W pv, mv;
    int score;
};
template <class W>
SD_HD inline MotifEditCol<W> motif_edit_fresh(int L) { return MotifEditCol<W>{(W)~(W)0, (W)0, L}; }
// One base: eq = the match word of its class.  top = the horizontal delta of row 0: 0 for the search (a match may start
// anywhere), 1 for the anchored recurrence.
template <class W>
SD_HD inline void motif_edit_step(MotifEditCol<W>& c, W eq, int L, W top) {
    const W xv = eq | c.mv;
    const W xh = (W)((((W)(eq & c.pv) + c.pv) ^ c.pv) | eq);
    W ph = c.mv | (W)~(xh | c.pv);
    W mh = c.pv & xh;
    c.score += (int)((ph >> (L - 1)) & 1) - (int)((mh >> (L - 1)) & 1);
    ph = (W)(ph << 1) | top;
    mh = (W)(mh << 1);
    c.pv = mh | (W)~(xv | ph);
    c.mv = ph & xv;
}
SD_HD inline int motif_edit_sat(int score, int K) { return score > K ? K + 1 : score; }
// is the end whose value is s1 a hit, s2 the value before it and s0 the one behind it (all saturated at K + 1)
SD_HD inline bool motif_edit_is_hit(int s2, int s1, int s0, int K) { return s1 <= K && s1 <= s0 && (s1 < s2 || s1 == 0); }

// The start of the hit that ends just before position j (j bases of the read lie before it): the recurrence anchored at j
// over the reversed pattern and the bases j - 1, j - 2, ...; after t bases its bottom value is ed(P, read[j - t .. j)).
// d(j) is the least of them over t <= L + K, and the smallest such t is the matched length; t - L bounds the value from
// below, so the walk ends once t - L reaches the best value: at most L + d(j) bases, never before the read's first.
// eq_rev(p) -> the match word of the reversed pattern for base p.
template <class W, class Eq>
SD_HD inline void motif_edit_start(int L, int K, int64_t j, Eq&& eq_rev, int* length, int* edits) {
    MotifEditCol<W> c = motif_edit_fresh<W>(L);
    int best = L, len = 0;
    const int tmax = j < L + K ? (int)j : L + K;
    for (int t = 1; t <= tmax && t - L < best; ++t) {
        motif_edit_step<W>(c, eq_rev(j - t), L, (W)1);
        if (c.score < best) { best = c.score; len = t; }
    }
    *length = len;
    *edits = best;
}

// The scan of the ends whose last base p lies in [a, b) of a read of n bases given as its planes (sd_autocorr.hpp):
// on_hit(p) for every hit, p ascending.  The column starts fresh L + K bases before a, or at the read's first base, and
// runs one base past the stretch for d(j + 1); behind the read's last base the value is infinite.  Only bases of the read
// are touched: plane words 0 .. (n - 1) / 64.
template <class W, class F>
SD_HD inline void motif_edit_scan(const uint64_t* lo, const uint64_t* hi, const uint64_t* v, int64_t n, int64_t a, int64_t b,
                                  const MotifEditEq<W>& eq, int L, int K, F&& on_hit) {
    if (a >= n) return;
    const int64_t first = a > L + K ? a - (L + K) : 0, last = b < n ? b : n;
    MotifEditCol<W> c = motif_edit_fresh<W>(L);
    int s2 = K + 1, s1 = K + 1;   // the values of the two ends before p; before the read's first base: L > K
    uint64_t wl = 0, wh = 0, wv = 0;
    for (int64_t p = first; p <= last; ++p) {
        int s0 = K + 1;
        if (p < n) {
            if (p == first || (p & 63) == 0) { wl = lo[p >> 6]; wh = hi[p >> 6]; wv = v[p >> 6]; }
            const int bit = (int)(p & 63);
            motif_edit_step<W>(c, motif_edit_eq<W>(eq, (wl >> bit) & 1, (wh >> bit) & 1, (wv >> bit) & 1), L, (W)0);
            s0 = motif_edit_sat(c.score, K);
        }
        if (p > a && motif_edit_is_hit(s2, s1, s0, K)) on_hit(p - 1);
        s2 = s1;
        s1 = s0;
    }
}
// the match word of base p for motif_edit_start, from the planes and the five words of the reversed pattern
template <class W>
SD_HD inline W motif_edit_eq_at(const uint64_t* lo, const uint64_t* hi, const uint64_t* v, int64_t p, const MotifEditEq<W>& eq) {
    const int bit = (int)(p & 63);
    return motif_edit_eq<W>(eq, (lo[p >> 6] >> bit) & 1, (hi[p >> 6] >> bit) & 1, (v[p >> 6] >> bit) & 1);
}

// tiles of a read of n bases: one workgroup's 256 stretches; a read without bases has none
SD_HD inline int64_t motif_edit_tiles(int64_t n) { return (n + MOTIF_EDIT_TILE - 1) / MOTIF_EDIT_TILE; }

// ---- the compiled form of a request (host) -----------------------------------------------------------------------------
struct MotifEditSet {
    int32_t K = 0;
    MotifSet set;                 // pattern-strands in canonical order (sd_motif.hpp), compiled with no mismatches
    std::vector<uint64_t> eq;     // MOTIF_EDIT_WORDS per pattern-strand
};

inline bool motif_edit_compile(const char* const* patterns, int64_t n_motifs, int64_t K, MotifEditSet& out, std::string& err) {
    out = MotifEditSet();
    if (K < 0 || K > MOTIF_EDIT_KMAX) { err = "edits = " + std::to_string(K) + ", must be 0 .. " + std::to_string(MOTIF_EDIT_KMAX); return false; }
    if (!motif_compile(nullptr, patterns, n_motifs, 0, out.set, err)) return false;
    out.K = (int32_t)K;
    for (const MotifStrand& q : out.set.ps) {
        if (q.npos <= K) {
            err = "motif 'motif " + std::to_string(q.motif) + "': " + std::to_string(q.npos) + " constrained positions with " +
                  std::to_string(K) + " edits allowed: it would hit everywhere";
            return false;
        }
        const uint64_t all = q.L == 64 ? ~(uint64_t)0 : (((uint64_t)1 << q.L) - 1);
        uint64_t w[MOTIF_EDIT_CLASSES] = {all, all, all, all, all};
        for (int x = 0; x < q.npos; ++x) {
            const uint32_t p = out.set.pos[(size_t)(q.pos_off + x)];
            const uint64_t bit = (uint64_t)1 << (p & 63);
            const int set = (int)(p >> 8) & 15;
            for (int c = 0; c < 4; ++c)
                if (!((set >> c) & 1)) w[c] &= ~bit;
            w[4] &= ~bit;
        }
        for (int c = 0; c < MOTIF_EDIT_CLASSES; ++c) out.eq.push_back(w[c]);
        for (int c = 0; c < MOTIF_EDIT_CLASSES; ++c) {
            uint64_t r = 0;
            for (int i = 0; i < q.L; ++i)
                if ((w[c] >> i) & 1) r |= (uint64_t)1 << (q.L - 1 - i);
            out.eq.push_back(r);
        }
    }
    return true;
}

}  // namespace sd
