// sd_seam_dev.hpp -- the seam merge (PostProcessing, main.cpp:287-302; sd_host.hpp: seam_merge_inplace) in pieces, as
// plain C++ that compiles for the host and for the device: the kernels of sd_rows_dev.hip and the host self-test
// (sd_seam_pieces_selftest) run this text.
//
// The merge is a sequential scan whose whole state is one index.  At position i of a read's N records it looks at
// b[i+1 .. i+6]; if b[i] covers more than half of some b[j] there, it keeps b[i], keeps b[j+1] unchecked and goes on at
// j + 2 (at most i + 8); otherwise it keeps b[i] and goes on at i + 1.  Cut the record list into pieces of S >= 8
// records: a scan that enters piece p at one of the offsets 0..7 leaves it at one of the offsets 0..7 of piece p + 1.
//   exit table   per piece, for every entry offset e: where the scan that starts at p*S + e first reaches (p+1)*S or
//                beyond, as an offset from (p+1)*S -- eight values of 0..7 in one 32-bit word (4 bits each)
//   chain        the true entry of piece p + 1 is the exit of piece p for its true entry; piece 0 is entered at 0.
//                The tables are maps 8 -> 8, and maps compose: seam_compose
//   keep flags   every piece scans once more from its true entry and flags what the scan keeps; the unchecked b[j+1]
//                may lie in the next piece, whose own scan then flags the same record (or not: it is skipped there)
// The scan reads at most 8 records of the same read beyond its piece.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SD_HD __host__ __device__
#else
#define SD_HD
#endif

namespace sd {

constexpr int SEAM_REACH = 8;                  // a step moves the scan at most this far
constexpr uint32_t SEAM_IDENTITY = 0x76543210u;   // the exit table that maps every entry to itself

// One step of the scan at position i < N of the records b[0 .. N): the position it goes on at; *extra = the record
// that is kept unchecked behind a dropped run (j + 1), or -1.  b[i] itself is always kept.
template <class Rec>
SD_HD inline int64_t seam_step(const Rec* b, int64_t N, int64_t i, int64_t* extra) {
    *extra = -1;
    const int64_t lim = i + 7 < N ? i + 7 : N;
    const int32_t ei = b[i].end;
    for (int64_t j = i + 1; j < lim; ++j) {
        const int32_t sj = b[j].start;
        if ((ei - sj) * 2 > (b[j].end - sj)) {
            if (j + 1 < N) *extra = j + 1;
            return j + 2;
        }
    }
    return i + 1;
}

// Records [lo, hi) of piece p of a read of N records cut into pieces of S.
SD_HD inline void seam_piece_range(int64_t N, int32_t S, int64_t p, int64_t* lo, int64_t* hi) {
    *lo = p * S;
    const int64_t e = *lo + S;
    *hi = e < N ? e : N;
}

// Exit table of piece p, in one pass from the piece's last record to its first: where the scan that stands at `pos`
// leaves the piece is where the scan that stands at its next position does, and that position is at most 8 ahead -- so
// a window of eight 4-bit exits (those of pos + 1 .. pos + 8) is all the state, and behind the piece's end the window is
// the identity.  When pos reaches the piece's first record the window IS the table.  (The last piece of a read has no
// successor: its table is never applied.)
template <class Rec>
SD_HD inline uint32_t seam_piece_exits(const Rec* b, int64_t N, int32_t S, int64_t p) {
    int64_t lo, hi;
    seam_piece_range(N, S, p, &lo, &hi);
    uint32_t win = hi == lo + S ? SEAM_IDENTITY : 0u;
    for (int64_t pos = hi - 1; pos >= lo; --pos) {
        int64_t extra;
        const int64_t next = seam_step(b, N, pos, &extra);
        win = (win << 4) | ((win >> (4 * (int)(next - pos - 1))) & 7u);
    }
    return win;
}

SD_HD inline int seam_exit(uint32_t tab, int entry) { return (int)((tab >> (4 * entry)) & 7u); }

// The table of "first, then then".
SD_HD inline uint32_t seam_compose(uint32_t first, uint32_t then) {
    uint32_t r = 0;
    for (int e = 0; e < SEAM_REACH; ++e) r |= (uint32_t)seam_exit(then, seam_exit(first, e)) << (4 * e);
    return r;
}

// Keep flags of piece p, entered at offset `entry`: keep[x] = 1 for every record x of the read the scan keeps while it
// is inside the piece.  keep has N entries, zeroed by the caller; two pieces may set the same flag.
template <class Rec>
SD_HD inline void seam_piece_keep(const Rec* b, int64_t N, int32_t S, int64_t p, int entry, uint8_t* keep) {
    int64_t lo, hi;
    seam_piece_range(N, S, p, &lo, &hi);
    int64_t i = lo + entry;
    while (i < hi) {
        int64_t extra;
        const int64_t next = seam_step(b, N, i, &extra);
        keep[i] = 1;
        if (extra >= 0) keep[extra] = 1;
        i = next;
    }
}

// Pieces of a read of N records.
SD_HD inline int64_t seam_piece_count(int64_t N, int32_t S) { return (N + S - 1) / S; }

}  // namespace sd
