// sd_hor.hpp -- higher-order repeat units of the rows of the final TSV (--hor): the rule, written once for host and
// device, as plain C++ that compiles for both (in the manner of sd_split.hpp).  sd_hor.hip holds the host form and
// the C-ABI (sd_hor_*, include/sd_hip.h); the library has no kernels for it yet.
//
// Input: the rows of the final TSV in file order -- read, start, end (inclusive), key, usable.  key = 2 m + s names monomer
// m of the monomer file on strand s (1 = the reverse complement), -1 = no monomer; a row is usable when it is reliable and
// key >= 0.  M monomers, G >= 0 the widest gap in bases that adjacency bridges, C >= 1 the fewest pairs behind an edge.
//
// Rows x, x + 1 are adjacent when they belong to one read, both are usable, their strands agree and
// 0 <= start[x+1] - end[x] - 1 <= G (hor_adjacent).  An adjacent pair adds 1 to T[m_x][m_x+1] on the forward strand and to
// T[m_x+1][m_x] on the reverse strand (hor_cell: a reverse read walks the array backwards); rows[m] counts the usable rows
// of m.  succ(a) = the b of largest T[a][b], pred(b) = the a of largest T[a][b], ties to the smallest index (hor_arg_key),
// each defined when that count is >= C.  The edge a -> b is kept when succ(a) = b and pred(b) = a, so kept edges form
// simple cycles and simple paths (hor_orders): an order, rotated to its smallest monomer (cycle) or begun at its head
// (path), positions 1-based, orders sorted by their smallest monomer; an order of more than HOR_PMAX monomers is not
// numbered and its monomers are on no order.
//
// A unit is a maximal run of rows in which every consecutive pair is adjacent, on one order, with positions rising on the
// forward strand and falling on the reverse strand (hor_continues); a usable row on an order whose predecessor does not
// continue into it is a head.  A unit has at most HOR_PMAX rows; its mask holds bit pos - 1 per row, its name the positions
// present as ascending ranges joined by '_' (hor_name).
#pragma once

#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#ifndef SD_HD
#define SD_HD __host__ __device__
#endif
#else
#ifndef SD_HD
#define SD_HD
#endif
#endif

namespace sd {

constexpr int HOR_MMAX = 2048;        // monomers: T is at most 32 MB
constexpr int HOR_PMAX = 64;          // monomers of an order, rows of a unit, bits of a mask
constexpr int HOR_NAME_MAX = 192;     // bytes of a name with its terminator (the longest: 32 single positions, 90 bytes)
constexpr int HOR_CYCLE = 0, HOR_PATH = 1;

SD_HD inline bool hor_usable(int32_t key, int usable, int32_t M) { return usable != 0 && key >= 0 && key < 2 * M; }
SD_HD inline int32_t hor_mono(int32_t key) { return key >> 1; }
SD_HD inline int hor_strand(int32_t key) { return key & 1; }

// rows x, x + 1 (both usable): read, end, key of x; read, start, key of x + 1
SD_HD inline bool hor_adjacent(int32_t read0, int64_t end0, int32_t key0, int32_t read1, int64_t start1, int32_t key1, int64_t G) {
    if (read0 != read1 || hor_strand(key0) != hor_strand(key1)) return false;
    const int64_t gap = start1 - end0 - 1;
    return gap >= 0 && gap <= G;
}

// the cell of T an adjacent pair adds to
SD_HD inline int64_t hor_cell(int32_t key0, int32_t key1, int32_t M) {
    const int64_t a = hor_mono(key0), b = hor_mono(key1);
    return hor_strand(key0) ? b * M + a : a * M + b;
}

// an argmax as a maximum: the larger count wins, then the smaller index (counts stay below 2^31, indices below 2^11)
SD_HD inline uint64_t hor_arg_key(int64_t count, int32_t idx) { return ((uint64_t)count << 11) | (uint64_t)(HOR_MMAX - 1 - idx); }
SD_HD inline int64_t hor_arg_count(uint64_t key) { return (int64_t)(key >> 11); }
SD_HD inline int32_t hor_arg_idx(uint64_t key) { return HOR_MMAX - 1 - (int32_t)(key & (HOR_MMAX - 1)); }

// does the unit of row x go on into row x + 1: the pair is adjacent, (h0, p0) / (h1, p1) = order and position of their monomers
SD_HD inline bool hor_continues(bool adjacent, int strand, int32_t h0, int32_t p0, int32_t h1, int32_t p1) {
    if (!adjacent || h0 < 0 || h0 != h1) return false;
    return strand ? p1 < p0 : p1 > p0;
}

// the name of a mask into buf (HOR_NAME_MAX bytes), 0-terminated -> its length; mask 0 gives ""
SD_HD inline int hor_name(uint64_t mask, char* buf) {
    int at = 0;
    auto num = [&](int v) {
        if (v >= 10) buf[at++] = (char)('0' + v / 10);
        buf[at++] = (char)('0' + v % 10);
    };
    for (int p = 1; p <= HOR_PMAX;) {
        if (!((mask >> (p - 1)) & 1)) { ++p; continue; }
        int q = p;
        while (q < HOR_PMAX && ((mask >> q) & 1)) ++q;   // positions p .. q are present
        if (at) buf[at++] = '_';
        num(p);
        if (q > p) { buf[at++] = '-'; num(q); }
        p = q + 1;
    }
    buf[at] = 0;
    return at;
}

// the rows of a call, column by column (host or device pointers)
struct HorRows {
    const int32_t* read;
    const int64_t* start;
    const int64_t* end;
    const int32_t* key;
    const uint8_t* usable;
    int64_t n;
    int32_t M;
    int64_t G;
};

SD_HD inline bool hor_row_usable(const HorRows& r, int64_t x) { return hor_usable(r.key[x], r.usable[x], r.M); }

// are rows x, x + 1 adjacent (x + 1 < n)
SD_HD inline bool hor_pair_adjacent(const HorRows& r, int64_t x) {
    return hor_row_usable(r, x) && hor_row_usable(r, x + 1) &&
           hor_adjacent(r.read[x], r.end[x], r.key[x], r.read[x + 1], r.start[x + 1], r.key[x + 1], r.G);
}

// row x against the orders: bit 0 = it lies on an order, bit 1 = it is the head of a unit
SD_HD inline int hor_row_flags(const HorRows& r, const int32_t* hor, const int32_t* pos, int64_t x) {
    if (!hor_row_usable(r, x)) return 0;
    const int32_t m = hor_mono(r.key[x]);
    if (hor[m] < 0) return 0;
    if (x > 0 && hor_row_usable(r, x - 1)) {
        const int32_t m0 = hor_mono(r.key[x - 1]);
        if (hor_continues(hor_pair_adjacent(r, x - 1), hor_strand(r.key[x]), hor[m0], pos[m0], hor[m], pos[m])) return 1;
    }
    return 3;
}

// The orders over the argmaxes of T (host only: M numbers).  arg: per monomer {succ, its count, pred, its count}.
// hor[m] = the order of m (0-based: H<hor + 1>) or -1, pos[m] = its position (1-based) or 0; kind / len per order;
// long_first / long_len: the orders of more than HOR_PMAX monomers, by their first monomer.
struct HorOrders {
    std::vector<int32_t> hor, pos, kind, len, long_first, long_len;
};
inline HorOrders hor_orders(const int64_t* arg, int32_t M, int64_t C) {
    HorOrders o;
    o.hor.assign((size_t)M, -1);
    o.pos.assign((size_t)M, 0);
    std::vector<int32_t> next((size_t)M, -1), prev((size_t)M, -1);
    for (int32_t a = 0; a < M; ++a) {
        const int64_t b = arg[4 * a], cnt = arg[4 * a + 1];
        if (cnt < C || b < 0 || b >= M) continue;
        if (arg[4 * b + 3] >= C && arg[4 * b + 2] == a) { next[(size_t)a] = (int32_t)b; prev[(size_t)b] = a; }
    }
    std::vector<char> seen((size_t)M, 0);
    for (int32_t m = 0; m < M; ++m) {   // ascending: m is the smallest monomer of its component
        if (seen[(size_t)m] || (next[(size_t)m] < 0 && prev[(size_t)m] < 0)) continue;
        int32_t head = m;
        bool cycle = false;
        while (prev[(size_t)head] >= 0) {
            head = prev[(size_t)head];
            if (head == m) { cycle = true; break; }
        }
        std::vector<int32_t> mem;
        for (int32_t x = head; x >= 0 && !seen[(size_t)x]; x = next[(size_t)x]) { seen[(size_t)x] = 1; mem.push_back(x); }
        if ((int)mem.size() > HOR_PMAX) {
            o.long_first.push_back(head);
            o.long_len.push_back((int32_t)mem.size());
            continue;
        }
        const int32_t id = (int32_t)o.kind.size();
        o.kind.push_back(cycle ? HOR_CYCLE : HOR_PATH);
        o.len.push_back((int32_t)mem.size());
        for (size_t i = 0; i < mem.size(); ++i) { o.hor[(size_t)mem[i]] = id; o.pos[(size_t)mem[i]] = (int32_t)i + 1; }
    }
    return o;
}

}  // namespace sd
