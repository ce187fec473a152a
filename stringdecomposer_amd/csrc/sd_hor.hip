// sd_hor.hip -- higher-order repeat units of the rows of the final TSV (--hor).  sd_hor.hpp holds the rule, as text that
// compiles for host and device; this file holds the host form on the thread pool and the C-ABI (include/sd_hip.h:
// sd_hor_*).  There is little arithmetic here: one pass over the rows for the transitions, the argmaxes of an M x M table,
// one pass for the head flags, a prefix count per block of rows, one pass for the records.  The device form (kernels on
// rows that lie in HBM) is not in this file: DESIGN.md section 3.5 says why.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "sd_pipeline.hpp"
#include "sd_host.hpp"
#include "sd_hor.hpp"

namespace sd {

// the record of the unit whose head is row x: keep[y] = 1 at heads, on[y] = 1 on an order
SD_HD inline sd_hor_unit hor_unit_at(const HorRows& r, const int32_t* hor, const int32_t* pos, const uint8_t* keep, const uint8_t* on,
                                     int64_t x) {
    const int32_t m = hor_mono(r.key[x]);
    uint64_t mask = (uint64_t)1 << (pos[m] - 1);
    int64_t y = x + 1;
    while (y < r.n && y - x < HOR_PMAX && !keep[y] && on[y]) {
        mask |= (uint64_t)1 << (pos[hor_mono(r.key[y])] - 1);
        ++y;
    }
    sd_hor_unit u;
    u.first_row = x;
    u.start = r.start[x];
    u.end = r.end[y - 1];
    u.mask = mask;
    u.read = r.read[x];
    u.n_rows = (int32_t)(y - x);
    u.order = hor[m];
    u.strand = hor_strand(r.key[x]);
    return u;
}

}  // namespace sd

namespace sdi {
namespace {

// what a call returns
struct HorOut {
    int64_t* T;
    int64_t* rows;
    int32_t *hor, *pos, *kind, *len, *lfirst, *llen, *row_unit;
    sd_hor_unit* units;
    int64_t cap;
    int64_t* info;
};

int hor_args(const char* who, int64_t n_rows, int32_t n_mono, int64_t G, int64_t C, const HorOut& o, bool inputs_missing, char* errbuf,
             size_t errlen) {
    const std::string w = std::string(who) + ": ";
    if (n_mono < 1) { set_err(errbuf, errlen, w + "n_mono = " + std::to_string(n_mono) + ", must be 1 .. " + std::to_string(sd::HOR_MMAX)); return SD_ERR_PARAM; }
    if (n_mono > sd::HOR_MMAX) {
        set_err(errbuf, errlen, w + "n_mono = " + std::to_string(n_mono) + ", at most " + std::to_string(sd::HOR_MMAX) + " monomers are supported");
        return SD_ERR_UNSUPPORTED;
    }
    if (G < 0) { set_err(errbuf, errlen, w + "G = " + std::to_string(G) + ", must be 0 or more"); return SD_ERR_PARAM; }
    if (C < 1) { set_err(errbuf, errlen, w + "C = " + std::to_string(C) + ", must be 1 or more"); return SD_ERR_PARAM; }
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 31)) {
        set_err(errbuf, errlen, w + "n_rows = " + std::to_string(n_rows) + ", must be 0 .. 2^31 - 1");
        return SD_ERR_PARAM;
    }
    if (o.cap < 0) { set_err(errbuf, errlen, w + "cap_units = " + std::to_string(o.cap) + ", must be 0 or more"); return SD_ERR_PARAM; }
    if (inputs_missing || !o.T || !o.rows || !o.hor || !o.pos || !o.kind || !o.len || !o.lfirst || !o.llen || !o.info ||
        (n_rows > 0 && !o.row_unit) || (o.cap > 0 && !o.units)) {
        set_err(errbuf, errlen, w + "missing argument");
        return SD_ERR_PARAM;
    }
    return SD_OK;
}

int hor_key_check(const char* who, const int32_t* key, int64_t n, int32_t M, char* errbuf, size_t errlen) {
    for (int64_t x = 0; x < n; ++x)
        if (key[x] < -1 || key[x] >= 2 * M) {
            set_err(errbuf, errlen, std::string(who) + ": key " + std::to_string(key[x]) + " of row " + std::to_string(x) + " lies outside -1 .. " +
                                        std::to_string(2 * M - 1));
            return SD_ERR_PARAM;
        }
    return SD_OK;
}

// the orders into the caller's arrays; info[0], info[2]
void hor_orders_out(const sd::HorOrders& ord, int32_t M, const HorOut& o) {
    std::memcpy(o.hor, ord.hor.data(), sizeof(int32_t) * (size_t)M);
    std::memcpy(o.pos, ord.pos.data(), sizeof(int32_t) * (size_t)M);
    for (int32_t i = 0; i < M; ++i) {
        o.kind[i] = (size_t)i < ord.kind.size() ? ord.kind[(size_t)i] : 0;
        o.len[i] = (size_t)i < ord.len.size() ? ord.len[(size_t)i] : 0;
        o.lfirst[i] = (size_t)i < ord.long_first.size() ? ord.long_first[(size_t)i] : -1;
        o.llen[i] = (size_t)i < ord.long_len.size() ? ord.long_len[(size_t)i] : 0;
    }
    o.info[0] = (int64_t)ord.kind.size();
    o.info[2] = (int64_t)ord.long_first.size();
}

int hor_cap_refusal(const char* who, int64_t n_units, int64_t cap, char* errbuf, size_t errlen) {
    set_err(errbuf, errlen, std::string(who) + ": " + std::to_string(n_units) + " units, cap_units is " + std::to_string(cap));
    return SD_ERR_PARAM;
}

// ---- the host form --------------------------------------------------------------------------------------------------
constexpr int64_t HOR_HOST_BLOCK = 1 << 16;   // rows of a host block

int hor_host(const char* who, const sd::HorRows& r, int64_t C, int threads, const HorOut& o, char* errbuf, size_t errlen) {
    const int32_t M = r.M;
    const int64_t n = r.n, cells = (int64_t)M * M, blocks = (n + HOR_HOST_BLOCK - 1) / HOR_HOST_BLOCK;
    threads = std::max(1, threads);
    std::memset(o.T, 0, sizeof(int64_t) * (size_t)cells);
    std::memset(o.rows, 0, sizeof(int64_t) * (size_t)M);
    o.info[0] = o.info[1] = o.info[2] = o.info[3] = 0;
    // transitions: a block's own table where it is small, atomic adds into T where it is not
    const bool local = cells + M <= (1 << 14);
    std::mutex merge;
    sd::parallel_for(blocks, threads, 1, [&](int64_t b) {
        std::vector<int64_t> mine(local ? (size_t)(cells + M) : 0, 0);
        const int64_t lo = b * HOR_HOST_BLOCK, hi = std::min(n, lo + HOR_HOST_BLOCK);
        for (int64_t x = lo; x < hi; ++x) {
            if (!sd::hor_row_usable(r, x)) continue;
            const int32_t m = sd::hor_mono(r.key[x]);
            if (local) ++mine[(size_t)(cells + m)];
            else __atomic_fetch_add(o.rows + m, (int64_t)1, __ATOMIC_RELAXED);
            if (x + 1 >= n || !sd::hor_pair_adjacent(r, x)) continue;
            const int64_t c = sd::hor_cell(r.key[x], r.key[x + 1], M);
            if (local) ++mine[(size_t)c];
            else __atomic_fetch_add(o.T + c, (int64_t)1, __ATOMIC_RELAXED);
        }
        if (local) {
            std::lock_guard<std::mutex> g(merge);
            for (int64_t i = 0; i < cells; ++i) o.T[i] += mine[(size_t)i];
            for (int32_t m = 0; m < M; ++m) o.rows[m] += mine[(size_t)(cells + m)];
        }
    });
    // argmaxes: rows by monomer, columns in strips of 64 (T is walked row by row)
    std::vector<int64_t> arg((size_t)4 * M);
    sd::parallel_for(M, threads, 8, [&](int64_t a) {
        uint64_t k = 0;
        for (int32_t b = 0; b < M; ++b) k = std::max(k, sd::hor_arg_key(o.T[a * M + b], b));
        arg[(size_t)(4 * a)] = sd::hor_arg_idx(k);
        arg[(size_t)(4 * a + 1)] = sd::hor_arg_count(k);
    });
    sd::parallel_for((M + 63) / 64, threads, 1, [&](int64_t s) {
        uint64_t k[64] = {0};
        const int32_t b0 = (int32_t)s * 64, nb = std::min(64, M - b0);
        for (int32_t a = 0; a < M; ++a)
            for (int32_t j = 0; j < nb; ++j) k[j] = std::max(k[j], sd::hor_arg_key(o.T[(int64_t)a * M + b0 + j], a));
        for (int32_t j = 0; j < nb; ++j) {
            arg[(size_t)(4 * (b0 + j) + 2)] = sd::hor_arg_idx(k[j]);
            arg[(size_t)(4 * (b0 + j) + 3)] = sd::hor_arg_count(k[j]);
        }
    });
    const sd::HorOrders ord = sd::hor_orders(arg.data(), M, C);
    hor_orders_out(ord, M, o);
    // flags, unit numbers, records
    std::vector<uint8_t> keep((size_t)n + 1, 0), on((size_t)n + 1, 0);
    std::vector<int64_t> base((size_t)blocks + 1, 0);
    sd::parallel_for(blocks, threads, 1, [&](int64_t b) {
        const int64_t lo = b * HOR_HOST_BLOCK, hi = std::min(n, lo + HOR_HOST_BLOCK);
        int64_t heads = 0;
        for (int64_t x = lo; x < hi; ++x) {
            const int f = sd::hor_row_flags(r, o.hor, o.pos, x);
            keep[(size_t)x] = (uint8_t)(f >> 1);
            on[(size_t)x] = (uint8_t)(f & 1);
            heads += f >> 1;
        }
        base[(size_t)b + 1] = heads;
    });
    for (int64_t b = 0; b < blocks; ++b) base[(size_t)b + 1] += base[(size_t)b];
    const int64_t n_units = base[(size_t)blocks];
    o.info[1] = n_units;
    sd::parallel_for(blocks, threads, 1, [&](int64_t b) {
        const int64_t lo = b * HOR_HOST_BLOCK, hi = std::min(n, lo + HOR_HOST_BLOCK);
        int64_t u = base[(size_t)b];
        for (int64_t x = lo; x < hi; ++x) {
            u += keep[(size_t)x];
            o.row_unit[x] = on[(size_t)x] ? (int32_t)(u - 1) : -1;
        }
    });
    if (n_units > o.cap) return hor_cap_refusal(who, n_units, o.cap, errbuf, errlen);
    sd::parallel_for(blocks, threads, 1, [&](int64_t b) {
        const int64_t lo = b * HOR_HOST_BLOCK, hi = std::min(n, lo + HOR_HOST_BLOCK);
        for (int64_t x = lo; x < hi; ++x)
            if (keep[(size_t)x]) o.units[o.row_unit[x]] = sd::hor_unit_at(r, o.hor, o.pos, keep.data(), on.data(), x);
    });
    return SD_OK;
}

// the columns of final rows on the host
struct HorColumns {
    std::vector<int32_t> read, key;
    std::vector<int64_t> start, end;
    std::vector<uint8_t> usable;
    sd::HorRows view(int32_t M, int64_t G) const { return sd::HorRows{read.data(), start.data(), end.data(), key.data(), usable.data(), (int64_t)read.size(), M, G}; }
};

}  // namespace
}  // namespace sdi

extern "C" {

int sd_hor_rows(const int32_t* read, const int64_t* start, const int64_t* end, const int32_t* key, const uint8_t* usable, int64_t n_rows,
                int32_t n_mono, int64_t G, int64_t C, int32_t threads, int64_t* T, int64_t* rows, int32_t* hor, int32_t* pos,
                int32_t* order_kind, int32_t* order_len, int32_t* long_first, int32_t* long_len, int32_t* row_unit, sd_hor_unit* units,
                int64_t cap_units, int64_t info[4], char* errbuf, size_t errlen) try {
    static const char* who = "sd_hor_rows";
    const HorOut o{T, rows, hor, pos, order_kind, order_len, long_first, long_len, row_unit, units, cap_units, info};
    int rc = hor_args(who, n_rows, n_mono, G, C, o, n_rows > 0 && (!read || !start || !end || !key || !usable), errbuf, errlen);
    if (rc || (rc = hor_key_check(who, key, n_rows, n_mono, errbuf, errlen))) return rc;
    return hor_host(who, sd::HorRows{read, start, end, key, usable, n_rows, n_mono, G}, C, threads, o, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_hor_final_host(const sd_final_row* rows_in, int64_t n_rows, int32_t n_mono, int64_t G, int64_t C, int32_t threads, int64_t* T,
                      int64_t* rows, int32_t* hor, int32_t* pos, int32_t* order_kind, int32_t* order_len, int32_t* long_first,
                      int32_t* long_len, int32_t* row_unit, sd_hor_unit* units, int64_t cap_units, int64_t info[4], char* errbuf,
                      size_t errlen) try {
    static const char* who = "sd_hor_final_host";
    const HorOut o{T, rows, hor, pos, order_kind, order_len, long_first, long_len, row_unit, units, cap_units, info};
    int rc = hor_args(who, n_rows, n_mono, G, C, o, n_rows > 0 && !rows_in, errbuf, errlen);
    if (rc) return rc;
    HorColumns c;
    c.read.resize((size_t)n_rows);
    c.key.resize((size_t)n_rows);
    c.start.resize((size_t)n_rows);
    c.end.resize((size_t)n_rows);
    c.usable.resize((size_t)n_rows);
    sd::parallel_for(n_rows, std::max(1, (int)threads), 1 << 14, [&](int64_t x) {
        const sd_final_row& f = rows_in[x];
        c.read[(size_t)x] = f.read;
        c.start[(size_t)x] = f.start;
        c.end[(size_t)x] = f.end;
        c.key[(size_t)x] = f.best;
        c.usable[(size_t)x] = f.reliable == 1 ? 1 : 0;
    });
    if ((rc = hor_key_check(who, c.key.data(), n_rows, n_mono, errbuf, errlen))) return rc;
    return hor_host(who, c.view(n_mono, G), C, threads, o, errbuf, errlen);
} catch (const std::bad_alloc&) {
    return SD_ERR_INTERNAL;
}

int sd_hor_name(uint64_t mask, char* buf) { return buf ? sd::hor_name(mask, buf) : 0; }

void sd_hor_info(int64_t info[4]) {
    info[0] = sd::HOR_MMAX;
    info[1] = sd::HOR_PMAX;
    info[2] = sd::HOR_NAME_MAX;
    info[3] = 0;
}

}  // extern "C"
