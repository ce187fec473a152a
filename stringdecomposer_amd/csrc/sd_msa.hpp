// sd_msa.hpp -- the row of one pair of --msa (include/sd_hip.h: SD_MSA_PITCH), as plain C++ that compiles for host and
// device: the sink of the walk of nw_pair (sd_msa.hip: NwMsa is this text over a row in LDS or HBM) and of the host
// fold of an edlib path (sd_post.hip: fold_path_msa).  The steps are those of NwProf (sd_nw_kernel.hpp) -- a pair against
// rc(m): position p -> L-1-p, insertion slot h -> L-h, bases complemented -- written into the pair's own row instead of
// added to its monomer's counters.
#pragma once

#include <cstdint>

#include "../../include/sd_hip.h"
#include "sd_final_dev.hpp"   // SD_HD

namespace sd {

enum : uint8_t { MSA_ST_NONE = 0, MSA_ST_DONE = 1, MSA_ST_LEFT = 2 };

struct MsaRow {
    uint8_t* row;   // SD_MSA_PITCH(L) bytes, cleared by msa_row_clear
    int L;
    bool rc;
    SD_HD int base(int b) const { return rc && b < 4 ? 3 - b : b; }
    SD_HD void diag(int p, int b) { row[rc ? L - 1 - p : p] = (uint8_t)base(b); }
    SD_HD void del(int p) { row[rc ? L - 1 - p : p] = (uint8_t)SD_MSA_DEL; }
    SD_HD void ins(int h, int) {
        uint8_t* c = row + L + (rc ? L - h : h);
        const uint8_t v = *c;
        if (v < 255) *c = (uint8_t)(v + 1);   // saturates: 255 means 255 or more
    }
};

// the four bytes at offset b (a multiple of 4) of a row nobody has computed: SD_MSA_NONE below L, 0 from L on
SD_HD inline uint32_t msa_clear_word(int b, int L) {
    if (b + 4 <= L) return 0x01010101u * (uint32_t)SD_MSA_NONE;
    uint32_t w = 0;
    for (int k = 0; k < 4; ++k)
        if (b + k < L) w |= (uint32_t)SD_MSA_NONE << (8 * k);
    return w;
}

// (host form; the kernels clear with 16-byte stores of msa_clear_word)
inline void msa_row_clear(uint8_t* row, int L) {
    const int pitch = SD_MSA_PITCH(L);
    for (int i = 0; i < pitch; ++i) row[i] = i < L ? (uint8_t)SD_MSA_NONE : (uint8_t)0;
}

}  // namespace sd
