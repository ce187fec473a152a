// sd_final_prof_dev.hpp -- the plan of the column profiles of a device-final job (SD_FLAG_DEVICE_PROFILE), as plain C++
// that compiles for host and device: which (segment, template) pair a kept row yields and who folds it.  The kernels of
// sd_final_prof_dev.hip and sd_final_profile_host call this one text.  The segment is the one the selection measured
// (final_seg_len: Python's slicing of read.seq[start : end + 1]), the template the row's own interleaved one, and the
// limits are those of nw_profile_device (sd_nw.hip): sd_nw_profile takes templates up to 512 bp and segments up to
// 1024 bp that edlib walks by its block traceback; every other pair is folded by the host (profile_host).
#pragma once

#include "sd_final_dev.hpp"

namespace sd {

constexpr int FPROF_TMAX = 512;     // the longest template of a set the kernel takes
constexpr int FPROF_QMAX = 1024;    // the longest segment

enum : uint8_t { FPROF_NONE = 0, FPROF_DEV = 1, FPROF_HOST = 2 };

// A pair on its way to the host fold: 16 bytes.
struct FProfHostPair {
    int64_t start;   // in the job's text
    int32_t len;
    int32_t il;      // interleaved template
};
static_assert(sizeof(FProfHostPair) == 16, "FProfHostPair layout");

struct FProfPair {
    int64_t start;   // first base of the segment in the job's text
    int32_t len;
    int32_t il;      // interleaved template (2 m: monomer m, 2 m + 1: its reverse complement)
    uint8_t cls;     // FPROF_*
};

// first base of read.seq[start : end + 1] inside the read (the clamp of final_seg_len)
SD_HD inline int64_t final_seg_first(int64_t start, int64_t read_len) {
    const int64_t lim = read_len < 0 ? INT64_MAX : read_len;
    const int64_t s0 = start > 0 ? start : 0;
    return s0 > lim ? lim : s0;
}

// The pair of a kept row (start, end: read coordinates, end inclusive) of a read of read_len bases whose text begins at
// text_off; il = the row's own interleaved template, tlen its length, tmax the longest template of the set.
SD_HD inline FProfPair final_prof_pair(int64_t start, int64_t end, int64_t read_len, int64_t text_off, int32_t il, int32_t tlen,
                                       int32_t tmax) {
    FProfPair p;
    p.start = text_off + final_seg_first(start, read_len);
    p.len = (int32_t)final_seg_len(start, end, read_len);
    p.il = il;
    if (p.len <= 0 || tlen <= 0) p.cls = FPROF_NONE;   // no alignment (main.py:30-33): not an instance
    else if (tmax <= FPROF_TMAX && p.len <= FPROF_QMAX && !final_seg_splits(p.len, tlen)) p.cls = FPROF_DEV;
    else p.cls = FPROF_HOST;
    return p;
}

}  // namespace sd
