"""The refusals of the analyses' C entries (--lags, --heatmap, --autocorr, --dotplot, --split) at the C-ABI: return code and
the whole text, case by case.  The argument checks are shared code (csrc/sd_job_dev.hpp); the texts below are what the
library said before they were, taken from a build of that commit, and no device is needed to be refused."""
import ctypes as C

import numpy as np
import pytest

from stringdecomposer_amd import lib

OK, PARAM, UNSUP, NODEV = lib.SD_OK, lib.SD_ERR_PARAM, lib.SD_ERR_UNSUPPORTED, lib.SD_ERR_NO_DEVICE
ERRLEN = 1024
TEXT = b"ACGTACGTACGTACGT"


def i64(*v):
    return np.array(v, dtype=np.int64)


def ptr(a):
    return None if a is None else a.ctypes.data


def no_device():
    """what a *_dev entry answers to valid arguments that need no kernel, by the machine"""
    return (NODEV, "no usable HIP device") if lib.device_count() == 0 else (OK, "")


# ---- segment calls: (seqlen, starts, ends, n_seg, group_off, n_groups) -> (code, text behind "<entry>: ") ----------------
SEGMENT_CASES = {
    "null group_off": ((16, i64(0), i64(3), 1, None, 1), PARAM, "missing argument"),
    "group_off[0] != 0": ((16, i64(0), i64(3), 1, i64(1, 1), 1), PARAM, "the groups do not cover the segments"),
    "group_off[n_groups] != n_seg": ((16, i64(0, 4), i64(3, 7), 2, i64(0, 1), 1), PARAM, "the groups do not cover the segments"),
    "starts < 0": ((16, i64(0, -1), i64(3, 7), 2, i64(0, 2), 1), PARAM, "segment 1 lies outside the text"),
    "ends >= seqlen": ((16, i64(0, 4), i64(16, 7), 2, i64(0, 2), 1), PARAM, "segment 0 lies outside the text"),
    # (the check comes before any read of the text: 16 bytes stand for 2^27)
    "2^27 bases": ((1 << 27, i64(0), i64((1 << 27) - 1), 1, i64(0, 1), 1), UNSUP, "a segment of 2^27 bases or more"),
    "n_seg = 0": ((16, i64(0), i64(0), 0, i64(0, 0), 1), OK, None),
}


def segment_call(entry, case):
    """-> (code, message or None where the entry has no errbuf)"""
    L = lib.load()
    seqlen, st, en, n_seg, go, G = SEGMENT_CASES[case][0]
    err = C.create_string_buffer(ERRLEN)
    dist, matches = np.zeros(4 * 64, dtype=np.int32), np.zeros(4 * 64, dtype=np.int32)
    sums = np.zeros(3 * 64 * 4, dtype=np.int64)
    cls = (C.c_int64 * 3)()
    lead = (TEXT, seqlen, ptr(st), ptr(en), n_seg, ptr(go), G)
    if entry == "sd_lag_segments":
        return L.sd_lag_segments(*lead, 2, 1, ptr(dist), ptr(matches), ptr(sums)), None
    if entry == "sd_lag_segments_dev":
        return L.sd_lag_segments_dev(*lead, 2, 0, 1, ptr(dist), ptr(matches), ptr(sums)), None
    if entry == "sd_heat_segments":
        return L.sd_heat_segments(*lead, 2, 0, 0, 0, 1, ptr(sums), err, ERRLEN), err.value.decode()
    return L.sd_heat_segments_dev(*lead, 2, 0, 0, 0, 1, ptr(sums), cls, err, ERRLEN), err.value.decode()


@pytest.mark.parametrize("case", list(SEGMENT_CASES))
@pytest.mark.parametrize("entry", ["sd_lag_segments", "sd_lag_segments_dev", "sd_heat_segments", "sd_heat_segments_dev"])
def test_segment_calls(entry, case):
    _, code, text = SEGMENT_CASES[case]
    want = "" if text is None else "%s: %s" % (entry, text)
    if case == "n_seg = 0" and entry.endswith("_dev"):
        code, want = no_device()
    rc, msg = segment_call(entry, case)
    assert rc == code
    assert msg is None or msg == want


# ---- calls on final rows in host memory ------------------------------------------------------------------------------------
def final_rows(*reads_of_rows):
    rows = np.zeros(len(reads_of_rows), dtype=lib.final_dtype())
    for i, r in enumerate(reads_of_rows):
        rows[i]["read"], rows[i]["start"], rows[i]["end"] = r, 4 * i, 4 * i + 3
    return rows


FINAL_CASES = {
    "negative read_off": (final_rows(0, 0), i64(-1, 8), i64(8, 8), "negative read offset or length, or no text"),
    "negative read_lens": (final_rows(0, 0), i64(0, 8), i64(8, -8), "negative read offset or length, or no text"),
    "a row of no read": (final_rows(0, 2), i64(0, 8), i64(8, 8), "row 1 has a read index outside the reads"),
    "rows out of read order": (final_rows(1, 0), i64(0, 8), i64(8, 8), "the rows are not in the order of their reads"),
}


@pytest.mark.parametrize("case", list(FINAL_CASES))
def test_heat_final_host(case):
    rows, ro, rl, text = FINAL_CASES[case]
    err = C.create_string_buffer(ERRLEN)
    sums = np.zeros(3 * 16, dtype=np.int64)
    cls = (C.c_int64 * 3)()
    rc = lib.load().sd_heat_final_host(ptr(rows), len(rows), TEXT, ptr(ro), ptr(rl), 2, 1, 0, 0, 0, 1, ptr(sums), 3, cls, err, ERRLEN)
    assert rc == PARAM
    assert err.value.decode() == "sd_heat_final_host: " + text


@pytest.mark.parametrize("case", ["negative read_off", "negative read_lens", "a row of no read"])
def test_lag_final_host(case):
    rows, ro, rl, _ = FINAL_CASES[case]
    dist, matches, sums = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32), np.zeros(3 * 2 * 2, dtype=np.int64)
    rc = lib.load().sd_lag_final_host(ptr(rows), len(rows), TEXT, ptr(ro), ptr(rl), 2, 2, 1, ptr(dist), ptr(matches), ptr(sums))
    assert rc == PARAM   # (no errbuf in this entry)


# ---- reads calls in host memory: (text, read_off, an output or not) ----------------------------------------------------------
READS_CASES = {
    "null read_off": (TEXT, None, True, "missing or negative read offset"),
    "negative offset": (TEXT, i64(-1), True, "missing or negative read offset"),
    "null text with bases": (None, i64(0), True, "missing argument"),
    "null output with cells": (TEXT, i64(0), False, "missing argument"),
}


@pytest.mark.parametrize("case", list(READS_CASES))
def test_autocorr_host(case):
    text, ro, out, want = READS_CASES[case]
    err = C.create_string_buffer(ERRLEN)
    counts, rl = np.zeros(64, dtype=np.int64), i64(16)
    rc = lib.load().sd_autocorr_host(text, ptr(ro), ptr(rl), 1, 2, 4, 0, 1, ptr(counts) if out else None, err, ERRLEN)
    assert rc == PARAM
    assert err.value.decode() == "sd_autocorr_host: " + want


@pytest.mark.parametrize("case", list(READS_CASES))
def test_dotplot_host(case):
    text, ro, out, want = READS_CASES[case]
    err = C.create_string_buffer(ERRLEN)
    kmers, shared, rl = np.zeros(8, dtype=np.int32), np.zeros(64, dtype=np.int32), i64(16)
    rc = lib.load().sd_dotplot_host(text, ptr(ro), ptr(rl), 1, 2, 4, 0, 1, 0, 1, ptr(kmers), None, ptr(shared) if out else None,
                                    None, err, ERRLEN)
    assert rc == PARAM
    assert err.value.decode() == "sd_dotplot_host: " + want


# ---- every *_dev entry, valid small arguments, a device that does not exist ------------------------------------------------
def dev_calls():
    L = lib.load()
    st, en, go = i64(0, 4), i64(3, 7), i64(0, 2)
    ro, rl = i64(0), i64(16)
    i32 = [np.zeros(256, dtype=np.int32) for _ in range(4)]
    big = np.zeros(1024, dtype=np.int64)
    rows = final_rows(0, 0)
    sym = np.zeros((4, 8), dtype=np.uint8)
    cen = np.zeros((2, 8), dtype=np.uint8)
    cls, info = (C.c_int64 * 3)(), (C.c_int64 * 4)()
    keep = (st, en, go, ro, rl, i32, big, rows, sym, cen, cls, info)
    a, b, c, d = (ptr(x) for x in i32)
    # (where the arguments name device memory, host addresses stand in: the device is looked at before they are)
    return keep, {
        "sd_lag_segments_dev": lambda err: L.sd_lag_segments_dev(TEXT, 16, ptr(st), ptr(en), 2, ptr(go), 1, 2, 1000, 1, a, b, ptr(big)),
        "sd_lag_final_dev": lambda err: L.sd_lag_final_dev(ptr(rows), 2, ptr(big), ptr(ro), ptr(rl), 1, 2, 1000, None, a, b, ptr(big), cls,
                                                           err, ERRLEN),
        "sd_heat_segments_dev": lambda err: L.sd_heat_segments_dev(TEXT, 16, ptr(st), ptr(en), 2, ptr(go), 1, 2, 0, 0, 1000, 1, ptr(big), cls,
                                                                   err, ERRLEN),
        "sd_heat_final_dev": lambda err: L.sd_heat_final_dev(ptr(rows), 2, ptr(big), ptr(ro), ptr(rl), 1, 2, 0, 0, 1000, None, ptr(big), 1, cls,
                                                             err, ERRLEN),
        "sd_autocorr_dev": lambda err: L.sd_autocorr_dev(TEXT, ptr(ro), ptr(rl), 1, 2, 4, 0, 1000, 1, ptr(big), err, ERRLEN),
        "sd_autocorr_reads_dev": lambda err: L.sd_autocorr_reads_dev(ptr(big), ptr(ro), ptr(rl), 1, 2, 4, 0, 1000, None, ptr(big), err, ERRLEN),
        "sd_dotplot_dev": lambda err: L.sd_dotplot_dev(TEXT, ptr(ro), ptr(rl), 1, 2, 4, 0, 1, 0, 1000, a, None, b, None, err, ERRLEN),
        "sd_dotplot_reads_dev": lambda err: L.sd_dotplot_reads_dev(ptr(big), ptr(ro), ptr(rl), 1, 2, 4, 0, 1, 0, 1000, None, a, None, b, None,
                                                                   err, ERRLEN),
        "sd_split_dev": lambda err: L.sd_split_dev(ptr(sym), 4, 8, 8, 2, 2, 1, 4, 1000, 1, ptr(cen), a, b, c, d, info, err, ERRLEN),
    }


@pytest.mark.parametrize("entry", ["sd_lag_segments_dev", "sd_lag_final_dev", "sd_heat_segments_dev", "sd_heat_final_dev", "sd_autocorr_dev",
                                   "sd_autocorr_reads_dev", "sd_dotplot_dev", "sd_dotplot_reads_dev", "sd_split_dev"])
def test_device_1000(entry):
    """the argument checks have passed when the device is looked at, and the device is looked at before anything is done"""
    keep, calls = dev_calls()   # (keep: the arrays behind the addresses)
    err = C.create_string_buffer(ERRLEN)
    rc = calls[entry](err)
    code, want = (NODEV, "no usable HIP device") if lib.device_count() == 0 else (PARAM, "device 1000 does not exist")
    assert rc == code
    if entry != "sd_lag_segments_dev":   # (no errbuf in that entry)
        assert err.value.decode() == want
    assert keep
