"""Profiles folded on the device (SD_FLAG_DEVICE_PROFILE), the parts that need no device: the new C-ABI entries are
exported and declared, the flag is refused where it cannot work before any device is touched, and the plan of the
pairs (csrc/sd_final_prof_dev.hpp, run on the host by sd_final_profile_host) gives the counts of the existing host fold
(lib.profile_segments(device=None), pinned to tests/profile_ref.py by test_profile_cpu.py) on segments clamped here."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import device_profile_cases as dpc
from conftest import ROOT

from stringdecomposer_amd import formats, lib, synth

NEW = ("sd_stream_profile_dev", "sd_stream_profile_stats", "sd_final_profile_dev", "sd_final_profile_host")


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    m = re.search(r"#define\s+SD_FLAG_DEVICE_PROFILE\s+(\d+)\b", header)
    assert m and int(m.group(1)) == lib.FLAG_DEVICE_PROFILE == 4096


def _refused(names=None, **kw):
    mn, ms = synth.make_monomers(4, seed=2)
    with pytest.raises(lib.SdError) as e:
        lib.Stream(ms, mono_names=names or mn, device_profile=True, **kw)
    assert e.value.code == lib.SD_ERR_PARAM
    assert "SD_FLAG_DEVICE_PROFILE" in e.value.msg and "SD_FLAG_DEVICE_FINAL" in e.value.msg
    return e.value.msg


def test_refused_on_a_raw_stream():
    assert "final-mode" in _refused()
    assert "final-mode" in _refused(device_final=True)


def test_refused_without_device_final():
    assert "needs SD_FLAG_DEVICE_FINAL" in _refused(final=True)


def test_refused_with_several_devices():
    """(checked before the device list itself: no device is looked for)"""
    assert "one entry" in _refused(final=True, device_final=True, devices=[0, 0])


def test_refused_with_a_repeated_name():
    mn, _ = synth.make_monomers(4, seed=2)
    names = list(mn)
    names[3] = names[1]
    msg = _refused(names=names, final=True, device_final=True)
    assert "is not unique: a profile needs one template per name" in msg


def test_refused_with_the_host_profile_flag():
    assert "SD_FLAG_PROFILE" in _refused(final=True, device_final=True, profile=True)


def test_without_a_device():
    """The accepted combination gets as far as the device."""
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    mn, ms = synth.make_monomers(4, seed=2)
    with pytest.raises(lib.SdError) as e:
        lib.Stream(ms, final=True, mono_names=mn, device_final=True, device_profile=True)
    assert e.value.code == lib.SD_ERR_NO_DEVICE
    one = np.zeros(2, dtype=np.int64)
    with pytest.raises(lib.SdError) as e:
        lib.final_profile_device("", one[:1], np.zeros((0, 4), dtype=np.int32), one[:1], [], ["ACGT"])
    assert e.value.code == lib.SD_ERR_NO_DEVICE


def test_null_handles_are_refused():
    L = lib.load()
    err = C.create_string_buffer(256)
    n = C.c_int64()
    out = (C.c_double * 4)()
    assert L.sd_stream_profile_dev(None, 0, None, 0, None, C.byref(n), err, 256) == lib.SD_ERR_PARAM
    assert L.sd_stream_profile_stats(None, out) == lib.SD_ERR_PARAM
    pairs = (C.c_int64 * 2)()
    tl = (C.c_int32 * 1)(4)
    assert L.sd_final_profile_host(b"", None, 0, None, None, None, lib._strs([b"ACGT"]), tl, 1, 0, 1, None, pairs) == lib.SD_ERR_PARAM


def _boundary_case():
    """Three monomers of 171 bp; four reads, the second without rows.  Kept and dropped rows of mutated instances, then
    rows of exactly 1, 1023, 1024 and 1025 bases, a row whose end lies past its read's end and a row that begins behind
    its read's end (length 0)."""
    ms = [m.decode() for m in synth.make_monomers(3, seed=4)[1]]
    seq, st, en, pt = dpc.segments(ms, 60, seed=8)
    r = random.Random(3)
    pos = len(seq)
    for ln in (1, 1023, 1024, 1025):
        seq += "".join(r.choice("ACGT") for _ in range(ln))
        st.append(pos)
        en.append(pos + ln - 1)
        pt.append(r.randrange(6))
        pos += ln
    keep = [0 if i % 4 == 3 else 1 for i in range(60)] + [1, 1, 1, 1]
    case = dpc.as_rows(seq, st, en, pt, 3, [0, 20, 45, 64], keep, empty_read=1)
    # the last read: 150 more bases, a row that runs 500 past its end and one that starts 10 behind it
    case["text"] += "".join(r.choice("ACGT") for _ in range(150))
    case["read_off"][-1] += 150
    rl = int(case["read_off"][-1] - case["read_off"][-2])
    extra = np.array([[1, rl - 150, rl + 500, 0], [4, rl + 10, rl + 200, 0], [2, rl - 90, rl - 1, 0]], dtype=np.int32)
    case["rows"] = np.concatenate([case["rows"], extra])
    case["row_off"][-1] += 3
    case["keep"] = np.concatenate([case["keep"], np.array([1, 1, 0], dtype=np.uint8)])
    return ms, case


def test_host_plan_equals_the_host_fold():
    ms, case = _boundary_case()
    want, short, long_ = dpc.expected(case, ms, threads=4)
    assert long_ == 1 and 0 in np.diff(case["row_off"]) and 0 in case["keep"]
    got, pairs = lib.final_profile_host(case["text"], case["read_off"], case["rows"], case["row_off"], case["keep"], ms, threads=4)
    dpc.same(got, want)
    assert pairs == (short, long_)
    # 45 kept instances + 4 boundary rows + the row cut at its read's end; the row behind the end is no instance
    assert sum(formats.profile_instances(c) for c in got) == short + long_ == 45 + 4 + 1


def test_host_plan_sends_kilobase_sets_to_the_host():
    ms = [m.decode() for m in synth.make_monomers(2, seed=6, length=600)[1]]
    seq, st, en, pt = dpc.segments(ms, 12, seed=2)
    case = dpc.as_rows(seq, st, en, pt, 2, [0, 5, 12], [1] * 12)
    want, short, long_ = dpc.expected(case, ms, threads=4)
    got, pairs = lib.final_profile_host(case["text"], case["read_off"], case["rows"], case["row_off"], case["keep"], ms, threads=4)
    dpc.same(got, want)
    assert pairs == (0, 12)


def test_bad_arguments_are_refused():
    ms, case = _boundary_case()
    bad = case["rows"].copy()
    bad[5, 0] = 6
    for kw in (dict(rows=bad), dict(read_off=case["read_off"][::-1].copy())):
        a = dict(case, **kw)
        with pytest.raises(lib.SdError) as e:
            lib.final_profile_host(a["text"], a["read_off"], a["rows"], a["row_off"], a["keep"], ms)
        assert e.value.code == lib.SD_ERR_PARAM
