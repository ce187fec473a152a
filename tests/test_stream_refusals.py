"""The refusals of lib.Stream(...) for its modes and of the collect and peek calls, code and text, against
tests/golden/stream_refusals.json: callers match on these texts, which mode_refusal, wrong_call and on_oldest_job of
csrc/sd_stream.hip hold.  "create": every combination of final, profile,
device_rows, device_final, device_profile and devices=[0, 0] that is refused before any device is looked for.
"create_device": the combinations with a device list whose refusal follows the check of the list, so a device has to be
there.  "per_call": for one stream of each of the four modes, every collect and peek call that does not belong to the
mode, made with a job waiting, and the calls that do belong, made with none."""
import ctypes as C
import json
import os

import pytest
import torch  # noqa: F401  (collect_device and collect_final_device use it: its HIP runtime is loaded before the library's)

from conftest import GOLDEN

from stringdecomposer_amd import lib, synth

GOLD = os.path.join(GOLDEN, "stream_refusals.json")


def golden():
    with open(GOLD) as f:
        return json.load(f)


def create(kw):
    """lib.Stream(**kw) on four monomers -> {"code", "text"} of its refusal (code 0: it was made)"""
    mn, ms = synth.make_monomers(4, seed=2)
    try:
        lib.Stream(ms, mono_names=mn, **kw).close()
    except lib.SdError as e:
        return {"code": e.code, "text": e.msg}
    return {"code": lib.SD_OK, "text": ""}


def test_create_refusals():
    cases = golden()["create"]
    assert len(cases) == 50 and len({c["text"] for c in cases}) == 10
    for c in cases:
        assert c["code"] == lib.SD_ERR_PARAM
        assert create(c["args"]) == {"code": c["code"], "text": c["text"]}, c["args"]


@pytest.mark.gpu
def test_create_refusals_behind_the_device_list():
    cases = golden()["create_device"]
    assert len(cases) == 5 and len({c["text"] for c in cases}) == 3
    for c in cases:
        assert c["code"] == lib.SD_ERR_PARAM
        assert create(c["args"]) == {"code": c["code"], "text": c["text"]}, c["args"]


MODES = {"raw_host": {}, "raw_device": {"device_rows": True}, "final_host": {"final": True},
         "final_device": {"final": True, "device_final": True}}
# the calls that belong to a mode: the first collects the job through lib.Stream
OWN = {"raw_host": ["sd_stream_collect"], "raw_device": ["sd_stream_collect_dev", "sd_stream_peek_dev"],
       "final_host": ["sd_stream_collect_final"], "final_device": ["sd_stream_collect_final_dev", "sd_stream_peek_final_dev"]}


def c_calls(st):
    """name -> the C call on st with arguments that pass its argument check (a refused call touches none of them)"""
    L, h, e = st.L, st.h, st._err
    rows, frows, off, alt = C.POINTER(lib.Rec)(), C.POINTER(lib.FinalRec)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_double)()
    n, nr, nk = C.c_int64(), C.c_int32(), C.c_int32()
    buf = C.c_void_p(C.addressof(C.create_string_buffer(64)))   # (host memory; no refused call looks at it)
    return {
        "sd_stream_collect": lambda: L.sd_stream_collect(h, C.byref(rows), C.byref(off), C.byref(n), e, 4096),
        "sd_stream_collect_final": lambda: L.sd_stream_collect_final(h, C.byref(frows), C.byref(off), C.byref(n), C.byref(alt), e, 4096),
        "sd_stream_peek_dev": lambda: L.sd_stream_peek_dev(h, C.byref(nr), C.byref(n), e, 4096),
        "sd_stream_collect_dev": lambda: L.sd_stream_collect_dev(h, None, 0, buf, None, C.byref(n), e, 4096),
        "sd_stream_peek_final_dev": lambda: L.sd_stream_peek_final_dev(h, C.byref(nr), C.byref(n), C.byref(nk), e, 4096),
        "sd_stream_collect_final_dev": lambda: L.sd_stream_collect_final_dev(h, None, 0, buf, None, None, C.byref(n), e, 4096),
    }


def per_call(mode):
    """One stream of the mode, one read of one chunk: [{"mode", "call", "jobs", "code", "text"}] of every call that does
    not belong to it with the job waiting and, the job collected, of every call that does."""
    mn, ms = synth.make_monomers(4, seed=2)
    _, rs = synth.make_reads(ms, 1, read_len=1500, seed=5)
    assert len(lib.chunk_plan(len(rs[0]))) == 1
    st = lib.Stream(ms, mono_names=mn, **MODES[mode])
    try:
        calls = c_calls(st)
        out = []

        def refused(name, jobs):
            st._err.value = b""
            code = calls[name]()
            out.append({"mode": mode, "call": name, "jobs": jobs, "code": code, "text": st._err.value.decode()})

        st.submit(rs)
        for name in sorted(calls):
            if name not in OWN[mode]:
                refused(name, 1)
        # the refused calls left the job: it is collected, with its rows
        got = {"raw_host": st.collect, "raw_device": st.collect_device, "final_host": st.collect,
               "final_device": st.collect_final_device}[mode]()
        n_rows = got if mode == "raw_host" else len(got.rows) if mode == "final_host" else got.n_rows
        assert n_rows > 0
        for name in OWN[mode]:
            refused(name, 0)
        return out
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_per_call_refusals(mode):
    want = [c for c in golden()["per_call"] if c["mode"] == mode]
    assert len(want) == 6 and all(c["code"] == lib.SD_ERR_PARAM and c["text"] for c in want)
    assert sum(c["jobs"] for c in want) == 6 - len(OWN[mode])
    for c in want:
        if not c["jobs"]:
            assert c["text"] == c["call"] + " without a submitted job"
    assert per_call(mode) == want
