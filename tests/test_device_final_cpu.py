"""Final rows selected on the device (SD_FLAG_DEVICE_FINAL), the parts that need no device: the new C-ABI entries are
exported and declared, the flag is refused where it cannot work before any device is touched, and the host's selection
on identity words (sd_final_select_host: PostProcessor::select, what the kernels of csrc/sd_final_dev.hip must equal)
equals an independent Python restatement of the reference command line's rule on word sets built to hit its corners."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import final_select_cases as fsc
from conftest import ROOT

from stringdecomposer_amd import lib, synth

NEW = ("sd_stream_peek_final_dev", "sd_stream_collect_final_dev", "sd_final_select_dev", "sd_final_select_host")


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    m = re.search(r"#define\s+SD_FLAG_DEVICE_FINAL\s+(\d+)\b", header)
    assert m and int(m.group(1)) == lib.FLAG_DEVICE_FINAL == 2048


def _refused(**kw):
    mn, ms = synth.make_monomers(4, seed=2)
    with pytest.raises(lib.SdError) as e:
        lib.Stream(ms, mono_names=mn, device_final=True, **kw)
    assert e.value.code == lib.SD_ERR_PARAM
    return e.value.msg


def test_refused_on_a_raw_stream():
    msg = _refused()
    assert "DEVICE_FINAL" in msg and "final-mode" in msg


def test_refused_with_profile():
    msg = _refused(final=True, profile=True)
    assert "DEVICE_FINAL" in msg and "PROFILE" in msg


def test_refused_with_several_devices():
    """(checked before the device list itself: no device is looked for)"""
    msg = _refused(final=True, devices=[0, 0])
    assert "DEVICE_FINAL" in msg and "one entry" in msg


def test_refused_with_device_rows():
    """The refusal of SD_FLAG_DEVICE_ROWS in final mode stands, in its own words."""
    msg = _refused(final=True, device_rows=True)
    assert "final" in msg and "DEVICE_ROWS" in msg


def test_null_handles_are_refused():
    L = lib.load()
    err = C.create_string_buffer(256)
    n, nr, nk = C.c_int64(), C.c_int32(), C.c_int32()
    assert L.sd_stream_peek_final_dev(None, C.byref(nr), C.byref(n), C.byref(nk), err, 256) == lib.SD_ERR_PARAM
    assert L.sd_stream_collect_final_dev(None, None, 0, None, None, None, C.byref(n), err, 256) == lib.SD_ERR_PARAM


def test_without_a_device():
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    mn, ms = synth.make_monomers(4, seed=2)
    with pytest.raises(lib.SdError) as e:
        lib.Stream(ms, final=True, mono_names=mn, device_final=True)
    assert e.value.code == lib.SD_ERR_NO_DEVICE


def _check(case, min_identity):
    want, want_off, want_alt, want_und, ties = fsc.select(case, min_identity)
    got, und = lib.final_select_host(case["names"], case["seqs"], case["rows"], case["row_off"], case["widx"], case["words"],
                                     case["hwords"], case["read_len"], min_identity=min_identity,
                                     second_best=case["second_best"], lr_coef=fsc.COEF)
    assert und == want_und
    assert got.row_off.tolist() == want_off
    assert got.rows.tolist() == want
    if case["second_best"]:
        assert got.alt.tolist() == want_alt
    else:
        assert got.alt is None
    return want, want_und, ties


@pytest.mark.parametrize("min_identity", [0, 95])
@pytest.mark.parametrize("second_best", [False, True])
@pytest.mark.parametrize("n_mono", [1, 3, 12])
def test_host_selection_equals_the_python_rule(n_mono, second_best, min_identity):
    case = fsc.make(n_mono, second_best)
    n = len(case["rows"])
    want, und, (tie_k, tie_h) = _check(case, min_identity)
    # four words decide nothing and one segment is long enough for the split; the 19-kb one is not
    assert und == 5
    if second_best and n_mono > 1:
        assert tie_k * 3 >= n and tie_h * 3 >= n, "ties: %d among keys, %d among homopolymer ranks, of %d rows" % (tie_k, tie_h, n)
    if second_best and n_mono == 1:
        # T = 2: the one other key cannot tie with itself, and the two homopolymer words are equal with probability
        # (3^2 + 2^2 + 2^2 + 1 + 1) / 9^2 = 19 / 81 = 23.5 % (the multiplicities of the five identities among fsc.PAIRS):
        # 469 of 2 000 rows expected, standard deviation 19 -- a fifth of the rows is five deviations below that
        assert tie_k == 0 and tie_h * 5 >= n, "ties: %d among homopolymer ranks, of %d rows" % (tie_h, n)
    if min_identity:
        assert 0 < len(want) < n - und, "the threshold must split the rows"
        assert min(r[7] for r in want) == 95.0
    else:
        assert len(want) == n - und
    if second_best and n_mono == 1:   # the only other key is the reverse complement
        assert {r[4] for r in want} == {0, 1} and all(r[3] + r[4] == 1 for r in want)
    if n_mono >= 3:
        assert len(set(case["names"])) == n_mono - 1   # one repeated name: n_keys < T


def test_rows_at_the_threshold():
    """d = 5, m = 95 and d = 10, m = 190 are exactly 95 and kept at -i 95; 94.9 and 94 are dropped."""
    case = fsc.make(3, True)
    want, _, _, _, _ = fsc.select(case, 95)
    kept = {(r[1], r[2]) for r in want}
    at = lambda b: (int(case["rows"][b, 1]), int(case["rows"][b, 2]))   # noqa: E731
    assert at(3) in kept and at(6) in kept and at(4) not in kept and at(5) not in kept
    got, _ = lib.final_select_host(case["names"], case["seqs"], case["rows"], case["row_off"], case["widx"], case["words"],
                                   case["hwords"], case["read_len"], min_identity=95, second_best=True, lr_coef=fsc.COEF)
    assert {(int(r["start"]), int(r["end"])) for r in got.rows} == kept


def test_padding_is_zero_and_empty_inputs():
    case = fsc.make(3, True)
    got, _ = lib.final_select_host(case["names"], case["seqs"], case["rows"], case["row_off"], case["widx"], case["words"],
                                   case["hwords"], case["read_len"], second_best=True, lr_coef=fsc.COEF)
    raw = np.frombuffer(got.rows.tobytes(), dtype=np.uint8).reshape(-1, 80)
    assert not raw[:, 4:8].any() and not raw[:, 73:80].any()
    none = fsc.make(3, True, no_reads=True)
    got, und = lib.final_select_host(none["names"], none["seqs"], none["rows"], none["row_off"], none["widx"], none["words"],
                                     none["hwords"], none["read_len"], second_best=True, lr_coef=fsc.COEF)
    assert len(got.rows) == 0 and got.row_off.tolist() == [0] and und == 0


def test_bad_arguments_are_refused():
    case = fsc.make(3, False, n_rows=50)
    bad = case["widx"].copy()
    bad[7] = len(case["words"])
    for kw in (dict(widx=bad), dict(row_off=case["row_off"][::-1].copy())):
        a = dict(case, **kw)
        with pytest.raises(lib.SdError) as e:
            lib.final_select_host(a["names"], a["seqs"], a["rows"], a["row_off"], a["widx"], a["words"], None, a["read_len"],
                                  lr_coef=fsc.COEF)
        assert e.value.code == lib.SD_ERR_PARAM
