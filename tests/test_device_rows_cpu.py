"""Rows assembled on the device, the parts that need no device: the piece functions the kernels run (exit tables, their
composition, keep flags -- csrc/sd_seam_dev.hpp through sd_seam_pieces_selftest) against the literal host merge, and the
new C-ABI entries: exported, declared, refusing bad arguments before any work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seam_cases
from conftest import ROOT

from stringdecomposer_amd import lib, synth

NEW = ("sd_stream_peek_dev", "sd_stream_collect_dev", "sd_engine_rows_dev", "sd_seam_merge_dev", "sd_seam_pieces_selftest")


@pytest.fixture(scope="module")
def cases():
    lists = seam_cases.all_lists()
    return lists, seam_cases.pack(lists), seam_cases.expected(lists)


def test_lists_do_merge(cases):
    lists, _, exp = cases
    assert len(lists) >= 3000
    dropping = sum(1 for lst, e in zip(lists, exp) if len(e) < len(lst))
    assert dropping * 3 >= len(lists), "%d of %d lists drop a record" % (dropping, len(lists))


@pytest.mark.parametrize("piece", seam_cases.PIECES + [0])
def test_pieces_equal_the_literal_merge(cases, piece):
    lists, (recs, off), exp = cases
    rows, row_off = lib.seam_pieces_host(recs, off, piece)
    assert int(row_off[0]) == 0 and int(row_off[-1]) == len(rows) == sum(len(e) for e in exp)
    for r in range(len(lists)):
        assert seam_cases.rows_of(rows, row_off, r) == exp[r], "list %d (%d records), piece %d" % (r, len(lists[r]), piece)


@pytest.mark.parametrize("name", sorted(seam_cases.handmade()))
def test_handmade_lists(name):
    lst = seam_cases.handmade()[name]
    exp = lib.seam_merge(lst)
    assert len(exp) < len(lst), "the list was made to drop records"
    for piece in seam_cases.PIECES + [0]:
        recs, off = seam_cases.pack([lst, [], lst])
        rows, row_off = lib.seam_pieces_host(recs, off, piece)
        assert [seam_cases.rows_of(rows, row_off, r) for r in range(3)] == [exp, [], exp], "piece %d" % piece


def test_handmade_lists_are_what_they_say():
    """The jumps lie where the names put them (the lists would test nothing if an edit moved them)."""
    hm = seam_cases.handmade()
    kept = {k: [r[1] // 100 for r in lib.seam_merge(v)] for k, v in hm.items()}
    assert kept["jump_to_end"] == [0]
    assert kept["jump_to_end_two_pieces"] == [0, 1, 2]
    assert kept["kept_unchecked_first_of_piece"] == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]
    assert kept["lands_on_boundary"] == [0, 1, 2, 3, 4, 5, 7] + list(range(8, 20))
    assert kept["lands_on_boundary_plus_7"] == list(range(8)) + [14] + list(range(15, 20))
    assert kept["chained_jumps"] == list(range(8)) + [14, 15, 17] + list(range(18, 24)) + [30] + list(range(31, 40))


def test_symbols_exported_and_declared():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert re.search(r"#define\s+SD_FLAG_DEVICE_ROWS\s+1024\b", header)
    assert lib.FLAG_DEVICE_ROWS == 1024


@pytest.mark.parametrize("piece", [1, 3, 7, -1])
def test_short_pieces_are_refused(piece):
    recs, off = seam_cases.pack([seam_cases._plain(10)])
    with pytest.raises(lib.SdError) as e:
        lib.seam_pieces_host(recs, off, piece)
    assert e.value.code == lib.SD_ERR_PARAM
    n = C.c_int64()
    # (device pointers are not looked at before the arguments are checked)
    rc = lib.load().sd_seam_merge_dev(None, off.ctypes.data, 1, piece, 0, None, None, off.ctypes.data, C.byref(n))
    assert rc == lib.SD_ERR_PARAM


def test_bad_offsets_are_refused():
    recs, _ = seam_cases.pack([seam_cases._plain(10)])
    rows = np.empty((10, 4), dtype=np.int32)
    out = np.empty(3, dtype=np.int64)
    n = C.c_int64()
    for off in ([1, 5, 10], [0, 7, 5]):
        o = np.array(off, dtype=np.int64)
        rc = lib.load().sd_seam_pieces_selftest(recs.ctypes.data, o.ctypes.data, 2, 8, rows.ctypes.data, out.ctypes.data, C.byref(n))
        assert rc == lib.SD_ERR_PARAM


def test_null_handles_are_refused():
    L = lib.load()
    err = C.create_string_buffer(256)
    n, nr = C.c_int64(), C.c_int32()
    assert L.sd_stream_peek_dev(None, C.byref(nr), C.byref(n), err, 256) == lib.SD_ERR_PARAM
    assert L.sd_stream_collect_dev(None, None, 0, None, None, C.byref(n), err, 256) == lib.SD_ERR_PARAM
    assert L.sd_engine_rows_dev(None, None, 0, None, None, C.byref(n), err, 256) == lib.SD_ERR_PARAM


def test_final_mode_refuses_device_rows():
    """Checked before any device is touched: the message says why."""
    mn, ms = synth.make_monomers(4, seed=2)
    with pytest.raises(lib.SdError) as e:
        lib.Stream(ms, final=True, mono_names=mn, device_rows=True)
    assert e.value.code == lib.SD_ERR_PARAM
    assert "final" in e.value.msg and "DEVICE_ROWS" in e.value.msg


def test_device_entries_without_device():
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    recs, off = seam_cases.pack([seam_cases._plain(10)])
    n = C.c_int64()
    rc = lib.load().sd_seam_merge_dev(recs.ctypes.data, off.ctypes.data, 1, 8, 0, None, recs.ctypes.data, off.ctypes.data, C.byref(n))
    assert rc == lib.SD_ERR_NO_DEVICE
    mn, ms = synth.make_monomers(4, seed=2)
    with pytest.raises(lib.SdError) as e:
        lib.Stream(ms, device_rows=True)
    assert e.value.code == lib.SD_ERR_NO_DEVICE
