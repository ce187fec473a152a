"""Reads in device memory, the parts that need no device: the three C-ABI entries are declared, exported and reject bad
arguments before any work, and lib.DeviceReads builds the offset / length arrays the library is given (checked on a
stub with the tensor interface; torch is not needed)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from stringdecomposer_amd import lib

NEW = ("sd_stream_submit_dev", "sd_engine_load_reads_dev", "sd_pack_bases_dev")


class _Dev:
    def __init__(self, kind="cuda", index=0):
        self.type, self.index = kind, index


class StubTensor:
    """What lib.DeviceReads reads of a tensor: data_ptr / is_cuda / dtype / shape / stride / device."""

    def __init__(self, shape, strides=None, dtype="torch.uint8", cuda=True, ptr=0x7F0000001000, index=0):
        self.shape = tuple(shape)
        if strides is None:
            strides, acc = [], 1
            for d in reversed(self.shape):
                strides.insert(0, acc)
                acc *= d
        self._strides = tuple(strides)
        self.dtype = dtype
        self.is_cuda = cuda
        self.device = _Dev("cuda" if cuda else "cpu", index if cuda else None)
        self._ptr = ptr

    def data_ptr(self):
        return self._ptr

    def stride(self):
        return self._strides


def test_symbols_declared_exported_and_callable():
    L = lib.load()
    with open(os.path.join(ROOT, "include", "sd_hip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in lib.EXPORTS, name
        assert callable(getattr(L, name)), name


def test_null_handles_are_param_errors():
    L = lib.load()
    err = C.create_string_buffer(256)
    off = (C.c_int64 * 1)(0)
    ln = (C.c_int64 * 1)(10)
    n = C.c_int64()
    assert L.sd_stream_submit_dev(None, C.c_void_p(0x1000), off, ln, 1, None, err, 256) == lib.SD_ERR_PARAM
    assert L.sd_engine_load_reads_dev(None, C.c_void_p(0x1000), off, ln, 1, None, C.byref(n), err, 256) == lib.SD_ERR_PARAM


def test_pack_bases_dev_rejects_bad_arguments_before_any_work():
    L = lib.load()
    bad = C.c_int64(7)
    # a negative count, and chunks without a source: SD_ERR_PARAM, nothing touched
    assert L.sd_pack_bases_dev(None, None, None, -1, 0, None, None, None, None, C.byref(bad)) == lib.SD_ERR_PARAM
    assert L.sd_pack_bases_dev(None, None, None, 1, 0, None, None, None, None, C.byref(bad)) == lib.SD_ERR_PARAM
    assert bad.value == 7
    # no chunks: nothing to do
    assert L.sd_pack_bases_dev(None, None, None, 0, 0, None, None, None, None, C.byref(bad)) == lib.SD_OK
    assert bad.value == -1


def _rejected(*a, **kw):
    with pytest.raises(lib.SdError) as ei:
        lib.DeviceReads(*a, **kw)
    assert ei.value.code == lib.SD_ERR_PARAM
    return ei.value.msg


def test_device_reads_rejects_what_the_library_cannot_take():
    assert "uint8" in _rejected(StubTensor((100,), dtype="torch.int8"), [100])
    assert "uint8" in _rejected(StubTensor((100,), dtype="torch.float32"), [100])
    assert "HIP device" in _rejected(StubTensor((100,), cuda=False), [100])
    assert "contiguous" in _rejected(StubTensor((4, 50), strides=(100, 2)), [10] * 4)
    assert "contiguous" in _rejected(StubTensor((100,), strides=(2,)), [10])
    assert "longer" in _rejected(StubTensor((4, 50)), [10, 51, 10, 10])        # a length beyond the row width
    assert "rows" in _rejected(StubTensor((4, 50)), [10] * 5)                  # more lengths than rows
    assert "past the buffer" in _rejected(StubTensor((100,)), [60, 41])        # running sum beyond the tensor
    assert "past the buffer" in _rejected(StubTensor((100,)), [10], offsets=[95])
    assert "past the buffer" in _rejected((0x1000, 64, 0), [65])
    assert "past the buffer" in _rejected(StubTensor((100,)), [10], offsets=[-1])
    assert "offsets" in _rejected(StubTensor((100,)), [10, 10], offsets=[0])
    _rejected(StubTensor((2, 3, 4)), [1])
    _rejected(b"ACGT", [4])


def test_device_reads_arrays_1d():
    t = StubTensor((1000,), ptr=0x7F0000002003)
    d = lib.DeviceReads(t, [5, 1, 300, 694], stream=0)
    assert (d.ptr, d.nbytes, d.device, d.stream, d.n, d.bp) == (0x7F0000002003, 1000, 0, 0, 4, 1000)
    assert d.read_off == [0, 5, 6, 306] and d.read_lens == [5, 1, 300, 694]
    assert list(d.c_off)[:4] == d.read_off and list(d.c_lens)[:4] == d.read_lens
    assert d.data is t


def test_device_reads_arrays_2d_padded():
    # rows of width 50 in a buffer whose rows are 64 bytes apart (a slice of a wider tensor), on device 3
    t = StubTensor((4, 50), strides=(64, 1), index=3)
    d = lib.DeviceReads(t, [50, 1, 17, 49], stream=0x1234)
    assert d.read_off == [0, 64, 128, 192] and d.read_lens == [50, 1, 17, 49]
    assert (d.nbytes, d.device, d.stream) == (3 * 64 + 50, 3, 0x1234)
    # fewer lengths than rows: the first rows
    assert lib.DeviceReads(StubTensor((4, 50)), [7, 8], stream=0).read_off == [0, 50]


def test_device_reads_arrays_explicit_offsets():
    # any order, gaps, overlap: taken as given
    d = lib.DeviceReads(StubTensor((1000,)), [10, 20, 30], offsets=[900, 0, 5], stream=0)
    assert list(d.c_off)[:3] == [900, 0, 5] and list(d.c_lens)[:3] == [10, 20, 30]
    d = lib.DeviceReads(StubTensor((4, 50)), [50, 50], offsets=[150, 3], stream=0)
    assert d.read_off == [150, 3]
    d = lib.DeviceReads((0xABC000, 4096, 1), [4096])
    assert (d.ptr, d.nbytes, d.device, d.stream, d.read_off) == (0xABC000, 4096, 1, 0, [0])
    assert lib.DeviceReads((0, 0, 0), []).n == 0


def test_stream_none_without_a_tensor_module_is_the_null_stream():
    # the stub's module has no cuda.current_stream: the null stream
    assert lib.DeviceReads(StubTensor((10,)), [10]).stream == 0
