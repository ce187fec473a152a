"""The device prefix scan of the post-pass units (csrc/sd_scan_dev.hpp) alone, through sd_scan_selftest: at the edges of a
wave, of a tile of 256 items and of a round of 256 tiles of the one-workgroup pass over the tile sums, with values whose
total leaves 32 bits, and with the tile sums kept as int32 the way the units that count flags keep them.  The expected
value is numpy's cumsum in int64 in every case."""
import numpy as np
import pytest
import torch   # noqa: F401  (before the library is loaded: one HIP runtime in the process)

from stringdecomposer_amd import lib

pytestmark = pytest.mark.gpu

# 65 535 .. 65 537 items are 256 and 257 tiles (the second round of the pass over the tile sums); 131 075 items are more than
# two rounds and a last tile of 3 items
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 65535, 65536, 65537, 131075]


def _values(kind, n):
    if kind == "zeros":
        return np.zeros(n, dtype=np.int64)
    if kind == "ones":
        return np.ones(n, dtype=np.int64)
    r = np.random.default_rng(n + 1)
    return r.integers(0, (1024 if kind == "to_1024" else 1 << 40) + 1, size=n, dtype=np.int64)


def _expected(v):
    want = np.zeros(len(v) + 1, dtype=np.int64)
    np.cumsum(v, dtype=np.int64, out=want[1:])
    return want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["zeros", "ones", "to_1024", "to_2_40"])
def test_scan_equals_cumsum(kind, n):
    v = _values(kind, n)
    want = _expected(v)
    if kind == "to_2_40" and n >= 511:
        assert want[-1] > 1 << 32 and (want[n // 2:] > 1 << 32).all()   # the total and most bases lie beyond 32 bits
    got = lib.scan_selftest(v)
    assert got.shape == want.shape and (got == want).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["zeros", "ones", "to_1024"])
def test_scan_with_int32_tile_sums(kind, n):
    """a tile holds at most 256 x 1024: its sum fits an int32, the bases and the total are int64 all the same"""
    v = _values(kind, n)
    got = lib.scan_selftest(v, tile_sums_32=True)
    assert (got == _expected(v)).all()
