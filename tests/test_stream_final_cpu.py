"""CPU-only checks of the final mode of the stream (sd_stream_create_final / lib.Stream(final=True)): its argument checks
come before any device work, it refuses to run without a GPU, and formats.final_rows turns its typed rows into the
command line's text.  No device compute happens here."""
import ctypes as C

import numpy as np
import pytest

from stringdecomposer_amd import formats, lib, synth

COEF = (-31.48494996, 0.41784018, 0.69186882)


def _create_final(names, seqs, lens=None, n_mono=None, coef=COEF, **kw):
    """sd_stream_create_final through the raw C-ABI, so that NULL arguments reach the library."""
    L = lib.load()
    p = lib.make_params(**kw)
    ms = [lib._b(s) for s in seqs]
    ml = None if lens is False else (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms])
    h = C.c_void_p()
    err = C.create_string_buffer(4096)
    rc = L.sd_stream_create_final(C.byref(h), C.byref(p), None if names is None else lib._strs(names), lib._strs(ms), ml,
                                  len(ms) if n_mono is None else n_mono, 1, 0, 1,
                                  None if coef is None else (C.c_double * 3)(*coef), err, 4096)
    if h:
        L.sd_stream_destroy(h)
    return rc, err.value.decode()


def test_final_stream_argument_checks_come_first():
    """Missing names, no monomers, no coefficients and bad parameters are SD_ERR_PARAM with or without a GPU."""
    mn, ms = synth.make_monomers(4, seed=3)
    rc, msg = _create_final(None, ms)
    assert rc == lib.SD_ERR_PARAM and "name" in msg
    rc, _ = _create_final(mn, ms, n_mono=0)
    assert rc == lib.SD_ERR_PARAM
    rc, _ = _create_final(mn, ms, n_mono=-1)
    assert rc == lib.SD_ERR_PARAM
    rc, _ = _create_final(mn, ms, lens=False)
    assert rc == lib.SD_ERR_PARAM
    rc, msg = _create_final(mn, ms, coef=None)
    assert rc == lib.SD_ERR_PARAM and "coefficients" in msg
    rc, _ = _create_final(mn, ms, part_size=0)
    assert rc == lib.SD_ERR_PARAM
    rc, _ = _create_final(mn, [ms[0], b""] + list(ms[2:]))
    assert rc == lib.SD_ERR_EMPTY
    with pytest.raises(lib.SdError) as e:   # a name list that does not match the monomers (caught in Python)
        lib.Stream(ms, final=True, mono_names=mn[:-1])
    assert e.value.code == lib.SD_ERR_PARAM


def test_final_stream_entry_points_reject_null_handles():
    L = lib.load()
    rows, off, alt = C.POINTER(lib.FinalRec)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_double)()
    n = C.c_int64()
    assert L.sd_stream_collect_final(None, C.byref(rows), C.byref(off), C.byref(n), C.byref(alt), None, 0) == lib.SD_ERR_PARAM
    nk = C.c_int32()
    assert L.sd_stream_keys(None, None, 0, C.byref(nk)) == lib.SD_ERR_PARAM
    v = (C.c_double * 4)()
    assert L.sd_stream_final_stats(None, v) == lib.SD_ERR_PARAM


def test_final_stream_without_device():
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    mn, ms = synth.make_monomers(6, seed=2)
    for sb in (False, True):
        with pytest.raises(lib.SdError) as e:
            lib.Stream(ms, final=True, mono_names=mn, second_best=sb)
        assert e.value.code == lib.SD_ERR_NO_DEVICE
    rc, _ = _create_final(mn, ms)
    assert rc == lib.SD_ERR_NO_DEVICE


def test_final_dtype_is_the_c_layout():
    dt = lib.final_dtype()
    assert dt.itemsize == C.sizeof(lib.FinalRec) == 80
    for f, _ in lib.FinalRec._fields_:
        assert dt.fields[f][1] == getattr(lib.FinalRec, f).offset, f


def test_final_rows_format_as_the_command_line():
    """formats.final_rows on hand-made typed rows: key indices become names (-1: None), identities print with %.2f,
    and every kept block gives one _alt row per key with '*' on its own key."""
    keys = ["m0", "m0'", "m1", "m1'"]
    dt = lib.final_dtype()
    rows = np.zeros(3, dtype=dt)
    rows[0] = (0, 10, 180, 1, 2, 1, 0, 91.234, 80.0, 95.0, 90.005, 1)
    rows[1] = (0, 181, 350, 2, -1, -1, -1, 70.0, -1.0, -1.0, -1.0, 0)
    rows[2] = (1, 0, 170, 0, 3, 0, 3, 100.0, 99.999, 100.0, 12.5, 1)
    alt = np.array([[1.0, 91.234, 80.0, 3.0], [0.0, 0.0, 70.0, 0.0], [100.0, 1.0, 2.0, 99.999]])
    fin, alts = formats.final_rows(lib.FinalRows(rows, np.array([0, 2, 3, 3]), alt), ["rA", "rB", "rC"], keys)
    assert formats.format_final(fin) == (
        "rA\tm0'\t10\t180\t91.23\tm1\t80.00\tm0'\t95.00\tm0\t90.00\t+\n"   # (90.005 is 90.00499... as a double)
        "rA\tm1\t181\t350\t70.00\tNone\t-1.00\tNone\t-1.00\tNone\t-1.00\t?\n"
        "rB\tm0\t0\t170\t100.00\tm1'\t100.00\tm0\t100.00\tm1'\t12.50\t+\n")
    text = formats.format_alt(alts)
    assert text.splitlines()[:4] == ["rA\tm0\t10\t180\t1.00\t-", "rA\tm0'\t10\t180\t91.23\t*",
                                     "rA\tm1\t10\t180\t80.00\t-", "rA\tm1'\t10\t180\t3.00\t-"]
    assert len(alts) == 12 and [a.best for a in alts].count(True) == 3
    # the text round-trips through the readers
    assert formats.format_final(formats.parse_final(formats.format_final(fin))) == formats.format_final(fin)
    fin_light, alt_light = formats.final_rows((rows, None, None), ["rA", "rB"], keys)
    assert alt_light == [] and len(fin_light) == 3
