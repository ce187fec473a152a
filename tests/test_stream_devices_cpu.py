"""CPU-only checks of the stream on several devices (sd_stream_create_devices / sd_stream_create_final_devices,
lib.Stream(devices=...)): the device list is checked before any work starts, with the checks and messages of
sd_run_files_devices, and neither create runs without a GPU.  No device compute happens here."""
import ctypes as C

import pytest

from stringdecomposer_amd import lib, synth

COEF = (-31.48494996, 0.41784018, 0.69186882)


def _create(devices, n_devices=None, final=False, out=True, params=True, **kw):
    """Either create through the raw C-ABI, so that NULL arguments reach the library; returns (rc, message)."""
    L = lib.load()
    mn, ms = synth.make_monomers(4, seed=3)
    p = lib.make_params(**kw)
    bs = [lib._b(s) for s in ms]
    ml = (C.c_int32 * len(bs))(*[len(s) for s in bs])
    devs = None if devices is None else (C.c_int32 * max(len(devices), 1))(*devices)
    n = len(devices or []) if n_devices is None else n_devices
    h = C.c_void_p()
    err = C.create_string_buffer(4096)
    hp = C.byref(h) if out else None
    pp = C.byref(p) if params else None
    if final:
        rc = L.sd_stream_create_final_devices(hp, pp, devs, n, lib._strs(mn), lib._strs(bs), ml, len(bs), 1, 0, 1,
                                              (C.c_double * 3)(*COEF), err, 4096)
    else:
        rc = L.sd_stream_create_devices(hp, pp, devs, n, lib._strs(bs), ml, len(bs), 1, err, 4096)
    if h:
        L.sd_stream_destroy(h)
    return rc, err.value.decode()


@pytest.mark.parametrize("final", [False, True])
def test_device_list_checks(final):
    """An empty list, more than 16 entries, a NULL list or handle, and a negative ordinal are SD_ERR_PARAM; an ordinal
    beyond the visible devices is SD_ERR_NO_DEVICE -- with or without a GPU, as sd_run_files_devices."""
    who = "sd_stream_create_final_devices" if final else "sd_stream_create_devices"
    rc, msg = _create([], final=final)
    assert rc == lib.SD_ERR_PARAM and msg == who + ": 1 to 16 device entries"
    rc, msg = _create([0] * 17, final=final)
    assert rc == lib.SD_ERR_PARAM and msg == who + ": 1 to 16 device entries"
    rc, msg = _create(None, n_devices=2, final=final)
    assert rc == lib.SD_ERR_PARAM and msg == who + ": 1 to 16 device entries"
    rc, _ = _create([0, 0], out=False, final=final)
    assert rc == lib.SD_ERR_PARAM
    rc, _ = _create([0, 0], params=False, final=final)
    assert rc == lib.SD_ERR_PARAM
    rc, msg = _create([-1, 0], final=final)
    assert rc == lib.SD_ERR_PARAM and msg.startswith("device -1 does not exist (")
    rc, msg = _create([1000, 0], final=final)
    assert rc == lib.SD_ERR_NO_DEVICE and msg.startswith("device 1000 does not exist (")
    rc, _ = _create([0, 0], final=final, part_size=0)   # the parameters are checked as by the plain creates
    assert rc == lib.SD_ERR_PARAM


def test_device_list_messages_match_run_files():
    """The same list gives the same code and text from the stream and from sd_run_files_devices."""
    L = lib.load()
    p = lib.make_params()
    for devs in ([], [0] * 17, [-3], [0, 1000]):
        arr = (C.c_int32 * max(len(devs), 1))(*devs)
        err = C.create_string_buffer(4096)
        rc = L.sd_run_files_devices(b"r.fa", b"m.fa", C.byref(p), arr, len(devs), b"a", b"b", b"c", None, 0, 0,
                                    (C.c_double * 3)(*COEF), err, 4096)
        rc2, msg2 = _create(devs)
        assert rc2 == rc
        assert msg2.replace("sd_stream_create_devices", "sd_run_files_devices") == err.value.decode()


def test_stream_devices_without_device():
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    for final in (False, True):
        for devs in ([0], [0, 0], [0, 1, 2]):
            rc, msg = _create(devs, final=final)
            assert rc == lib.SD_ERR_NO_DEVICE and msg == "device 0 does not exist (0 HIP devices visible)"
    mn, ms = synth.make_monomers(6, seed=2)
    for kw in ({}, {"final": True, "mono_names": mn}, {"final": True, "mono_names": mn, "second_best": True}):
        for devs in ([0], [0, 0]):
            with pytest.raises(lib.SdError) as e:
                lib.Stream(ms, devices=devs, **kw)
            assert e.value.code == lib.SD_ERR_NO_DEVICE


def test_stream_bad_device_list_from_python():
    """lib.Stream(devices=...) raises SdError with the library's code, GPU or not."""
    mn, ms = synth.make_monomers(4, seed=1)
    for devs, code in (([], lib.SD_ERR_PARAM), (list(range(17)), lib.SD_ERR_PARAM), ([-1], lib.SD_ERR_PARAM),
                       ([0, 4096], lib.SD_ERR_NO_DEVICE)):
        for kw in ({}, {"final": True, "mono_names": mn}):
            with pytest.raises(lib.SdError) as e:
                lib.Stream(ms, devices=devs, **kw)
            assert e.value.code == code


def test_device_stats_of_no_stream():
    assert lib.load().sd_stream_device_stats(None, None, None, 0) == 0
