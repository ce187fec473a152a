"""Several devices in one process (--gpus / --devices, sd_run_files_devices): what is checked without a GPU -- the
command line's refusals, the C-ABI's argument checks and the host-only self-test of the batch dealing."""
import os
import subprocess
import sys

import pytest

from stringdecomposer_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
READS = os.path.join(GOLDEN, "test_data", "read.fa")
MONOS = os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa")


def _cli(args, out, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), READS, MONOS, "-o", out] + args,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)


def _no_outputs(out):
    return not any(os.path.exists(os.path.join(out, "final_decomposition" + s)) for s in ("_raw.tsv", ".tsv", "_alt.tsv"))


def test_multi_device_selftest():
    """The planner cuts contiguous, covering, equal-share batches, at least 2N of them for N = 1..16 entries; batches
    completing on several threads in shuffled order are consumed in batch order, slice by slice; a batch that fails on
    one pipeline, also while it drains, ends the job on every driver thread (the driver loop itself over a host-only
    model of the pipeline); an abort frees all."""
    lib.multi_device_selftest()


def test_cli_more_gpus_than_visible_is_refused(tmp_path):
    n = lib.device_count()
    out = str(tmp_path / "o")
    p = _cli(["--gpus", str(max(2, n + 1))], out)
    err = p.stderr.decode()
    assert p.returncode != 0
    assert "unrecognized arguments" not in err
    assert "HIP device" in err and "visible" in err, err
    assert _no_outputs(out)


def test_cli_missing_device_ordinal_is_refused(tmp_path):
    n = lib.device_count()
    out = str(tmp_path / "o")
    bad = max(1, n)
    p = _cli(["--devices", "0,%d" % bad], out)
    err = p.stderr.decode()
    assert p.returncode != 0
    assert "unrecognized arguments" not in err
    assert "device %d does not exist" % min(d for d in (0, bad) if d >= n) in err, err
    assert err.strip().count("\n") == 0   # one line
    assert _no_outputs(out)


def test_cli_gpus_and_devices_are_mutually_exclusive(tmp_path):
    p = _cli(["--gpus", "1", "--devices", "0"], str(tmp_path / "o"))
    assert p.returncode != 0
    assert "not allowed with" in p.stderr.decode()


@pytest.mark.parametrize("lst", ["0,x", "", "0,,1", "-1", "0;1"])
def test_cli_malformed_device_list_is_refused(tmp_path, lst):
    out = str(tmp_path / "o")
    p = _cli(["--devices", lst], out)
    assert p.returncode != 0
    assert "--devices" in p.stderr.decode() and "unrecognized arguments" not in p.stderr.decode()
    assert _no_outputs(out)


def test_cli_several_devices_inside_a_distributed_launch_is_refused(tmp_path):
    out = str(tmp_path / "o")
    p = _cli(["--gpus", "2"], out, env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0
    assert "WORLD_SIZE=2" in p.stderr.decode()
    assert _no_outputs(out)


def test_cli_zero_gpus_and_too_many_entries_are_refused(tmp_path):
    out = str(tmp_path / "o")
    p = _cli(["--gpus", "0"], out)
    assert p.returncode != 0 and "--gpus 0" in p.stderr.decode()
    p = _cli(["--devices", ",".join(["0"] * 17)], out)
    assert p.returncode != 0 and "at most 16" in p.stderr.decode()
    assert _no_outputs(out)


def test_c_abi_device_list_checks(tmp_path):
    """sd_run_files_devices checks the whole list before it starts anything: 0 or 17 entries and negative ordinals are
    SD_ERR_PARAM, an ordinal beyond the visible devices SD_ERR_NO_DEVICE naming it; no output file is created."""
    o = [str(tmp_path / x) for x in ("raw.tsv", "final.tsv", "alt.tsv")]
    n = lib.device_count()
    for devs, code, word in (([], lib.SD_ERR_PARAM, "device entries"), ([0] * 17, lib.SD_ERR_PARAM, "device entries"),
                             ([-1], lib.SD_ERR_PARAM, "device -1"), ([n + 98], lib.SD_ERR_NO_DEVICE, "device %d" % (n + 98))):
        with pytest.raises(lib.SdError) as ei:
            lib.run_files(READS, MONOS, o[0], o[1], o[2], devices=devs)
        assert ei.value.code == code and word in ei.value.msg, ei.value.msg
    assert not any(os.path.exists(x) for x in o)
