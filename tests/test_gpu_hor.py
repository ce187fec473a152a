"""--hor behind a decomposition on the device: the command line's three files against formats applied to the host form on
the rows it wrote, and the three reference TSVs against a run without the flag."""
import os
import subprocess
import sys

import pytest

import test_hor_cpu as cpu
from conftest import GOLDEN
from stringdecomposer_amd import formats, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = os.path.join(GOLDEN, "test_data")
THREADS = 8


def run_cli(out_dir, *extra):
    cmd = [sys.executable, "-m", "stringdecomposer_amd.main", os.path.join(TD, "read.fa"), cpu.DXZ1, "-o", out_dir, "-t", "4"] + list(extra)
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=150)


def test_command_line(tmp_path):
    plain, hor = str(tmp_path / "plain"), str(tmp_path / "hor")
    r = run_cli(plain)
    assert r.returncode == 0, r.stderr
    r = run_cli(hor, "--hor")
    assert r.returncode == 0, r.stderr
    for f in ("final_decomposition.tsv", "final_decomposition_raw.tsv", "final_decomposition_alt.tsv"):
        a, b = os.path.join(plain, f), os.path.join(hor, f)
        if os.path.exists(a) or os.path.exists(b):
            assert open(a, "rb").read() == open(b, "rb").read(), f
    cols, mono, reads = cpu.golden_columns(os.path.join(hor, "final_decomposition.tsv"), cpu.DXZ1)
    host = lib.hor_rows(*cols, 12, threads=THREADS)
    for name, rows, fmt in (("_hor.tsv", formats.hor_units(host, reads), formats.format_hor),
                            ("_hor_orders.tsv", formats.hor_orders(host, mono), formats.format_hor_orders),
                            ("_hor_variants.tsv", formats.hor_variants(host), formats.format_hor_variants)):
        with open(os.path.join(hor, "final_decomposition" + name), newline="") as f:
            assert f.read() == fmt(rows), name
    units = formats.read_hor(os.path.join(hor, "final_decomposition_hor.tsv"))
    assert len(units) == 47 and sum(u.name == "1-12" and u.complete == 1 for u in units) == 45 and {u.strand for u in units} == {"-"}
    assert [v.name for v in formats.read_hor_variants(os.path.join(hor, "final_decomposition_hor_variants.tsv"))][0] == "1-12"


def test_command_line_with_a_gap_and_beside_other_reports(tmp_path):
    out = str(tmp_path / "o")
    r = run_cli(out, "--hor", "--hor-gap", "400", "--hor-min-count", "2", "-i", "95", "--second-best", "--lags", "2")
    assert r.returncode == 0, r.stderr
    orders = formats.read_hor_orders(os.path.join(out, "final_decomposition_hor_orders.tsv"))
    assert {o.kind for o in orders} == {"path"} and "".join(o.monomer[0] for o in orders) == "FGHJKACDE" and orders[-1].count == 0
    assert os.path.getsize(os.path.join(out, "final_decomposition_lags.tsv")) > 0
