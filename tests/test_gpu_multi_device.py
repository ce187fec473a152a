"""Several devices in one process (--gpus / --devices, sd_run_files_devices) on the GPU.  Repeated ordinals run several
pipelines on one device, which is how the form is checked on a machine with one GPU; every output must be
byte-identical to the single-device path and to the reference.  Every run is a child process, one at a time."""
import hashlib
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "bin", "stringdecomposer")
OUTS = ("final_decomposition_raw.tsv", "final_decomposition.tsv", "final_decomposition_alt.tsv")

pytestmark = pytest.mark.gpu


def _cli(args, timeout=600):
    return subprocess.run([sys.executable, BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)


def _child(code, timeout=900):
    """Runs `code` in a fresh Python process (the repository on its path); returns its last stdout line as JSON."""
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + textwrap.dedent(code)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def _read(out, fn):
    with open(os.path.join(out, fn), "rb") as f:
        return f.read()


def _device_count():
    return _child("from stringdecomposer_amd import lib; import json; print(json.dumps(lib.device_count()))", timeout=120)


FINAL_CASES = ["td_second_best", "td_light", "syn64_second_best", "tiled_second_best", "long_block"]


@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
@pytest.mark.parametrize("name", FINAL_CASES)
def test_reference_goldens_with_repeated_devices(name, devices, tmp_path):
    """The committed outputs of the unmodified reference command line, through --devices 0,0 and 0,0,0."""
    d = os.path.join(GOLDEN, "final", name)
    with open(os.path.join(d, "params.json")) as f:
        c = json.load(f)
    out = str(tmp_path / "o")
    p = _cli([os.path.join(GOLDEN, x) for x in c["inputs"]] + ["-o", out, "-t", "8", "--devices", devices] + c["args"])
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert hashlib.sha256(_read(out, OUTS[0])).hexdigest() == c["raw_sha256"]
    with open(os.path.join(d, "final.tsv"), "rb") as f:
        assert _read(out, OUTS[1]) == f.read()
    assert hashlib.sha256(_read(out, OUTS[2])).hexdigest() == c["alt_sha256"]
    with open(os.path.join(out, "stringdecomposer.log")) as f:
        assert "HIP devices of this process: " + devices in f.read()


def test_both_data_forms_many_batches_match_single_device(tmp_path):
    """A synthetic read set and the one-sequence read.fa, cut into more than 6 batches: the files of 2 and 3 pipelines
    on device 0 equal the single-device run's, and every entry was dealt at least one batch; a one-entry list (the
    n_devices == 1 route of sd_run_files_devices) gives the same files and the same batch counts as the plain call."""
    res = _child("""
        import json, os
        from stringdecomposer_amd import lib, synth
        d = %r
        mn, ms = synth.make_monomers(12, seed=5)
        rn, rs = synth.make_reads(ms, 40, read_len=30000, seed=5)
        synth.write_fasta(os.path.join(d, "r.fa"), rn, rs, width=80)
        synth.write_fasta(os.path.join(d, "m.fa"), mn, ms)
        forms = [(os.path.join(d, "r.fa"), os.path.join(d, "m.fa"), 40000),
                 (%r, %r, 15000)]
        res = []
        for k, (rfa, mfa, rows) in enumerate(forms):
            for sb in (False, True):
                got = {}
                for devs in (None, [0], [0, 0], [0, 0, 0]):
                    tag = "%%d_%%d_%%s" %% (k, sb, devs and len(devs))
                    o = [os.path.join(d, tag + x) for x in ("raw.tsv", "fin.tsv", "alt.tsv")]
                    lib.run_files(rfa, mfa, o[0], o[1], o[2], second_best=sb, threads=8, max_batch_rows=rows, devices=devs)
                    st = lib.last_run_device_stats()
                    got[tag] = ([open(x, "rb").read() for x in o], st, lib.last_run_stats()["batches"])
                base = got["%%d_%%d_None" %% (k, sb)]
                for devs in (1, 2, 3):
                    files, st, nb = got["%%d_%%d_%%d" %% (k, sb, devs)]
                    res.append(dict(form=k, second_best=sb, devices=devs, same=files == base[0], rows=files[0].count(b"\\n"),
                                    alt=len(files[2]), entries=[e["batches"] for e in st], batches=nb,
                                    busy=[e["busy_ms"] for e in st], base_batches=base[2],
                                    base_entries=[e["batches"] for e in base[1]]))
        print(json.dumps(res))
    """ % (str(tmp_path), os.path.join(GOLDEN, "test_data", "read.fa"), os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa")))
    assert len(res) == 12
    for r in res:
        if r["devices"] == 1:
            assert r["batches"] == r["base_batches"] and r["entries"] == r["base_entries"] == [r["batches"]], r
        assert r["same"], r
        assert r["rows"] > 100 and (r["alt"] > 0) == r["second_best"], r
        assert len(r["entries"]) == r["devices"] and min(r["entries"]) >= 1, r
        assert sum(r["entries"]) == r["batches"] > 6, r
        assert min(r["busy"]) > 0, r


def test_full_size_c5_and_c4_raw_tsv_match_the_reference_with_two_pipelines(tmp_path):
    """C5 (one 200-Mb sequence, -s -2,-3,-4,2) and C4 (256 reads x 50 kb, 64 monomers) through
    lib.run_files(devices=[0, 0]): the raw TSVs hash to what the reference binary printed."""
    res = _child("""
        import hashlib, json, os
        from stringdecomposer_amd import lib, synth
        d = %r
        th = min(64, os.cpu_count() or 1)
        out = {}
        mn, ms = synth.make_monomers(12, seed=1)
        rn, rs = synth.make_reads(ms, 100, read_len=2_000_000, seed=7)
        synth.write_fasta(os.path.join(d, "c5.fa"), ["chr"], [b"".join(rs)], width=80)
        synth.write_fasta(os.path.join(d, "c5m.fa"), mn, ms)
        del rs
        o = [os.path.join(d, x) for x in ("raw.tsv", "fin.tsv", "alt.tsv")]
        lib.run_files(os.path.join(d, "c5.fa"), os.path.join(d, "c5m.fa"), o[0], o[1], o[2], scoring=(-2, -3, -4, 2),
                      threads=th, devices=[0, 0])
        out["c5"] = hashlib.sha256(open(o[0], "rb").read()).hexdigest()
        out["c5_entries"] = [e["batches"] for e in lib.last_run_device_stats()]
        os.remove(os.path.join(d, "c5.fa"))
        mn, ms = synth.make_monomers(64, seed=11)
        rn, rs = synth.make_reads(ms, 256, read_len=50000, seed=14)
        synth.write_fasta(os.path.join(d, "c4.fa"), rn, rs, width=80)
        synth.write_fasta(os.path.join(d, "c4m.fa"), mn, ms)
        lib.run_files(os.path.join(d, "c4.fa"), os.path.join(d, "c4m.fa"), o[0], o[1], o[2], threads=th, devices=[0, 0])
        out["c4"] = hashlib.sha256(open(o[0], "rb").read()).hexdigest()
        out["c4_entries"] = [e["batches"] for e in lib.last_run_device_stats()]
        print(json.dumps(out))
    """ % str(tmp_path), timeout=1200)
    with open(os.path.join(GOLDEN, "fullsize_sha256.json")) as f:
        gold = json.load(f)
    assert res["c5"] == gold["c5"]["sha256"]
    assert res["c4"] == gold["c4"]["sha256"]
    assert min(res["c5_entries"]) >= 1 and min(res["c4_entries"]) >= 1


def test_record_stream_with_two_pipelines_equals_single_device(tmp_path):
    inp = [os.path.join(GOLDEN, "test_data", "read.fa"), os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa")]
    outs = {}
    for tag, extra in (("one", []), ("two", ["--devices", "0,0"])):
        out = str(tmp_path / tag)
        p = _cli(inp + ["-o", out, "-t", "8", "--second-best", "--records", "-b", "2000"] + extra)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        outs[tag] = [_read(out, fn) for fn in OUTS + ("final_decomposition_raw.sdr",)]
    assert outs["one"] == outs["two"]
    assert len(outs["two"][3]) > 0


def test_other_flags_with_repeated_devices(tmp_path):
    """-s, --ed_thr, -b / -v and -i through --devices 0,0 equal the single-device run."""
    inp = [os.path.join(GOLDEN, "test_data", "read.fa"), os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa")]
    flags = ["--scoring=-2,-3,-4,2", "--ed_thr", "40", "-b", "3000", "-v", "400", "-i", "60", "--second-best"]
    outs = {}
    for tag, extra in (("one", []), ("two", ["--devices", "0,0"])):
        out = str(tmp_path / tag)
        p = _cli(inp + ["-o", out, "-t", "8"] + flags + extra)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        outs[tag] = [_read(out, fn) for fn in OUTS]
    assert outs["one"] == outs["two"] and outs["one"][0]


def test_real_multi_gpu(tmp_path):
    n = _device_count()
    if n < 2:
        pytest.skip("one HIP device visible: --devices 0,1 and --gpus <all> need two or more GPUs")
    c = json.load(open(os.path.join(GOLDEN, "final", "td_second_best", "params.json")))
    inp = [os.path.join(GOLDEN, x) for x in c["inputs"]]
    for extra in (["--devices", "0,1"], ["--gpus", str(n)]):
        out = str(tmp_path / extra[1].replace(",", "_"))
        p = _cli(inp + ["-o", out, "-t", "8"] + c["args"] + extra)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        assert hashlib.sha256(_read(out, OUTS[0])).hexdigest() == c["raw_sha256"]
        with open(os.path.join(GOLDEN, "final", "td_second_best", "final.tsv"), "rb") as f:
            assert _read(out, OUTS[1]) == f.read()
        assert hashlib.sha256(_read(out, OUTS[2])).hexdigest() == c["alt_sha256"]


def test_bad_ordinal_names_the_device_and_writes_nothing(tmp_path):
    out = str(tmp_path / "o")
    inp = [os.path.join(GOLDEN, "test_data", "read.fa"), os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa")]
    p = _cli(inp + ["-o", out, "--devices", "0,99"], timeout=120)
    assert p.returncode != 0
    assert "device 99" in p.stdout.decode()
    assert not any(os.path.exists(os.path.join(out, fn)) for fn in OUTS)


def test_gpus_1_is_the_single_device_path(tmp_path):
    """--gpus 1 takes today's path: the same batch count in sd_last_run_stats as no flag at all (fresh caches both)."""
    inp = [os.path.join(GOLDEN, "test_data", "read.fa"), os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa")]
    res = _child("""
        import json
        from stringdecomposer_amd import lib, main
        res = []
        for extra in ([], ["--gpus", "1"]):
            lib.release_cache()
            main.main(%r + ["-o", %r + "/" + str(len(extra)), "-t", "8", "--second-best"] + extra)
            res.append([lib.last_run_stats()["batches"], [e["batches"] for e in lib.last_run_device_stats()]])
        print(json.dumps(res))
    """ % (inp, str(tmp_path)))
    assert res[0] == res[1]
    assert res[0][0] >= 1 and len(res[0][1]) == 1
