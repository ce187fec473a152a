"""Lenient input and FASTQ on the host (no GPU): sd::FastaFile through lib.fasta_load, the normalisation rule through
lib.normalize_host, and both once more inside a stand-alone program built with AddressSanitizer / UBSan.

The default stays the reference's: the disguised files still fail with today's code and message (goldens err_lowercase,
err_crlf); only lenient=True reads them, and then gives exactly what the canonical file gives."""
import os
import random
import shutil
import subprocess

import pytest

from conftest import CASES, GOLDEN, ROOT, load_case

from stringdecomposer_amd import lib

import lenient_cases as lc

PAIRS = [(os.path.join(CASES, c, "reads.fa"), os.path.join(CASES, c, "monomers.fa"))
         for c in ("syn12_N_multiline", "weird_templates", "single_monomer")]
FILES = [p for pair in PAIRS for p in pair] + [os.path.join(GOLDEN, "test_data", "read.fa"),
                                               os.path.join(GOLDEN, "test_data", "DXZ1_star_monomers.fa")]


@pytest.mark.parametrize("path", FILES, ids=lambda p: "/".join(p.split(os.sep)[-2:]))
def test_lenient_load_gives_what_the_canonical_file_gives(path, tmp_path):
    want = lib.fasta_load(path)
    recs = lc.read_records(path)
    assert [s for _, s in recs] == want[1]
    assert lib.fasta_load(lc.write(tmp_path / "d.fa", lc.disguise(recs, seed=3)), lenient=True) == want
    # FASTQ needs no flag; disguised FASTQ needs the flag
    assert lib.fasta_load(lc.write(tmp_path / "c.fq", lc.fastq(recs))) == want
    assert lib.fasta_load(lc.write(tmp_path / "c.fq", lc.fastq(recs)), lenient=True) == want
    assert lib.fasta_load(lc.write(tmp_path / "d.fq", lc.fastq(recs, seed=4)), lenient=True) == want
    # the canonical file itself is read the same way by the lenient index
    assert lib.fasta_load(path, lenient=True) == want


def test_has_n_reflects_the_normalised_text(tmp_path):
    assert lib.fasta_load(lc.write(tmp_path / "a.fa", b">r\nacgt\n"), lenient=True) == (["r"], [b"ACGT"], False)
    assert lib.fasta_load(lc.write(tmp_path / "b.fa", b">r\nacgtr\n"), lenient=True) == (["r"], [b"ACGTN"], True)
    assert lib.fasta_load(lc.write(tmp_path / "c.fq", b"@r\nACKT\n+\nIIII\n"), lenient=True) == (["r"], [b"ACNT"], True)


def test_strict_load_still_fails_as_today(tmp_path):
    low = load_case("err_lowercase")
    with pytest.raises(lib.SdError) as e:
        lib.fasta_load(low["reads"])
    assert e.value.code == lib.SD_ERR_SYMBOL == low["returncode"] and e.value.msg == low["stderr_tail"][0]
    crlf = load_case("err_crlf")
    with pytest.raises(lib.SdError) as e:
        lib.fasta_load(crlf["reads"])
    # (the golden's line was recorded with its trailing white space -- the CR itself -- stripped)
    assert e.value.code == lib.SD_ERR_SYMBOL and e.value.msg.endswith(": \r") and e.value.msg.strip() == crlf["stderr_tail"][0].strip()
    # ... and both load in lenient mode
    assert lib.fasta_load(low["reads"], lenient=True)[1] == [s.upper() for _, s in lc.read_records(low["reads"])]
    lib.fasta_load(crlf["reads"], lenient=True)
    for reads, _ in PAIRS:
        recs = lc.read_records(reads)
        name = recs[0][0].split()[0].decode()
        with pytest.raises(lib.SdError) as e:     # lower case only: the first base is the first offender
            lib.fasta_load(lc.write(tmp_path / "l.fa", lc.disguise(recs, lower_only=True)))
        assert e.value.code == lib.SD_ERR_SYMBOL
        assert e.value.msg == "ERROR: Sequence %s contains undefined symbol (not ACGT): %s" % (name, chr(recs[0][1][0]).lower())
        with pytest.raises(lib.SdError) as e:     # the whole disguise: a lower-case base, a code or the CR, whichever is first
            lib.fasta_load(lc.write(tmp_path / "d.fa", lc.disguise(recs, seed=3)))
        assert e.value.code == lib.SD_ERR_SYMBOL and e.value.msg.startswith("ERROR: Sequence %s contains undefined symbol (not ACGT): " % name)
        with pytest.raises(lib.SdError) as e:
            lib.fasta_load(lc.write(tmp_path / "d.fq", lc.fastq(recs, seed=3)))
        assert e.value.code == lib.SD_ERR_SYMBOL
        assert lib.fasta_load(lc.write(tmp_path / "c.fq", lc.fastq(recs)))[1] == [s for _, s in recs]


@pytest.mark.parametrize("name,text", [
    ("no plus line", b"@r1\nACGT\nIIII\n@r2\nAC\n+\nII\n"),
    ("quality line one byte short", b"@r1\nACGT\n+\nIIII\n@r2\nACGT\n+\nIII\n"),
    ("cut inside the last record", b"@r1\nACGT\n+\nIIII\n@r2\nACGT\n+"),
    ("cut inside the last quality line", b"@r1\nACGT\n+\nIIII\n@r2\nACGT\n+\nII"),
    ("two-line sequence", b"@r1\nAC\nGT\n+\nIIII\n"),
])
@pytest.mark.parametrize("lenient", [False, True])
def test_malformed_fastq_is_a_format_error(name, text, lenient, tmp_path):
    with pytest.raises(lib.SdError) as e:
        lib.fasta_load(lc.write(tmp_path / "m.fq", text), lenient=lenient)
    assert e.value.code == lib.SD_ERR_FORMAT
    assert "FASTQ record %d" % (1 if name in ("no plus line", "two-line sequence") else 2) in e.value.msg


@pytest.mark.parametrize("text,byte", [(b">r\nAC\rGT\n", "\r"), (b">r\r\nACUGT\r\n", "U"), (b">r\nAC*T\n", "*"),
                                       (b"@r\nAC-T\n+\nIIII\n", "-"), (b">r\nAC\xc3T\n", None), (b">r\nAC9T\n", "9")])
def test_bytes_the_rule_leaves_alone_are_symbol_errors_in_lenient_mode_too(text, byte, tmp_path):
    with pytest.raises(lib.SdError) as e:
        lib.fasta_load(lc.write(tmp_path / "s.fa", text), lenient=True)
    assert e.value.code == lib.SD_ERR_SYMBOL
    assert e.value.msg.startswith("ERROR: Sequence r contains undefined symbol (not ACGT): ")
    if byte is not None:
        assert e.value.msg.endswith(": " + byte)


def test_normalize_host_against_the_rule():
    every = bytes(range(256))
    assert lib.normalize_host(every) == lc.rule(every)
    rng = random.Random(7)
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 4097):
        for pick in (lambda: rng.randrange(256), lambda: rng.choice(b"ACGTNacgtnRYSWKMBDHVryswkmbdhvU*-\r\nEe")):
            data = bytes(pick() for _ in range(n))
            want, st = lc.rule(data)
            assert lib.normalize_host(data) == (want, st)
            buf = bytearray(data)
            out, st2 = lib.normalize_host(buf, inplace=True)
            assert out is buf and bytes(buf) == want and st2 == st
    # the rule is idempotent, and the identity on canonical text
    assert lib.normalize_host(lc.rule(every)[0])[0] == lc.rule(every)[0]
    assert lib.normalize_host(b"ACGTN" * 11) == (b"ACGTN" * 11, [0, 0, 0, 55])


def test_flag_and_stats_are_bound():
    p = lib.make_params(lenient=True, flags=lib.FLAG_PROGRESS)
    assert p.reserved[1] == lib.FLAG_LENIENT | lib.FLAG_PROGRESS and lib.FLAG_LENIENT == 8192
    assert lib.make_params().reserved[1] == 0
    assert set(lib.last_run_input_stats()) == {"lower", "ambiguity", "cr", "copied", "fastq", "lenient"}


def test_cli_refuses_lenient_with_ref_compat_and_with_a_multi_process_launch(tmp_path):
    exe = [os.sys.executable, os.path.join(ROOT, "bin", "stringdecomposer"), FILES[0], FILES[1], "-o", str(tmp_path / "o"), "--lenient"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(exe + ["--ref-compat"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == lib.SD_ERR_PARAM and b"--ref-compat" in p.stderr and b"upper-case" in p.stderr
    p = subprocess.run(exe, env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == lib.SD_ERR_PARAM and b"--gpus N" in p.stderr and b"--devices" in p.stderr
    assert not os.path.exists(tmp_path / "o")       # before any work


def test_host_code_under_address_and_ub_sanitizers(tmp_path):
    """tools/lenient_host_check.cpp with the library's host-only unit, as a program of its own: the lenient / FASTQ index
    and sd_normalize_host on an empty file, a file without a final newline, CR as the last byte, a FASTQ of one record
    and records at an 8-MB slab boundary.  Nothing is loaded into this interpreter."""
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path / "lenient_host_check")
    b = subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tools", "lenient_host_check.cpp"),
                        os.path.join(ROOT, "stringdecomposer_amd", "csrc", "sd_host_api.hip"), "-lpthread", "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0, b.stdout.decode()[-3000:]
    work = tmp_path / "w"
    work.mkdir()
    r = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"lenient_host_check ok" in r.stdout, r.stdout.decode()[-3000:]
