"""`talc --both-strands` and the both-strands symbols of the library, as far as they go without a GPU
(docs/both_strands.md): the option table, its parse errors, the banner and the config line, the ABI additions."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from talc_amd import build as B
from talc_amd import lib as T

TALC = os.path.join(B.OUT, "talc")
SYMBOLS = ["talc_counter_set_both_strands", "talc_counter_add_counts", "talc_table_build_device_both_strands",
           "talc_table_from_arrays_device_both_strands"]


@pytest.fixture(scope="module")
def cli():
    B.build_cli()
    assert os.path.exists(TALC)
    return TALC


def run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_help_lists_both_strands(cli, tmp_path):
    r = run(cli, ["--help"], tmp_path)
    assert r.returncode == 0 and b"--both-strands" in r.stdout


def test_both_strands_with_auto_strand_is_a_parse_error_naming_both(cli, tmp_path):
    for extra in (["-SR", "x"], ["--SRReads", "x.fq"]):
        r = run(cli, ["reads.fa", "-k", "21", "--both-strands", "--auto-strand"] + extra, tmp_path)
        assert r.returncode == 1
        text = r.stdout + r.stderr
        assert b"--both-strands" in text and b"--auto-strand" in text
    # each of them alone parses (the run then ends on the unreadable input, main.cpp:219)
    for flag in ("--both-strands", "--auto-strand"):
        assert run(cli, ["missing.fa", "-k", "21", "-SR", "x", flag], tmp_path).returncode == 0


def test_banner_and_config_line_only_with_the_flag(cli, tmp_path):
    a = run(cli, ["missing.fa", "-k", "21", "-SR", "x", "--both-strands", "-o", "both"], tmp_path)
    b = run(cli, ["missing.fa", "-k", "21", "-SR", "x", "-o", "plain"], tmp_path)
    assert a.returncode == 0 and b.returncode == 0
    assert b"* Kmers are taken on both strands                    *\n" in a.stdout and b"directional" not in a.stdout
    assert b"* Kmers are assumed directional                      *\n" in b.stdout and b"both strands" not in b.stdout
    ca = (tmp_path / "both.config.txt").read_bytes().splitlines()
    cb = (tmp_path / "plain.config.txt").read_bytes().splitlines()
    i = ca.index(b"queryMode=memory")
    assert ca[i + 1] == b"Both strands? 1"
    assert ca[:i + 1] + ca[i + 2:] == [ln.replace(b"plain", b"both") for ln in cb]
    assert not any(b"Both strands" in ln for ln in cb)


def test_library_loads_and_exports_the_both_strands_symbols():
    L = ctypes.CDLL(T.lib_path())
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert T.lib().talc_counter_add_counts.argtypes is not None
    with open(os.path.join(B.INCLUDE, "talc_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name + "(" in header
    assert "#define TALC_ABI_VERSION 1" in header


def test_python_both_strands_needs_a_device():
    p = T.default_params(k=21)
    km, ct = np.array([5], dtype=np.uint64), np.array([3], dtype=np.uint32)
    with pytest.raises(T.TalcError):
        T.Table.from_arrays(km, ct, p, both_strands=True)
    with pytest.raises(T.TalcError):
        T.Table.from_files("x.dump", None, p, both_strands=True)
    if T.device_count() <= 0:      # no host fold: the device builders say so themselves
        with pytest.raises(T.TalcError, match="error -4:"):
            T.Table.from_arrays(km, ct, p, device=0, both_strands=True)
