"""The correction map's reference (tests/corr_map_ref.py: the expected segments of a read from the oracle's trace alone)
against the oracle's own corrected read, the reach conditions of the input sets the GPU tests use
(tests/test_gpu_corr_map.py), and what of the feature can be asked without a GPU: the exported symbols, the argument
checks, the command line's options."""
import ctypes as C
import os
import subprocess

import pytest

import corr_map_ref as M
import parity_util as PU
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

TALC = os.path.join(B.OUT, "talc")
MAP_SYMBOLS = ["talc_ctx_set_map", "talc_batch_num_segments", "talc_batch_fetch_map", "talc_batch_fetch_corrected_masked"]


def check_set(s):
    """Every read's pieces add up to the oracle's record; the segments tile it; none overlaps its neighbour in the read."""
    for seq, e in zip(s.reads, s.exp):
        assert "".join(e["pieces"]) == e["out"]
        pos = 0
        for (kind, rs, rl, os_, ol), p in zip(e["segs"], e["pieces"]):
            assert os_ == pos and ol == len(p) and rs + rl <= len(seq)
            assert kind == M.CORRECTED or ol == rl
            pos += ol
        assert pos == len(e["out"])
        assert len(e["segs"]) == (2 * e["R"] + 1 if e["status"] == 0 else 1)
        assert M.raw_overlaps(e["segs"]) == 0
        assert M.masked(e).upper() == e["out"]
        if e["status"] != 0:
            assert e["segs"] == [(M.RAW, 0, len(seq), 0, len(seq))]


@pytest.mark.parametrize("name", list(M.SETS))
def test_reference_map_reproduces_the_oracle_record(name):
    s = M.map_set(name)
    check_set(s)
    c = s.counts()
    print(name, c)
    assert c["corrected"] >= 150 and c["S"] > 0 and c["C"] > 0 and c["R"] > 0
    assert c["head_corrected"] > 0 and c["tail_corrected"] > 0
    if name in ("default", "reverse"):
        assert c["zero_corrected"] > 0 and c["zero_raw"] > 0          # a bridge of length 0; a gap the anchors closed
    if name == "paralog-maxb4":
        assert c["head_long"] + c["tail_long"] > 0                    # a border beyond max_border_length
    if name == "k31":
        assert c["head_long"] > 0 and c["tail_long"] > 0
        assert sum(1 for e in s.exp if e["R"] == 1) > 0               # one region: head, solid, tail


def test_reverse_set_is_the_default_set_flipped():
    a, b = M.map_set("default"), M.map_set("reverse")
    for x, y in zip(a.exp, b.exp):
        assert x["status"] == y["status"]
        if x["status"] == 0:
            assert y["out"] == M.revcomp(x["out"])
    assert a.counts() == b.counts()


@pytest.mark.parametrize("graph", M.COMB_SETS)
def test_reference_map_of_comb_reads(graph):
    s = M.comb_set(graph)
    check_set(s)
    print(graph, s.counts(), sorted(e["R"] for e in s.exp))
    assert len(s.exp) >= 10 and all(e["status"] == 0 and e["R"] >= 100 for e in s.exp)


def test_map_symbols_are_exported_and_listed():
    L = T.lib()
    for name in MAP_SYMBOLS:
        assert hasattr(L, name), name
        assert name in T.ABI_SYMBOLS
    assert T.SEGMENT_DTYPE.itemsize == 20 and T.SEGMENT_DTYPE == M.SEGMENT_DTYPE
    assert (T.SEG_SOLID, T.SEG_CORRECTED, T.SEG_RAW) == (M.SOLID, M.CORRECTED, M.RAW)


def test_map_calls_check_their_arguments():
    L = T.lib()
    assert L.talc_ctx_set_map(None, 1) == -1                          # TALC_ERR_INVALID
    assert L.talc_batch_num_segments(None) == 0
    assert L.talc_batch_fetch_map(None, None, None, 0, None) == -1
    assert L.talc_batch_fetch_corrected_masked(None, None, None, 0, None, None) == -1
    assert L.talc_last_error()


def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


@pytest.fixture(scope="module")
def clidata(tmp_path_factory):
    d = tmp_path_factory.mktemp("mapcli")
    S = Synth(target_kmers=150_000, k=21, seed=77)
    S.write_dump(str(d / "sr.dump"))
    S.write_fasta(str(d / "reads.fa"), 0, 20)
    return d


def test_cli_lists_the_map_options(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0 and b"--corr-map" in r.stdout and b"--soft-mask" in r.stdout


@pytest.mark.skipif(PU.T.device_count() > 0, reason="only meaningful on a host without a GPU")
def test_cli_map_options_without_a_gpu_fail_like_the_plain_command(clidata, tmp_path):
    base = [str(clidata / "reads.fa"), "-k", "21", "-SR", str(clidata / "sr.dump")]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain = run(base + ["-o", "x"], tmp_path / "a")
    r = run(base + ["--corr-map", "--soft-mask", "-o", "x"], tmp_path / "b")
    assert plain.returncode == 2 and b"no CPU fallback" in plain.stderr
    assert r.returncode == 2 and b"no CPU fallback" in r.stderr       # not 1: the options parse
    assert (tmp_path / "a" / "x.config.txt").read_bytes() == (tmp_path / "b" / "x.config.txt").read_bytes()


def test_cli_pass_through_map_and_mask(clidata, tmp_path):
    """Without a table (-qm jellyfish2 with neither -jf2 nor a .jf: no GPU needed) nothing is corrected: one RAW line per
    read, every base in lower case; without the options the files are the plain run's."""
    base = [str(clidata / "reads.fa"), "-k", "21", "-SR", str(clidata / "sr.dump"), "-qm", "jellyfish2", "--batch-reads", "7"]
    plain = run(base + ["-o", "p"], tmp_path)
    r = run(base + ["--corr-map", "--soft-mask", "-o", "m"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, (plain.stderr, r.stderr)
    assert not (tmp_path / "p.map.tsv").exists()
    fa, ma = (tmp_path / "p.fa").read_text().splitlines(), (tmp_path / "m.fa").read_text().splitlines()
    assert len(fa) == len(ma) and (tmp_path / "p.log").read_bytes() == (tmp_path / "m.log").read_bytes()
    names, lens = [], []
    for a, b in zip(fa, ma):
        if a.startswith(">"):
            assert a == b
            names.append(a[1:])
            lens.append(0)
        else:
            assert b == a.lower() and b != a
            lens[-1] += len(a)
    want = ["%s\tR\t0\t%d\t0\t%d" % (n, L, L) for n, L in zip(names, lens)]
    assert (tmp_path / "m.map.tsv").read_text().splitlines() == want and len(want) == 20
