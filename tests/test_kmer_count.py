"""The short-read k-mer counter without a GPU: the numpy reference of the counting contract (tests/kmer_ref.py) against a
naive counter, the CLI's --SRReads / --SRCountsOut options, the counter's refusal without a GPU, and the synthetic short
reads (docs/kmer_counting.md)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmer_ref as R
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

TALC = os.path.join(B.OUT, "talc")


@pytest.mark.parametrize("k", [18, 21, 31])
def test_reference_counter_matches_naive_counter(k):
    recs = R.hand_records()
    bases, offs = R.records_to_arrays(recs)
    u, c = R.count(bases, offs, k)
    want = R.naive_count(recs, k)
    assert dict(zip(u.tolist(), c.tolist())) == dict(want)
    assert int(c.sum()) == sum(want.values()) > 0
    # windows never span two records: the same bytes as ONE record give more windows
    u1, c1 = R.count(*R.records_to_arrays(["".join(recs)]), k)
    assert int(c1.sum()) > int(c.sum())


def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_cli_srreads_parse_errors(tmp_path):
    base = ["reads.fa", "-k", "21"]
    for extra, why in (
        (["--SRReads", "a.fq", "-SR", "x.dump"], b"exclude each other"),
        (["--SRReads", "a.fq", "-qm", "jellyfish2"], b"jellyfish2"),
        (["-SR", "x.dump", "--SRCountsOut", "o.dump"], b"--SRCountsOut needs --SRReads"),
        (["--SRCountsOut", "o.dump"], b"-SR"),
    ):
        r = run(base + extra, tmp_path)
        assert r.returncode == 1, (extra, r.stderr)
        assert why in r.stderr and b"unknown option" not in r.stderr, (extra, r.stderr)
    r = run(base, tmp_path)   # neither: today's message
    assert r.returncode == 1 and b"option requires a value: -SR, --SRCounts" in r.stderr


def test_cli_help_lists_the_counting_options(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    assert b"--SRReads" in r.stdout and b"--SRCountsOut" in r.stdout


@pytest.mark.skipif(T.device_count() > 0, reason="only meaningful on a host without a GPU")
def test_cli_srreads_fails_loudly_without_gpu(tmp_path):
    (tmp_path / "reads.fa").write_text(">r\n" + "ACGT" * 30 + "\n")
    (tmp_path / "a.fq").write_text("@s\n" + "ACGT" * 30 + "\n+\n" + "I" * 120 + "\n")
    r = run(["reads.fa", "-k", "21", "--SRReads", "a.fq", "-o", "x"], tmp_path)
    assert r.returncode == 2 and b"no CPU fallback" in r.stderr, r.stderr


@pytest.mark.skipif(T.device_count() > 0, reason="only meaningful on a host without a GPU")
def test_counter_create_without_gpu_is_a_device_error():
    L = T.lib()
    p = T.default_params()
    h = C.c_void_p()
    assert L.talc_counter_create(C.byref(p), 0, 0, C.byref(h)) == -4      # TALC_ERR_DEVICE
    assert not h.value
    with pytest.raises(T.TalcError):
        T.KmerCounter(p)


def test_synth_short_reads_depend_on_seed_and_index_only(tmp_path):
    S = Synth(target_kmers=200_000, k=21, seed=4)
    b_all, o_all = S.short_reads(0, 5000, length=150, sub_rate=0.01, n_rate=0.002)
    assert len(o_all) == 5001 and int(o_all[-1]) == len(b_all)
    lens = np.diff(o_all.astype(np.int64))
    assert lens.max() == 150 and (lens == 150).mean() > 0.99
    text = bytes(b_all)
    assert set(text) <= set(b"ACGTN") and b"N" in text
    whole = [text[int(o_all[i]):int(o_all[i + 1])] for i in range(5000)]
    pieces = []
    for first, n in ((0, 1), (1, 4095), (4096, 3), (4099, 901)):   # any batching, either side of the parallel threshold
        b, o = S.short_reads(first, n, length=150, sub_rate=0.01, n_rate=0.002)
        pieces += [bytes(b[int(o[i]):int(o[i + 1])]) for i in range(n)]
    assert pieces == whole
    assert S.short_reads(7, 1, length=150, sub_rate=0.01, n_rate=0.002)[0].tobytes() == whole[7]
    # another seed gives other reads; the FASTQ writer writes the same reads
    assert Synth(target_kmers=200_000, k=21, seed=5).short_reads(0, 10)[0].tobytes() != S.short_reads(0, 10)[0].tobytes()
    S.write_short_fastq(str(tmp_path / "s.fq"), 10, 20, length=150, sub_rate=0.01, n_rate=0.002)
    lines = (tmp_path / "s.fq").read_bytes().split(b"\n")
    assert lines[0] == b"@sr_000000010" and lines[2] == b"+"
    assert [lines[4 * i + 1] for i in range(20)] == whole[10:30]
    assert all(len(lines[4 * i + 3]) == len(lines[4 * i + 1]) for i in range(20))
