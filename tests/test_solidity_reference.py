"""The solidity report's reference (tests/solidity_ref.py, numpy) against a brute-force loop over positions and bases on
hand-made cases, its two kinds of lookup against each other, and what of the feature can be asked without a GPU: the
exported symbols, the argument checks, the command line's option on the path that needs no table."""
import os
import random
import subprocess

import numpy as np
import pytest

import solidity_ref as S
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

TALC = os.path.join(B.OUT, "talc")
SYMBOLS = ["talc_batch_solidity", "talc_batch_fetch_solidity", "talc_ctx_get_solidity_timing"]
K = 11


def rand_seq(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def table_of(seq, k, count=lambda i: 5, skip=()):
    """{packed k-mer: count(position)} of the k-mers of seq, without the positions in `skip` (first occurrence wins)."""
    t = {}
    for i in range(len(seq) - k + 1):
        if i not in skip:
            t.setdefault(S.pack(seq[i:i + k]), count(i))
    return t


def both(seq, k, minc, table):
    got, want = S.row(seq, k, minc, S.dict_lookup(table)), S.brute_row(seq, k, minc, table)
    assert got == want, (seq, got, want)
    return got


G = rand_seq(400, 3)
assert len(table_of(G, K)) == len(G) - K + 1      # (no k-mer twice: a position's count is its own)


@pytest.mark.parametrize("L", [0, K - 1, K, K + 1])
def test_short_lengths(L):
    seq = G[:L]
    r = both(seq, K, 2, table_of(G, K))
    n = max(0, L - K + 1)
    assert r == (n, n, n, 1 if n else 0, L if n else 0, 0)
    assert both(seq, K, 2, {}) == (n, 0, 0, 0, 0, n)


def test_all_solid_and_none_solid():
    n = len(G) - K + 1
    assert both(G, K, 2, table_of(G, K)) == (n, n, n, 1, len(G), 0)
    assert both(G, K, 2, {}) == (n, 0, 0, 0, 0, n)
    assert both(G, K, 6, table_of(G, K)) == (n, 0, 0, 0, 0, n)       # every count below MIN_COUNT


def test_one_solid_kmer_alone():
    for p in (0, 57, len(G) - K):
        t = {S.pack(G[p:p + K]): 9}
        n = len(G) - K + 1
        assert both(G, K, 2, t) == (n, 1, 1, 1, K, max(p, n - 1 - p))


@pytest.mark.parametrize("gap", [1, K - 1, K, K + 1])
def test_two_runs_and_the_weak_run_between_them(gap):
    """Runs [10, 20) and [20 + gap, 40): their bases [10, 19 + K) and [20 + gap, 39 + K) overlap while gap < K."""
    skip = set(range(0, 10)) | set(range(20, 20 + gap)) | set(range(40, 400))
    r = both(G, K, 2, table_of(G, K, skip=skip))
    n = len(G) - K + 1
    union = (39 + K) - 10 if gap < K else (19 + K - 10) + (39 + K - 20 - gap)
    assert r == (n, 30 - gap, 30 - gap, 2, union, n - 40)
    assert both(G[:60], K, 2, table_of(G, K, skip=skip))[5] == max(10, gap, 60 - K + 1 - 40)


def test_n_inside_a_kmer():
    seq = G[:100] + "N" + G[101:200]
    r = both(seq, K, 2, table_of(G, K))
    n = 200 - K + 1
    assert r == (n, n - K, n - K, 2, 199, K)                          # the K k-mers over the N; every base but the N covered
    assert both(S.dna5(G[:50] + "ryk" + G[53:90].lower()), K, 2, table_of(G, K))[5] == K + 2


def test_counts_at_min_count_and_above_it():
    t = table_of(G, K, count=lambda i: (3, 4, 2, 50)[i % 4])
    r = both(G, K, 3, t)
    n = len(G) - K + 1
    assert r[1] == sum(1 for i in range(n) if i % 4 != 2) and r[2] == sum(1 for i in range(n) if i % 4 in (1, 3))
    assert r[1] != r[2] and r[3] == (n + 1) // 4 + (1 if n % 4 in (1, 2) else 0) and r[5] == 1


def test_random_masks_against_the_brute_force_loop():
    rng = random.Random(11)
    for case in range(60):
        L = rng.choice([K, K + 3, 64, 65, 130, 300])
        seq = list(rand_seq(L, 100 + case))
        for _ in range(rng.randrange(0, 4)):
            seq[rng.randrange(L)] = "N"
        seq = "".join(seq)
        skip = {i for i in range(L) if rng.random() < rng.choice([0.05, 0.5, 0.95])}
        t = table_of(seq.replace("N", "A"), K, count=lambda i: (1, 2, 3, 40)[i % 4], skip=skip)
        both(seq, K, rng.choice([2, 3]), t)


def test_dict_lookup_and_host_lookup_agree_on_a_generated_table():
    syn = Synth(target_kmers=20_000, k=21, seed=5)
    p = T.default_params(k=21, min_count=3)
    keys, cnts = syn.dump_arrays()
    tab = T.Table.from_arrays(keys, cnts, p)
    d = {}
    for km, c in zip(keys.tolist(), cnts.tolist()):
        if c >= 3:
            d.setdefault(km, c)
    bases, offs = syn.reads(0, 30)
    seqs = [S.dna5(bytes(bases[int(offs[i]):int(offs[i + 1])]).decode()) for i in range(30)]
    a, b = S.rows(seqs, 21, 3, S.dict_lookup(d)), S.rows(seqs, 21, 3, S.host_lookup(tab))
    assert (a == b).all() and a["n_solid"].sum() > 1000 and (a["n_solid"] != a["n_in"]).any()
    assert (S.rows([S.revcomp(s) for s in seqs], 21, 3, S.dict_lookup(d))["n_solid"] < a["n_solid"]).any()   # directional
    tab.close()


def test_solidity_symbols_are_exported_and_listed():
    L = T.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in T.ABI_SYMBOLS
    assert T.SOLIDITY_DTYPE.itemsize == 24 and T.SOLIDITY_DTYPE == S.DTYPE and T.SOLIDITY_FIELDS == S.FIELDS


def test_solidity_calls_check_their_arguments():
    L = T.lib()
    assert L.talc_batch_solidity(None, None) == -1                    # TALC_ERR_INVALID
    assert L.talc_batch_fetch_solidity(None, None, None, None) == -1
    assert L.talc_ctx_get_solidity_timing(None, None, None) == -1
    assert L.talc_last_error()


def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_cli_lists_the_option(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0 and b"--solidity" in r.stdout


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_cli_without_a_table_reports_zero_counts(tmp_path, rev):
    """-qm jellyfish2 with neither a program nor a .jf: the reference's dead path, no table and no GPU.  Every count is 0;
    n_kmers and longest_weak (every position is weak) follow from the length.  The other files are those of a run without the option."""
    reads = ["", G[:20], G[:21], G[:22], G[:300].lower(), G[:100] + "NNRY" + G[104:250]]
    names = ["r%d" % i for i in range(len(reads))]
    (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, reads)))
    (tmp_path / "sr.dump").write_text("")
    args = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "-qm", "jellyfish2", "--batch-reads", "4"] + (["-rev"] if rev else [])
    a, b = run(args + ["--solidity", "-o", "sol"], tmp_path), run(args + ["-o", "plain"], tmp_path)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr.decode(), b.stderr.decode())
    lines = (tmp_path / "sol.solidity.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["read_name", "status", "raw_length", "corr_length"] + ["raw_" + f for f in S.FIELDS] + ["corr_" + f for f in S.FIELDS]
    want = []
    for n, r in zip(names, reads):
        nk = max(0, len(r) - 20)
        row = [nk, 0, 0, 0, 0, nk]                                     # (the contract on an empty table: every position is weak)
        want.append("\t".join(map(str, [n, 2 if len(r) > 21 else 1, len(r), len(r)] + row + row)))
    assert lines[1:] == want
    total = sum(len(r) for r in reads)
    assert ("[TALC]: solid bases: raw 0 of %d (0.00 %%), corrected 0 of %d (0.00 %%)" % (total, total)).encode() in a.stdout
    assert b"solid bases" not in b.stdout and not (tmp_path / "plain.solidity.tsv").exists()
    for ext in (".fa", ".log", ".stats_basics.txt"):
        assert (tmp_path / ("sol" + ext)).read_bytes() == (tmp_path / ("plain" + ext)).read_bytes(), ext
    assert (tmp_path / "sol.config.txt").read_bytes().replace(b"sol", b"plain") == (tmp_path / "plain.config.txt").read_bytes()
    assert a.stdout.replace(b"sol.fa", b"plain.fa").splitlines()[:-2] == b.stdout.splitlines()[:-1]
