"""Auto strand without a GPU (docs/auto_strand.md): the numpy contract (tests/strand_ref.py) against a plain loop, against the
solidity contract and against the decision rule's tie cases; the ABI's new names; the command line's no-table path."""
import os
import subprocess

import numpy as np
import pytest

import solidity_ref as S
import strand_ref as R
from talc_amd import build as B
from talc_amd import lib as T

TALC = os.path.join(B.OUT, "talc")
K, MINC = 5, 2


def rnd(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n).tolist())


def table_of(parts, k):
    """{packed k-mer: count} of (sequence, count) parts; the first count a k-mer gets stays."""
    t = {}
    for seq, c in parts:
        for i in range(len(seq) - k + 1):
            t.setdefault(S.pack(seq[i:i + k]), c)
    return t


@pytest.fixture(scope="module")
def hand():
    """X with counts above MIN_COUNT, Y (unrelated) with counts equal to it, and reads spliced from both strands."""
    rng = np.random.default_rng(5)
    X, Y = rnd(rng, 120), rnd(rng, 120)
    table = table_of([(X, 7), (Y, MINC)], K)
    table[S.pack("ACGT" + "A")] = 1          # below MIN_COUNT: in the dict, never solid
    reads = ["", "ACG", X[:K - 1], X[:K], X[:K + 1], X, S.revcomp(X), Y, S.revcomp(Y), X[:40] + S.revcomp(Y[10:70]) + rnd(rng, 30),
             X[:30].lower() + "n" + X[31:60], "NNNNNNNN", X[:20] + "R" + S.revcomp(X[50:90]) + "-" + Y[:30], rnd(rng, 200),
             "ACGTA", "TACGT", X[3:50] + S.revcomp(X[3:50])]
    return table, reads


def test_rows_equal_the_plain_loop(hand):
    table, reads = hand
    got = R.rows(reads, K, MINC, S.dict_lookup(table))
    for i, s in enumerate(reads):
        assert tuple(got[i].tolist()) == R.brute_row(s, K, MINC, table), (i, s)
    # the hand cases reach what they are there for
    assert got["n_kmers"][:5].tolist() == [0, 0, 0, 1, 2]
    assert got["reverse"].sum() >= 3 and (got["reverse"] == 0).sum() >= 8
    assert (got["fwd_solid"] != got["fwd_in"]).any() and (got["rc_solid"] != got["rc_in"]).any()
    assert tuple(got[11].tolist()) == (4, 0, 0, 0, 0, 0)                       # all N
    assert got[14].tolist()[1:5] == (0, 0, 0, 0) and got[15].tolist()[1:5] == (0, 0, 0, 0)   # a count below MIN_COUNT


def test_rows_equal_the_solidity_contract_in_both_orientations(hand):
    """The forward fields are n_solid / n_in of S, the rc fields those of revcomp(S): what a plain and a -rev context's raw
    solidity rows report."""
    table, reads = hand
    look = S.dict_lookup(table)
    got = R.rows(reads, K, MINC, look)
    for i, s in enumerate(reads):
        d = S.dna5(s)
        f, r = S.row(d, K, MINC, look), S.row(S.revcomp(d), K, MINC, look)
        assert got[i]["n_kmers"] == f[0] == r[0]
        assert (got[i]["fwd_solid"], got[i]["fwd_in"]) == (f[1], f[2]), i
        assert (got[i]["rc_solid"], got[i]["rc_in"]) == (r[1], r[2]), i


def test_a_palindromic_kmer_counts_in_both():
    k = 6
    pal = "ACGCGT"
    assert S.revcomp(pal) == pal
    table = {S.pack(pal): 9}
    got = R.rows(["TT" + pal + "TT"], k, MINC, S.dict_lookup(table))[0]
    assert got.tolist() == (5, 1, 1, 1, 1, 0)
    assert R.revcomp_packed(np.array([S.pack(pal), S.pack("AAAAAC")], np.uint64), k).tolist() == [S.pack(pal), S.pack("GTTTTT")]


def test_the_three_tie_cases():
    rng = np.random.default_rng(9)
    lo, hi = rnd(rng, 90), rnd(rng, 90)
    table = table_of([(lo, MINC), (hi, MINC + 5)], 9)
    look = S.dict_lookup(table)
    # rc_in == fwd_in (both 0) with rc_solid larger: reverse
    a = R.row(S.revcomp(lo[:60]), 9, MINC, look)
    assert a[2] == a[4] == 0 and a[3] > a[1] and a[5] == 1
    # all equal: forward — nothing solid at all, and a read that is its own reverse complement
    b = R.row(rnd(rng, 80), 9, MINC, look)
    assert b[1:] == (0, 0, 0, 0, 0)
    own = hi[:40] + S.revcomp(hi[:40])
    c = R.row(own, 9, MINC, look)
    assert S.revcomp(own) == own and c[1] == c[3] > 0 and c[2] == c[4] > 0 and c[5] == 0
    # rc_in > fwd_in with rc_solid < fwd_solid: reverse
    d = R.row(lo[:80] + S.revcomp(hi[:30]), 9, MINC, look)
    assert d[4] > d[2] and d[3] < d[1] and d[5] == 1
    assert [R.choose(*x) for x in ((5, 0, 6, 0), (5, 2, 5, 2), (9, 0, 2, 1), (0, 0, 0, 0), (3, 3, 9, 2))] == [1, 0, 1, 0, 0]


def test_abi_names_and_argument_checks():
    L = T.lib()
    for name in ("talc_ctx_set_auto_strand", "talc_batch_strand", "talc_batch_fetch_strand", "talc_ctx_get_strand_timing"):
        assert hasattr(L, name) and name in T.ABI_SYMBOLS
    assert T.STRAND_DTYPE.itemsize == 24 and T.STRAND_DTYPE == R.DTYPE and T.STRAND_FIELDS == R.FIELDS
    assert L.talc_abi_version() == 1
    assert L.talc_ctx_set_auto_strand(None, 1) == -1                  # TALC_ERR_INVALID
    assert L.talc_batch_strand(None, None) == -1
    assert L.talc_batch_fetch_strand(None, None, None) == -1
    assert L.talc_ctx_get_strand_timing(None, None) == -1
    assert hasattr(T.Context, "auto_strand") and hasattr(T.Context, "strand_timing") and hasattr(T.Batch, "strand")


# ---------------------------------------------------------------- the command line without a table
def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.fixture(scope="module")
def reads_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("strand_cli")
    rng = np.random.default_rng(2)
    reads = [rnd(rng, n) for n in (300, 20, 21, 22, 0, 150, 75)]
    reads[5] = reads[5][:70].lower() + "N" + reads[5][71:]
    (d / "reads.fa").write_text("".join(">r%d/x\n%s\n" % (i, s) for i, s in enumerate(reads)))
    (d / "sr.dump").write_text("")
    return d, reads


def test_cli_no_table_path_writes_the_rows_and_the_summary(reads_file, tmp_path):
    d, reads = reads_file
    base = [str(d / "reads.fa"), "-k", "21", "-SR", str(d / "sr.dump"), "-qm", "jellyfish2", "--batch-reads", "3", "--corr-edits"]
    for sub in ("with", "without"):
        (tmp_path / sub).mkdir()
    a, p = run(base + ["--auto-strand", "-o", "o"], tmp_path / "with"), run(base + ["-o", "o"], tmp_path / "without")
    assert a.returncode == 0 and p.returncode == 0, (a.stderr, p.stderr)
    lines = (tmp_path / "with" / "o.strand.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["read_name", "status", "n_kmers", "fwd_solid", "fwd_in", "rc_solid", "rc_in", "strand"]
    want = ["\t".join(["r%d/x" % i, str(T.READ_NO_SOLID_KMER if len(s) > 21 else T.READ_SKIPPED_SHORT), str(max(0, len(s) - 20)), "0", "0", "0", "0", "+"])
            for i, s in enumerate(reads)]
    assert lines[1:] == want
    out = a.stdout.decode().splitlines()
    line = "[TALC]: strand: %d forward, 0 reverse of %d reads" % (len(reads), len(reads))
    assert out.count(line) == 1 and out.index(line) == len(out) - 2
    assert [x for x in out if x != line] == p.stdout.decode().splitlines()
    assert not (tmp_path / "without" / "o.strand.tsv").exists()
    for ext in (".fa", ".log", ".stats_basics.txt", ".edits.tsv", ".config.txt"):
        fa, fp = tmp_path / "with" / ("o" + ext), tmp_path / "without" / ("o" + ext)
        assert fa.exists() == fp.exists() and (not fa.exists() or fa.read_bytes() == fp.read_bytes()), ext
    assert (tmp_path / "with" / "o.fa").read_text().count(">") == len(reads)


def test_cli_auto_strand_with_rev_is_a_parse_error(reads_file, tmp_path):
    d, _ = reads_file
    base = [str(d / "reads.fa"), "-k", "21", "-SR", str(d / "sr.dump"), "-qm", "jellyfish2", "-o", "o"]
    for extra in (["--auto-strand", "-rev"], ["--reverse", "--auto-strand"]):
        r = run(base + extra, tmp_path)
        assert r.returncode == 1 and b"--auto-strand" in r.stderr
    assert not (tmp_path / "o.strand.tsv").exists()
    assert run(base + ["--auto-strand"], tmp_path).returncode == 0
