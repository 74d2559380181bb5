"""The per-base support's reference (tests/support_ref.py, numpy) against a brute-force double loop over bases and k-mer
positions on hand-made cases, its two identities with the solidity row of the same sequence, the ends of the Phred form, and
what of the feature can be asked without a GPU: the exported symbols, the argument checks, the command line's options on
the path that needs no table."""
import os
import random
import subprocess

import numpy as np
import pytest

import solidity_ref as S
import support_ref as P
from talc_amd import build as B
from talc_amd import lib as T

TALC = os.path.join(B.OUT, "talc")
SYMBOLS = ["talc_batch_support", "talc_batch_support_bytes", "talc_batch_fetch_support", "talc_ctx_get_support_timing"]
K = 11
FORMS = [None, (2, 40), (0, 93), (7, 7)]


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
    """cover of seq, the numpy form held against the double loop in every byte form."""
    for form in FORMS:
        got, want = P.bytes_of(seq, k, minc, S.dict_lookup(table), form), P.brute(seq, k, minc, table, form)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (seq, form, got.tolist(), want.tolist())
    cov = P.cover(seq, k, minc, S.dict_lookup(table))
    row = S.row(seq, k, minc, S.dict_lookup(table))
    assert int(cov.sum()) == k * row[1] and int((cov > 0).sum()) == row[4]          # the two identities
    assert ((0 <= cov) & (cov <= P.span(len(seq), k))).all()
    return cov


G = rand_seq(400, 3)
assert len(table_of(G, K)) == len(G) - K + 1      # (no k-mer twice: a position's count is its own)
FULL = table_of(G, K)


@pytest.mark.parametrize("L", [0, K - 1, K, K + 1, 2 * K - 2, 2 * K - 1])
def test_short_lengths(L):
    seq = G[:L]
    n = max(0, L - K + 1)
    spn = P.span(L, K)
    assert spn.tolist() == [min(j, n - 1) - max(0, j - K + 1) + 1 if n else 0 for j in range(L)]
    assert both(seq, K, 2, FULL).tolist() == spn.tolist()            # all solid: cover = span
    assert both(seq, K, 2, {}).tolist() == [0] * L
    if n:
        assert spn.max() == min(n, K) and spn[0] == 1 and spn[-1] == 1
    q = P.bytes_of(seq, K, 2, S.dict_lookup(FULL), (2, 40))
    assert q.tolist() == [33 + (40 if n else 2)] * L                   # a read without a k-mer has the lowest quality


def test_all_solid_ramps_and_none_solid():
    cov = both(G, K, 2, FULL)
    L = len(G)
    assert cov[:K].tolist() == list(range(1, K + 1)) and cov[-K:].tolist() == list(range(K, 0, -1)) and (cov[K:-K] == K).all()
    assert (P.bytes_of(G, K, 2, S.dict_lookup(FULL), (2, 40)) == 33 + 40).all()     # cover = span everywhere: qmax
    assert both(G, K, 2, {}).tolist() == [0] * L
    assert (P.bytes_of(G, K, 2, S.dict_lookup({}), (2, 40)) == 33 + 2).all()
    assert both(G, K, 6, FULL).tolist() == [0] * L                    # every count below MIN_COUNT


def test_one_solid_kmer_alone():
    for p in (0, 57, len(G) - K):
        cov = both(G, K, 2, {S.pack(G[p:p + K]): 9})
        assert cov.tolist() == [1 if p <= j < p + K else 0 for j in range(len(G))]


@pytest.mark.parametrize("gap", [1, K - 1, K, K + 1])
def test_two_runs_and_the_weak_run_between_them(gap):
    """Solid runs [10, 20) and [20 + gap, 40): a base between them is held by solid k-mers of both while gap < K."""
    skip = set(range(0, 10)) | set(range(20, 20 + gap)) | set(range(40, 400))
    cov = both(G, K, 2, table_of(G, K, skip=skip))
    solid = np.zeros(len(G) - K + 1, dtype=np.int64)
    solid[10:20] = 1
    solid[20 + gap:40] = 1
    assert cov.tolist() == [int(solid[max(0, j - K + 1):j + 1].sum()) for j in range(len(G))]
    # a weak run of exactly `gap` positions: the base gap - 1 + ... in its middle loses exactly min(gap, K) of its K k-mers
    assert cov[19 + gap] == K - min(gap, K) and (cov[10 + K - 1:20] == K).all()
    between = cov[20:20 + gap + K - 1]
    assert (between.min() == 0) == (gap >= K)


def test_n_inside_a_window():
    seq = G[:100] + "N" + G[101:200]
    cov = both(seq, K, 2, FULL)
    assert cov[100] == 0 and cov[99] == 1 and cov[101] == 1 and cov[100 - K] == K and cov[100 + K] == K
    both(S.dna5(G[:50] + "ryk" + G[53:90].lower()), K, 2, FULL)


def test_counts_at_min_count_and_above_it():
    t = table_of(G, K, count=lambda i: (3, 4, 2, 50)[i % 4])
    at, above = both(G, K, 3, t), both(G, K, 4, t)
    mid = slice(K, len(G) - K)
    assert (at[mid] == K - len([i for i in range(K) if i % 4 == 2])).sum() > 0 and (above[mid] < at[mid]).all()


def test_random_masks_against_the_brute_force_loop():
    rng = random.Random(11)
    for case in range(40):
        L = rng.choice([K, K + 3, 64, 65, 130, 300])
        seq = list(rand_seq(L, 100 + case))
        for _ in range(rng.randrange(0, 4)):
            seq[rng.randrange(L)] = "N"
        seq = "".join(seq)
        skip = {i for i in range(L) if rng.random() < rng.choice([0.05, 0.5, 0.95])}
        t = table_of(seq.replace("N", "A"), K, count=lambda i: (1, 2, 3, 40)[i % 4], skip=skip)
        both(seq, K, rng.choice([2, 3]), t)


def test_phred_ends_and_flooring():
    cov, spn = np.array([0, 1, 1, 2, 3, 5, 0]), np.array([1, 1, 2, 3, 3, 11, 0])
    assert P.phred_of(cov, spn, 7, 7).tolist() == [40] * 7                                        # qmin == qmax
    assert P.phred_of(cov, spn, 0, 93).tolist() == [33, 126, 33 + 46, 33 + 62, 126, 33 + 42, 33]   # 93 // 2, 186 // 3, 465 // 11
    assert P.phred_of(cov, spn, 2, 40).tolist() == [35, 73, 35 + 19, 35 + 25, 73, 35 + 17, 35]     # 38 // 2, 76 // 3, 190 // 11
    # at the ends of a read span < K: the quality is floored over span, not over K
    seq = G[:40]
    q = P.bytes_of(seq, K, 2, S.dict_lookup({S.pack(G[0:K]): 9, S.pack(G[2:2 + K]): 9}), (0, 93))
    assert q[:4].tolist() == [33 + 93, 33 + 46, 33 + 62, 33 + 46]     # cover / span = 1/1, 1/2, 2/3, 2/4
    for bad in [(5, 4), (0, 94), (-1, 3)]:
        with pytest.raises(AssertionError):
            P.phred_of(cov, spn, *bad)


def test_the_kernels_reciprocal_table_divides_exactly():
    """k_base_support divides by span with (q * ceil(2^20 / d)) >> 20: exact for every q <= 93 * 31 and d in 1 .. 31, below 2^32."""
    for d in range(1, 32):
        m = ((1 << 20) + d - 1) // d
        q = np.arange(0, 93 * 31 + 1, dtype=np.uint64)
        assert int(q[-1]) * m < 1 << 32 and np.array_equal((q * np.uint64(m)) >> np.uint64(20), q // np.uint64(d))


def test_support_symbols_are_exported_and_listed():
    L = T.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in T.ABI_SYMBOLS
    assert (T.SUPPORT_RAW, T.SUPPORT_RECORD) == (0, 1)
    import ctypes as C
    assert C.sizeof(T.SupportParams) == 16


def test_support_calls_check_their_arguments():
    L = T.lib()
    assert L.talc_batch_support(None, None, None) == -1                # TALC_ERR_INVALID
    assert L.talc_batch_fetch_support(None, None, None, 0, None) == -1
    assert L.talc_ctx_get_support_timing(None, None) == -1
    assert L.talc_batch_support_bytes(None) == 0
    assert L.talc_last_error()


def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_cli_lists_the_options(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0 and b"--fastq" in r.stdout and b"--qual-range MIN,MAX" in r.stdout


@pytest.mark.parametrize("extra,qmin", [([], 2), (["--qual-range", "0,60"], 0), (["--qual-range", "17,17", "-rev"], 17), (["--soft-mask", "--trim", "--split"], 2)],
                         ids=["default", "range", "reverse", "pieces"])
def test_cli_without_a_table_writes_the_lowest_quality(tmp_path, extra, qmin):
    """-qm jellyfish2 with neither a program nor a .jf: the reference's dead path, no table and no GPU.  Every base has the
    quality MIN; the other files are those of a run without --fastq."""
    reads = ["", G[:20], G[:21], G[:22], G[:300].lower(), G[:100] + "NNRY" + G[104:250]]
    names = ["r%d" % i for i in range(len(reads))]
    (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, reads)))
    (tmp_path / "sr.dump").write_text("")
    args = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "-qm", "jellyfish2", "--batch-reads", "4"]
    plain_extra = [x for i, x in enumerate(extra) if x != "--qual-range" and (i == 0 or extra[i - 1] != "--qual-range")]
    a, b = run(args + extra + ["--fastq", "-o", "fq"], tmp_path), run(args + plain_extra + ["-o", "plain"], tmp_path)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr.decode(), b.stderr.decode())
    recs = P.parse_fastq((tmp_path / "fq.fq").read_text())
    fa = P.parse_fasta((tmp_path / "fq.fa").read_text())
    assert [(n, s) for n, s, q in recs] == fa and [n for n, s in fa] == names
    assert [len(s) for n, s in fa] == [len(r) for r in reads]
    assert all(q == chr(33 + qmin) * len(s) for n, s, q in recs)
    if "--soft-mask" in extra:
        assert recs[4][1] == G[:300].lower()
    for ext in (".fa", ".log", ".stats_basics.txt", ".trim.fa", ".split.fa"):
        fa_, fp = tmp_path / ("fq" + ext), tmp_path / ("plain" + ext)
        assert fa_.exists() == fp.exists() and (not fa_.exists() or fa_.read_bytes() == fp.read_bytes()), ext
    assert (tmp_path / "fq.config.txt").read_bytes().replace(b"fq", b"plain") == (tmp_path / "plain.config.txt").read_bytes()
    assert a.stdout.replace(b"fq.fa", b"plain.fa") == b.stdout
    assert not (tmp_path / "plain.fq").exists()
    for ext in (".trim.fq", ".split.fq"):                               # without a table nothing has a trusted base: empty, as the .fa
        assert (tmp_path / ("fq" + ext)).exists() == ("--trim" in extra) and (not (tmp_path / ("fq" + ext)).exists() or (tmp_path / ("fq" + ext)).read_bytes() == b"")


@pytest.mark.parametrize("args", [["--qual-range", "2,40"], ["--fastq", "--qual-range", "40"], ["--fastq", "--qual-range", "a,b"], ["--fastq", "--qual-range", "5,4"],
                                  ["--fastq", "--qual-range", "0,94"], ["--fastq", "--qual-range", "-1,40"], ["--fastq", "--qual-range", "2.5,40"],
                                  ["--fastq", "--qual-range"]],
                         ids=["no-fastq", "one-number", "letters", "min-above-max", "above-93", "negative", "fraction", "no-value"])
def test_cli_qual_range_errors(tmp_path, args):
    (tmp_path / "reads.fa").write_text(">r\n" + G[:50] + "\n")
    (tmp_path / "sr.dump").write_text("")
    r = run([str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "-qm", "jellyfish2", "-o", "x"] + args, tmp_path)
    assert r.returncode == 1 and r.stderr.startswith(b"talc: ") and not (tmp_path / "x.fq").exists()
