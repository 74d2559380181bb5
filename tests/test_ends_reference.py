"""The long-read end clean-up's contract (docs/read_ends.md) on the CPU: tests/ends_ref.py's numpy form against its plain
loops, the tail rule, the kept-interval formula, the binding table, and the command line's parse errors."""
import os
import subprocess

import numpy as np
import pytest

import ends_ref as R
from talc_amd import build as B
from talc_amd import lib as T

TALC = os.path.join(B.OUT, "talc")
SSP, VNP = "TTTCTGTTGGTGCTGATATTGCTGGG", "ACTTGCCTGTCGCTCTATCTTC"
P24 = "GATCCGTAGCTTGACCATGCAGTC"


def same(a, b):
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, (len(bad), int(bad[0]), a[bad[0]].tolist(), b[bad[0]].tolist())


def test_sellers_by_hand():
    # the distance of the pattern to the best substring that ends at e: top row 0, first column i
    assert R.sellers_plain(b"ACGT", b"") == [4]
    assert R.sellers_plain(b"ACGT", b"ACGT") == [4, 3, 2, 1, 0]
    assert R.sellers_plain(b"ACGT", b"TTACGTT") == [4, 3, 3, 3, 2, 1, 0, 1]     # (a lone T already matches the last letter)
    assert R.sellers_plain(b"ACGT", b"ACT") == [4, 3, 2, 1]              # one deletion
    assert R.sellers_plain(b"ACGT", b"ACNT")[-1] == 1                     # N matches nothing, not even itself
    assert R.sellers_plain(b"ACNT", b"ACNT")[-1] == 1


def test_hand_cases():
    kw = dict(adapters=[P24], max_error_pct=20, poly_min=8, window=64)
    assert R.head_plain(P24 + "T" * 10 + "GCA", **kw) == (24, 1, 0, 10)
    assert R.head_plain("GG" + P24 + "T" * 7 + "GCA", **kw) == (26, 1, 0, 0)                # a run below poly_min
    assert R.head_plain("T" * 9 + "C" + "T" * 9 + "GG", **kw) == (0, 0, 0, 19)             # 9, 7, 16: the C is absorbed
    assert R.head_plain("T" * 9 + "CCCCC" + "T" * 9, **kw) == (0, 0, 0, 9)                 # 9, -1, 8: it ends the run
    assert R.head_plain(P24.lower() + "t" * 10, **kw) == (24, 1, 0, 10)                     # upper-cased first
    assert R.head_plain("NNNN", **kw) == (0, 0, 0, 0) and R.head_plain("", **kw) == (0, 0, 0, 0)
    assert R.head_plain(P24[:12] + "N" + P24[13:] + "A", **kw) == (24, 1, 1, 0)
    assert R.head_plain("A" * 64 + P24, **kw) == (0, 0, 0, 0)                               # beyond the window
    assert R.head_plain("A" * 40 + P24, **kw) == (64, 1, 0, 0)                              # ends with it
    # the adapter whose match ends last; the lowest index among equal ends
    assert R.head_plain(SSP + "CA" + VNP, adapters=[SSP, VNP], window=64)[:3] == (50, 2, 0)
    assert R.head_plain(SSP + "CA" + VNP, adapters=[VNP, SSP, VNP], window=64)[:3] == (50, 1, 0)
    assert R.head_plain(SSP + "CA" + VNP, adapters=[SSP, VNP], window=32)[:3] == (26, 1, 0)
    # the smallest D wins inside one adapter, the largest e among equal D
    assert R.head_plain(P24[:-1] + "AGGGG", **kw)[:3] == (24, 1, 1)                        # D = 1 at 23 (deletion) and at 24 (substitution)
    row = R.row_plain("T" * 20 + "GCGC" + "A" * 30, poly_min=8)
    assert row == (0, 20, 0, 30, 0, 0, 0, 0, 20, 4, 0)                                      # both ends have a run: orient 0
    assert R.row_plain("GCGC" + "A" * 30, poly_min=8)[-1] == 1 and R.row_plain("T" * 30 + "GCGC", poly_min=8)[-1] == -1


def test_a_leading_mismatch_is_an_interruption_the_score_absorbs():
    # score(1) = -2, then +1 per T: the maximum 10 is reached at j = 13, so the run is 13 bases although it starts with a C
    assert R.head_plain("C" + "T" * 12, poly_min=8) == (0, 0, 0, 13)
    assert R.head_plain("C" + "T" * 2 + "G", poly_min=8) == (0, 0, 0, 0)    # never above score(0) = 0: p = 0


def random_reads(rng, n):
    reads = []
    for i in range(n):
        s = R.random_seq(rng, int(rng.integers(0, 400)))
        if i % 3 == 0:
            s = R.random_seq(rng, int(rng.integers(0, 40))) + R.mutate(rng, (SSP, VNP, P24)[i % 5 % 3], int(rng.integers(0, 7)), "SIDN") + "T" * int(rng.integers(0, 40)) + s
        if i % 4 == 0:
            s = s + "A" * int(rng.integers(0, 60)) + R.revcomp(R.mutate(rng, (VNP, SSP)[i % 2], int(rng.integers(0, 6)), "SID")).decode() + R.random_seq(rng, int(rng.integers(0, 20)))
        if i % 5 == 0:
            s = "T" * int(rng.integers(0, 30)) + "C" * int(rng.integers(0, 3)) + "T" * int(rng.integers(0, 30)) + s
        if i % 7 == 0:
            s = s.lower()
        if i % 11 == 0 and s:
            at = int(rng.integers(len(s)))
            s = s[:at] + "NRn-"[i % 4] + s[at + 1:]
        reads.append(s)
    return reads


@pytest.mark.parametrize("kw", [dict(adapters=[SSP, VNP], max_error_pct=20, poly_min=12, window=512),
                                dict(adapters=[SSP, VNP, P24, P24[:12]], max_error_pct=30, poly_min=8, window=64),
                                dict(adapters=[P24], max_error_pct=0, poly_min=0, window=32),
                                dict(adapters=[], max_error_pct=20, poly_min=10, window=100)])
def test_numpy_form_equals_the_plain_loops_on_500_random_reads(kw):
    reads = random_reads(np.random.default_rng(len(kw["adapters"]) + kw["window"]), 500)
    a, b = R.rows(reads, **kw), R.rows_plain(reads, **kw)
    same(a, b)
    if kw["adapters"] and kw["max_error_pct"]:
        assert (a["head_adapter"] > 0).sum() > 50 and (a["tail_adapter"] > 0).sum() > 30 and (a["head_adapter_err"] > 0).sum() > 20
    if kw["poly_min"]:
        assert (a["head_poly_len"] > 0).sum() > 30 and (a["tail_poly_len"] > 0).sum() > 30
    assert (a["kept_start"].astype(np.int64) + a["kept_len"] <= [len(r) for r in reads]).all()


def test_the_tail_is_the_head_of_the_reverse_complement():
    reads = random_reads(np.random.default_rng(4), 200)
    kw = dict(adapters=[SSP, VNP], max_error_pct=20, poly_min=12, window=128)
    fwd, rc = R.rows(reads, **kw), R.rows([R.revcomp(r) for r in reads], **kw)
    for h, t in (("head_adapter_len", "tail_adapter_len"), ("head_poly_len", "tail_poly_len"), ("head_adapter", "tail_adapter"), ("head_adapter_err", "tail_adapter_err")):
        assert (fwd[h] == rc[t]).all() and (fwd[t] == rc[h]).all()
    assert (fwd["orient"] == -rc["orient"]).all() and (fwd["kept_len"] == rc["kept_len"]).all()
    assert (rc["kept_start"].astype(np.int64) + rc["kept_len"] + np.minimum(fwd["kept_start"], [len(r) for r in reads]) >= 0).all()
    assert R.revcomp("acgtNn-x") == b"X-NNACGT"
    for r, w in zip(reads, fwd):
        assert R.head_plain(R.revcomp(r), **kw) == (w["tail_adapter_len"], w["tail_adapter"], w["tail_adapter_err"], w["tail_poly_len"])


@pytest.mark.parametrize("window", [32, 64])
def test_the_kept_interval_on_overlapping_claims(window):
    # the formula itself: kept_start = head, kept_len = L - head - min(tail, L - head)
    assert R.kept(100, 30, 20) == (30, 50) and R.kept(100, 30, 70) == (30, 0) and R.kept(100, 30, 90) == (30, 0)
    assert R.kept(100, 100, 100) == (100, 0) and R.kept(0, 0, 0) == (0, 0) and R.kept(1, 1, 1) == (1, 0) and R.kept(1, 0, 1) == (0, 0)
    kw = dict(adapters=[P24, R.revcomp(P24).decode()], max_error_pct=20, poly_min=8, window=window)
    W = window
    both = "TTG" + P24 + "CAA"                 # the one copy is adapter 1 of the head and adapter 2 of the tail
    cases = {0: "", 1: "T", 11: "T" * 11, W: "T" * W, 2 * W - 1: "T" * (W - 1) + "A" * W}
    cases[30] = both
    for L, s in cases.items():
        assert len(s) == L
        row = R.row_plain(s, **kw)
        same(R.rows([s], **kw), np.array([row], R.DTYPE))
        head, tail = row[0] + row[1], row[2] + row[3]
        assert (row[8], row[9]) == R.kept(L, head, tail) and row[8] + row[9] <= L
    assert R.row_plain(cases[0], **kw) == (0,) * 11 and R.row_plain(cases[1], **kw) == (0,) * 9 + (1, 0)
    assert R.row_plain(cases[11], **kw)[:4] == (0, 11, 0, 0) and R.row_plain(cases[11], **kw)[8:] == (11, 0, -1)
    assert R.row_plain(cases[W], **kw)[8:] == (W, 0, -1)
    r = R.row_plain(cases[2 * W - 1], **kw)
    assert (r[1], r[3], r[8], r[9], r[10]) == (W - 1, W, W - 1, 0, 0)
    r = R.row_plain(both, **kw)
    assert (r[0], r[2], r[4], r[6]) == (27, 27, 1, 2) and r[0] + r[2] > 30 and (r[8], r[9]) == (27, 0)


def test_the_binding_table_and_the_row():
    L = T.lib()
    for name in ("talc_ctx_set_ends", "talc_batch_ends", "talc_batch_fetch_ends", "talc_batch_create_clipped", "talc_ctx_get_ends_timing"):
        assert hasattr(L, name) and name in T.ABI_SYMBOLS
    assert T.ENDS_DTYPE == R.DTYPE and T.ENDS_DTYPE.itemsize == 32
    assert [T.ENDS_DTYPE.fields[f][1] for f in T.ENDS_DTYPE.names] == [0, 4, 8, 12, 16, 17, 18, 19, 20, 24, 28]
    assert L.talc_ctx_set_ends(None, b"", 20, 0, 512) == -1 and L.talc_ctx_get_ends_timing(None, None, None) == -1
    assert L.talc_batch_ends(None, None) == -1 and L.talc_batch_fetch_ends(None, None, None) == -1


BASE = ["reads.fa", "-k", "21", "-SR", "sr.dump", "-o", "o"]


@pytest.mark.parametrize("extra,word", [
    (["--LRAdapterErr", "10"], "--LRAdapterErr needs --LRAdapter"),
    (["--LRAdapterErr", "10", "--LRPolyA", "12"], "--LRAdapterErr needs --LRAdapter"),
    (["--LREndWindow", "100"], "--LREndWindow needs --LRAdapter or --LRPolyA"),
    (["--LRClip"], "--LRClip needs --LRAdapter or --LRPolyA"),
    (["--LRClip", "--LRPolyA", "0"], "--LRClip needs --LRAdapter or --LRPolyA"),
    (["--LRAdapter", "ACGTACGTACG"], "12..64"),
    (["--LRAdapter", "A" * 65], "12..64"),
    (["--LRAdapter", "ACGTACGTACGN"], "not one of ACGT"),
    (["--LRAdapter", P24] * 5, "at most 4"),
    (["--LRAdapter", P24, "--LRAdapterErr", "31"], "LRAdapterErr: 0..30"),
    (["--LRAdapter", P24, "--LRAdapterErr", "2.5"], "LRAdapterErr"),
    (["--LRPolyA", "7"], "LRPolyA"),
    (["--LRPolyA", "513"], "above LREndWindow 512"),
    (["--LRPolyA", "100", "--LREndWindow", "64"], "above LREndWindow 64"),
    (["--LRPolyA", "12", "--LREndWindow", "31"], "LREndWindow: 32..4096"),
    (["--LRPolyA", "12", "--LREndWindow", "4097"], "LREndWindow: 32..4096"),
    (["--LRAdapter"], "requires an argument"),
])
def test_cli_parse_errors_exit_1_and_write_nothing(tmp_path, extra, word):
    r = subprocess.run([TALC] + BASE + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and word in r.stderr.decode(), (r.returncode, r.stderr.decode())
    assert os.listdir(tmp_path) == []


def test_cli_help_names_the_options():
    r = subprocess.run([TALC, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0
    for opt in ("--LRAdapter", "--LRAdapterErr", "--LRPolyA", "--LREndWindow", "--LRClip"):
        assert opt.encode() in r.stdout
