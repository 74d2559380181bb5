"""The UMI read-out contract (docs/umi.md) without a GPU: the two statements of tests/umi_ref.py against each other and on
hand cases, and the kernel's lanes run one after another on the CPU (pure_umi_scan: the chunks and their warm-up, the
restarted columns, the traceback over them and the row) against them; the combined interval against host slicing; the
binding table; every refused setting's message; the command line's parse errors (exit 1, nothing written) and its refusal
without a table (exit 2)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ends_ref as R
import umi_ref as U
from talc_amd import build as B
from talc_amd import lib as T

_pure = None


def pure():
    global _pure
    if _pure is None:
        L = C.CDLL(os.path.join(B.OUT, "libtalc_pure.so"))
        L.pure_umi_scan.restype = C.c_int
        L.pure_umi_scan.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_char_p, C.c_uint64]
        L.pure_umi_kept.restype = None
        L.pure_umi_kept.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _pure = L
    return _pure


def lanes_scan(reads, pattern, pct, window=U.DEFAULT_WINDOW):
    """k_read_umi's lanes one after another on the CPU; (rows, message): rows is None when the setting is refused."""
    bases, off = R.batch(reads)
    if len(bases) == 0:
        bases = np.zeros(1, np.uint8)
    out = np.zeros(max(len(reads), 1), U.DTYPE)
    why = C.create_string_buffer(256)
    rc = pure().pure_umi_scan(R.as_bytes(pattern), pct, window, bases.ctypes.data, off.ctypes.data, len(reads), out.ctypes.data, why, 256)
    return (out[:len(reads)] if rc == 0 else None), why.value.decode()


def all_ways(reads, pattern, pct, window=U.DEFAULT_WINDOW, plain=True):
    want = U.rows(reads, pattern, pct, window)
    got, why = lanes_scan(reads, pattern, pct, window)
    assert got is not None, why
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    if plain:
        loops = U.rows_plain(reads, pattern, pct, window)
        bad = np.flatnonzero(loops != want)
        assert len(bad) == 0, (bad[:5], loops[bad[:5]], want[bad[:5]])
    return want


P12 = "GATTACAGNCTA"                 # 12 letters, one degenerate
P64 = "ACVV" * 16                    # 64 letters, 32 degenerate
SETTINGS = [(U.ANCHORED, T.UMI_DEFAULT_ERR, 256), (U.BARE, 10, 256), (P12, 30, 256), (P64, 30, 4096)]
JUNK, TAIL = "GGCC", "CAGTCAGGCA"    # around the hand cases' copies: neither holds a T


def test_the_patterns_are_what_the_settings_say():
    assert len(U.ANCHORED) == 42 and len(U.degenerate(U.ANCHORED)) == 16 and len(U.BARE) == 28 and len(U.degenerate(U.BARE)) == 16
    assert len(P12) == 12 and len(U.degenerate(P12)) == 1 and len(P64) == 64 and len(U.degenerate(P64)) == 32
    assert T.UMI_DEFAULT_ERR in (5, 10, 15, 20)


@pytest.mark.parametrize("setting", range(4))
def test_numpy_the_loops_and_the_lanes_agree_on_random_reads(setting):
    pattern, pct, window = SETTINGS[setting]
    rng = np.random.default_rng(100 + setting)
    k = pct * len(pattern) // 100
    reads = [U.plant(rng, R.random_seq(rng, int(rng.integers(0, 1501 - 2 * len(pattern) - 20))), pattern, int(rng.integers(0, 4)), k + 1) for _ in range(300)]
    assert max(len(r) for r in reads) <= 1500
    want = all_ways(reads, pattern, pct, window, plain=False)
    loops = U.rows_plain(reads[:60], pattern, pct, window)   # (the loops take their time: a sample)
    assert (loops == want[:60]).all()
    n = np.bincount(want["end"], minlength=3)
    assert n[1] >= 30 and n[2] >= 30 and n[0] >= 5 and (want["other_err"] != 255).sum() >= 10 and (want["err"] > 0).sum() >= 30, n
    assert (want["start"][want["end"] > 0] > 0).any() and (want["umi_len"][want["end"] > 0] == len(U.degenerate(pattern))).all()


# ---------------------------------------------------------------- hand cases
def combos(read, pattern=U.BARE):
    return {s[2:] for s in U.steps_plain(read, pattern)}


def test_every_branch_of_the_tracebacks_preference():
    """Reads found by search, kept as they were found: each holds a step where the named options all satisfy the equality."""
    cases = {
        (True, True, True, "D"): "TCTTCACCTTCGGCTTGCGATTGAGATTT",
        (True, True, False, "D"): "TTCCGGTTAAGGTAAGCTTAGACTTT",
        (True, False, True, "D"): "TTTGAGGGTTAGACTTGAGATTAGCCTTT",
        (False, True, True, "U"): "TTGTATAGCTTAGACTTGGAATTGACATTT",
        (False, True, False, "U"): "TTCCGGTTAAGGTAAGCTTAGACTTT",
        (False, False, True, "L"): "TTTCGCTTGGCATTGGCGCTTCTACCTTT",
    }
    reads = []
    for combo, copy in cases.items():
        read = JUNK + copy + TAIL
        assert combo in combos(read), (combo, combos(read))
        reads += [read, R.revcomp(read).decode()]
    want = all_ways(reads, U.BARE, 20)
    assert (want["end"][0::2] == 1).all() and (want["end"][1::2] == 2).all() and (want["err"] >= 1).all()
    assert (want["umi"][0::2] == want["umi"][1::2]).all() and (want["stop"][0::2] == want["stop"][1::2]).all()


INST = "TTTACGATTCAGCTTGACATTAGCGTTT"     # an exact copy of the bare pattern; its UMI is ACGACAGCGACAAGCG


def test_a_deleted_and_an_inserted_spacer_t_keep_the_umi():
    exact, gone, more = JUNK + INST + TAIL, JUNK + INST[:7] + INST[8:] + TAIL, JUNK + INST[:8] + "T" + INST[8:] + TAIL
    assert (True, True, False, "D") in combos(gone) and (True, False, True, "D") in combos(more)
    want = all_ways([exact, gone, more], U.BARE, 10)
    assert want["umi"].tolist() == [b"ACGACAGCGACAAGCG"] * 3 and want["err"].tolist() == [0, 1, 1]
    assert want["start"].tolist() == [4, 4, 4] and want["stop"].tolist() == [32, 31, 33]


def test_a_gap_an_n_a_lower_case_byte_and_a_mismatch_under_a_degenerate_position():
    gap = JUNK + INST[:4] + INST[5:] + TAIL           # one V has no base: walking back, the diagonal takes the three that are there, the first V faces the gap
    n = JUNK + INST[:5] + "N" + INST[6:] + TAIL
    lower = JUNK + INST[:5] + "g" + INST[6:].lower() + TAIL
    mismatch = JUNK + INST[:5] + "T" + INST[6:] + TAIL
    other = JUNK + INST[:5] + "x" + INST[6:] + TAIL
    want = all_ways([gap, n, lower, mismatch, other], U.BARE, 10)
    assert want["end"].tolist() == [1] * 5 and want["err"].tolist() == [1, 1, 0, 1, 1]
    umis = [u.decode() for u in want["umi"]]
    assert umis[0] == "-AGACAGCGACAAGCG" and umis[0] == U.end_plain(gap, U.BARE, 10)[3]
    assert umis[1:] == ["ACNACAGCGACAAGCG", "ACGACAGCGACAAGCG", "ACTACAGCGACAAGCG", "ACNACAGCGACAAGCG"]
    assert (want["umi_len"] == 16).all() and all(len(u) == 16 for u in umis)


def test_start_0_the_windows_last_column_and_a_copy_beyond_it():
    window = 64
    body = "GCAGGCCAGCAGGACCAGCAGCACGACGACGAGCAGGCAGCAGCACGGACGCAGGCAGCACC" * 3
    at0 = INST + body                                  # start = 0
    last = body[:window - 28] + INST + body            # stop = window
    beyond = body[:window - 27] + INST + body          # the copy's last letter lies outside: one error
    far = body[:window - 20] + INST + body             # too many outside
    want = all_ways([at0, last, beyond, far], U.BARE, 10, window)
    assert want["end"].tolist() == [1, 1, 1, 0] and want["start"].tolist() == [0, window - 28, window - 27, 0]
    assert want["stop"].tolist() == [28, window, window, 0] and want["err"].tolist() == [0, 0, 1, 0]
    assert want["umi"][3] == b"" and want["umi_len"][3] == 0 and want["other_err"][3] == 255
    assert want["kept_start"].tolist() == [28, window, window, 0] and want["kept_len"][3] == len(far)


def test_j0_is_clamped_at_0_and_cut_off_copies_pay_for_what_is_missing():
    """A copy whose first letters lie before the read's start: the restart column is column 0, where the state is the true one."""
    body = "GCAGGCCAGCAGGACCAGCAGCACGACGACGAGCAGG"
    reads = [INST[cut:] + body for cut in range(0, 4)] + [INST[2:12]]
    want = all_ways(reads, U.BARE, 10)
    assert want["end"].tolist() == [1, 1, 1, 0, 0] and want["err"].tolist() == [0, 1, 2, 0, 0] and want["start"].tolist() == [0] * 5
    assert want["stop"].tolist() == [28, 27, 26, 0, 0] and (want["stop"][:3] < 28 + 2).all()   # stop < m + k: j0 = 0


def test_the_largest_stop_among_equal_d():
    pattern = "GATTACAGNCTA"
    read = JUNK + "GATTACAGACTAA" + "CCGG" * 5            # ...CTA and ...CTAA: the trailing A replaces nothing, D is 0 once
    rep = JUNK + "GATTACAGACT" + "CCGG" * 5              # the last letter is missing: D = 1 at ...CT (a gap) and at ...CTC (a mismatch)
    want = all_ways([read, rep], pattern, 10)
    assert want["stop"].tolist() == [16, 16] and want["err"].tolist() == [0, 1] and want["start"].tolist() == [4, 4]
    Dlast = [U.end_plain(rep[:e], pattern, 10, 256) for e in (15, 16)]
    assert Dlast[0][0] == 1 and Dlast[1][0] == 1


def test_equal_err_at_both_ends_the_head_wins_and_other_err():
    body = "GCAGGCCAGCAGGACCAGCAGCACGACGACGAGCAGG" * 2
    inst2 = "TTTCCAGTTGACCTTACAGTTCGACTTT"
    sub = lambda s: s[:10] + "T" + s[11:]             # letter 11 is a V: T is a mismatch under it
    both = INST + body + R.revcomp(inst2).decode()
    head_worse = sub(INST) + body + R.revcomp(inst2).decode()
    tail_worse = INST + body + R.revcomp(sub(inst2)).decode()
    equal_1 = sub(INST) + body + R.revcomp(sub(inst2)).decode()
    only_tail = body + R.revcomp(inst2).decode()
    want = all_ways([both, head_worse, tail_worse, equal_1, only_tail], U.BARE, 10)
    assert want["end"].tolist() == [1, 2, 1, 1, 2] and want["err"].tolist() == [0, 0, 0, 1, 0] and want["other_err"].tolist() == [0, 1, 1, 1, 255]
    assert want["umi"][1] == b"CCAGGACCACAGCGAC" and want["umi"][4] == want["umi"][1] and want["umi"][0] == b"ACGACAGCGACAAGCG"
    assert want["umi"][3] == b"ACGACTGCGACAAGCG"
    L = len(both)
    assert want["kept_start"].tolist() == [28, 0, 28, 28, 0] and want["kept_len"].tolist() == [L - 28, L - 28, L - 28, L - 28, len(only_tail) - 28]


def test_the_tail_is_the_head_of_the_reverse_complement():
    rng = np.random.default_rng(3)
    reads = [U.plant(rng, R.random_seq(rng, int(rng.integers(0, 300))), U.BARE, 1, 3) for _ in range(60)]
    heads = all_ways(reads, U.BARE, 10, plain=False)
    tails = all_ways([R.revcomp(r).decode() for r in reads], U.BARE, 10, plain=False)
    one = heads["other_err"] == 255                    # (a read whose other end is accepted too may pick differently)
    assert one.sum() >= 30 and (heads["end"][one] == 1).sum() >= 30
    for f in ("err", "start", "stop", "umi", "umi_len"):
        assert (heads[f][one] == tails[f][one]).all(), f
    assert (tails["end"][one & (heads["end"] == 1)] == 2).all()
    assert (tails["kept_start"][one & (heads["end"] == 1)] == 0).all()


@pytest.mark.parametrize("window,length", [(256, 600), (256, 250), (1024, 1100)])
def test_the_lanes_around_every_chunk_border(window, length):
    """A copy (exact, or with k substitutions) ending at every column within m + k + 2 of every border between two of the 64
    chunks, head and tail: with chunks of 4 and of 16 columns that is every column a copy can end at."""
    rng = np.random.default_rng(window + length)
    pattern, pct = U.ANCHORED, 10
    m, k = len(pattern), 10 * len(pattern) // 100
    n = min(window, length)
    chunk = -(-n // 64)
    borders = list(range(chunk, n, chunk))
    ends = sorted({b + d for b in borders for d in range(-(m + k + 2), m + k + 3) if m <= b + d <= n})
    assert ends == list(range(m, n + 1))
    reads = []
    for e in ends:
        for edits in (0, k):
            copy = U.instance(rng, pattern)
            for at in rng.choice(m - 1, size=edits, replace=False).tolist():   # (not the last letter: the copy still ends at e)
                copy = copy[:at] + ("A" if "A" not in U.sets_of(pattern)[at] else "T") + copy[at + 1:]
            s = R.random_seq(rng, length)
            s = s[:e - m] + copy + s[e:]
            reads.append(R.revcomp(s).decode() if e % 3 == 1 else s)
    want = all_ways(reads, pattern, pct, window, plain=False)
    assert (want["end"] > 0).all() and (want["stop"][0::2] == ends).all() and (want["err"][0::2] == 0).all()
    assert (want["err"][1::2] <= k).all() and (want["err"][1::2] == k).sum() > len(ends) // 2
    assert (want["end"] == 1).sum() > len(ends) and (want["end"] == 2).sum() > len(ends) // 2


def test_every_iupac_letters_set():
    body = "GCAGGCCAGCAGGACCAGCAGCAC"
    for letter, bases in U.IUPAC.items():
        pattern = "GATTACAG" + letter + "CTAG" + ("" if len(bases) > 1 else "N")
        reads = [JUNK + "GATTACAG" + b + "CTAG" + "C" + body for b in "ACGTNacgt"]
        for pat in (pattern, pattern.lower()):
            want = all_ways(reads, pat, 0)
            assert want["end"].tolist() == [1 if b.upper() in bases else 0 for b in "ACGTNacgt"], letter
        if len(bases) > 1:
            assert [u.decode() for u in want["umi"] if u] == [b.upper() for b in "ACGTNacgt" if b.upper() in bases]


def test_the_combined_interval_is_host_slicing():
    rng = np.random.default_rng(9)
    out = np.zeros(2, np.uint32)
    for _ in range(3000):
        L = int(rng.integers(0, 40))
        head, tail, stop = (int(min(L, x)) for x in rng.integers(0, 50, 3))
        end = int(rng.integers(0, 3))
        ks, kl = U.kept(L, end, stop, head, tail)
        pure().pure_umi_kept(L, end, stop, head, tail, out.ctypes.data)
        assert (ks, kl) == (int(out[0]), int(out[1]))
        read = bytes(range(L))
        h, t = max(head, stop if end == 1 else 0), max(tail, stop if end == 2 else 0)
        assert read[ks:ks + kl] == read[h:][:max(0, L - h - t)] and ks + kl <= L
        assert U.kept(L, end, stop) == ((stop, L - stop) if end == 1 else (0, L - stop) if end == 2 else (0, L))


# ---------------------------------------------------------------- the binding table, the refused settings
def test_the_binding_table_and_the_row():
    L = T.lib()
    for name in ("talc_ctx_set_umi", "talc_batch_umi", "talc_batch_fetch_umi", "talc_ctx_get_umi_timing"):
        assert hasattr(L, name) and name in T.ABI_SYMBOLS
    assert T.UMI_DTYPE == U.DTYPE and T.UMI_DTYPE.itemsize == 56
    assert [T.UMI_DTYPE.fields[f][1] for f in T.UMI_DTYPE.names] == [0, 1, 2, 3, 4, 8, 12, 16, 20, 52]
    assert L.talc_ctx_set_umi(None, U.BARE.encode(), 10, 0) == -1 and L.talc_ctx_get_umi_timing(None, None) == -1
    assert L.talc_batch_umi(None, None) == -1 and L.talc_batch_fetch_umi(None, None, None) == -1
    assert L.talc_abi_version() == 1
    for name in ("set_umi", "umi_timing"):
        assert hasattr(T.Context, name)
    assert hasattr(T.Batch, "umi") and T.UMI_DEFAULT_WINDOW == U.DEFAULT_WINDOW


REFUSED = [
    ((U.BARE, 31, 256), "max_error_pct=31: at most 30"),
    ((U.BARE, 10, 31), "window=31: 32 .. 4096 (0: 256)"),
    ((U.BARE, 10, 4097), "window=4097: 32 .. 4096 (0: 256)"),
    ((U.BARE[:11], 10, 256), "pattern: 11 letters: 12 .. 64"),
    ((P64 + "A", 10, 256), "pattern: 65 letters: 12 .. 64"),
    (("GATTACAGXCTAG", 10, 256), "pattern: letter 9 is not one of ACGTRYSWKMBDHVN"),
    (("GATTACAG,CTAG", 10, 256), "pattern: letter 9 is not one of ACGTRYSWKMBDHVN"),
    (("GATTACAGACTAG", 10, 256), "pattern: 0 degenerate letters: 1 .. 32"),
    (("N" * 33 + "ACGT", 10, 256), "pattern: 33 degenerate letters: 1 .. 32"),
]


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_every_refused_setting_names_the_bad_value(case):
    (pattern, pct, window), message = REFUSED[case]
    rows, why = lanes_scan(["ACGT" * 20], pattern, pct, window)
    assert rows is None and why == message


def test_accepted_at_the_edges_of_the_ranges():
    for args in ((P64, 30, 4096), (P12, 0, 32), ("N" * 32 + "ACGT", 30, 0), (U.ANCHORED.lower(), 20, 0)):
        rows, why = lanes_scan(["ACGT" * 20], *args)
        assert rows is not None, why
    rows, why = lanes_scan(["ACGT" * 20], b"", 10, 256)              # no pattern: the setting is off
    assert rows is None and why == "the setting is off"
    long = "C" * 200 + U.ANCHORED.replace("V", "A") + "C" * 200          # window 0 is 256
    zero, _ = lanes_scan([long], U.ANCHORED, 20, 0)
    assert zero[0] == U.rows([long], U.ANCHORED, 20, 256)[0] and zero["end"][0] == 1 and zero["stop"][0] == 242


# ---------------------------------------------------------------- the command line
TALC = os.path.join(B.OUT, "talc")
BASE = ["reads.fa", "-k", "21", "-SR", "sr.dump", "-o", "o"]


@pytest.mark.parametrize("extra,word", [
    (["--LRUmiErr", "10"], "--LRUmiErr needs --LRUmi"),
    (["--LRUmiWindow", "100"], "--LRUmiWindow needs --LRUmi"),
    (["--LRUmi"], "requires an argument"),
    (["--LRUmi", U.BARE[:11]], "LRUmi: 11 letters: 12..64 are expected"),
    (["--LRUmi", P64 + "A"], "LRUmi: 65 letters: 12..64 are expected"),
    (["--LRUmi", "GATTACAGXCTAG"], "LRUmi: letter 9 is not one of ACGTRYSWKMBDHVN"),
    (["--LRUmi", "GATTACAGACTAG"], "LRUmi: 0 degenerate letters: 1..32 are expected"),
    (["--LRUmi", "N" * 33 + "ACGT"], "LRUmi: 33 degenerate letters: 1..32 are expected"),
    (["--LRUmi", U.BARE, "--LRUmiErr", "31"], "LRUmiErr: 0..30"),
    (["--LRUmi", U.BARE, "--LRUmiErr", "2.5"], "LRUmiErr"),
    (["--LRUmi", U.BARE, "--LRUmiErr", "-1"], "LRUmiErr"),
    (["--LRUmi", U.BARE, "--LRUmiWindow", "31"], "LRUmiWindow: 32..4096"),
    (["--LRUmi", U.BARE, "--LRUmiWindow", "4097"], "LRUmiWindow: 32..4096"),
    (["--LRClip"], "--LRClip needs"),
])
def test_cli_parse_errors_exit_1_and_write_nothing(tmp_path, extra, word):
    r = subprocess.run([TALC] + BASE + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and word in r.stderr.decode(), (r.returncode, r.stderr.decode())
    assert os.listdir(tmp_path) == []


def test_cli_help_names_the_options():
    r = subprocess.run([TALC, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0
    for opt in ("--LRUmi ", "--LRUmiErr", "--LRUmiWindow"):
        assert opt.encode() in r.stdout
    assert ("default %d" % T.UMI_DEFAULT_ERR).encode() in r.stdout[r.stdout.index(b"--LRUmiErr"):][:200]


@pytest.mark.parametrize("extra", [[], ["--LRClip"], ["--LRUmiErr", "15", "--LRUmiWindow", "64"]])
def test_cli_refuses_the_options_in_a_run_without_a_table(tmp_path, extra):
    (tmp_path / "reads.fa").write_text(">r\n" + "ACGT" * 30 + "\n")
    (tmp_path / "sr.dump").write_text("ACGTACGTACGTACGTACGTA 5\n")
    r = subprocess.run([TALC, "reads.fa", "-k", "21", "-SR", "sr.dump", "-qm", "jellyfish2", "-o", "o", "--LRUmi", U.ANCHORED] + extra, cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and b"no table" in r.stderr
    assert not (tmp_path / "o.fa").exists() and not (tmp_path / "o.umi.tsv").exists()
