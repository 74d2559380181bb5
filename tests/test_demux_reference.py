"""The barcode demultiplexing contract (docs/demux.md) without a GPU: the two statements of tests/demux_ref.py against each
other and on hand cases, and the kernel's lanes run one after another on the CPU (pure_demux_scan: the dealing of patterns to
slots, the chunks and their warm-up, the reductions and the call rule) against them; the geometry stated in lib.py against
the header's; the binding table; every refused setting's message; the command line's parse errors (exit 1, nothing written) and
its refusal without a table (exit 2)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import demux_ref as DR
import ends_ref as R
from talc_amd import build as B
from talc_amd import lib as T

_pure = None


def pure():
    global _pure
    if _pure is None:
        L = C.CDLL(os.path.join(B.OUT, "libtalc_pure.so"))
        L.pure_demux_scan.restype = C.c_int
        L.pure_demux_scan.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_char_p, C.c_uint64]
        L.pure_demux_geometry.restype = None
        L.pure_demux_geometry.argtypes = [C.c_uint32, C.c_void_p]
        L.pure_demux_place.restype = None
        L.pure_demux_place.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _pure = L
    return _pure


def lanes_scan(reads, barcodes, pct, margin, window=DR.DEFAULT_WINDOW, both_ends=False):
    """k_read_demux's lanes one after another on the CPU; (rows, message): rows is None when the setting is refused."""
    bases, off = R.batch(reads)
    if len(bases) == 0:
        bases = np.zeros(1, np.uint8)
    out = np.zeros(max(len(reads), 1), DR.DTYPE)
    why = C.create_string_buffer(256)
    text = barcodes if isinstance(barcodes, bytes) else ",".join(barcodes).encode()
    rc = pure().pure_demux_scan(text, pct, margin, window, int(both_ends), bases.ctypes.data, off.ctypes.data, len(reads), out.ctypes.data, why, 256)
    return (out[:len(reads)] if rc == 0 else None), why.value.decode()


def all_ways(reads, barcodes, pct, margin, window=DR.DEFAULT_WINDOW, both_ends=False, plain=True):
    want = DR.rows(reads, barcodes, pct, margin, window, both_ends)
    got, why = lanes_scan(reads, barcodes, pct, margin, window, both_ends)
    assert got is not None, why
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    if plain:
        loops = DR.rows_plain(reads, barcodes, pct, margin, window, both_ends)
        bad = np.flatnonzero(loops != want)
        assert len(bad) == 0, (bad[:5], loops[bad[:5]], want[bad[:5]])
    return want


BC24 = DR.barcode_set(96, 24, seed=11, min_dist=9)
BC12 = DR.barcode_set(12, 12, seed=12, min_dist=5)
BC16 = DR.barcode_set(17, 16, seed=13, min_dist=6)
# (barcodes, max_error_pct, min_margin, window, both_ends)
SETTINGS = [(BC24, 20, 2, 32, False),      # 96 barcodes: three passes of whole windows; k = 4
            (BC12, 30, 1, 256, True),      # 12 of 12 letters at 30 per cent (k = 3): two chunks per pattern
            (BC24[:1], 25, 0, 4096, False),   # one barcode: 32 chunks per pattern over the whole read, second = k + 1
            (BC16, 12, 1, 64, False)]      # 17: the first count without chunks; k = 1


def test_the_barcode_sets_keep_their_distance():
    assert len(set(BC24)) == 96 and DR.min_pairwise_distance(BC24) >= 9
    assert DR.min_pairwise_distance(BC12) >= 5 and DR.min_pairwise_distance(BC16) >= 6
    assert DR.edit_distances("ACGTACGTACGT", ["ACGTACGTACGT", "CGTACGTACGTA", "TTTTTTTTTTTT"]).tolist() == [0, 2, 9]


def random_reads(rng, count, barcodes, k, window):
    m = len(barcodes[0])
    reads = []
    for i in range(count):
        n = (0, 1500)[i] if i < 2 else int(rng.integers(0, 61)) if i % 6 == 5 else int(rng.integers(0, 1501))
        s = R.random_seq(rng, n)
        if i % 4 != 3 and n >= 2 * m + 20:                           # a copy at the head, one at the tail: within or over the bound
            h = int(rng.integers(len(barcodes)))
            t = h if rng.integers(4) else int(rng.integers(len(barcodes)))
            room = max(1, min(window, n // 2) - m - 2)
            at = int(rng.integers(0, room))
            hc = R.mutate(rng, barcodes[h], int(rng.integers(0, k + 3)), "SIDN")
            tc = R.revcomp(R.mutate(rng, barcodes[t], int(rng.integers(0, k + 3)), "SID")).decode()
            if i % 8 != 0:
                s = s[:at] + hc + s[at + len(hc):]
            if i % 8 != 1:
                at = int(rng.integers(0, room))
                s = s[:n - at - len(tc)] + tc + s[n - at:]
        reads.append(s.lower() if i % 7 == 0 else s)
    return reads


@pytest.mark.parametrize("setting", range(4))
def test_numpy_the_loops_and_the_lanes_agree_on_random_reads(setting):
    barcodes, pct, margin, window, both = SETTINGS[setting]
    k = pct * len(barcodes[0]) // 100
    reads = random_reads(np.random.default_rng(60 + setting), 300, barcodes, k, window)
    assert len(reads) == 300 and min(map(len, reads)) == 0 and max(map(len, reads)) > 1400
    want = all_ways(reads, barcodes, pct, margin, window, both, plain=True)
    seen = np.bincount(want["status"], minlength=5)
    assert seen[DR.NONE] >= 20 and seen[DR.BOTH] >= 20 and seen[DR.HEAD_ONLY] >= 10 and seen[DR.TAIL_ONLY] >= 10, seen
    if len(barcodes) > 1:
        assert seen[DR.CONFLICT] >= 1, seen
        uncalled = (want["head_best"] > 0) & (want["head_margin"] < margin)
        assert margin < 2 or uncalled.any()                          # an accepted best that the margin keeps from calling
        assert len(set(want["barcode"].tolist())) > min(len(barcodes), 10) // 2
    else:
        assert (want["head_margin"][want["head_best"] > 0] == k + 1 - want["head_err"][want["head_best"] > 0]).all()
    assert int(want["head_err"].max()) == k and int(want["tail_err"].max()) == k and (want["head_err"] == 0).any()
    if both:
        assert (want["barcode"][want["status"] != DR.BOTH] == 0).all()


# ---------------------------------------------------------------- hand cases
A24, B24, C24 = BC24[0], BC24[1], BC24[2]


def test_every_branch_of_the_end_rule():
    rng = np.random.default_rng(1)
    body = R.random_seq(rng, 300)
    k = 4                                                             # 20 per cent of 24
    sub = lambda s, n: R.mutate(rng, s, n, "S")
    reads = [A24 + body,                                             # 0: exact
             sub(A24, k) + body,                                     # 1: k substitutions: accepted
             sub(A24, k + 3) + body,                                 # 2: beyond the bound: nothing
             "", "A", body[:23],                                     # 3-5: an empty window, one byte, m - 1 bytes
             body[:40] + B24 + body[40:],                            # 6: inside the window, not at the start
             body[:240] + B24 + body[240:]]                          # 7: it ends at 264, beyond a window of 256
    want = all_ways(reads, [A24, B24, C24], 20, 2)
    h = lambda r: tuple(int(want[r][f]) for f in ("head_best", "head_err", "head_margin", "head_end"))
    assert h(0) == (1, 0, 5, 24) and want[0]["barcode"] == 1 and want[0]["status"] == DR.HEAD_ONLY
    assert h(1)[:2] == (1, 4) and h(1)[2] == 1 and want[1]["barcode"] == 0 and want[1]["status"] == DR.NONE      # accepted, margin 1 < 2: no call
    assert h(2) == (0, 0, 0, 0) and h(3) == (0, 0, 0, 0) and h(4) == (0, 0, 0, 0) and h(5) == (0, 0, 0, 0)
    assert h(6) == (2, 0, 5, 64) and h(7) == (0, 0, 0, 0)
    assert all_ways(reads[1:2], [A24, B24, C24], 20, 1)[0]["barcode"] == 1                                      # the same margin suffices for 1
    # the largest e among equal D: cost 1 at 53 (deletion), 54 (substitution), 55 (insertion)
    last = A24[-1]
    other = next(ch for ch in "ACGT" if ch != last and ch != A24[-2])
    tie = "G" * 30 + A24[:-1] + other + last + "G" * 40
    D = R.sellers_plain(A24.encode(), tie.encode())
    assert min(D[1:]) == 1 and [e for e, d in enumerate(D) if d == 1] == [53, 54, 55]
    row = all_ways([tie], [A24, B24], 20, 0)[0]
    assert (row["head_best"], row["head_err"], row["head_end"]) == (1, 1, 55)
    # the lowest index among barcodes of equal c: B24 with one substitution is at 1 from B24 and from its twin with another letter there
    twin = B24[:10] + next(ch for ch in "ACGT" if ch != B24[10]) + B24[11:]
    third = next(ch for ch in "ACGT" if ch not in (B24[10], twin[10]))
    read = B24[:10] + third + B24[11:] + body
    row = all_ways([read], [A24, twin, B24], 20, 0)[0]
    assert (row["head_best"], row["head_err"], row["head_margin"], row["barcode"]) == (2, 1, 0, 2)
    assert all_ways([read], [A24, B24, twin], 20, 0)[0]["head_best"] == 2


def test_two_identical_barcodes_tie_at_margin_0():
    rng = np.random.default_rng(2)
    read = A24 + R.random_seq(rng, 200) + R.revcomp(A24).decode()
    for margin, barcode in ((0, 1), (1, 0)):
        row = all_ways([read], [A24, A24, B24], 20, margin)[0]
        assert (row["head_best"], row["head_err"], row["head_margin"], row["tail_best"], row["tail_margin"]) == (1, 0, 0, 1, 0)
        assert row["barcode"] == barcode and row["status"] == (DR.BOTH if barcode else DR.NONE)


def test_n_and_lower_case():
    rng = np.random.default_rng(3)
    body = R.random_seq(rng, 100)
    reads = [A24.lower() + body.lower(), A24[:12] + "N" + A24[13:] + body, A24[:12] + "n" + A24[12:] + body, "N" * 100, A24[:12].lower() + A24[12:] + body]
    want = all_ways(reads, [A24.lower(), B24], 20, 2)
    assert [(int(r["head_best"]), int(r["head_err"]), int(r["head_end"])) for r in want] == [(1, 0, 24), (1, 1, 24), (1, 1, 25), (0, 0, 0), (1, 0, 24)]
    assert (want["status"] == [DR.HEAD_ONLY, DR.HEAD_ONLY, DR.HEAD_ONLY, DR.NONE, DR.HEAD_ONLY]).all()


def test_every_row_of_the_call_table():
    rng = np.random.default_rng(4)
    body = R.random_seq(rng, 300)
    rc = lambda s: R.revcomp(s).decode()
    reads = [A24 + body + rc(A24), A24 + body, body + rc(B24), A24 + body + rc(B24), body,
             R.mutate(rng, A24, 4, "S") + body + rc(A24)]            # 5: the head's margin falls short by one: tail only
    for both in (False, True):
        want = all_ways(reads, [A24, B24, C24], 20, 2, both_ends=both)
        assert want["status"].tolist() == [DR.BOTH, DR.HEAD_ONLY, DR.TAIL_ONLY, DR.CONFLICT, DR.NONE, DR.TAIL_ONLY]
        assert want["barcode"].tolist() == ([1, 0, 0, 0, 0, 0] if both else [1, 1, 2, 0, 0, 1])
        assert want[5]["head_best"] == 1 and want[5]["head_margin"] == 1 and want[3]["head_best"] == 1 and want[3]["tail_best"] == 2
    for h in range(3):
        for t in range(3):
            for both in (False, True):
                barcode, status = DR.read_call(h, t, both)
                assert status == (DR.NONE if not h and not t else DR.BOTH if h == t else DR.CONFLICT if h and t else DR.HEAD_ONLY if h else DR.TAIL_ONLY)
                assert barcode == (h if status == DR.BOTH else 0 if both or status in (DR.NONE, DR.CONFLICT) else h or t)


def test_the_tail_is_the_head_of_the_reverse_complement():
    rng = np.random.default_rng(5)
    reads = random_reads(rng, 60, BC24[:8], 4, 256)
    fwd = all_ways(reads, BC24[:8], 20, 1, plain=False)
    rev = all_ways([R.revcomp(r) for r in reads], BC24[:8], 20, 1, plain=False)
    for f in ("best", "err", "margin", "end"):
        assert (fwd["tail_" + f] == rev["head_" + f]).all() and (fwd["head_" + f] == rev["tail_" + f]).all()
    assert (fwd["barcode"] == rev["barcode"]).all() and (fwd["tail_best"] > 0).sum() > 10
    swap = {DR.HEAD_ONLY: DR.TAIL_ONLY, DR.TAIL_ONLY: DR.HEAD_ONLY}
    assert [swap.get(s, s) for s in fwd["status"].tolist()] == rev["status"].tolist()


def test_both_ends_of_a_short_read_claim_the_same_bytes():
    pal = A24 + R.revcomp(A24).decode()                              # 48 bytes: the head's copy is the tail's, read the other way
    for L in (24, 30, 48):
        row = all_ways([pal[:L // 2] + pal[48 - (L - L // 2):]], [A24, B24], 20, 2)[0]
        if L == 48:
            assert (row["barcode"], row["status"], row["head_end"], row["tail_end"]) == (1, DR.BOTH, 24, 24)
    one = all_ways([A24], [R.revcomp(A24).decode(), A24], 20, 2)[0]  # one read of m bytes: the head calls 2, the tail 1
    assert (one["head_best"], one["tail_best"], one["status"], one["barcode"]) == (2, 1, DR.CONFLICT, 0)


# ---------------------------------------------------------------- the lanes at their borders
def test_the_geometry_is_stated_once():
    g, p = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    changes = []
    for n in range(1, 97):
        pure().pure_demux_geometry(n, g.ctypes.data)
        chunks, passes, tail_slot = g.tolist()
        for window in (32, 100, 256, 4096):
            assert T.demux_geometry(n, window) == (chunks, passes, tail_slot, -(-window // chunks))
        assert T.demux_geometry(n)[:3] == (chunks, passes, tail_slot)
        if n <= 16:
            assert chunks == 64 // (2 * n) and passes == 1 and tail_slot == n * chunks and 2 * n * chunks <= 64
        else:
            assert chunks == 1 and tail_slot % 32 == 0 and n <= tail_slot < n + 32 and passes == -(-2 * n // 64) and tail_slot + n <= 64 * passes <= 192
        for end, b, q, width in ((0, 0, 0, 256), (1, n - 1, chunks - 1, 255), (1, 0, chunks // 2, 33)):
            pure().pure_demux_place(n, end, b, q, width, p.ctypes.data)
            chunk = T.demux_geometry(n, width)[3]
            assert p.tolist() == [(tail_slot if end else 0) + b * chunks + q, min(width, q * chunk), min(width, (q + 1) * chunk)]
        if n > 1 and (chunks, passes) != changes[-1][1:]:
            changes.append((n, chunks, passes))
        elif n == 1:
            changes.append((n, chunks, passes))
    # where the dealing changes: the chunk counts of 1 .. 16, whole windows from 17, a second pass at 33, a third at 65
    assert [c[0] for c in changes if c[1] == 1] == [17, 33, 65] and changes[0] == (1, 32, 1) and (11, 2, 1) in changes and T.demux_geometry(16)[:2] == (2, 1)


@pytest.mark.parametrize("n_barcodes", [1, 2, 16])
def test_the_lanes_around_every_chunk_border(n_barcodes):
    """A barcode (exact, or with k substitutions) ending at every column within m + k + 2 of every chunk border, head and tail."""
    rng = np.random.default_rng(n_barcodes)
    barcodes = BC24[:n_barcodes]
    window, k = 256, 4
    chunks, _, _, chunk = T.demux_geometry(n_barcodes, window)
    assert chunks >= 2 and chunk * chunks >= window
    borders = list(range(chunk, window, chunk))
    reads = []
    for b in borders:
        for d in range(-(24 + k + 2), 24 + k + 3):
            e = b + d
            if e < 24 or e > window:
                continue
            which = int(rng.integers(n_barcodes))
            copy = R.mutate(rng, barcodes[which], k if d % 2 else 0, "S")
            s = R.random_seq(rng, 600)
            s = s[:e - 24] + copy + s[e:]
            reads.append(R.revcomp(s).decode() if d % 3 == 1 else s)
    want = all_ways(reads, barcodes, 20, 0, window, plain=False)
    ends = np.where(want["head_best"] > 0, want["head_end"], want["tail_end"])
    assert ((want["head_best"] > 0) | (want["tail_best"] > 0)).all() and {b for b in borders if b >= 24} <= set(ends.tolist())
    assert (want["head_err"] == k).any() and (want["tail_err"] == k).any()


# ---------------------------------------------------------------- the binding table, the refused settings
def test_the_binding_table_and_the_row():
    L = T.lib()
    for name in ("talc_ctx_set_demux", "talc_batch_demux", "talc_batch_fetch_demux", "talc_ctx_get_demux_timing"):
        assert hasattr(L, name) and name in T.ABI_SYMBOLS
    assert T.DEMUX_DTYPE == DR.DTYPE and T.DEMUX_DTYPE.itemsize == 16
    assert [T.DEMUX_DTYPE.fields[f][1] for f in T.DEMUX_DTYPE.names] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 12]
    assert (T.DEMUX_NONE, T.DEMUX_BOTH, T.DEMUX_HEAD_ONLY, T.DEMUX_TAIL_ONLY, T.DEMUX_CONFLICT) == (DR.NONE, DR.BOTH, DR.HEAD_ONLY, DR.TAIL_ONLY, DR.CONFLICT)
    assert L.talc_ctx_set_demux(None, b"ACGTACGTACGT", 10, 0, 0, 0) == -1 and L.talc_ctx_get_demux_timing(None, None) == -1
    assert L.talc_batch_demux(None, None) == -1 and L.talc_batch_fetch_demux(None, None, None) == -1
    assert L.talc_abi_version() == 1
    for name in ("set_demux", "demux_timing"):
        assert hasattr(T.Context, name)
    assert hasattr(T.Batch, "demux") and T.DEMUX_DEFAULT_WINDOW == DR.DEFAULT_WINDOW


REFUSED = [
    (([A24], 31, 0, 256, 0), "max_error_pct=31: at most 30"),
    (([A24], 20, 0, 31, 0), "window=31: 32 .. 4096 (0: 256)"),
    (([A24], 20, 0, 4097, 0), "window=4097: 32 .. 4096 (0: 256)"),
    (([A24], 20, 0, 256, 2), "both_ends=2: 0 or 1"),
    (([A24] * 97, 20, 0, 256, 0), "barcodes: more than 96"),
    (([A24, A24[:11]], 20, 0, 256, 0), "barcodes: barcode 2 has 11 letters: 12 .. 64"),
    (([A24 * 3], 20, 0, 256, 0), "barcodes: barcode 1 has 72 letters: 12 .. 64"),
    (([A24, A24[:23]], 20, 0, 256, 0), "barcodes: barcode 2 has 23 letters, barcode 1 has 24: one length for all"),
    (([A24, ""], 20, 0, 256, 0), "barcodes: barcode 2 has 0 letters: 12 .. 64"),
    (([A24, A24[:5] + "N" + A24[6:]], 20, 0, 256, 0), "barcodes: barcode 2 has a letter that is not one of ACGTacgt"),
    (([A24], 20, 6, 256, 0), "min_margin=6: 0 .. k + 1 (5)"),
    (([A24[:12]], 0, 2, 256, 0), "min_margin=2: 0 .. k + 1 (1)"),
]


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_every_refused_setting_names_the_bad_value(case):
    (barcodes, pct, margin, window, both), message = REFUSED[case]
    rows, why = lanes_scan(["ACGT" * 20], barcodes, pct, margin, window, both)
    assert rows is None and why == message


def test_accepted_at_the_edges_of_the_ranges():
    for args in (([A24], 30, 8, 4096, 1), ([A24[:12]], 0, 1, 32, 0), ([A24 + A24 + A24[:16]], 30, 20, 0, 0), (BC24, 20, 5, 0, 1)):
        rows, why = lanes_scan(["ACGT" * 20], *args)
        assert rows is not None, why
    rows, why = lanes_scan(["ACGT" * 20], b"", 20, 0, 256, 0)         # no barcodes: the setting is off
    assert rows is None and why == "the setting is off"


# ---------------------------------------------------------------- the command line
TALC = os.path.join(B.OUT, "talc")
BASE = ["reads.fa", "-k", "21", "-SR", "sr.dump", "-o", "o"]
GOOD = ">bc01\n" + A24 + "\n>bc02 second\n" + B24[:12] + "\n" + B24[12:] + "\n"


@pytest.mark.parametrize("fasta,extra,word", [
    (None, ["--LRBarcodeErr", "10"], "--LRBarcodeErr needs --LRBarcodes"),
    (None, ["--LRBarcodeMargin", "1"], "--LRBarcodeMargin needs --LRBarcodes"),
    (None, ["--LRBarcodeWindow", "100"], "--LRBarcodeWindow needs --LRBarcodes"),
    (None, ["--LRBarcodeBothEnds"], "--LRBarcodeBothEnds needs --LRBarcodes"),
    (None, ["--LRDemuxOut"], "--LRDemuxOut needs --LRBarcodes"),
    (None, ["--LRBarcodes", "missing.fa"], "LRBarcodes: cannot read missing.fa"),
    (None, ["--LRBarcodes"], "requires an argument"),
    ("", ["--LRBarcodes", "bc.fa"], "LRBarcodes: no barcode in bc.fa"),
    (A24 + "\n", ["--LRBarcodes", "bc.fa"], "does not start with a '>' line"),
    (GOOD, ["--LRBarcodes", "bc.fa", "--LRBarcodeErr", "31"], "LRBarcodeErr: 0..30"),
    (GOOD, ["--LRBarcodes", "bc.fa", "--LRBarcodeErr", "2.5"], "LRBarcodeErr"),
    (GOOD, ["--LRBarcodes", "bc.fa", "--LRBarcodeWindow", "31"], "LRBarcodeWindow: 32..4096"),
    (GOOD, ["--LRBarcodes", "bc.fa", "--LRBarcodeWindow", "4097"], "LRBarcodeWindow: 32..4096"),
    (GOOD, ["--LRBarcodes", "bc.fa", "--LRBarcodeMargin", "6"], "LRBarcodeMargin: 6 is above k + 1 = 5"),
    (GOOD, ["--LRBarcodes", "bc.fa", "--LRBarcodeErr", "0", "--LRBarcodeMargin", "2"], "LRBarcodeMargin: 2 is above k + 1 = 1"),
    (GOOD, ["--LRBarcodes", "bc.fa", "--LRBarcodeMargin", "-1"], "LRBarcodeMargin"),
    (GOOD + ">bc01\n" + C24 + "\n", ["--LRBarcodes", "bc.fa"], "the name 'bc01' is given twice"),
    (">unclassified\n" + A24 + "\n", ["--LRBarcodes", "bc.fa"], "the name 'unclassified' is taken"),
    (">a/b\n" + A24 + "\n", ["--LRBarcodes", "bc.fa"], "the name 'a/b' cannot be a barcode's"),
    (">\n" + A24 + "\n", ["--LRBarcodes", "bc.fa"], "the name '' cannot be a barcode's"),
    (">" + "x" * 33 + "\n" + A24 + "\n", ["--LRBarcodes", "bc.fa"], "cannot be a barcode's"),
    (">a\n" + A24[:11] + "\n", ["--LRBarcodes", "bc.fa"], "the barcode a has 11 letters: 12..64"),
    (">a\n" + A24 * 3 + "\n", ["--LRBarcodes", "bc.fa"], "the barcode a has 72 letters: 12..64"),
    (">a\n" + A24 + "\n>b\n" + B24[:23] + "\n", ["--LRBarcodes", "bc.fa"], "the barcode b has 23 letters, a has 24: one length for all"),
    (">a\n" + A24[:5] + "N" + A24[6:] + "\n", ["--LRBarcodes", "bc.fa"], "the barcode a has a letter that is not one of ACGT"),
    ("".join(">b%d\n%s\n" % (i, s) for i, s in enumerate(BC24 + [A24])), ["--LRBarcodes", "bc.fa"], "more than 96 barcodes"),
])
def test_cli_parse_errors_exit_1_and_write_nothing(tmp_path, fasta, extra, word):
    if fasta is not None:
        (tmp_path / "bc.fa").write_text(fasta)
    r = subprocess.run([TALC] + BASE + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and word in r.stderr.decode(), (r.returncode, r.stderr.decode())
    assert os.listdir(tmp_path) == ([] if fasta is None else ["bc.fa"])


def test_cli_help_names_the_options():
    r = subprocess.run([TALC, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0
    for opt in ("--LRBarcodes", "--LRBarcodeErr", "--LRBarcodeMargin", "--LRBarcodeWindow", "--LRBarcodeBothEnds", "--LRDemuxOut"):
        assert opt.encode() in r.stdout


@pytest.mark.parametrize("extra", [[], ["--LRDemuxOut"], ["--LRBarcodeErr", "10", "--LRBarcodeMargin", "1", "--LRBarcodeWindow", "64", "--LRBarcodeBothEnds"]])
def test_cli_refuses_the_options_in_a_run_without_a_table(tmp_path, extra):
    (tmp_path / "reads.fa").write_text(">r\n" + "ACGT" * 30 + "\n")
    (tmp_path / "sr.dump").write_text("ACGTACGTACGTACGTACGTA 5\n")
    (tmp_path / "bc.fa").write_text(GOOD)
    r = subprocess.run([TALC, "reads.fa", "-k", "21", "-SR", "sr.dump", "-qm", "jellyfish2", "-o", "o", "--LRBarcodes", "bc.fa"] + extra, cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and b"no table" in r.stderr
    assert not (tmp_path / "o.fa").exists() and not (tmp_path / "o.demux.tsv").exists() and not (tmp_path / "o.bc01.fa").exists()
