"""Barcode demultiplexing on the device (docs/demux.md; k_read_demux, talc_batch_demux, the scan inside
talc_batch_create_clipped and talc_batch_create_split) against the contract in numpy (tests/demux_ref.py: never from a device
result).  Integers, tolerance 0.  Every case first asserts, from the reference alone, that its input reaches what it is there
for."""
import os
import subprocess

import numpy as np
import pytest

import chimera_ref as CR
import demux_ref as DR
import ends_ref as R
import parity_util as PU
import test_gpu_chimera as GC
import test_gpu_solidity as G
from memcheck_util import guards_checked
from talc_amd import build as B
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ERR_INVALID, ERR_STATE = -1, -6
SSP, VNP = CR.SSP, CR.VNP
BC24 = DR.barcode_set(96, 24, seed=11, min_dist=9)
A24, B24, C24 = BC24[:3]
SUB_PLACES = (3, 8, 12, 17, 21)                                          # apart: k substitutions there cost exactly k

_ctx = []


def ctx():
    """A context of its own over the shared table of test_gpu_solidity's default set."""
    if not _ctx:
        c = G.gen_set("default")
        _ctx.append(T.Context(c.ttab, c.p, 0))
    return _ctx[0]


def device_rows(reads, barcodes, pct, margin, window=DR.DEFAULT_WINDOW, both_ends=False):
    c = ctx()
    c.set_demux(barcodes, pct, margin, window, both_ends)
    try:
        b = c.batch(*R.batch(reads))
        try:
            return b.demux()
        finally:
            b.close()
    finally:
        c.set_demux()


def same_rows(got, want, what=""):
    assert got.dtype == DR.DTYPE and T.DEMUX_DTYPE == DR.DTYPE and len(got) == len(want), what
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def check(reads, what, barcodes, pct, margin, window=DR.DEFAULT_WINDOW, both_ends=False):
    want = DR.rows(reads, barcodes, pct, margin, window, both_ends)
    same_rows(device_rows(reads, barcodes, pct, margin, window, both_ends), want, what)
    return want


def subs(seq, places):
    s = list(seq)
    for at in places:
        s[at] = "ACGT"[("ACGT".index(s[at]) + 1) % 4]
    return "".join(s)


# ---------------------------------------------------------------- 1. one barcode ending at every column of a window
@pytest.mark.parametrize("level", [0, 4, 5])
def test_one_barcode_that_ends_at_every_column_of_a_window(level):
    rng = np.random.default_rng(500 + level)
    k, window, L = 20 * 24 // 100, 192, 400
    assert k == 4 and level in (0, k, k + 1)
    copy = subs(A24, SUB_PLACES[:level])
    ends = list(range(24, window + 1))
    reads = [R.random_seq(rng, e - 24) + copy + R.random_seq(rng, L - e) for e in ends]
    reads += [R.revcomp(r).decode() for r in reads]
    want = check(reads, "sweep, %d edits" % level, [A24], 20, 0, window)
    n = len(ends)
    if level <= k:
        assert (want["head_best"][:n] == 1).all() and (want["tail_best"][n:] == 1).all() and (want["barcode"] == 1).all()
        assert (want["head_err"][:n] <= level).all() and (want["head_err"][:n] == level).sum() >= n - 4
        assert (want["head_end"][:n] == ends).sum() >= n - 4 and (want["tail_end"][n:] == ends).sum() >= n - 4
        assert (want["head_margin"][:n] == k + 1 - want["head_err"][:n]).all()
    else:
        assert (want["barcode"] == 0).sum() >= 2 * n - 8                  # one edit too many: chance calls at most


def test_an_insertion_and_a_deletion():
    rng = np.random.default_rng(7)
    reads = []
    for kind in "ID":
        for n_edits in (1, 2, 4):
            for junk in (0, 3, 60):
                s = R.random_seq(rng, junk) + R.mutate(rng, B24, n_edits, kind) + R.random_seq(rng, 300)
                reads += [s, R.revcomp(s).decode()]
    want = check(reads, "indels", [A24, B24, C24], 20, 2)
    assert (want["head_best"][0::2] == 2).all() and (want["tail_best"][1::2] == 2).all()
    assert int(want["head_err"].max()) == 4 and (want["head_err"][0::2] >= 1).all() and len(set(want["head_end"][0:6:2].tolist())) > 1


# ---------------------------------------------------------------- 2. where the dealing of patterns to lanes changes
@pytest.mark.parametrize("n_barcodes", [1, 2, 16, 17, 32, 33, 64, 65, 96])
def test_the_first_and_the_last_pattern_of_every_pass(n_barcodes):
    rng = np.random.default_rng(n_barcodes)
    chunks, passes, tail_slot, _ = T.demux_geometry(n_barcodes)
    assert (chunks, passes) == {1: (32, 1), 2: (16, 1), 16: (2, 1), 17: (1, 1), 32: (1, 1), 33: (1, 2), 64: (1, 2), 65: (1, 3), 96: (1, 3)}[n_barcodes]
    barcodes = BC24[:n_barcodes]
    heads, tails = set(), set()
    for p in range(passes):                                              # the barcodes in the first and the last occupied slot of a pass, by end
        lo, hi = 64 * p, 64 * p + 63
        if chunks > 1:
            heads |= {0, n_barcodes - 1}
            tails |= {0, n_barcodes - 1}
            continue
        if lo < n_barcodes:
            heads |= {lo, min(hi, n_barcodes - 1)}
        if hi >= tail_slot and lo < tail_slot + n_barcodes:
            tails |= {max(lo, tail_slot) - tail_slot, min(hi, tail_slot + n_barcodes - 1) - tail_slot}
    reads, planted = [], []
    for h in sorted(heads):
        for t in sorted(tails):
            reads.append(R.random_seq(rng, int(rng.integers(0, 9))) + subs(barcodes[h], SUB_PLACES[:2]) + R.random_seq(rng, 500) +
                         R.revcomp(barcodes[t]).decode() + R.random_seq(rng, int(rng.integers(0, 9))))
            planted.append((h + 1, t + 1))
    want = check(reads, "%d barcodes" % n_barcodes, barcodes, 20, 2)
    assert [(int(r["head_best"]), int(r["tail_best"])) for r in want] == planted
    assert (want["status"] == [DR.BOTH if h == t else DR.CONFLICT for h, t in planted]).all() and (want["head_err"] == 2).all()


@pytest.mark.parametrize("n_barcodes", [1, 2, 16])
def test_a_barcode_around_every_chunk_border(n_barcodes):
    rng = np.random.default_rng(40 + n_barcodes)
    barcodes = BC24[:n_barcodes]
    window, k = 256, 4
    chunks, _, _, chunk = T.demux_geometry(n_barcodes, window)
    assert chunks >= 2 and chunk * chunks >= window
    borders = list(range(chunk, window, chunk))
    reads = []
    for b in borders:
        for d in range(-(24 + k + 2), 24 + k + 3):
            e = b + d
            if 24 <= e <= window:
                copy = subs(barcodes[int(rng.integers(n_barcodes))], SUB_PLACES[:k if d % 2 else 0])
                s = R.random_seq(rng, e - 24) + copy + R.random_seq(rng, 600 - e)
                reads.append(R.revcomp(s).decode() if d % 3 == 1 else s)
    want = check(reads, "chunk borders, %d barcodes" % n_barcodes, barcodes, 20, 0, window)
    ends = np.where(want["head_best"] > 0, want["head_end"], want["tail_end"])
    assert ((want["head_best"] > 0) | (want["tail_best"] > 0)).all() and {b for b in borders if b >= 24} <= set(ends.tolist())
    assert (want["head_err"] == k).any() and (want["tail_err"] == k).any()


# ---------------------------------------------------------------- 3. lengths, bounds, windows
@pytest.mark.parametrize("m,pct", [(12, 0), (12, 30), (64, 0), (64, 30)])
def test_the_shortest_and_the_longest_barcode_at_both_error_bounds(m, pct):
    rng = np.random.default_rng(3000 + m + pct)
    barcodes = DR.barcode_set(3, m, seed=m, min_dist=m // 3)
    k = pct * m // 100
    assert k == {(12, 0): 0, (12, 30): 3, (64, 0): 0, (64, 30): 19}[(m, pct)] and DR.min_pairwise_distance(barcodes) >= m // 3
    reads, level = [], []
    for n_edits in sorted({0, k, k + 1, min(k + 8, m - 2)}):
        for junk in (0, 5, 64, 150):
            for which in range(3):
                places = rng.choice(np.arange(1, m - 1), size=n_edits, replace=False).tolist()
                s = R.random_seq(rng, junk) + subs(barcodes[which], places) + R.random_seq(rng, 400)
                reads += [s, R.revcomp(s).decode()]
                level += [n_edits, n_edits]
                if n_edits:
                    reads.append(R.random_seq(rng, junk) + R.mutate(rng, barcodes[which], n_edits, "SID") + R.random_seq(rng, 400))
                    level.append(n_edits)
    want = check(reads, "barcodes of %d at %d per cent" % (m, pct), barcodes, pct, min(1, k + 1))
    level = np.array(level)
    found = (want["head_best"] > 0) | (want["tail_best"] > 0)
    assert found[level <= k].sum() >= (level <= k).sum() - 2 and max(k - 1, 0) <= int(max(want["head_err"].max(), want["tail_err"].max())) <= k
    assert not found[level > k + 4].any() if pct == 0 else True


@pytest.mark.parametrize("window", [32, 256, 4096])
def test_reads_around_the_window(window):
    rng = np.random.default_rng(window)
    m = 24
    pal = A24 + R.revcomp(A24).decode()                                  # in the middle of a read both ends claim it
    reads = []
    for L in (0, 1, m - 1, m, window - 1, window, 2 * window - 1):
        if L >= len(pal):
            at = (L - len(pal)) // 2
            s = R.random_seq(rng, at) + pal + R.random_seq(rng, L - at - len(pal))
        else:
            s = pal[:L]
        reads += [s, R.random_seq(rng, L)]
        if L >= m:
            reads += [A24 + R.random_seq(rng, L - m), R.random_seq(rng, L - m) + R.revcomp(B24).decode(), R.random_seq(rng, L - m) + B24]
    want = check(reads, "window %d" % window, [A24, B24, C24], 20, 2, window)
    assert [len(r) for r in reads[:6:2]] == [0, 1, 23] and (want["status"][:4] == 0).all()
    assert (want["status"] == DR.BOTH).sum() >= 1 and (want["status"] == DR.HEAD_ONLY).sum() >= 4 and (want["status"] == DR.TAIL_ONLY).sum() >= 4
    both = want[want["status"] == DR.BOTH]
    assert (both["head_end"] > m).any() and (np.abs(both["head_end"].astype(int) - both["tail_end"].astype(int)) <= 1).all()       # the palindrome's halves, from either end
    # a barcode that ends just inside and just outside the window
    edge = [R.random_seq(rng, window - m) + A24 + R.random_seq(rng, 4200), R.random_seq(rng, window - m + 8) + A24 + R.random_seq(rng, 4200)]
    want = check(edge, "window's edge", [A24, B24], 20, 2, window)
    assert want["head_best"].tolist() == [1, 0] and want[0]["head_end"] == window


def test_one_read_of_140_kb():
    rng = np.random.default_rng(140)
    reads = [R.random_seq(rng, 5) + BC24[95] + R.random_seq(rng, 140_000) + R.revcomp(BC24[95]).decode() + "ACG", R.random_seq(rng, 140_000)]
    want = check(reads, "140 kb", BC24, 20, 2)
    assert (want[0]["barcode"], want[0]["status"], want[0]["head_end"], want[0]["tail_end"]) == (96, DR.BOTH, 29, 27)


def test_every_row_of_the_call_table():
    rng = np.random.default_rng(4)
    body = R.random_seq(rng, 300)
    rc = lambda s: R.revcomp(s).decode()
    reads = [A24 + body + rc(A24), A24 + body, body + rc(B24), A24 + body + rc(B24), body,
             subs(A24, SUB_PLACES[:4]) + body + rc(A24)]                 # 5: the head's margin falls short by one: tail only
    for both in (False, True):
        want = check(reads, "call table", [A24, B24, C24], 20, 2, both_ends=both)
        assert want["status"].tolist() == [DR.BOTH, DR.HEAD_ONLY, DR.TAIL_ONLY, DR.CONFLICT, DR.NONE, DR.TAIL_ONLY]
        assert want["barcode"].tolist() == ([1, 0, 0, 0, 0, 0] if both else [1, 1, 2, 0, 0, 1])
        assert want[5]["head_best"] == 1 and want[5]["head_margin"] == 1 and want[5]["head_err"] == 4
    want = check(reads[:1], "identical barcodes", [A24, A24, B24], 20, 0)                      # a tie: margin 0, the lowest index
    assert (want[0]["barcode"], want[0]["head_margin"], want[0]["tail_margin"]) == (1, 0, 0)
    assert check(reads[:1], "identical barcodes", [A24, A24, B24], 20, 1)[0]["barcode"] == 0


def test_random_reads_with_96_barcodes():
    rng = np.random.default_rng(2)
    reads = [R.random_seq(rng, int(n)) for n in rng.integers(0, 300, 2000).tolist()]
    check(reads, "random reads", BC24, 25, 1, 64)                        # whatever the reference finds (a window of 64: the reference's time)


def test_random_reads_with_96_barcodes_over_the_default_window():
    rng = np.random.default_rng(3)
    reads = [R.random_seq(rng, int(n)) for n in rng.integers(200, 900, 250).tolist()]
    want = check(reads, "random reads, window 256", BC24, 25, 1)          # three passes of 256 columns on random content
    assert (want["head_best"] > 0).sum() + (want["tail_best"] > 0).sum() >= 20     # (870 of 4000 random ends accept at 25 per cent)


# ---------------------------------------------------------------- 4. clipped and split batches
ENDS_KW = dict(adapters=[SSP, VNP], max_error_pct=20, poly_min=12, window=512)
PCT, MIN_PIECE = 10, 100
DEMUX = (BC24, 20, 2)

_dressed = {}


def dressed():
    """200 generator reads, each behind barcode, junk, primer and poly-T and in front of the mirror image; every tenth joined
    to the next; the reference's rows; and what a clipped and a split batch give with demux off."""
    if not _dressed:
        c = G.gen_set("default")
        rng = np.random.default_rng(8)
        one = [DR.dress(rng, R.as_bytes(body).decode(), BC24[int(rng.integers(96))], (SSP, VNP), max_edits=3) for body in c.reads[:200]]
        reads, i = [], 0
        while i < len(one):
            if i % 10 == 9 and i + 1 < len(one):
                reads.append(one[i] + CR.joint(rng) + one[i + 1])
                i += 2
            else:
                reads.append(one[i])
                i += 1
        want = DR.rows(reads, *DEMUX)
        off = T.Context(c.ttab, c.p, 0)
        try:
            off.set_ends(**ENDS_KW)
            off.set_chimera(True, PCT, MIN_PIECE)
            base = (GC.everything_of(off, *R.batch(reads), clip=True, ends=True), GC.everything_of(off, *R.batch(reads), split=True, clip=True, ends=True),
                    GC.everything_of(off, *R.batch(reads), split=True))
        finally:
            off.close()
        _dressed.update(c=c, reads=reads, want=want, base=base)
    return _dressed


def with_demux(r):
    """The same three batches with demux on: (their outputs, their rows, the rows of a plain batch)."""
    on = T.Context(r["c"].ttab, r["c"].p, 0)
    try:
        on.set_ends(**ENDS_KW)
        on.set_chimera(True, PCT, MIN_PIECE)
        on.set_demux(*DEMUX)
        outs, rows = [], []
        for kw in (dict(clip=True, ends=True), dict(split=True, clip=True, ends=True), dict(split=True)):
            outs.append(GC.everything_of(on, *R.batch(r["reads"]), **kw))
            b = on.batch(*R.batch(r["reads"]), clip=kw.get("clip", False), split=kw.get("split", False))
            try:
                rows.append(b.demux())
                assert on.demux_timing() == 0.0                          # the rows came with the batch: nothing ran again
            finally:
                b.close()
        b = on.batch(*R.batch(r["reads"]))
        try:
            plain = b.demux()
        finally:
            b.close()
        return outs, rows, plain
    finally:
        on.close()


def same_outputs(got, base, what):
    GC.same_batches(got, base, what)
    assert (got["rows"] == base["rows"]).all() if "rows" in base else True
    if "pieces" in base:
        assert (got["pieces"] == base["pieces"]).all() and (got["hits"] == base["hits"]).all()


def test_clipped_and_split_batches_carry_the_rows_of_the_reads_as_they_came():
    r = dressed()
    want, n = r["want"], len(r["reads"])
    assert n == 181 and (want["status"] == DR.BOTH).sum() >= 150 and len(set(want["barcode"].tolist())) > 60       # from the reference alone
    assert int(want["head_err"].max()) >= 2 and r["base"][1]["n"] > n and r["base"][0]["n_bases"] < sum(map(len, r["reads"])) - 40 * n
    outs, rows, plain = with_demux(r)
    same_rows(plain, want, "plain batch")
    for got, what in zip(rows, ("clipped", "split and clipped", "split")):
        same_rows(got, want, what)
    for got, base, what in zip(outs, r["base"], ("clipped", "split and clipped", "split")):
        same_outputs(got, base, what)


@pytest.mark.parametrize("byte", [0xA5, 0xFF])
def test_clipped_and_split_batches_on_poisoned_memory_between_red_zones(byte):
    r = dressed()
    with guards_checked():
        with T.poisoned(byte):
            outs, rows, plain = with_demux(r)
    same_rows(plain, r["want"], "poisoned, plain")
    for got, what in zip(rows, ("clipped", "split and clipped", "split")):
        same_rows(got, r["want"], "poisoned, " + what)
    for got, base, what in zip(outs, r["base"], ("clipped", "split and clipped", "split")):
        same_outputs(got, base, "poisoned, " + what)


# ---------------------------------------------------------------- 5. no behaviour change, state errors, generations
def test_a_context_that_never_set_the_option_and_one_that_switched_it_off_again():
    c = G.gen_set("default")
    reads = c.reads[:80]
    never, other = T.Context(c.ttab, c.p, 0), T.Context(c.ttab, c.p, 0)
    try:
        other.set_demux(*DEMUX)
        other.set_demux()
        a = GC.everything_of(never, *PU.pack_reads(reads))
        b = GC.everything_of(other, *PU.pack_reads(reads))
        assert a["per"] == b["per"] and a["work"] == b["work"] and a["work"][1] > 0 and a["cov"] == b["cov"]
        assert [p[0].decode() for p in a["per"]] == c.run["records"][:80] and [p[1] for p in a["per"]] == c.run["st"][:80].tolist()
        assert never.demux_timing() == 0.0 and other.demux_timing() == 0.0
    finally:
        never.close()
        other.close()


def test_the_state_errors_and_the_refused_settings():
    c = G.gen_set("default")
    L = T.lib()
    one, other = T.Context(c.ttab, c.p, 0), T.Context(c.ttab, c.p, 0)
    rng = np.random.default_rng(9)
    reads = [A24 + R.random_seq(rng, 200) + R.revcomp(A24).decode(), B24 + R.random_seq(rng, 200), R.random_seq(rng, 200)]
    want = DR.rows(reads, [A24, B24], 20, 2)
    assert want["barcode"].tolist() == [1, 2, 0]
    bases, offs = R.batch(reads)
    b = one.batch(bases, offs)
    rows = np.zeros(3, DR.DTYPE)
    try:
        assert L.talc_batch_demux(one._h, b._h) == ERR_STATE and b"off" in L.talc_last_error()
        assert L.talc_batch_fetch_demux(one._h, b._h, rows.ctypes.data) == ERR_STATE and b"scan" in L.talc_last_error()
        one.set_ends(adapters=[SSP])
        cb = one.batch(bases, offs, clip=True)                           # made while the scan was off: it never gets rows
        one.set_demux([A24, B24], 20, 2)
        try:
            assert L.talc_batch_demux(one._h, cb._h) == ERR_STATE and b"clipped" in L.talc_last_error()
            assert L.talc_batch_fetch_demux(one._h, cb._h, rows.ctypes.data) == ERR_STATE
        finally:
            cb.close()
        for kw, word in ((dict(max_error_pct=31), "max_error_pct=31"), (dict(min_margin=6), "min_margin=6"), (dict(window=5000), "window=5000")):
            with pytest.raises(T.TalcError, match=word):
                one.set_demux([A24, B24], **{**dict(max_error_pct=20, min_margin=2), **kw})
        with pytest.raises(T.TalcError, match="barcode 2 has 23 letters"):
            one.set_demux([A24, B24[:23]])
        same_rows(b.demux(), want, "a refused setting changes nothing")
        assert L.talc_batch_demux(other._h, b._h) == ERR_INVALID           # another context's batch
        one.set_demux()
        assert L.talc_batch_demux(one._h, b._h) == ERR_STATE
        assert L.talc_batch_fetch_demux(one._h, b._h, rows.ctypes.data) == 0 and (rows == want).all()   # the rows of the last scan stay
    finally:
        b.close()
        one.close()
        other.close()


def test_a_new_setting_scans_again_and_the_same_setting_does_not():
    c = ctx()
    rng = np.random.default_rng(10)
    reads = [subs(A24, SUB_PLACES[:3]) + R.random_seq(rng, 300) for _ in range(50)]
    loose, tight = DR.rows(reads, [A24, B24], 20, 2), DR.rows(reads, [A24, B24], 10, 0)
    assert (loose["barcode"] == 1).all() and (tight["barcode"] == 0).all()
    b = c.batch(*R.batch(reads))
    try:
        c.set_demux([A24, B24], 20, 2)
        same_rows(b.demux(), loose, "first setting")
        assert c.demux_timing() > 0.0
        same_rows(b.demux(), loose, "the same setting")
        assert c.demux_timing() == 0.0                                   # nothing was launched
        c.set_demux([A24, B24], 10, 0)
        same_rows(b.demux(), tight, "second setting")
        assert c.demux_timing() > 0.0
    finally:
        b.close()
        c.set_demux()


# ---------------------------------------------------------------- 6. the command line
def test_cli_demux_with_clip_and_split_in_small_batches(tmp_path):
    c = G.gen_set("default")
    rng = np.random.default_rng(33)
    n = 60
    seqs = BC24[:12]
    bc_names = ["bc%02d" % (i + 1) for i in range(12)]
    one = []
    for i, body in enumerate(c.reads[:n]):
        body = R.as_bytes(body).decode()
        one.append(body if i % 7 == 3 else DR.dress(rng, body, seqs[i % 10], (SSP, VNP), max_edits=2))      # (two barcodes get no read)
    reads, i = [], 0
    while i < n:
        if i % 5 == 4 and i + 1 < n:                                     # joined to the next: a chimera whose ends carry two barcodes
            reads.append(one[i] + CR.joint(rng) + one[i + 1])
            i += 2
        else:
            reads.append(one[i])
            i += 1
    names = ["read%d/x" % i for i in range(len(reads))]
    want = DR.rows(reads, seqs, 20, 2)
    tight = DR.rows(reads, seqs, 10, 1, 64, True)
    seen = np.bincount(want["status"], minlength=5)
    assert seen[DR.BOTH] >= 25 and seen[DR.CONFLICT] >= 5 and seen[DR.NONE] >= 3 and seen[DR.HEAD_ONLY] + seen[DR.TAIL_ONLY] >= 2, seen
    assert set(want["barcode"].tolist()) == set(range(11)) and (tight["barcode"] != want["barcode"]).any()
    hits, _ = CR.hits(reads, [SSP, VNP], GC.PCT)
    pieces, piece_off, _, _ = CR.pieces([len(x) for x in reads], hits, GC.MIN_PIECE)
    piece_names = CR.piece_names(names, pieces)
    assert len(pieces) > len(reads) + 5
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    (tmp_path / "dressed.fa").write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, reads)))
    (tmp_path / "bc.fa").write_text("".join(">%s sample %d\n%s\n" % (nm, i, s) for i, (nm, s) in enumerate(zip(bc_names, seqs))))
    common = [str(tmp_path / "dressed.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7", "-o", "o"]
    lr = ["--LRAdapter", SSP, "--LRAdapter", VNP, "--LRPolyA", "12", "--LRSplit", "--LRClip"]
    bc = ["--LRBarcodes", str(tmp_path / "bc.fa")]
    runs = {}
    for d, args, env in (("full", lr + bc + ["--LRDemuxOut"], None), ("off", lr, None), ("full2", lr + bc + ["--LRDemuxOut", "--gpus", "2"], dict(os.environ, TALC_FAKE_GPUS="2")),
                         ("plain", bc + ["--LRBarcodeErr", "10", "--LRBarcodeMargin", "1", "--LRBarcodeWindow", "64", "--LRBarcodeBothEnds"], None)):
        (tmp_path / d).mkdir()
        runs[d] = subprocess.run([TALC] + common + args, cwd=tmp_path / d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert runs[d].returncode == 0, (d, runs[d].stderr.decode())
    read = lambda d, ext: (tmp_path / d / ("o" + ext)).read_bytes() if (tmp_path / d / ("o" + ext)).exists() else None
    for ext in (".fa", ".log", ".ends.tsv", ".chimera.tsv", ".chimera_pieces.tsv"):
        assert read("full", ext) == read("off", ext) and read("full2", ext) == read("full", ext), ext      # demux changes no other output
    name_of = lambda b: bc_names[int(b) - 1] if b else "-"

    def tsv(rows):
        out = ["read_name\traw_length\tbarcode\tstatus\thead_barcode\thead_err\thead_margin\thead_end\ttail_barcode\ttail_err\ttail_margin\ttail_end"]
        for nm, s, w in zip(names, reads, rows):
            out.append("\t".join([nm, str(len(s)), name_of(w["barcode"]), str(int(w["status"])), name_of(w["head_best"]), str(int(w["head_err"])), str(int(w["head_margin"])),
                                  str(int(w["head_end"])), name_of(w["tail_best"]), str(int(w["tail_err"])), str(int(w["tail_margin"])), str(int(w["tail_end"]))]))
        return out

    def counts(rows):
        out = ["barcode\treads\tbases"]
        lens = np.array([len(s) for s in reads])
        for b in list(range(1, 13)) + [0]:
            mine = rows["barcode"] == b
            out.append("%s\t%d\t%d" % (bc_names[b - 1] if b else "unclassified", int(mine.sum()), int(lens[mine].sum())))
        return out

    def line(rows):
        cls = rows["barcode"] > 0
        st = rows["status"]
        return "[TALC]: demux: %d reads, %d classified (%d both ends, %d head only, %d tail only), %d conflicts, %d without a barcode" % (
            len(rows), int(cls.sum()), int((cls & (st == DR.BOTH)).sum()), int((cls & (st == DR.HEAD_ONLY)).sum()), int((cls & (st == DR.TAIL_ONLY)).sum()),
            int((st == DR.CONFLICT).sum()), int((~cls & (st != DR.CONFLICT)).sum()))

    for d, rows in (("full", want), ("full2", want), ("plain", tight)):
        assert read(d, ".demux.tsv").decode().splitlines() == tsv(rows), d
        assert read(d, ".demux_counts.tsv").decode().splitlines() == counts(rows), d
        assert runs[d].stdout.decode().splitlines().count(line(rows)) == 1, (d, line(rows))
    assert b"demux:" not in runs["off"].stdout and read("off", ".demux.tsv") is None and read("plain", ".bc01.fa") is None
    assert b"correcting on 2 GPU(s)" in runs["full2"].stdout
    # the per-barcode files: every record of <o>.fa, byte for byte and in order, dealt by the reference's call of its source read
    records = [b">" + x for x in read("full", ".fa").split(b">")[1:]]
    assert [x.split(b"\n")[0][1:].decode() for x in records] == piece_names
    dealt = {nm: b"" for nm in bc_names + ["unclassified"]}
    for rec, p in zip(records, pieces):
        b = int(want[int(p["read"])]["barcode"])
        dealt[bc_names[b - 1] if b else "unclassified"] += rec
    assert sum(1 for v in dealt.values() if v) == 11 and dealt["bc11"] == b"" and dealt["bc12"] == b""
    for d in ("full", "full2"):
        for nm, text in dealt.items():
            assert read(d, ".%s.fa" % nm) == text, (d, nm)
    cfg = read("plain", ".config.txt").decode().splitlines()
    at = cfg.index("queryMode=memory")
    assert cfg[at + 1:at + 6] == ["LRBarcodes=" + str(tmp_path / "bc.fa"), "LRBarcodeErr=10", "LRBarcodeMargin=1", "LRBarcodeWindow=64", "LRBarcodeBothEnds=1"]
    assert "LRDemuxOut=1" in read("full", ".config.txt").decode().splitlines()
    assert read("off", ".config.txt") == read("full", ".config.txt").replace(("LRBarcodes=%s\nLRDemuxOut=1\n" % (tmp_path / "bc.fa")).encode(), b"")
