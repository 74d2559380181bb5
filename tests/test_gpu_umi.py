"""The UMI read-out on the device (docs/umi.md; k_read_umi, talc_batch_umi, the scan and the combined intervals inside
talc_batch_create_clipped and talc_batch_create_split) against the contract in numpy (tests/umi_ref.py: never from a device
result).  Integers and bytes, tolerance 0.  Every case first asserts, from the reference alone, that its input reaches what
it is there for."""
import os
import subprocess

import numpy as np
import pytest

import chimera_ref as CR
import ends_ref as R
import parity_util as PU
import test_gpu_chimera as GC
import test_gpu_solidity as G
import umi_ref as U
from memcheck_util import guards_checked
from talc_amd import build as B
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ERR_INVALID, ERR_STATE = -1, -6
VNP = CR.VNP
SSP23 = CR.SSP[:23]                                   # the strand-switch primer up to where the UMI begins
P12 = "GATTACAGNCTA"
P64 = "ACVV" * 16
GGG = U.BARE + "GGG"                                  # anchored behind the UMI: what is left of the primer once a split has cut at it
SUB_PLACES = (1, 5, 9, 37, 40)                        # fixed letters of the anchored pattern, apart: k substitutions there cost exactly k

_ctx = []


def ctx():
    """A context of its own over the shared table of test_gpu_solidity's default set."""
    if not _ctx:
        c = G.gen_set("default")
        _ctx.append(T.Context(c.ttab, c.p, 0))
    return _ctx[0]


def device_rows(reads, pattern, pct, window=U.DEFAULT_WINDOW):
    c = ctx()
    c.set_umi(pattern, pct, window)
    try:
        b = c.batch(*R.batch(reads))
        try:
            return b.umi()
        finally:
            b.close()
    finally:
        c.set_umi()


def same_rows(got, want, what=""):
    assert got.dtype == U.DTYPE and T.UMI_DTYPE == U.DTYPE and len(got) == len(want), what
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def check(reads, what, pattern, pct, window=U.DEFAULT_WINDOW):
    want = U.rows(reads, pattern, pct, window)
    same_rows(device_rows(reads, pattern, pct, window), want, what)
    return want


def subs(pattern, copy, places):
    """`copy` with a base outside the pattern letter's set (N where the set is all four) at each of `places`."""
    s = list(copy)
    for at in places:
        s[at] = next((b for b in "ATCG" if b not in U.sets_of(pattern)[at]), "N")
    return "".join(s)


# ---------------------------------------------------------------- 1. one pattern: every stop, every single edit, every border
@pytest.mark.parametrize("level", [0, 4, 5])
def test_one_pattern_that_ends_at_every_stop_of_a_window(level):
    rng = np.random.default_rng(600 + level)
    pattern, pct, window, L = U.ANCHORED, 10, 192, 400
    m, k = len(pattern), 10 * len(pattern) // 100
    assert k == 4 and level in (0, k, k + 1)
    stops = list(range(m, window + 1))
    reads = [R.random_seq(rng, e - m) + subs(pattern, U.instance(rng, pattern), SUB_PLACES[:level]) + R.random_seq(rng, L - e) for e in stops]
    reads += [R.revcomp(r).decode() for r in reads]
    want = check(reads, "sweep, %d edits" % level, pattern, pct, window)
    n = len(stops)
    if level <= k:
        assert (want["end"][:n] == 1).all() and (want["end"][n:] == 2).all() and (want["err"] <= level).all() and (want["err"] == level).sum() >= 2 * n - 8
        assert (want["stop"][:n] == stops).sum() >= n - 4 and (want["stop"][n:] == stops).sum() >= n - 4 and (want["umi_len"] == 16).all()
        assert (want["umi"][:n] == want["umi"][n:]).all() and len(set(want["umi"].tolist())) >= n - 4
    else:
        assert (want["end"] == 0).sum() >= 2 * n - 8                     # one edit too many: chance hits at most


@pytest.mark.parametrize("pattern", [U.ANCHORED, U.BARE])
def test_a_single_insertion_deletion_and_substitution_at_every_position(pattern):
    rng = np.random.default_rng(len(pattern))
    m = len(pattern)
    reads, kinds = [], []
    for at in range(m):
        copy = U.instance(rng, pattern)
        for kind, edited in (("S", subs(pattern, copy, [at])), ("I", copy[:at] + "ACGT"[int(rng.integers(4))] + copy[at:]), ("It", copy[:at] + "T" + copy[at:]),
                             ("D", copy[:at] + copy[at + 1:])):
            s = "GGCC" + edited + "CAGTCAGGCA" + R.random_seq(rng, 100)
            reads += [s, R.revcomp(s).decode()]
            kinds += [kind, kind]
    want = check(reads, "single edits", pattern, 10)
    umis = [u.decode() for u in want["umi"]]
    assert (want["end"][0::2] == 1).all() and (want["end"][1::2] == 2).all() and (want["err"] <= 1).all() and (want["err"] == 1).sum() >= len(reads) - 24
    # (an insertion before the copy's first or behind its last letter costs nothing, nor does a T inside the bare pattern's outer TTT runs)
    assert sum("-" in u for u in umis) >= 2 * len(U.degenerate(pattern)) - 2     # a deleted degenerate letter leaves a gap
    assert (want["umi"][0::2] == want["umi"][1::2]).all() and len(set(want["start"][0::2].tolist())) >= 2 and len(set(want["stop"].tolist())) >= 3
    ties = set()
    for s in reads[0::2]:
        ties |= {t[2:] for t in U.steps_plain(s, pattern)}
    assert {(True, True, False, "D"), (True, False, True, "D"), (False, True, False, "U"), (False, False, True, "L")} <= ties   # the TT spacers' ties


@pytest.mark.parametrize("window,length", [(256, 600), (256, 250), (1024, 1100)])
def test_a_pattern_around_every_chunk_border(window, length):
    rng = np.random.default_rng(window + length)
    pattern, pct = U.ANCHORED, 10
    m, k = len(pattern), 4
    n = min(window, length)
    chunk = -(-n // 64)
    stops = sorted({b + d for b in range(chunk, n, chunk) for d in range(-(m + k + 2), m + k + 3) if m <= b + d <= n})
    assert stops == list(range(m, n + 1))
    reads = []
    for e in stops:
        for edits in (0, k):
            copy = subs(pattern, U.instance(rng, pattern), rng.choice(m - 1, size=edits, replace=False).tolist())
            s = R.random_seq(rng, length)
            s = s[:e - m] + copy + s[e:]
            reads.append(R.revcomp(s).decode() if e % 3 == 1 else s)
    want = check(reads, "chunk borders", pattern, pct, window)
    assert (want["end"] > 0).all() and (want["stop"][0::2] == stops).all() and (want["err"][1::2] == k).sum() > len(stops) // 2
    assert (want["end"] == 1).sum() > len(stops) and (want["end"] == 2).sum() > len(stops) // 2


# ---------------------------------------------------------------- 2. sizes
@pytest.mark.parametrize("pattern,pct", [(P12, 0), (P12, 30), (P64, 0), (P64, 30)])
def test_the_shortest_and_the_longest_pattern_at_both_error_bounds(pattern, pct):
    m = len(pattern)
    rng = np.random.default_rng(3000 + m + pct)
    k = pct * m // 100
    assert k == {(12, 0): 0, (12, 30): 3, (64, 0): 0, (64, 30): 19}[(m, pct)]
    reads, level = [], []
    for n_edits in sorted({0, k, k + 1, min(k + 8, m - 2)}):
        for junk in (0, 5, 64, 150):
            for _ in range(3):
                places = rng.choice(np.arange(1, m - 1), size=n_edits, replace=False).tolist()
                s = R.random_seq(rng, junk) + subs(pattern, U.instance(rng, pattern), places) + R.random_seq(rng, 400)
                reads += [s, R.revcomp(s).decode()]
                level += [n_edits, n_edits]
                if n_edits:
                    reads.append(R.random_seq(rng, junk) + R.mutate(rng, U.instance(rng, pattern), n_edits, "SID") + R.random_seq(rng, 400))
                    level.append(n_edits)
    want = check(reads, "pattern of %d at %d per cent" % (m, pct), pattern, pct)
    level = np.array(level)
    assert (want["end"] > 0)[level <= k].sum() >= (level <= k).sum() - 2 and max(k - 1, 0) <= int(want["err"].max()) <= k
    assert (want["umi_len"][want["end"] > 0] == len(U.degenerate(pattern))).all() and (want["end"] == 1).any() and (want["end"] == 2).any()
    if pct == 0:
        assert (want["end"] == 0)[level > 1].sum() >= (level > 1).sum() - 2
    if m == 64:
        assert int(want["stop"].max()) >= 150 + 60


@pytest.mark.parametrize("window", [32, 256, 4096])
def test_reads_around_the_window(window):
    rng = np.random.default_rng(window)
    pattern, m = U.BARE, 28
    reads = []
    for L in (0, 1, m - 1, m, window - 1, window, 2 * window - 1):
        reads.append(R.random_seq(rng, L))
        copy = U.instance(rng, pattern)
        reads.append(copy[:L] if L < m else copy + R.random_seq(rng, L - m))
        if L >= m:
            reads += [R.random_seq(rng, L - m) + R.revcomp(copy).decode(), R.random_seq(rng, L - m) + copy,
                      R.random_seq(rng, (L - m) // 2) + copy + R.random_seq(rng, L - m - (L - m) // 2)]
    want = check(reads, "window %d" % window, pattern, 10, window)
    assert [len(r) for r in reads[:6]] == [0, 0, 1, 1, 27, 27] and want["end"][:6].tolist() == [0, 0, 0, 0, 0, 1] and want["kept_len"][:6].tolist() == [0, 0, 1, 1, 27, 0]
    assert (want[5]["err"], want[5]["stop"]) == (1, 27)                  # a copy cut off by the read's own end pays for the missing letter
    assert (want["end"] == 1).sum() >= 4 and (want["end"] == 2).sum() >= 4 and (want["stop"] == window).any() and (want["stop"] == 28).any()
    # a copy that ends just inside and just outside the window
    edge = [R.random_seq(rng, window - m) + U.instance(rng, pattern) + R.random_seq(rng, 4200), R.random_seq(rng, window - m + 8) + U.instance(rng, pattern) + R.random_seq(rng, 4200)]
    want = check(edge, "window's edge", pattern, 10, window)
    assert want["end"].tolist() == [1, 0] and want[0]["stop"] == window and want[0]["start"] == window - m


def test_one_read_of_140_kb():
    rng = np.random.default_rng(140)
    inst = U.instance(rng, U.ANCHORED)
    reads = [R.random_seq(rng, 5) + inst + R.random_seq(rng, 140_000) + "ACG", R.random_seq(rng, 140_000) + R.revcomp(inst).decode() + "ACG", R.random_seq(rng, 140_000)]
    want = check(reads, "140 kb", U.ANCHORED, 10)
    assert want["end"].tolist() == [1, 2, 0] and want["stop"].tolist() == [47, 45, 0] and want["start"].tolist() == [5, 3, 0]
    assert want["kept_len"].tolist() == [len(reads[0]) - 47, len(reads[1]) - 45, 140_000] and want["kept_start"].tolist() == [47, 0, 0]


@pytest.mark.parametrize("count,window,longest", [(2000, 64, 300), (250, 256, 900)])
def test_random_reads_with_planted_umis_in_about_half(count, window, longest):
    rng = np.random.default_rng(count)
    reads = []
    for _ in range(count):
        where = int(rng.integers(0, 4)) if rng.integers(2) else 0
        reads.append(U.plant(rng, R.random_seq(rng, int(rng.integers(0, longest))), U.BARE, where, 2))
    want = check(reads, "random reads, window %d" % window, U.BARE, 10, window)
    heads, tails = (want["end"] == 1).sum(), (want["end"] == 2).sum()
    assert heads >= 20 and tails >= 20 and (want["other_err"] != 255).sum() >= 20 and (want["end"] == 0).sum() >= 20, (heads, tails)
    assert (want["err"] > 0).sum() >= 20 and sum(b"-" in u for u in want["umi"].tolist()) >= 3


# ---------------------------------------------------------------- 3. clipped and split batches
ENDS_KW = dict(adapters=[SSP23, VNP], max_error_pct=20, poly_min=12, window=512)
PCT, MIN_PIECE = 10, 100
UMI = (GGG, 10, 256)

_dressed = {}


def dress(rng, body):
    """primer . UMI . GGG . transcript . poly-A . the other primer's reverse complement, or the reverse complement of it all."""
    s = SSP23 + R.mutate(rng, U.instance(rng, U.BARE), int(rng.integers(0, 3)), "SID") + "GGG" + body + "A" * int(rng.integers(15, 40)) + R.revcomp(VNP).decode()
    return s if rng.integers(2) else R.revcomp(s).decode()


def joined(rng, one, every):
    reads, i = [], 0
    while i < len(one):
        if i % every == every - 1 and i + 1 < len(one):
            reads.append(one[i] + CR.joint(rng) + one[i + 1])
            i += 2
        else:
            reads.append(one[i])
            i += 1
    return reads


def host_cut(reads, ends_on, split):
    """What the reference says of the reads: (the reads or pieces as they came, their end rows or None, their UMI rows, the
    reads cut at the rows' intervals, the pieces or None)."""
    pieces = None
    if split:
        hits, _ = CR.hits(reads, ENDS_KW["adapters"], PCT)
        pieces = CR.pieces([len(x) for x in reads], hits, MIN_PIECE)[0]
        reads = [x.decode() for x in CR.cut(reads, pieces)]
    erows = R.rows(reads, **ENDS_KW) if ends_on else None
    urows = U.rows(reads, *UMI, claims=U.claims_of(erows) if ends_on else None)
    return reads, erows, urows, [x.decode() for x in U.clip(reads, urows)], pieces


MODES = (("clipped", dict(clip=True), True), ("clipped, ends off", dict(clip=True), False), ("split and clipped", dict(split=True, clip=True), True))


def dressed():
    """200 generator reads dressed with primer, UMI and poly-A, in either orientation; every tenth joined to the next; the
    reference's rows; and what plain batches of the reads cut on the host give with the UMI setting off.  (A split needs the
    adapters, so there is no split with the ends off.)"""
    if not _dressed:
        c = G.gen_set("default")
        rng = np.random.default_rng(8)
        reads = joined(rng, [dress(rng, R.as_bytes(body).decode()) for body in c.reads[:200]], 10)
        off = T.Context(c.ttab, c.p, 0)
        want, base = {}, {}
        try:
            for what, kw, ends_on in MODES:
                want[what] = host_cut(reads, ends_on, kw.get("split", False))
                base[what] = GC.everything_of(off, *PU.pack_reads(want[what][3]))
            off.set_ends(**ENDS_KW)
            off.set_chimera(True, PCT, MIN_PIECE)
            base["split"] = GC.everything_of(off, *R.batch(reads), split=True)
            base["ends"] = GC.everything_of(off, *R.batch(reads), clip=True, ends=True)["rows"]
        finally:
            off.close()
        want["split"] = host_cut(reads, False, True)
        _dressed.update(c=c, reads=reads, want=want, base=base)
    return _dressed


def with_umi(r):
    """The batches with the UMI setting on: {what: (outputs, UMI rows)}."""
    on = T.Context(r["c"].ttab, r["c"].p, 0)
    got = {}
    try:
        on.set_umi(*UMI)
        for what, kw, ends_on in MODES + (("split", dict(split=True), True),):
            on.set_ends(**ENDS_KW) if ends_on else on.set_ends()
            on.set_chimera(True, PCT, MIN_PIECE) if ends_on else on.set_chimera(False)
            outs = GC.everything_of(on, *R.batch(r["reads"]), ends=ends_on, **kw)
            b = on.batch(*R.batch(r["reads"]), **kw)
            try:
                rows = b.umi()
                assert on.umi_timing() == 0.0                            # the rows came with the batch: nothing ran again
            finally:
                b.close()
            got[what] = (outs, rows)
        return got
    finally:
        on.close()


def check_batches(r, got, prefix=""):
    for what, (outs, rows) in got.items():
        came, erows, urows, cut, pieces = r["want"][what]
        same_rows(rows, urows, prefix + what)
        if what != "split":
            GC.same_batches(outs, r["base"][what], prefix + what)
        else:                                                            # nothing is cut: the batch of a context without the setting
            GC.same_batches(outs, r["base"]["split"], prefix + what)
        if erows is not None and what != "split":
            assert (outs["rows"] == erows).all(), what                   # the end rows keep what k_read_ends wrote
        if pieces is not None:
            assert (outs["pieces"] == pieces).all()
    assert (got["clipped"][0]["rows"] == r["base"]["ends"]).all()        # ... those of a context without the UMI setting


def test_clipped_and_split_batches_cut_at_the_combined_intervals():
    r = dressed()
    n = len(r["reads"])
    for what, _, ends_on in MODES:
        came, erows, urows, cut, pieces = r["want"][what]
        assert (urows["end"] == 1).sum() >= 50 and (urows["end"] == 2).sum() >= 50 and (urows["err"] > 0).sum() >= 40, what
        assert sum(len(a) for a in cut) < sum(len(a) for a in came) - 30 * len(came)
        if ends_on:                                                      # the UMI's claim is the larger at its end, the end rule's at the other
            own = (urows["kept_start"] > erows["kept_start"]).sum() + (urows["kept_len"] < erows["kept_len"]).sum()
            assert own >= 150 and (urows["kept_len"] + urows["stop"] < [len(x) for x in came]).sum() >= 150
    assert n == 181 and len(r["want"]["split and clipped"][0]) > n + 10 and (r["want"]["split"][2]["end"] > 0).sum() >= 150
    check_batches(r, with_umi(r))


@pytest.mark.parametrize("byte", [0xA5, 0xFF])
def test_clipped_and_split_batches_on_poisoned_memory_between_red_zones(byte):
    r = dressed()
    with guards_checked():
        with T.poisoned(byte):
            got = with_umi(r)
            plain = device_rows(r["reads"], *UMI)
    same_rows(plain, U.rows(r["reads"], *UMI), "poisoned, plain")
    check_batches(r, got, "poisoned, ")


# ---------------------------------------------------------------- 4. no behaviour change, state errors, generations
def test_a_context_that_never_set_the_option_and_one_that_switched_it_off_again():
    c = G.gen_set("default")
    reads = c.reads[:80]
    never, other = T.Context(c.ttab, c.p, 0), T.Context(c.ttab, c.p, 0)
    try:
        other.set_umi(*UMI)
        other.set_umi()
        a = GC.everything_of(never, *PU.pack_reads(reads))
        b = GC.everything_of(other, *PU.pack_reads(reads))
        assert a["per"] == b["per"] and a["work"] == b["work"] and a["work"][1] > 0 and a["cov"] == b["cov"]
        assert [p[0].decode() for p in a["per"]] == c.run["records"][:80] and [p[1] for p in a["per"]] == c.run["st"][:80].tolist()
        assert never.umi_timing() == 0.0 and other.umi_timing() == 0.0
        for x in (never, other):                                         # ... and a clipped batch is refused as before
            with pytest.raises(T.TalcError, match="the end clean-up is off"):
                x.batch(*PU.pack_reads(reads), clip=True)
    finally:
        never.close()
        other.close()


def test_the_state_errors_and_the_refused_settings():
    c = G.gen_set("default")
    L = T.lib()
    one, other = T.Context(c.ttab, c.p, 0), T.Context(c.ttab, c.p, 0)
    rng = np.random.default_rng(9)
    inst = U.instance(rng, U.ANCHORED)
    reads = [inst + R.random_seq(rng, 200), R.random_seq(rng, 200) + R.revcomp(inst).decode(), R.random_seq(rng, 200)]
    want = U.rows(reads, U.ANCHORED, 10)
    assert want["end"].tolist() == [1, 2, 0]
    bases, offs = R.batch(reads)
    b = one.batch(bases, offs)
    rows = np.zeros(3, U.DTYPE)
    try:
        assert L.talc_batch_umi(one._h, b._h) == ERR_STATE and b"off" in L.talc_last_error()
        assert L.talc_batch_fetch_umi(one._h, b._h, rows.ctypes.data) == ERR_STATE and b"scan" in L.talc_last_error()
        one.set_ends(adapters=[SSP23])
        cb = one.batch(bases, offs, clip=True)                           # made while the read-out was off: it never gets rows
        one.set_umi(U.ANCHORED, 10)
        try:
            assert L.talc_batch_umi(one._h, cb._h) == ERR_STATE and b"clipped" in L.talc_last_error()
            assert L.talc_batch_fetch_umi(one._h, cb._h, rows.ctypes.data) == ERR_STATE
        finally:
            cb.close()
        one.set_ends()
        cb = one.batch(bases, offs, clip=True)                           # the UMI alone clips; there are no end rows then
        try:
            assert cb.n_bases == int(want["kept_len"].sum()) and (cb.umi() == want).all()
            assert L.talc_batch_fetch_ends(one._h, cb._h, None) == ERR_STATE
        finally:
            cb.close()
        for kw, word in ((dict(max_error_pct=31), "max_error_pct=31"), (dict(window=5000), "window=5000"), (dict(pattern="ACGTACGTACGTA"), "0 degenerate letters"),
                         (dict(pattern=U.BARE[:11]), "11 letters"), (dict(pattern=U.BARE + "X"), "letter 29 is not one of")):
            with pytest.raises(T.TalcError, match=word):
                one.set_umi(**{**dict(pattern=U.ANCHORED, max_error_pct=10), **kw})
        same_rows(b.umi(), want, "a refused setting changes nothing")
        assert one.umi_timing() > 0.0
        assert L.talc_batch_umi(other._h, b._h) == ERR_INVALID             # another context's batch
        one.set_umi()
        assert L.talc_batch_umi(one._h, b._h) == ERR_STATE
        assert L.talc_batch_fetch_umi(one._h, b._h, rows.ctypes.data) == 0 and (rows == want).all()   # the rows of the last scan stay
    finally:
        b.close()
        one.close()
        other.close()


def test_a_new_setting_scans_again_and_the_same_setting_does_not():
    c = ctx()
    rng = np.random.default_rng(10)
    reads = [subs(U.ANCHORED, U.instance(rng, U.ANCHORED), SUB_PLACES[:3]) + R.random_seq(rng, 300) for _ in range(50)]
    loose, tight = U.rows(reads, U.ANCHORED, 10), U.rows(reads, U.ANCHORED, 5)
    assert (loose["end"] == 1).all() and (loose["err"] == 3).all() and (tight["end"] == 0).all()
    b = c.batch(*R.batch(reads))
    try:
        c.set_umi(U.ANCHORED, 10)
        same_rows(b.umi(), loose, "first setting")
        assert c.umi_timing() > 0.0
        same_rows(b.umi(), loose, "the same setting")
        assert c.umi_timing() == 0.0                                     # nothing was launched
        c.set_umi(U.ANCHORED, 5)
        same_rows(b.umi(), tight, "second setting")
        assert c.umi_timing() > 0.0
    finally:
        b.close()
        c.set_umi()


# ---------------------------------------------------------------- 5. the command line
def test_cli_umi_with_clip_and_split_in_small_batches(tmp_path):
    c = G.gen_set("default")
    rng = np.random.default_rng(34)
    n = 60
    one = [R.as_bytes(body).decode() if i % 7 == 3 else dress(rng, R.as_bytes(body).decode()) for i, body in enumerate(c.reads[:n])]
    reads = joined(rng, one, 5)
    names = ["read%d/x" % i for i in range(len(reads))]
    # with the adapters: split, every piece clipped by both claims; without: the UMI alone clips the reads as they came
    hits, _ = CR.hits(reads, [SSP23, VNP], PCT)
    pieces = CR.pieces([len(x) for x in reads], hits, MIN_PIECE)[0]
    cut = [x.decode() for x in CR.cut(reads, pieces)]
    piece_names = CR.piece_names(names, pieces)
    full_rows = U.rows(cut, *UMI, claims=U.claims_of(R.rows(cut, **ENDS_KW)))
    alone_rows = U.rows(reads, GGG, 15, 128)
    assert len(pieces) > len(reads) + 5 and (full_rows["end"] == 1).sum() >= 10 and (full_rows["end"] == 2).sum() >= 10 and (full_rows["end"] == 0).sum() >= 5
    assert (alone_rows["end"] > 0).sum() >= 30 and (alone_rows["other_err"] != 255).sum() >= 1 and (full_rows["err"] > 0).sum() >= 5
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    fasta = lambda nms, seqs: "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(nms, seqs))
    (tmp_path / "dressed.fa").write_text(fasta(names, reads))
    (tmp_path / "host_full.fa").write_text(fasta(piece_names, [x.decode() for x in U.clip(cut, full_rows)]))
    (tmp_path / "host_alone.fa").write_text(fasta(names, [x.decode() for x in U.clip(reads, alone_rows)]))
    common = ["-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7", "-o", "o"]
    lr = ["--LRAdapter", SSP23, "--LRAdapter", VNP, "--LRPolyA", "12", "--LRSplit", "--LRClip"]
    umi = ["--LRUmi", GGG]
    alone = ["--LRUmi", GGG.lower(), "--LRUmiErr", "15", "--LRUmiWindow", "128", "--LRClip"]
    runs = {}
    for d, args, env in (("full", ["dressed.fa"] + lr + umi, None), ("full2", ["dressed.fa"] + lr + umi + ["--gpus", "2"], dict(os.environ, TALC_FAKE_GPUS="2")),
                         ("host_full", ["host_full.fa"], None), ("alone", ["dressed.fa"] + alone, None), ("host_alone", ["host_alone.fa"], None),
                         ("off", ["dressed.fa"] + lr, None)):
        (tmp_path / d).mkdir()
        runs[d] = subprocess.run([TALC, str(tmp_path / args[0])] + args[1:] + common, cwd=tmp_path / d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert runs[d].returncode == 0, (d, runs[d].stderr.decode())
    read = lambda d, ext: (tmp_path / d / ("o" + ext)).read_bytes() if (tmp_path / d / ("o" + ext)).exists() else None
    for ext in (".fa", ".log"):
        assert read("full", ext) == read("host_full", ext), ext             # the reads cut beforehand on the host, under their names
        assert read("full2", ext) == read("full", ext), ext
        assert read("alone", ext) == read("host_alone", ext), ext
    assert read("full", ".fa") != read("off", ".fa") and read("full", ".chimera_pieces.tsv") == read("off", ".chimera_pieces.tsv")
    assert read("full", ".ends.tsv") == read("off", ".ends.tsv") and read("alone", ".ends.tsv") is None    # the end rows keep what the end scan wrote

    def tsv(nms, seqs, rows):
        out = ["read_name\tlength\tend\terr\tother_err\tstart\tstop\tumi\tkept_start\tkept_len"]
        for nm, s, w in zip(nms, seqs, rows):
            out.append("\t".join([nm, str(len(s)), str(int(w["end"])), str(int(w["err"])), "-" if w["other_err"] == 255 else str(int(w["other_err"])), str(int(w["start"])),
                                  str(int(w["stop"])), w["umi"].decode() if w["end"] else "-", str(int(w["kept_start"])), str(int(w["kept_len"]))]))
        return out

    def line(rows):
        both = rows["other_err"] != 255
        return "[TALC]: umi: %d reads, %d at the head, %d at the tail, %d at both ends, %d without" % (
            len(rows), int(((rows["end"] == 1) & ~both).sum()), int(((rows["end"] == 2) & ~both).sum()), int(both.sum()), int((rows["end"] == 0).sum()))

    for d, nms, seqs, rows in (("full", piece_names, cut, full_rows), ("full2", piece_names, cut, full_rows), ("alone", names, reads, alone_rows)):
        assert read(d, ".umi.tsv").decode().splitlines() == tsv(nms, seqs, rows), d
        assert runs[d].stdout.decode().splitlines().count(line(rows)) == 1, (d, line(rows))
    assert b"umi:" not in runs["off"].stdout and read("off", ".umi.tsv") is None and read("host_full", ".umi.tsv") is None
    assert b"correcting on 2 GPU(s)" in runs["full2"].stdout
    cfg = read("alone", ".config.txt").decode().splitlines()
    assert [x for x in cfg if x.startswith("LR")] == ["LRClip=1", "LRUmi=" + GGG.lower(), "LRUmiErr=15", "LRUmiWindow=128"]
    assert read("off", ".config.txt") == read("full", ".config.txt").replace(("LRUmi=%s\n" % GGG).encode(), b"")
