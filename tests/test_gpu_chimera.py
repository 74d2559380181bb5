"""The chimera scan and the split batch on the device (docs/chimeras.md; k_read_chimera, k_gather,
talc_batch_create_split) against the contract in numpy (tests/chimera_ref.py: never from a device result), and a split batch
against a plain batch of the pieces cut on the host.  Integers and bytes, tolerance 0.  Every case first asserts, from the
reference alone, that its input reaches what it is there for."""
import os
import subprocess

import numpy as np
import pytest

import chimera_ref as CR
import ends_ref as R
import parity_util as PU
import test_gpu_solidity as G
from memcheck_util import fetch_all, guards_checked, per_read
from talc_amd import build as B
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
SSP, VNP = CR.SSP, CR.VNP
P24 = "GATCCGTAGCTTGACCATGCAGTC"                                         # 24 letters: k_a = 4 at 20 per cent
SUB_PLACES = (3, 8, 12, 17, 21)                                          # apart: k substitutions there cost exactly k

_ctx = {}


def ctx_of(name="default"):
    """A context of its own over the shared table of one of test_gpu_solidity's sets."""
    if name not in _ctx:
        c = G.gen_set(name)
        _ctx[name] = (c, T.Context(c.ttab, c.p, 0))
    return _ctx[name]


def same_hits(got, want, what=""):
    assert got.dtype == CR.HIT_DTYPE and T.CHIMERA_DTYPE == CR.HIT_DTYPE
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def device_hits(reads, adapters, pct):
    _, ctx = ctx_of()
    ctx.set_ends(adapters=adapters)
    ctx.set_chimera(True, pct)
    try:
        b = ctx.batch(*R.batch(reads))
        try:
            return b.chimera()
        finally:
            b.close()
    finally:
        ctx.set_chimera(False)
        ctx.set_ends()


def check(reads, what, adapters, pct):
    want, woff = CR.hits(reads, adapters, pct)
    got, goff = device_hits(reads, adapters, pct)
    same_hits(got, want, what)
    assert (goff == woff).all()
    return want


def subs(seq, places):
    s = list(seq)
    for at in places:
        s[at] = "ACGT"[("ACGT".index(s[at]) + 1) % 4]
    return "".join(s)


def planted(rng, length, ends, copy):
    """A random read of `length` bytes with `copy` written over it so that it ends at every e of `ends` (whole copies only)."""
    s = list(R.random_seq(rng, length))
    for e in ends:
        if len(copy) <= e <= length:
            s[e - len(copy):e] = copy
    return "".join(s)


# ---------------------------------------------------------------- 1. a primer ending at every column
@pytest.mark.parametrize("level", [0, 4, 5])
def test_a_primer_that_ends_at_every_column_of_a_read(level):
    rng = np.random.default_rng(300 + level)
    ka = 20 * 24 // 100
    assert ka == 4 and level in (0, ka, ka + 1)
    copy = subs(P24, SUB_PLACES[:level])
    L = 700
    ends = list(range(1, L + 1))
    reads = []
    for e in ends:                                           # (a copy cut off by the read's start where e < 24)
        part = copy[max(0, 24 - e):]
        reads.append(R.random_seq(rng, e - len(part)) + part + R.random_seq(rng, L - e))
    reads += [R.revcomp(r).decode() for r in reads]
    assert all(len(r) == L for r in reads)
    want = check(reads, "sweep, %d edits" % level, [P24], 20)
    n = len(ends)
    for e in range(24, L + 1):                               # every whole copy: found where it lies, at its cost, on its strand
        for read, strand, at in ((e - 1, 0, e), (n + e - 1, 1, L - e + 24)):
            mine = want[(want["read"] == read) & (want["end"] == at) & (want["strand"] == strand)]
            if level <= ka:
                assert len(mine) == 1 and mine[0]["start"] == at - 24 and mine[0]["err"] == level, (e, strand, mine)
            else:
                assert len(mine) == 0
    if level <= ka:
        assert len(want) >= 2 * (L - 23)
    else:
        assert len(want) < 40                                # one edit too many: chance hits at most


# ---------------------------------------------------------------- 2. tile and chunk borders of long reads
@pytest.mark.parametrize("length,adapters,deltas", [(20_000, [P24], range(-42, 43, 2)), (20_000, [P24, SSP, VNP, P24[::-1]], range(-48, 49, 12)),
                                                    (140_000, [P24], range(-40, 41, 8))])
def test_primers_around_every_chunk_and_tile_border_of_a_long_read(length, adapters, deltas):
    rng = np.random.default_rng(length + len(adapters))
    lanes, chunk, tile = T.chimera_geometry(length, 2 * len(adapters))
    assert chunk == T.CHIMERA_CHUNK_MAX and tile == lanes * chunk and length > 2 * tile      # several tiles, the last one partial
    assert length % tile != 0 and length % chunk != 0
    borders = list(range(chunk, length, chunk))
    assert any(b % tile == 0 for b in borders)
    copy = subs(P24, SUB_PLACES[:2])
    reads = []
    for d in deltas:
        ends = [b + d for b in borders]
        reads.append(planted(rng, length, ends, copy if d % 2 else P24))
        reads.append(R.revcomp(planted(rng, length, ends, copy)).decode())
    want = check(reads, "borders of %d" % length, adapters, 20)
    per_read_hits = np.bincount(want["read"], minlength=len(reads))
    assert (per_read_hits >= len(borders) - 1).all()         # one per border (the last may not fit into the read)
    assert set(np.unique(want["strand"]).tolist()) == {0, 1}
    on_border = np.isin(want["end"], borders) | np.isin(want["start"], borders)
    assert on_border.sum() >= len(borders)                   # hits that end and hits that start exactly on a border


# ---------------------------------------------------------------- 3. edits of each kind, lengths, bounds
def test_edits_of_each_kind_lower_case_and_n():
    rng = np.random.default_rng(17)
    reads, kinds = [], []
    for kind in ("S", "I", "D", "N"):
        for n_edits in (1, 2, 4, 5):
            for junk in (0, 1, 7, 333):
                reads.append(R.random_seq(rng, junk) + R.mutate(rng, P24, n_edits, kind) + R.random_seq(rng, 90 + junk))
                kinds.append(kind)
    for junk in (0, 13, 400):
        reads.append((R.random_seq(rng, junk) + P24 + R.random_seq(rng, 90)).lower())
        reads.append(R.random_seq(rng, junk) + R.mutate(rng, P24, 2, "S").lower() + "N" * 30 + P24)
        kinds += ["lower", "lower"]
    reads += [R.revcomp(r).decode() for r in reads]
    want = check(reads, "edits", [P24], 20)
    n = len(kinds)
    for kind in ("S", "I", "D", "N", "lower"):
        mine = [i for i, k in enumerate(kinds) if k == kind]
        found = [i for i in mine if (want["read"] == i).any()]
        assert len(found) >= 4 and (kind == "lower" or len(found) < len(mine)), (kind, len(found))      # accepted and rejected ones
        assert max(int(want["err"][want["read"] == i].max()) for i in found) > 0
    assert (want["strand"][want["read"] < n] == 0).all() and (want["strand"][want["read"] >= n] == 1).all()
    lens = (want["end"] - want["start"]).astype(int)
    assert lens.min() < 24 < lens.max()                                                                # deletions and insertions move the start


@pytest.mark.parametrize("m,pct", [(12, 0), (12, 30), (64, 0), (64, 30)])
def test_the_shortest_and_the_longest_adapter_at_both_error_bounds(m, pct):
    rng = np.random.default_rng(2000 + m + pct)
    ad = R.random_seq(rng, m)
    k = pct * m // 100
    assert k == {(12, 0): 0, (12, 30): 3, (64, 0): 0, (64, 30): 19}[(m, pct)]
    reads, level = [], []
    for n_edits in sorted({0, k, k + 1, min(k + 8, m - 2)}):
        for junk in (0, 5, 64, 129, 1400):
            places = rng.choice(np.arange(1, m - 1), size=n_edits, replace=False).tolist()
            reads.append(R.random_seq(rng, junk) + subs(ad, places) + R.random_seq(rng, 120))
            level.append(n_edits)
            if n_edits:
                reads.append(R.random_seq(rng, junk) + R.mutate(rng, ad, n_edits, "SID") + R.random_seq(rng, 120))
                level.append(n_edits)
    reads += [R.revcomp(r).decode() for r in reads]
    want = check(reads, "adapter of %d at %d per cent" % (m, pct), [ad], pct)
    n = len(level)
    for i, lv in enumerate(level):
        if lv <= k:
            assert ((want["read"] == i) & (want["strand"] == 0)).any() and ((want["read"] == n + i) & (want["strand"] == 1)).any()
    assert int(want["err"].max()) == k


def test_four_adapters_tandem_copies_and_a_palindrome():
    rng = np.random.default_rng(23)
    ads = [SSP, VNP, P24, R.random_seq(rng, 40)]
    mix = R.random_seq(rng, 50).join([SSP, R.revcomp(VNP).decode(), P24, ads[3], R.revcomp(ads[3]).decode(), R.mutate(rng, SSP, 2), VNP])
    tandem = R.random_seq(rng, 31) + SSP * 5 + R.random_seq(rng, 40)
    joint = "A" * 40 + R.revcomp(VNP).decode() + SSP
    want = check([mix, tandem, joint, R.revcomp(mix).decode(), ""], "four adapters", ads, 10)
    assert sorted(set(want["adapter"][want["read"] == 0].tolist())) == [1, 2, 3, 4]
    t = want[(want["read"] == 1) & (want["adapter"] == 1)]
    assert len(t) == 5 and (t["end"] - t["start"] == 26).all() and (np.diff(t["end"]) == 26).all()      # copies laid end to end: one hit each
    j = want[want["read"] == 2]
    assert len(j) == 2 and j[0]["end"] == j[1]["start"] == 62 and j["strand"].tolist() == [1, 0]       # two abutting hits
    # a sequence equal to its own reverse complement: both strands hit at one place
    half = R.random_seq(rng, 12)
    pal = half + R.revcomp(half).decode()
    assert R.revcomp(pal).decode() == pal
    read = R.random_seq(rng, 300) + pal + R.random_seq(rng, 300)
    want = check([read], "palindrome", [pal], 10)
    at = want[want["end"] == 324]
    assert at["strand"].tolist() == [0, 1] and (at["start"] == 300).all()


def test_short_reads_and_the_ends_of_a_read():
    rng = np.random.default_rng(29)
    reads = ["", "A", P24[:23], P24, P24.lower(), P24 + R.random_seq(rng, 60), R.random_seq(rng, 60) + P24, P24[:11], "N" * 100,
             P24[:12] + "N" + P24[12:], R.random_seq(rng, T.CHIMERA_CHUNK_MIN * 32 - 1) + P24, R.random_seq(rng, T.CHIMERA_CHUNK_MIN * 32 + 1) + P24]
    want = check(reads, "short reads", [P24], 20)
    whole = want[want["read"] == 3]
    assert len(whole) == 1 and whole[0]["start"] == 0 and whole[0]["end"] == 24 and whole[0]["err"] == 0      # a read that is one primer
    assert (want["read"] == 2).sum() == 1 and want[want["read"] == 2][0]["err"] == 1                           # m - 1 letters: one edit
    assert (want["read"] == 5).any() and want[want["read"] == 5][0]["start"] == 0                              # a hit at start 0
    assert want[want["read"] == 6][-1]["end"] == 84                                                            # ... and at end L
    assert not (want["read"] == 8).any() and want[want["read"] == 9][0]["err"] == 1


# ---------------------------------------------------------------- 4. many hits, and none
RANDOM12 = "ACGTTGCAAGTC"


def test_the_random_12_letter_setting():
    rng = np.random.default_rng(31)
    reads = [R.random_seq(rng, int(n)) for n in rng.integers(0, 3000, 200).tolist()]
    want = check(reads, "12 letters at 30 per cent", [RANDOM12], 30)
    assert len(want) > 2 * sum(len(r) for r in reads) // 1000                      # hits in bulk, on both strands
    assert (want["strand"] == 0).sum() > 100 and (want["strand"] == 1).sum() > 100
    lens = np.array([len(r) for r in reads])
    pieces, off, dropped, _ = CR.pieces(lens.tolist(), want, 100)
    assert dropped > 100 and (np.diff(off.astype(np.int64)) == 0).any()            # overlapping hits, dropped pieces, reads that keep none


def test_more_hits_than_the_first_buffer_holds():
    rng = np.random.default_rng(37)
    ordinary = lambda: R.random_seq(rng, 200) + SSP + R.random_seq(rng, 200)          # one primer each
    reads = [ordinary() for _ in range(25)] + [SSP * 1100] + [ordinary() for _ in range(25)]
    want, _ = CR.hits(reads, [SSP], 10)
    first = 1024 + 2 * len(reads)
    assert len(want) > first and (want["read"] == 25).sum() >= 1100                # the reference alone: the second scan must run
    got, off = device_hits(reads, [SSP], 10)
    same_hits(got, want, "tandem read")
    assert int(off[26] - off[25]) == int((want["read"] == 25).sum()) and len(got) > first


def test_random_reads_with_the_real_primers():
    rng = np.random.default_rng(2)
    reads = [R.random_seq(rng, int(n)) for n in rng.integers(30, 1400, 2000).tolist()]
    check(reads, "random reads", [SSP, VNP], 10)                                   # whatever the reference finds


# ---------------------------------------------------------------- 5. a split batch against a plain batch of the pieces
ENDS_KW = dict(adapters=[SSP, VNP], max_error_pct=20, poly_min=12, window=512)
PCT, MIN_PIECE = 10, 100


def everything_of(ctx, bases, offs, clip=False, split=False, ends=False):
    ctx.record_map(True)
    b = ctx.batch(bases, offs, clip=clip, split=split)
    try:
        n = b.n_reads
        b.coverage()
        cov = [x.tobytes() for x in b.fetch_coverage()]
        b.structure()
        struct = {k: v.tobytes() for k, v in b.fetch_structure().items()}
        rc = b.correct()
        t = ctx.timing()
        work = (rc, t.n_trail_steps, t.n_dp_cells, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)
        per = per_read(fetch_all(b), n)
        r = dict(cov=cov, struct=struct, work=work, per=per, n=n, n_bases=b.n_bases)
        if ends:
            r["rows"] = b.ends()
        if split:
            r["hits"], r["hit_off"] = b.chimera()
            r["pieces"], r["piece_off"] = b.split_pieces()
        r["strand"] = b.strand() if ctx._auto else None
        return r
    finally:
        b.close()
        ctx.record_map(False)


_equiv = {}


def equivalence(name):
    if name not in _equiv:
        c, plain = ctx_of(name)
        reads = [x.decode() for x in CR.dress(np.random.default_rng(5), c.reads[:200])]
        hits, hit_off = CR.hits(reads, ENDS_KW["adapters"], PCT)
        pieces, piece_off, dropped, _ = CR.pieces([len(x) for x in reads], hits, MIN_PIECE)
        cut = [x.decode() for x in CR.cut(reads, pieces)]
        rows = R.rows(cut, **ENDS_KW)
        clipped = [x.decode() for x in R.clip(cut, rows)]
        rev, auto = T.Context(c.ttab, T.default_params(k=c.k, reverse=1), 0), T.Context(c.ttab, c.p, 0)
        auto.auto_strand()
        r = dict(c=c, reads=reads, hits=hits, hit_off=hit_off, pieces=pieces, piece_off=piece_off, cut=cut, rows=rows, clipped=clipped, dropped=dropped)
        try:
            for mode, ctx in (("plain", plain), ("rev", rev), ("auto", auto)):
                ctx.set_ends(**ENDS_KW)
                ctx.set_chimera(True, PCT, MIN_PIECE)
                r[mode] = (everything_of(ctx, *R.batch(reads), split=True), everything_of(ctx, *PU.pack_reads(cut)),
                           everything_of(ctx, *R.batch(reads), split=True, clip=True, ends=True), everything_of(ctx, *PU.pack_reads(clipped)))
                ctx.set_chimera(False)
                ctx.set_ends()
        finally:
            rev.close()
            auto.close()
        _equiv[name] = r
    return _equiv[name]


def same_batches(got, base, what):
    assert got["n"] == base["n"] and got["n_bases"] == base["n_bases"], what
    assert got["cov"] == base["cov"], what
    for k in base["struct"]:
        assert got["struct"][k] == base["struct"][k], (what, k)
    assert got["work"] == base["work"], what
    for i in range(base["n"]):
        assert got["per"][i] == base["per"][i], (what, i, [j for j, (x, y) in enumerate(zip(got["per"][i], base["per"][i])) if x != y])
    if base["strand"] is not None:
        assert got["strand"].tobytes() == base["strand"].tobytes(), what


@pytest.mark.parametrize("name", ["default", "k31"])
@pytest.mark.parametrize("mode", ["plain", "rev", "auto"])
def test_a_split_batch_equals_a_batch_of_the_pieces(name, mode):
    r = equivalence(name)
    n = len(r["reads"])
    joined = len(r["c"].reads[:200]) - n
    assert joined >= 18 and len(r["hits"]) >= 2 * joined - 4                          # from the reference alone: two primers per joint
    cutreads = np.diff(r["piece_off"].astype(np.int64)) > 1
    assert cutreads.sum() >= joined - 2 and len(r["pieces"]) > n
    assert sum(len(a) < len(b) for a, b in zip(r["clipped"], r["cut"])) >= joined - 2   # the poly-A the cut leaves is clipped
    split, base, split_clip, base_clip = r[mode]
    for got in (split, split_clip):
        same_hits(got["hits"], r["hits"], "%s %s" % (name, mode))
        assert (got["hit_off"] == r["hit_off"]).all()
        assert got["pieces"].dtype == CR.PIECE_DTYPE and (got["pieces"] == r["pieces"]).all() and (got["piece_off"] == r["piece_off"]).all()
    same_batches(split, base, "%s %s split" % (name, mode))
    same_batches(split_clip, base_clip, "%s %s split and clipped" % (name, mode))
    assert (split_clip["rows"] == r["rows"]).all()                                    # the end rows of the pieces
    if mode != "rev":
        assert sum(p[1] == T.READ_CORRECTED for p in split["per"]) >= n // 2 and split["work"][1] > 0


@pytest.mark.parametrize("byte", [0xA5, 0xFF])
def test_a_split_batch_on_poisoned_memory_between_red_zones(byte):
    r = equivalence("default")
    base, base_clip = r["plain"][1], r["plain"][3]
    with guards_checked():
        with T.poisoned(byte):
            ctx = T.Context(r["c"].ttab, r["c"].p, 0)
            try:
                ctx.set_ends(**ENDS_KW)
                ctx.set_chimera(True, PCT, MIN_PIECE)
                got = everything_of(ctx, *R.batch(r["reads"]), split=True)
                got_clip = everything_of(ctx, *R.batch(r["reads"]), split=True, clip=True, ends=True)
                b = ctx.batch(*R.batch(r["reads"]))                                  # ... and the scan alone, on a plain batch
                plain_hits, _ = b.chimera()
                b.close()
            finally:
                ctx.close()
    same_hits(got["hits"], r["hits"], "poisoned, split")
    same_hits(plain_hits, r["hits"], "poisoned, plain")
    same_batches(got, base, "poisoned, split")
    same_batches(got_clip, base_clip, "poisoned, split and clipped")


# ---------------------------------------------------------------- 6. no behaviour change, state errors
def test_a_context_that_never_set_the_option_and_one_that_switched_it_off_again():
    c = G.gen_set("default")
    reads = c.reads[:80]
    never, other = T.Context(c.ttab, c.p, 0), T.Context(c.ttab, c.p, 0)
    try:
        other.set_ends(**ENDS_KW)
        other.set_chimera(True, PCT, MIN_PIECE)
        other.set_chimera(False)
        other.set_ends()
        a = everything_of(never, *PU.pack_reads(reads))
        b = everything_of(other, *PU.pack_reads(reads))
        assert a["per"] == b["per"] and a["work"] == b["work"] and a["work"][1] > 0 and a["cov"] == b["cov"]
        assert [p[0].decode() for p in a["per"]] == c.run["records"][:80] and [p[1] for p in a["per"]] == c.run["st"][:80].tolist()
        assert never.chimera_timing() == (0.0, 0.0) and other.chimera_timing() == (0.0, 0.0)
    finally:
        never.close()
        other.close()


def test_the_state_errors_and_the_refused_settings():
    c = G.gen_set("default")
    L = T.lib()
    ctx, other = T.Context(c.ttab, c.p, 0), T.Context(c.ttab, c.p, 0)
    reads = [x.decode() for x in CR.dress(np.random.default_rng(9), c.reads[:12], every=3)]
    want, _ = CR.hits(reads, [SSP, VNP], PCT)
    assert len(want) >= 6
    bases, offs = R.batch(reads)
    n = len(reads)
    b = ctx.batch(bases, offs)
    hits = np.zeros(64, CR.HIT_DTYPE)
    h = T.C.c_void_p()
    create = lambda clip: L.talc_batch_create_split(ctx._h, bases.ctypes.data, offs.ctypes.data, n, clip, T.C.byref(h))
    try:
        assert L.talc_batch_chimera(ctx._h, b._h) == ERR_STATE and b"off" in L.talc_last_error()
        assert L.talc_batch_fetch_chimera(ctx._h, b._h, hits.ctypes.data, 64, None) == ERR_STATE and b"scan" in L.talc_last_error()
        assert L.talc_batch_fetch_split(ctx._h, b._h, None, None) == ERR_STATE
        assert create(0) == ERR_STATE
        ctx.set_chimera(True, PCT)                                                   # on, but the ends setting holds no adapter
        assert L.talc_batch_chimera(ctx._h, b._h) == ERR_STATE and b"adapter" in L.talc_last_error()
        assert create(0) == ERR_STATE
        ctx.set_ends(poly_min=12)                                                    # still none
        assert L.talc_batch_chimera(ctx._h, b._h) == ERR_STATE and create(1) == ERR_STATE
        ctx.set_ends(adapters=[SSP, VNP])
        with pytest.raises(T.TalcError, match="max_error_pct"):
            ctx.set_chimera(True, 31)
        with pytest.raises(T.TalcError, match="min_piece"):
            ctx.set_chimera(False, 10, 0xFFFFFFFF)                                   # a refused setting changes nothing: still on
        got, _ = b.chimera()
        same_hits(got, want, "plain batch")
        cb = ctx.batch(bases, offs, clip=True)                                       # a clipped batch no longer holds the reads as they came
        try:
            assert L.talc_batch_chimera(ctx._h, cb._h) == ERR_STATE and b"clipped" in L.talc_last_error()
            assert L.talc_batch_fetch_chimera(ctx._h, cb._h, hits.ctypes.data, 64, None) == ERR_STATE
        finally:
            cb.close()
        assert L.talc_batch_num_chimera_hits(b._h) == len(want)
        assert L.talc_batch_fetch_chimera(ctx._h, b._h, hits.ctypes.data, len(want) - 1, None) == ERR_CAPACITY
        assert str(len(want)).encode() in L.talc_last_error()
        assert L.talc_batch_chimera(other._h, b._h) == ERR_INVALID                    # another context's batch
        ctx.set_chimera(True, 0)                                                     # a new setting: the hits follow it
        same_hits(b.chimera()[0], CR.hits(reads, [SSP, VNP], 0)[0], "second setting")
        ctx.set_ends(adapters=[VNP])                                                 # ... and the adapters of the ends setting
        same_hits(b.chimera()[0], CR.hits(reads, [VNP], 0)[0], "other adapters")
        ctx.set_chimera(False)
        assert L.talc_batch_chimera(ctx._h, b._h) == ERR_STATE
        assert L.talc_batch_fetch_chimera(ctx._h, b._h, hits.ctypes.data, 64, None) == 0   # the hits of the last scan stay
    finally:
        b.close()
        ctx.close()
        other.close()


# ---------------------------------------------------------------- 7. the command line
def test_cli_split_and_clipped_run_equals_a_plain_run_on_the_pieces(tmp_path):
    c = G.gen_set("default")
    n = 60
    reads = [x.decode() for x in CR.dress(np.random.default_rng(31), c.reads[:n], every=5)]
    names = ["read%d/x" % i for i in range(len(reads))]
    hits, hit_off = CR.hits(reads, [SSP, VNP], PCT)
    pieces, piece_off, dropped, dropped_bases = CR.pieces([len(x) for x in reads], hits, MIN_PIECE)
    cut = [x.decode() for x in CR.cut(reads, pieces)]
    rows = R.rows(cut, **ENDS_KW)
    clipped = [x.decode() for x in R.clip(cut, rows)]
    piece_names = CR.piece_names(names, pieces)
    assert len(reads) == n - 12 and len(hits) >= 24 and len(pieces) >= len(reads) + 10 and all(len(x) > 0 for x in clipped)
    assert sum(len(a) < len(b) for a, b in zip(clipped, cut)) >= 10 and any("_c2" in x for x in piece_names)
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    (tmp_path / "dressed.fa").write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, reads)))
    (tmp_path / "pieces.fa").write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(piece_names, clipped)))
    common = ["-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7", "-o", "o", "--read-stats"]
    lr = ["--LRAdapter", SSP, "--LRAdapter", VNP, "--LRPolyA", "12"]
    runs = {}
    for d, args, env in (("split", ["dressed.fa"] + lr + ["--LRSplit", "--LRClip"], None), ("host", ["pieces.fa"], None), ("report", ["dressed.fa"] + lr + ["--LRChimeras"], None),
                         ("dressed", ["dressed.fa"] + lr, None), ("split2", ["dressed.fa"] + lr + ["--LRSplit", "--LRClip", "--gpus", "2"], dict(os.environ, TALC_FAKE_GPUS="2"))):
        (tmp_path / d).mkdir()
        runs[d] = subprocess.run([TALC, str(tmp_path / args[0])] + args[1:] + common, cwd=tmp_path / d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert runs[d].returncode == 0, (d, runs[d].stderr.decode())
    read = lambda d, ext: (tmp_path / d / ("o" + ext)).read_bytes() if (tmp_path / d / ("o" + ext)).exists() else None
    for ext in (".fa", ".log", ".stats_basics.txt"):
        assert read("split", ext) == read("host", ext), ext                 # the pieces, cut and clipped, under their names
        assert read("split2", ext) == read("split", ext), ext
        assert read("report", ext) == read("dressed", ext), ext             # without --LRSplit nothing but the report is new
    assert read("split", ".fa") != read("dressed", ".fa") and len(read("split", ".stats_basics.txt").splitlines()) > n // 2
    lines = read("split", ".chimera.tsv").decode().splitlines()
    assert lines[0] == "read_name\traw_length\tadapter\tstrand\tstart\tend\terr"
    assert lines[1:] == ["\t".join([names[int(h["read"])], str(len(reads[int(h["read"])])), str(int(h["adapter"])), "-" if h["strand"] else "+", str(int(h["start"])),
                                    str(int(h["end"])), str(int(h["err"]))]) for h in hits]
    assert read("report", ".chimera.tsv") == read("split", ".chimera.tsv") == read("split2", ".chimera.tsv")
    plines = read("split", ".chimera_pieces.tsv").decode().splitlines()
    assert plines[0] == "piece_name\tread_name\tstart\tlen"
    assert plines[1:] == ["\t".join([pn, names[int(p["read"])], str(int(p["start"])), str(int(p["len"]))]) for pn, p in zip(piece_names, pieces)]
    assert read("split2", ".chimera_pieces.tsv") == read("split", ".chimera_pieces.tsv")
    assert read("report", ".chimera_pieces.tsv") is None and read("dressed", ".chimera.tsv") is None and read("host", ".chimera.tsv") is None
    # the end report of a split run is that of the pieces
    elines = read("split", ".ends.tsv").decode().splitlines()
    assert [x.split("\t")[0] for x in elines[1:]] == piece_names and [int(x.split("\t")[-2]) for x in elines[1:]] == [len(x) for x in clipped]
    line = "[TALC]: chimeras: %d reads, %d hits in %d reads, %d pieces kept, %d pieces dropped (%d bases)" % (
        len(reads), len(hits), len(np.unique(hits["read"])), len(pieces), dropped, dropped_bases)
    for d in ("split", "report", "split2"):
        assert runs[d].stdout.decode().splitlines().count(line) == 1, (d, line)
    assert b"chimeras:" not in runs["dressed"].stdout and b"correcting on 2 GPU(s)" in runs["split2"].stdout
    cfg = read("split", ".config.txt").decode().splitlines()
    at = cfg.index("queryMode=memory")
    assert cfg[at + 1:at + 6] == ["LRAdapter=" + SSP, "LRAdapter=" + VNP, "LRPolyA=12", "LRClip=1", "LRSplit=1"]
    assert read("dressed", ".config.txt") == read("report", ".config.txt").replace(b"LRChimeras=1\n", b"")

