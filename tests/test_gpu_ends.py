"""The long-read end clean-up on the device (docs/read_ends.md; k_read_ends, k_gather, talc_batch_create_clipped) against
the contract in numpy (tests/ends_ref.py: never from a device result), and a clipped batch against a plain batch of the reads
clipped on the host.  Integers and bytes, tolerance 0.  Every case first asserts, from the reference alone, that its input
reaches what it is there for."""
import os
import subprocess

import numpy as np
import pytest

import ends_ref as R
import parity_util as PU
import test_gpu_solidity as G
from memcheck_util import fetch_all, guards_checked, per_read
from talc_amd import build as B
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ERR_INVALID, ERR_STATE = -1, -6
SSP, VNP = "TTTCTGTTGGTGCTGATATTGCTGGG", "ACTTGCCTGTCGCTCTATCTTC"      # the two real primers (26 and 22 letters)
P24 = "GATCCGTAGCTTGACCATGCAGTC"                                         # 24 letters: k_a = 4 at 20 per cent


def same_rows(got, want, what=""):
    assert got.dtype == R.DTYPE and len(got) == len(want)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


_ctx = {}


def ctx_of(name="default"):
    """A context of its own over the shared table of one of test_gpu_solidity's sets (the sets' own contexts never see ends)."""
    if name not in _ctx:
        c = G.gen_set(name)
        _ctx[name] = (c, T.Context(c.ttab, c.p, 0))
    return _ctx[name]


def device_rows(reads, **kw):
    """Batch.ends() of a plain batch, and the rows of a clipped batch of the same reads with its texts."""
    c, ctx = ctx_of()
    ctx.set_ends(**kw)
    try:
        bases, offs = R.batch(reads)
        b = ctx.batch(bases, offs)
        try:
            plain = b.ends()
        finally:
            b.close()
        return plain
    finally:
        ctx.set_ends()


def check(reads, what, **kw):
    want = R.rows(reads, **kw)
    same_rows(device_rows(reads, **kw), want, what)
    return want


def subs(seq, places):
    """`seq` with the letters at `places` replaced by the next letter of ACGT."""
    s = list(seq)
    for at in places:
        s[at] = "ACGT"[("ACGT".index(s[at]) + 1) % 4]
    return "".join(s)


# ---------------------------------------------------------------- 1. end-position sweep
SUB_PLACES = (3, 8, 12, 17, 21)          # inside the primer, apart: k substitutions there cost exactly k


def sweep_reads(rng, ends, level):
    """For every e of `ends`: a read whose head holds P24 with `level` substitutions so that the copy ends at e (a copy cut
    off by the read's start where e < 24), and the reverse complement of such a read."""
    planted = subs(P24, SUB_PLACES[:level])
    heads = []
    for e in ends:
        copy = planted[max(0, len(planted) - e):]
        heads.append(R.random_seq(rng, e - len(copy)) + copy + R.random_seq(rng, 70))
    return heads + [R.revcomp(h).decode() for h in heads]


@pytest.mark.parametrize("window,ends", [(192, tuple(range(1, 193))), (4096, (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096))])
def test_a_primer_that_ends_at_every_position_of_the_window(window, ends):
    rng = np.random.default_rng(100 + window)
    kw = dict(adapters=[P24], max_error_pct=20, poly_min=0, window=window)
    ka = 20 * 24 // 100
    assert ka == 4 and ka + 1 == len(SUB_PLACES)
    for level in (0, ka, ka + 1):
        reads = sweep_reads(rng, ends, level)
        want = check(reads, "sweep, %d edits, window %d" % (level, window), **kw)
        n = len(ends)
        whole = np.array([e >= 24 for e in ends])
        head, tail = want[:n], want[n:]
        if level <= ka:      # every whole copy is found, where it ends, at its cost, at the head and mirrored at the tail
            assert (head["head_adapter_len"][whole] == np.array(ends)[whole]).all() and (head["head_adapter_err"][whole] == level).all()
            assert (tail["tail_adapter_len"][whole] == np.array(ends)[whole]).all() and (tail["tail_adapter_err"][whole] == level).all()
            assert (head["head_adapter"][whole] == 1).all() and (tail["tail_adapter"][whole] == 1).all()
            assert (head["kept_start"][whole] == np.array(ends)[whole]).all()
        else:                # one edit too many: rejected everywhere
            assert (head["head_adapter"] == 0).all() and (tail["tail_adapter"] == 0).all() and (want["kept_start"] == 0).all()
        if window == 192:    # a copy cut off by the read's start pays for its missing letters: the short ones are rejected
            assert (head["head_adapter"][:24 - ka - 1] == 0).all()


# ---------------------------------------------------------------- 2. edits and tie rules
def test_edits_of_each_kind_junk_and_the_tie_rules():
    rng = np.random.default_rng(7)
    kw = dict(adapters=[P24], max_error_pct=20, poly_min=0, window=512)
    reads, kinds = [], []
    for kind in ("S", "I", "D", "N"):
        for n_edits in (1, 2, 4, 5):
            for junk in (0, 1, 7, 40):
                reads.append(R.random_seq(rng, junk) + R.mutate(rng, P24, n_edits, kind) + R.random_seq(rng, 90))
                kinds.append((kind, n_edits))
    for junk in (0, 13, 40):
        reads.append((R.random_seq(rng, junk) + P24 + R.random_seq(rng, 90)).lower())
        reads.append(R.random_seq(rng, junk) + R.mutate(rng, P24, 2, "S").lower() + R.random_seq(rng, 90))
        kinds += [("lower", 0), ("lower", 2)]
    reads += [R.revcomp(r).decode() for r in reads]
    want = check(reads, "edits", **kw)
    n = len(kinds)
    for kind in ("S", "I", "D", "N", "lower"):
        mine = np.array([k[0] == kind for k in kinds])
        found = want["head_adapter"][:n][mine] == 1
        assert found.sum() >= 4 and (kind == "lower" or (~found).sum() >= 2), (kind, int(found.sum()))     # accepted and rejected ones
        assert (want["head_adapter_err"][:n][mine][found] > 0).any()
    assert (want["tail_adapter"][n:] == want["head_adapter"][:n]).all() and (want["tail_adapter_len"][n:] == want["head_adapter_len"][:n]).all()

    # a tie on D goes to the largest e: the primer's last letter replaced (cost 1 at e = 23 as a deletion, at 24 as a
    # substitution), and the letter itself behind it (cost 1 at 25 as an insertion)
    last = P24[-1]
    other = next(ch for ch in "ACGT" if ch != last and ch != P24[-2])
    assert "G" not in (last, other)
    ties = [P24[:-1] + other + "G" * 40, P24[:-1] + other + last + "G" * 40, "GG" + P24[:-1] + other + last + "G" * 40]
    for s, e in zip(ties, (24, 25, 27)):
        D = R.sellers_plain(P24.encode(), s.encode())
        assert min(D[1:]) == 1 and sum(d == 1 for d in D[1:]) >= 2 and max(i for i, d in enumerate(D) if d == 1) == e
    want = check(ties + [R.revcomp(s).decode() for s in ties], "ties", **kw)
    assert want["head_adapter_len"][:3].tolist() == [24, 25, 27] and want["tail_adapter_len"][3:].tolist() == [24, 25, 27]
    assert (want["head_adapter_err"][:3] == 1).all()

    # two adapters: the one whose match ends last; the lowest index when both end at the same place
    two = [SSP + R.random_seq(rng, 30) + VNP + R.random_seq(rng, 80), VNP + R.random_seq(rng, 30) + R.mutate(rng, SSP, 3, "S") + R.random_seq(rng, 80),
           R.random_seq(rng, 9) + VNP + R.random_seq(rng, 80)]
    want = check(two + [R.revcomp(s).decode() for s in two], "two adapters", adapters=[SSP, VNP], max_error_pct=20, poly_min=0, window=512)
    assert want["head_adapter"][:3].tolist() == [2, 1, 2] and want["head_adapter_len"][:3].tolist() == [78, 78, 31]
    assert want["tail_adapter"][3:].tolist() == [2, 1, 2]
    want = check(two, "the same adapter twice", adapters=[VNP, VNP, SSP], max_error_pct=20, poly_min=0, window=512)
    assert want["head_adapter"].tolist() == [1, 3, 1]


@pytest.mark.parametrize("m,pct", [(12, 0), (12, 30), (64, 0), (64, 30)])
def test_the_shortest_and_the_longest_adapter_at_both_error_bounds(m, pct):
    rng = np.random.default_rng(1000 + m + pct)
    ad = R.random_seq(rng, m)
    k = pct * m // 100
    assert k == {(12, 0): 0, (12, 30): 3, (64, 0): 0, (64, 30): 19}[(m, pct)]      # 19: the longest warm-up, m + k = 83 columns
    reads, level = [], []
    top = min(k + 8, m - 2)             # far over the bound: substitutions at random places often cost less than their number
    for n_edits in sorted({0, k, k + 1, top}):
        for junk in (0, 5, 64, 129, 400):
            places = rng.choice(np.arange(1, m - 1), size=n_edits, replace=False).tolist()
            reads.append(R.random_seq(rng, junk) + subs(ad, places) + R.random_seq(rng, 120))
            level.append(n_edits)
            if n_edits:
                reads.append(R.random_seq(rng, junk) + R.mutate(rng, ad, n_edits, "SID") + R.random_seq(rng, 120))
                level.append(n_edits)
    reads += [R.revcomp(r).decode() for r in reads]
    want = check(reads, "adapter of %d at %d per cent" % (m, pct), adapters=[ad], max_error_pct=pct, poly_min=0, window=512)
    n = len(level)
    level = np.array(level)
    assert (want["head_adapter"][:n][level <= k] == 1).all() and (want["tail_adapter"][n:][level <= k] == 1).all()
    if m == 64:      # (a 12-mer within 3 edits occurs by chance; a 64-mer that far over its bound does not)
        assert (want["head_adapter"][:n][level == top] == 0).sum() >= 5
    assert int(want["head_adapter_err"][:n].max()) == k


# ---------------------------------------------------------------- 3. poly runs
def test_poly_runs():
    rng = np.random.default_rng(11)
    W, PM = 512, 12
    kw = dict(adapters=[SSP, VNP], max_error_pct=20, poly_min=PM, window=W)
    body = lambda n=200: "G" + R.random_seq(rng, n) + "C"          # (neither a T behind a head run nor an A before a tail run)
    lens = (PM - 1, PM, 63, 64, 65, 255, 256, W, W + 40)
    heads = ["T" * n + body() for n in lens]
    tails = [body() + "A" * n for n in lens]
    want = check(heads + tails, "run lengths", **kw)
    capped = [0 if n < PM else min(n, W) for n in lens]
    assert want["head_poly_len"][:len(lens)].tolist() == capped and want["tail_poly_len"][len(lens):].tolist() == capped
    assert (want["orient"][:len(lens)] == [-1 if x else 0 for x in capped]).all() and (want["orient"][len(lens):] == [1 if x else 0 for x in capped]).all()
    # interruptions the score absorbs (20 T, C, 20 T: 20, 18, 38; 5 T, CC, 20 T: 5, 1, 21; an N, lower case) and ones that end
    # the run (12 T, 7 C, 13 T: 12, -2, 11; a C after 11 T; every second base)
    inter = ["T" * 20 + "C" + "T" * 20 + body(), "T" * 5 + "CC" + "T" * 20 + body(), "T" * 12 + "C" * 7 + "T" * 13 + body(), "T" * 30 + "N" + "T" * 30 + body(),
             "t" * 40 + body(), "T" * 11 + "C" + body(), "CT" * 40 + body()]
    want = check(inter + [R.revcomp(s).decode() for s in inter], "interruptions", **kw)
    assert want["head_poly_len"][:7].tolist() == [41, 27, 12, 61, 40, 0, 0] and want["tail_poly_len"][7:].tolist() == [41, 27, 12, 61, 40, 0, 0]
    # a run behind a primer (no slack: the run starts where the primer ends, so a base between them is an interruption the score
    # has to absorb: -2, then 50 T: 51), without one, both ends on one read
    dressed = [R.random_seq(rng, 6) + R.mutate(rng, SSP, 2, "S") + "T" * 50 + body(), SSP + "G" + "T" * 50 + body(), "T" * 50 + body() + "A" * 33 + R.revcomp(VNP).decode(),
               R.random_seq(rng, 3) + SSP + "T" * 25 + body() + "A" * 70 + R.revcomp(R.mutate(rng, VNP, 3, "S")).decode() + R.random_seq(rng, 11), "T" * 700, "A" * 700,
               "T" * 100, "T" * 20 + body(40) + "A" * 20]
    want = check(dressed, "primer and run", **kw)
    assert want["head_adapter"].tolist() == [1, 1, 0, 1, 0, 0, 0, 0] and want["head_poly_len"].tolist() == [50, 51, 50, 25, W, 0, 100, 20]
    assert want["tail_adapter"].tolist() == [0, 0, 2, 2, 0, 0, 0, 0] and want["tail_poly_len"].tolist() == [0, 0, 33, 70, 0, W, 0, 20]
    assert want["kept_len"][4:7].tolist() == [700 - W, 700 - W, 0] and want["orient"].tolist() == [-1, -1, 0, 0, -1, 1, -1, 0]


# ---------------------------------------------------------------- 4. short reads, one long read
def test_short_reads_overlapping_claims_and_a_long_read():
    rng = np.random.default_rng(13)
    c, _ = ctx_of()
    W = 64
    kw = dict(adapters=[P24, R.revcomp(P24).decode()], max_error_pct=20, poly_min=8, window=W)
    both = "TTG" + P24 + "CAA"                                  # 30 bytes: the same copy is adapter 1 of the head and adapter 2 of the tail
    reads = ["", "T", "A", "ACGTTGCATTA", R.random_seq(rng, c.k), "T" * c.k, R.random_seq(rng, W - 1), "T" * (W - 1), both, P24, P24[:20],
             "T" * (W - 1) + "A" * W, "T" * 30 + "A" * 30, R.random_seq(rng, 10) + P24 + "T" * W + "A" * (2 * W - 1 - 34 - W), ""]
    assert [len(r) for r in reads[:4]] == [0, 1, 1, 11] and len(reads[11]) == 2 * W - 1 == len(reads[13])
    want = check(reads, "short reads", **kw)
    i = reads.index(both)
    assert want[i]["head_adapter"] == 1 and want[i]["tail_adapter"] == 2 and want[i]["head_adapter_len"] + want[i]["tail_adapter_len"] > 30      # both claim the middle
    assert want[i]["kept_len"] == 0 and want[i]["kept_start"] == 27
    assert want[11]["kept_len"] == 0 and want[11]["head_poly_len"] == W - 1 and want[11]["tail_poly_len"] == W
    assert want[13]["kept_len"] == 0 and want[13]["kept_start"] == 34 + W
    assert (want["kept_start"].astype(np.int64) + want["kept_len"] <= [len(r) for r in reads]).all()
    # a clipped batch of them: its texts are the kept intervals, its rows those of the reads as given
    _, ctx = ctx_of()
    ctx.set_ends(**kw)
    try:
        b = ctx.batch(*R.batch(reads), clip=True)
        try:
            same_rows(b.ends(), want, "clipped batch of short reads")
            assert b.n_bases == int(want["kept_len"].sum())
            raw, _ = b.support(source="raw")                    # (one byte per base of the batch's own reads)
            assert len(raw) == b.n_bases
        finally:
            b.close()
    finally:
        ctx.set_ends()
    long_read = R.random_seq(rng, 3) + R.mutate(rng, SSP, 3, "S") + "T" * 90 + "G" + R.random_seq(rng, 140_000) + "C" + "A" * 150 + R.revcomp(VNP).decode()
    want = check([long_read, R.revcomp(long_read).decode()], "140 kb", adapters=[SSP, VNP], max_error_pct=20, poly_min=12, window=512)
    assert want["head_adapter"].tolist() == [1, 2] and want["tail_adapter"].tolist() == [2, 1] and want["head_poly_len"].tolist() == [90, 150]
    assert want["kept_len"][0] == 140_002 and want["kept_len"][1] == 140_002


# ---------------------------------------------------------------- 5. no false finds
def test_random_reads_have_no_ends():
    rng = np.random.default_rng(2)
    lens = rng.integers(30, 1400, 2000)
    reads = [R.random_seq(rng, int(n)) for n in lens.tolist()]
    want = check(reads, "random reads", adapters=[SSP, VNP], max_error_pct=20, poly_min=12, window=512)
    assert (want["kept_start"] == 0).all() and (want["kept_len"] == lens).all() and (want["orient"] == 0).all()
    assert not want["head_adapter"].any() and not want["tail_adapter"].any()


# ---------------------------------------------------------------- 6. equivalence with a plain batch of the clipped reads
ENDS_KW = dict(adapters=[SSP, VNP], max_error_pct=20, poly_min=12, window=512)


def dress(reads, seed):
    """Generator reads with primers (within the error bound, behind 0 to 30 bases of junk) and tails: half of them with a
    head primer, half with a poly-T head, half with a tail primer, half with a poly-A tail, in every combination."""
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(reads):
        hp, ht, tp, ta = i % 4 in (0, 1), i % 4 in (1, 2), (i // 4) % 4 in (0, 1), (i // 4) % 4 in (1, 2)
        head = (R.random_seq(rng, int(rng.integers(0, 31))) + R.mutate(rng, SSP, int(rng.integers(0, 5)), "SID") if hp else "") + ("T" * int(rng.integers(12, 80)) if ht else "")
        tail = ("A" * int(rng.integers(12, 80)) if ta else "") + (R.revcomp(R.mutate(rng, VNP, int(rng.integers(0, 4)), "SID")).decode() + R.random_seq(rng, int(rng.integers(0, 31))) if tp else "")
        out.append(head + r + tail)
    return out


def everything_of(ctx, bases, offs, clip):
    """memcheck_util.everything for a batch made either way, with the coverage and the structure in front."""
    ctx.record_map(True)
    b = ctx.batch(bases, offs, clip=clip)
    try:
        n = len(offs) - 1
        b.coverage()
        cov = [x.tobytes() for x in b.fetch_coverage()]
        b.structure()
        st = b.fetch_structure()
        struct = {k: v.tobytes() for k, v in st.items()}
        rc = b.correct()
        t = ctx.timing()
        work = (rc, t.n_trail_steps, t.n_dp_cells, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)
        per = per_read(fetch_all(b), n)
        rows = b.ends() if clip else None
        strand = b.strand() if ctx._auto else None
        return dict(cov=cov, struct=struct, work=work, per=per, rows=rows, strand=strand)
    finally:
        b.close()
        ctx.record_map(False)


_equiv = {}


def equivalence(name):
    if name not in _equiv:
        c, plain = ctx_of(name)
        reads = dress(c.reads, 5)
        want = R.rows(reads, **ENDS_KW)
        clipped = [x.decode() for x in R.clip(reads, want)]
        rev, auto = T.Context(c.ttab, T.default_params(k=c.k, reverse=1), 0), T.Context(c.ttab, c.p, 0)
        auto.auto_strand()
        r = dict(c=c, reads=reads, want=want, clipped=clipped)
        try:
            for mode, ctx in (("plain", plain), ("rev", rev), ("auto", auto)):
                ctx.set_ends(**ENDS_KW)
                r[mode] = (everything_of(ctx, *R.batch(reads), clip=True), everything_of(ctx, *PU.pack_reads(clipped), clip=False))
                ctx.set_ends()
        finally:
            rev.close()
            auto.close()
        _equiv[name] = r
    return _equiv[name]


@pytest.mark.parametrize("name", ["default", "k31"])
@pytest.mark.parametrize("mode", ["plain", "rev", "auto"])
def test_a_clipped_batch_equals_a_batch_of_the_clipped_reads(name, mode):
    r = equivalence(name)
    want, n = r["want"], len(r["reads"])
    for f in ("head_adapter", "tail_adapter", "head_poly_len", "tail_poly_len"):       # the reference alone puts a quarter in each class
        assert int((want[f] > 0).sum()) >= n // 4, (f, int((want[f] > 0).sum()))
    assert int((want["kept_len"] < [len(x) for x in r["reads"]]).sum()) >= 3 * n // 4
    # the reference clips the dressing and nothing else: what it keeps is the generator's read, for most reads to the base
    assert sum(a == b for a, b in zip(r["clipped"], r["c"].reads)) >= n // 2
    got, base = r[mode]
    same_rows(got["rows"], want, "%s %s" % (name, mode))
    assert got["cov"] == base["cov"]
    for k in base["struct"]:
        assert got["struct"][k] == base["struct"][k], k
    assert got["work"] == base["work"] and (got["work"][1] > 0 or mode == "rev")      # (-rev: these reads have nothing to search)
    for i in range(n):
        assert got["per"][i] == base["per"][i], (name, mode, i, [j for j, (x, y) in enumerate(zip(got["per"][i], base["per"][i])) if x != y])
    if mode == "auto":       # the vote sees the kept intervals, not the reads as given
        assert got["strand"].tobytes() == base["strand"].tobytes()
    if mode != "rev":        # (the table is directional: under -rev these reads have next to no solid k-mer)
        assert sum(p[1] == T.READ_CORRECTED for p in got["per"]) >= n // 2


@pytest.mark.parametrize("byte", [0xA5, 0xFF])
def test_a_clipped_batch_on_poisoned_memory_between_red_zones(byte):
    """Nothing the scan or the gather leaves depends on what device memory held, and neither writes outside its buffers
    (the hooks of talc_devmem.h): the staging buffers, the rows and the batch's text are all cached buffers."""
    r = equivalence("default")
    base = r["plain"][1]                                   # the plain batch of the host-clipped reads, unpoisoned
    with guards_checked():
        with T.poisoned(byte):
            ctx = T.Context(r["c"].ttab, r["c"].p, 0)
            try:
                ctx.set_ends(**ENDS_KW)
                got = everything_of(ctx, *R.batch(r["reads"]), clip=True)
                b = ctx.batch(*R.batch(r["reads"]))        # ... and the scan alone, on a plain batch
                plain_rows = b.ends()
                b.close()
            finally:
                ctx.close()
    same_rows(got["rows"], r["want"], "poisoned, clipped")
    same_rows(plain_rows, r["want"], "poisoned, plain")
    assert got["per"] == base["per"] and got["work"] == base["work"] and got["cov"] == base["cov"]


# ---------------------------------------------------------------- 7. no behaviour change
def test_a_context_that_never_set_ends_and_one_that_switched_them_off_again():
    c = G.gen_set("default")
    reads = c.reads[:80]
    never, other = T.Context(c.ttab, c.p, 0), T.Context(c.ttab, c.p, 0)
    try:
        other.set_ends(**ENDS_KW)
        other.set_ends()
        a = everything_of(never, *PU.pack_reads(reads), clip=False)
        b = everything_of(other, *PU.pack_reads(reads), clip=False)
        assert a["per"] == b["per"] and a["work"] == b["work"] and a["work"][1] > 0 and a["cov"] == b["cov"]
        assert [p[0].decode() for p in a["per"]] == c.run["records"][:80] and [p[1] for p in a["per"]] == c.run["st"][:80].tolist()
        assert never.ends_timing() == (0.0, 0.0) and other.ends_timing() == (0.0, 0.0)
    finally:
        never.close()
        other.close()


def test_the_state_errors_and_the_refused_settings():
    c = G.gen_set("default")
    L = T.lib()
    ctx, other = T.Context(c.ttab, c.p, 0), T.Context(c.ttab, c.p, 0)
    reads = dress(c.reads[:8], 9)
    bases, offs = R.batch(reads)
    b = ctx.batch(bases, offs)
    rows = np.zeros(8, R.DTYPE)
    h = T.C.c_void_p()
    try:
        assert L.talc_batch_ends(ctx._h, b._h) == ERR_STATE and b"off" in L.talc_last_error()            # ends are off
        assert L.talc_batch_fetch_ends(ctx._h, b._h, rows.ctypes.data) == ERR_STATE and b"scan" in L.talc_last_error()   # no scan has run
        assert L.talc_batch_create_clipped(ctx._h, bases.ctypes.data, offs.ctypes.data, 8, T.C.byref(h)) == ERR_STATE
        for bad, word in ((dict(adapters=["ACGTACGTACG"]), "12"), (dict(adapters=["ACGTACGTACGN"]), "ACGT"), (dict(adapters=[P24] * 5), "more than 4"),
                          (dict(adapters=[P24], max_error_pct=31), "max_error_pct"), (dict(poly_min=7), "poly_min"), (dict(poly_min=600), "poly_min"),
                          (dict(poly_min=40, window=32), "poly_min"), (dict(poly_min=8, window=31), "window"), (dict(poly_min=8, window=4097), "window"),
                          (dict(adapters=["A" * 65]), "64")):
            with pytest.raises(T.TalcError, match=word):
                ctx.set_ends(**bad)
        assert L.talc_batch_ends(ctx._h, b._h) == ERR_STATE                                              # a refused setting sets nothing
        ctx.set_ends(**ENDS_KW)
        assert L.talc_batch_fetch_ends(ctx._h, b._h, rows.ctypes.data) == ERR_STATE
        same_rows(b.ends(), R.rows(reads, **ENDS_KW), "plain batch")
        assert L.talc_batch_ends(other._h, b._h) == ERR_INVALID                                          # another context's batch
        ctx.set_ends(adapters=[SSP], window=0)                                                           # 0: 512; a new setting, the rows follow it
        same_rows(b.ends(), R.rows(reads, adapters=[SSP], max_error_pct=20, poly_min=0, window=512), "second setting")
        ctx.set_ends()
        assert L.talc_batch_ends(ctx._h, b._h) == ERR_STATE
        assert L.talc_batch_fetch_ends(ctx._h, b._h, rows.ctypes.data) == 0                              # the rows of the last scan stay
    finally:
        b.close()
        ctx.close()
        other.close()


def test_a_clipped_batch_keeps_its_rows_and_never_scans_again():
    """The span rule: a span's time changes only when its kernel is launched.  After the clipped batch a scan of another,
    larger batch leaves its own time in the span; asking the clipped batch for its rows must leave that time as it is."""
    c = G.gen_set("default")
    ctx = T.Context(c.ttab, c.p, 0)
    reads = dress(c.reads[:40], 21)
    want = R.rows(reads, **ENDS_KW)
    try:
        ctx.set_ends(**ENDS_KW)
        b = ctx.batch(*R.batch(reads), clip=True)
        scan0, gather0 = ctx.ends_timing()
        assert scan0 > 0 and gather0 > 0
        big = ctx.batch(*R.batch(dress(c.reads, 22)))
        big.ends()
        scan1, gather1 = ctx.ends_timing()
        assert scan1 > 0 and scan1 != scan0 and gather1 == gather0
        same_rows(b.ends(), want, "clipped batch, asked again")
        assert ctx.ends_timing() == (scan1, gather1)
        ctx.set_ends(adapters=[VNP])                      # a later setting does not reach back: the batch was made from these rows
        same_rows(b.ends(), want, "clipped batch, after another setting")
        ctx.set_ends()                                    # ... nor does switching off
        same_rows(b.ends(), want, "clipped batch, ends off")
        assert ctx.ends_timing() == (scan1, gather1)
        b.correct()                                       # the batch is an ordinary one: its reads are the kept intervals
        out, oo, st = b.fetch_corrected()
        assert len(oo) == 41 and b.n_bases == int(want["kept_len"].sum())
        b.close()
        big.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 8. the command line
def test_cli_clipped_run_equals_a_plain_run_on_the_clipped_reads(tmp_path):
    c = G.gen_set("default")
    n = 60
    reads = dress(c.reads[:n], 31)
    want = R.rows(reads, **ENDS_KW)
    clipped = [x.decode() for x in R.clip(reads, want)]
    assert int((want["kept_len"] < [len(x) for x in reads]).sum()) >= n // 2 and all(len(x) > 0 for x in clipped)
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    names = ["read%d/x" % i for i in range(n)]
    (tmp_path / "dressed.fa").write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, reads)))
    (tmp_path / "clipped.fa").write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, clipped)))
    common = ["-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7", "-o", "o", "--read-stats"]
    lr = ["--LRAdapter", SSP, "--LRAdapter", VNP, "--LRPolyA", "12"]
    runs = {}
    for d, args, env in (("clip", ["dressed.fa"] + lr + ["--LRClip"], None), ("host", ["clipped.fa"], None), ("report", ["dressed.fa"] + lr, None),
                         ("dressed", ["dressed.fa"], None), ("clip2", ["dressed.fa"] + lr + ["--LRClip", "--gpus", "2"], dict(os.environ, TALC_FAKE_GPUS="2"))):
        (tmp_path / d).mkdir()
        runs[d] = subprocess.run([TALC, str(tmp_path / args[0])] + args[1:] + common, cwd=tmp_path / d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert runs[d].returncode == 0, (d, runs[d].stderr.decode())
    read = lambda d, ext: (tmp_path / d / ("o" + ext)).read_bytes() if (tmp_path / d / ("o" + ext)).exists() else None
    for ext in (".fa", ".log", ".stats_basics.txt"):
        assert read("clip", ext) == read("host", ext), ext                  # the clipped reads under their names
        assert read("clip2", ext) == read("clip", ext), ext
        assert read("report", ext) == read("dressed", ext), ext             # without --LRClip nothing but the report is new
    assert read("clip", ".fa") != read("dressed", ".fa") and len(read("clip", ".stats_basics.txt").splitlines()) > n // 2
    lines = read("clip", ".ends.tsv").decode().splitlines()
    assert lines[0] == "read_name\traw_length\thead_adapter\thead_adapter_len\thead_adapter_err\thead_poly\ttail_adapter\ttail_adapter_len\ttail_adapter_err\ttail_poly\tkept_start\tkept_len\torient"
    assert lines[1:] == ["\t".join([nm, str(len(s))] + [str(int(w[f])) for f in ("head_adapter", "head_adapter_len", "head_adapter_err", "head_poly_len", "tail_adapter",
                                                                               "tail_adapter_len", "tail_adapter_err", "tail_poly_len", "kept_start", "kept_len", "orient")])
                         for nm, s, w in zip(names, reads, want)]
    assert read("report", ".ends.tsv") == read("clip", ".ends.tsv") == read("clip2", ".ends.tsv")
    assert read("dressed", ".ends.tsv") is None and read("host", ".ends.tsv") is None
    n_ad = int(((want["head_adapter"] > 0) | (want["tail_adapter"] > 0)).sum())
    n_poly = int(((want["head_poly_len"] > 0) | (want["tail_poly_len"] > 0)).sum())
    n_bases = sum(len(s) for s in reads) - int(want["kept_len"].sum())
    line = "[TALC]: read ends: %d reads, %d with an adapter, %d with a poly run, %d bases clipped" % (n, n_ad, n_poly, n_bases)
    assert runs["clip"].stdout.decode().splitlines().count(line) == 1 and b"read ends:" not in runs["dressed"].stdout
    assert b"correcting on 2 GPU(s)" in runs["clip2"].stdout
    cfg = read("clip", ".config.txt").decode().splitlines()
    at = cfg.index("queryMode=memory")
    assert cfg[at + 1:at + 5] == ["LRAdapter=" + SSP, "LRAdapter=" + VNP, "LRPolyA=12", "LRClip=1"]
    assert read("dressed", ".config.txt") == read("host", ".config.txt").replace(b"clipped.fa", b"dressed.fa")
