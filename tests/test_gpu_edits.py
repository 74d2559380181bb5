"""The edit scripts on the device (docs/correction_edits.md; k_edit_align, k_edit_count, k_edit_pack) against the numpy
contract (tests/edits_ref.py): single pairs through talc_test_edit_script at every length where the device code takes
another path, and batches, where the reference is fed with that batch's own map, records and reads.  All comparisons are
integers and bytes."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import corr_map_ref as M
import edits_ref as E
import edits_util as U
import parity_util as PU
import pieces_ref as P
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
CONTENTS = ("equal", "edits", "homopolymer", "mismatch", "one-N")


def ctx_of(s):
    if s.pair.ctx is None:
        s.pair.upload(0)
    return s.pair.ctx


@pytest.fixture(scope="module")
def ctx():
    return ctx_of(M.map_set("default"))


def rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n)) if n else ""


def mutated(rng, a, rate=0.12):
    """a with about `rate` edits per base: substitutions, insertions and deletions in equal parts."""
    out = []
    for c in a:
        u = rng.random()
        if u < rate / 3:
            out.append(rng.choice([x for x in "ACGT" if x != c]))
        elif u < 2 * rate / 3:
            out += [c, rng.choice(list("ACGT"))]
        elif u >= rate:
            out.append(c)
    return "".join(out)


def pair_of(content, la, lb, rng):
    if content == "equal":             # the shorter is a prefix of the longer
        s = rnd(rng, max(la, lb))
        return s[:la], s[:lb]
    if content == "homopolymer":       # the most ties
        return "A" * la, "A" * lb
    if content == "mismatch":
        return "A" * la, "C" * lb
    a = rnd(rng, la)
    b = (mutated(rng, a) + rnd(rng, lb))[:lb]
    if content == "one-N":             # N against a base, and (lengths of equal parity) N against N
        a = a[:la // 2] + "N" + a[la // 2 + 1:] if la else a
        if lb and (la + lb) % 2 == 0:
            b = b[:lb // 2] + "N" + b[lb // 2 + 1:]
    return a, b


def check_pair(ctx, a, b, max_cells=0, what=""):
    want = E.pair_ops(a, b, max_cells)
    ops, dist = ctx.test_edit_script(a, b, max_cells)
    assert np.array_equal(ops, want), (what, len(a), len(b), T.cigar_text(ops)[:80], E.cigar_text(want)[:80])
    cost = int((want[(want & 15) != E.OP_EQ] >> 4).sum())
    aligned = len(a) * len(b) <= (max_cells or E.DEFAULT_MAX_CELLS)
    assert dist == (cost if aligned else -1), (what, len(a), len(b), dist, cost)
    return want


def check_grid(ctx, sizes_a, sizes_b, content, seed):
    rng = np.random.default_rng(seed)
    for la in sizes_a:
        for lb in sizes_b:
            a, b = pair_of(content, la, lb, rng)
            check_pair(ctx, a, b, 0, content)


@pytest.mark.parametrize("content", CONTENTS)
def test_pairs_around_a_word_and_a_text_chunk(ctx, content):
    """0, 1 and one below, at and above 64 and 128 on each side, in all combinations: a pattern word is 64 positions, the
    text is consumed in chunks of 64 bases, the longer side is the pattern (both orders occur)."""
    sizes = (0, 1, 63, 64, 65, 127, 129)
    check_grid(ctx, sizes, sizes, content, 1)


@pytest.mark.parametrize("content", CONTENTS)
def test_pairs_where_the_delta_words_leave_lds(ctx, content):
    """edit_in_lds: at most 16 words per column and 4 * words * (shorter length) <= 1024.  128 x 128 is the largest
    square in LDS (2 words); with 3 words (129 .. 192 positions) the shorter side may have 85; with 16 words (1024
    positions) 16, and a 17th word is global whatever the other side."""
    for la, lb in ((127, 128), (128, 127), (128, 128), (129, 128), (128, 129)):
        check_grid(ctx, (la,), (lb,), content, 2)
    check_grid(ctx, (129, 192), (84, 85, 86), content, 3)
    check_grid(ctx, (84, 85, 86), (192,), content, 4)
    check_grid(ctx, (1023, 1024, 1025), (15, 16, 17), content, 5)
    check_grid(ctx, (16, 17), (1024, 1025), content, 6)


@pytest.mark.parametrize("content", CONTENTS)
def test_pairs_around_a_pattern_block(ctx, content):
    """A block is 4096 pattern positions (64 lanes of 64 bits); beyond it the blocks hand each other the horizontal
    deltas of their last row, one word of +1 and one of -1 per 64 text bases.  70 and 130 bases on the other side: two
    and three words of carries; 63, 64 and 65 against two and three blocks: where the number of carry words changes."""
    check_grid(ctx, (4095, 4096, 4097), (70,), content, 7)
    check_grid(ctx, (130,), (4095, 4096, 4097, 8193), content, 8)
    check_grid(ctx, (4097, 8193), (63, 64, 65), content, 9)
    check_grid(ctx, (63, 64, 65), (4097,), content, 10)


def test_the_largest_measured_pair_and_the_cap_at_its_product(ctx):
    rng = np.random.default_rng(9)
    a = rnd(rng, 1601)
    b = (mutated(rng, a) + rnd(rng, 1593))[:1593]
    want = check_pair(ctx, a, b, 0, "1601 x 1593")
    assert len(want) > 100
    assert np.array_equal(check_pair(ctx, a, b, 1601 * 1593, "at the cap"), want)
    un = check_pair(ctx, a, b, 1601 * 1593 - 1, "one below")
    assert un.tolist() == [1601 << 4 | E.OP_D, 1593 << 4 | E.OP_I]
    assert np.array_equal(check_pair(ctx, a, b, 1 << 62, "a cap beyond what the scratch holds acts as 1 << 29"), want)
    L = T.lib()
    n = np.zeros(1, dtype=np.uint64)
    ops = np.zeros(4, dtype=np.uint32)
    assert L.talc_test_edit_script(ctx._h, b"AAC", 3, b"ACA", 3, 0, ops.ctypes.data, 1, n.ctypes.data, None) == ERR_CAPACITY and int(n[0]) > 1


@contextlib.contextmanager
def corrected(ctx, bases, offs, on=True):
    """A fresh batch, corrected with the map on (or off)."""
    ctx.record_map(on)
    b = ctx.batch(bases, offs)
    try:
        b.rc = b.correct()
        yield b
    finally:
        b.close()
        ctx.record_map(False)


def args_of(b, reads):
    """What edits_ref.edits takes, from the batch itself."""
    segs, so = b.fetch_map()
    out, oo, st = b.fetch_corrected()
    return reads, segs, so, out, oo


def same(got, want, what):
    for g, w, n in zip(got, want, ("ops", "op_offsets", "rows")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), \
            (what, n, g.shape, w.shape, np.nonzero(g != w)[0][:6].tolist() if g.shape == w.shape else None)


def check(b, args, max_cells=0, what=""):
    want = E.edits(*args, max_cells=max_cells)
    got = b.edits(max_cells)
    same(got, want, (what, max_cells))
    assert int(T.lib().talc_batch_num_edit_ops(b._h)) == len(want[0])
    return want


@pytest.mark.parametrize("name", list(M.SETS))
def test_edits_equal_the_reference(name):
    s = M.map_set(name)
    with corrected(ctx_of(s), *s.packed()) as b:
        args = args_of(b, s.reads)
        full = check(b, args, 0, name)
        capped = check(b, args, 4096, name)
        assert full[2]["n_unaligned"].sum() == 0 and full[2]["n_mismatch"].sum() > 0 and full[2]["n_ins"].sum() > 0 and full[2]["n_del"].sum() > 0
        segs = args[1]
        c = segs[segs["kind"] == M.CORRECTED]
        cells = c["raw_len"].astype(np.int64) * c["out_len"]
        if name == "default":   # from the reference: the cap leaves some segments unaligned and aligns others
            assert int(capped[2]["n_unaligned"].sum()) == int((cells > 4096).sum()) > 0 and int(((cells > 0) & (cells <= 4096)).sum()) > 0
            segs_o, so_o, rec_o, ro_o, _ = P.from_expected(s.exp)   # ... and against the map rebuilt from the oracle's trace
            same(b.edits(0), E.edits(s.reads, segs_o, so_o, rec_o, ro_o), "oracle-derived")
        print(name, "= X I D", [int(full[2][f].sum()) for f in ("n_match", "n_mismatch", "n_ins", "n_del")], "ops", len(full[0]),
              "unaligned at 4096:", int(capped[2]["n_unaligned"].sum()), "ms", ctx_of(s).edits_timing())


def plan_of(segs, max_cells, budget_words):
    """(rounds, global pairs, the largest pair's words) of the host's planner (talc_edit_plan.h, through the host test
    library) over the CORRECTED segments of a map."""
    c = segs[segs["kind"] == M.CORRECTED]
    pairs = list(zip(c["raw_len"].tolist(), c["out_len"].tolist()))
    glob = [U.words(n, m) for n, m in pairs if n and m and n * m <= max_cells and not U.pure().pure_edit_in_lds(n, m)]
    return U.plan(pairs, max_cells, budget_words)[0], len(glob), max(glob)


def test_edits_in_several_rounds():
    """The k = 31 set has the largest pairs.  With a scratch budget of exactly the largest pair's words every global pair
    that does not fit beside its neighbours starts a round: the tasks of a round start at an offset into the task list,
    their words at 0.  Same result as with the full budget; one word less and that pair fits no round."""
    s = M.map_set("k31")
    with corrected(ctx_of(s), *s.packed()) as b:
        args = args_of(b, s.reads)
        want = check(b, args, 0, "one round")
        _, nglob, biggest = plan_of(args[1], E.DEFAULT_MAX_CELLS, 1 << 27)
        for budget in (8 * biggest, 24 * biggest):
            rounds = plan_of(args[1], E.DEFAULT_MAX_CELLS, budget // 8)[0]
            assert 2 <= rounds <= nglob, (budget, rounds, nglob)
            same(b.edits(0, scratch_bytes=budget), want, ("rounds", rounds))
            print("k31:", nglob, "global pairs, budget", budget, "bytes:", rounds, "rounds")
        assert T.lib().talc_test_batch_edits(ctx_of(s)._h, b._h, 0, 8 * biggest - 8) == ERR_INVALID
        same(b.edits(0), want, "after the rounds")


@pytest.mark.parametrize("graph", M.COMB_SETS)
def test_edits_of_reads_with_more_than_64_segments(graph):
    """The comb reads of the map tests (201 - 245 segments) and reads of 63, 65, 127 and 129 segments: where a pass of 64
    segments ends, with the open op carried across."""
    s = M.comb_set(graph)
    reads = s.reads + U.reads_with_regions(s, (31, 32, 63, 64))
    with corrected(ctx_of(s), *PU.pack_reads(reads)) as b:
        args = args_of(b, reads)
        nseg = np.diff(args[2].astype(np.int64)).tolist()
        assert nseg[-4:] == [63, 65, 127, 129] and min(nseg[:-4]) >= 201
        check(b, args, 0, graph)
        check(b, args, 300, graph)


def test_edits_of_passed_through_reads_and_of_the_empty_read():
    s0 = M.map_set("default")
    ctx = ctx_of(s0)
    reads = U.edge_reads(s0)
    with corrected(ctx, *PU.pack_reads(reads)) as b:
        args = args_of(b, reads)
        st = b.fetch_corrected()[2]
        assert st[0] == T.READ_SKIPPED_SHORT and (st == T.READ_NO_SOLID_KMER).any() and (st == T.READ_CORRECTED).any()
        ops, oo, rows = check(b, args, 0, "edge inputs")
        for i, r in enumerate(reads):
            if st[i] != T.READ_CORRECTED:
                assert ops[int(oo[i]):int(oo[i + 1])].tolist() == ([len(r) << 4 | E.OP_EQ] if r else [])
    with corrected(ctx, *PU.pack_reads([""])) as b:
        ops, oo, rows = b.edits()
        assert len(ops) == 0 and oo.tolist() == [0, 0] and rows.tolist() == [(0, 0, 0, 0, 0, 0)]
    s = M.map_set("reverse")   # under -rev a passed-through record is the reverse complement: still L '=', nothing compared
    reads = [M.revcomp(r) for r in reads]
    with corrected(ctx_of(s), *PU.pack_reads(reads)) as b:
        check(b, args_of(b, reads), 0, "edge inputs, reverse")


def test_edits_of_reads_that_failed(monkeypatch):
    """TALC_TEST_TINY_CAPS with TALC_TEST_FAIL_RETRY_ALLOC: reads end as TALC_READ_ERROR, one RAW segment each: L '='."""
    s = M.map_set("default")
    ctx_of(s)
    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "1")
    monkeypatch.setenv("TALC_TEST_FAIL_RETRY_ALLOC", "1")
    ctx2 = T.Context(s.pair.ttab, s.pair.p, 0)
    try:
        with corrected(ctx2, *s.packed()) as b:
            assert b.rc == T.WARN_READ_ERRORS
            st = b.fetch_corrected()[2]
            assert (st == T.READ_ERROR).any() and (st == T.READ_CORRECTED).any()
            ops, oo, rows = check(b, args_of(b, s.reads), 0, "failed reads")
            assert (rows["n_ops"][st == T.READ_ERROR] == 1).all() and rows["n_mismatch"].sum() > 0
    finally:
        ctx2.close()


def test_edit_calls_report_state_and_capacity():
    s = M.map_set("default")
    ctx = ctx_of(s)
    reads = s.reads[:20]
    bases, offs = PU.pack_reads(reads)
    L = T.lib()
    oo = np.zeros(21, dtype=np.uint64)
    rows = np.zeros(20, dtype=T.EDIT_ROW_DTYPE)

    def fetch(b, ops=None, cap=0, off=True, rw=True):
        return L.talc_batch_fetch_edits(ctx._h, b._h, None if ops is None else ops.ctypes.data, cap, oo.ctypes.data if off else None,
                                        rows.ctypes.data if rw else None)

    ctx.record_map(True)
    b = ctx.batch(bases, offs)
    try:
        assert L.talc_batch_edits(ctx._h, b._h, 0) == ERR_STATE                        # not corrected yet
        assert fetch(b) == ERR_STATE and L.talc_batch_num_edit_ops(b._h) == 0
        ctx.record_map(False)
        b.correct()
        assert L.talc_batch_edits(ctx._h, b._h, 0) == ERR_STATE                        # corrected without the map
        ctx.record_map(True)
        b.correct()
        assert fetch(b) == ERR_STATE                                                   # talc_batch_edits has not run
        assert L.talc_test_batch_edits(ctx._h, b._h, 0, 64) == ERR_INVALID and fetch(b) == ERR_STATE   # not a budget
        assert L.talc_batch_edits(ctx._h, b._h, 0) == 0
        want = E.edits(*args_of(b, reads))
        n = int(L.talc_batch_num_edit_ops(b._h))
        assert n == len(want[0]) > 20
        assert fetch(b) == 0 and np.array_equal(oo, want[1]) and np.array_equal(rows, want[2])   # offsets and rows only
        ops = np.zeros(n, dtype=np.uint32)
        assert fetch(b, ops, n - 1) == ERR_CAPACITY and str(n).encode() in L.talc_last_error()
        assert fetch(b, ops, n, False, False) == 0 and np.array_equal(ops, want[0])
        assert L.talc_batch_edits(ctx._h, b._h, 1 << 62) == 0 and L.talc_batch_num_edit_ops(b._h) == n   # acts as 1 << 29
        b.correct()                                                                    # a correction forgets the edits
        assert L.talc_batch_num_edit_ops(b._h) == 0 and fetch(b) == ERR_STATE
    finally:
        b.close()
        ctx.record_map(False)


def everything_else(ctx, b):
    segs, so = b.fetch_map()
    out, oo, st = b.fetch_corrected()
    msk, moo, mst = b.fetch_corrected(soft_mask=True)
    raw, cor = b.solidity()
    pieces = b.pieces(P.SPLIT, 30)
    return dict(segs=segs, so=so, out=out, oo=oo, st=st, msk=msk, moo=moo, mst=mst, raw=raw, cor=cor, pbytes=pieces[0], poff=pieces[1], pcs=pieces[2], rpo=pieces[3])


def test_edits_change_nothing_else_and_a_second_call_replaces_the_first():
    """A run with and a run without talc_batch_edits: records, statuses, map, masked records, solidity rows, pieces and
    work counters are equal; a second call with another cap replaces the first result."""
    s = M.map_set("reverse")
    ctx = ctx_of(s)
    reads = s.reads[:120]
    bases, offs = PU.pack_reads(reads)
    with corrected(ctx, bases, offs) as b:
        t = ctx.timing()
        plain = dict(everything_else(ctx, b), rc=b.rc, work=(t.n_trail_steps, t.n_dp_cells))
    with corrected(ctx, bases, offs) as b:
        args = args_of(b, reads)
        first = check(b, args, 0, "first")
        second = check(b, args, 2000, "second")                     # replaces the first
        assert second[2]["n_unaligned"].sum() > 0 and len(second[0]) != len(first[0])
        t = ctx.timing()
        after = dict(everything_else(ctx, b), rc=b.rc, work=(t.n_trail_steps, t.n_dp_cells))
        same(b.edits(0), first, "after the other reports")
        assert all(a >= 0 for a in ctx.edits_timing())
    assert plain["work"] == after["work"] and plain["work"][0] > 0 and plain["rc"] == after["rc"]
    for k in plain:
        if k not in ("rc", "work"):
            assert np.array_equal(plain[k], after[k]), k


def cli(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_cli_edits_file(tmp_path, rev):
    """Several --batch-reads batches: <o>.edits.tsv against the reference's text over the oracle-derived maps, the summary
    line's sums, and every other file against a run without the option."""
    S = Synth(target_kmers=150_000, k=21, seed=77)
    S.write_dump(str(tmp_path / "sr.dump"))
    S.write_fasta(str(tmp_path / "reads.fa"), 0, 60)
    lines = (tmp_path / "reads.fa").read_text().splitlines()
    names, reads = [x[1:] for x in lines[0::2]], lines[1::2]
    if rev:   # (k-mers are directional: -rev corrects the reads of the opposite strand)
        reads = [M.revcomp(r) for r in reads]
        (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, reads)))
    pair = PU.Pair(target_kmers=150_000, k=21, seed=77, reverse=int(rev))
    exp = [M.expected(pair.otab, r) for r in reads]
    segs, so, rec, ro, _ = P.from_expected(exp)
    status = [e["status"] for e in exp]
    seen = [rev and st != 0 for st in status]
    CAP = 3000
    result = E.edits(reads, segs, so, rec, ro, CAP)
    assert 0 < int(result[2]["n_unaligned"].sum())
    args = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7"] + (["-rev"] if rev else [])
    a = cli(args + ["--corr-edits", "--max-edit-cells", str(CAP), "-o", "ed"], tmp_path)
    p = cli(args + ["-o", "plain"], tmp_path)
    assert a.returncode == 0 and p.returncode == 0, (a.stderr.decode(), p.stderr.decode())
    got = (tmp_path / "ed.edits.tsv").read_text().split("\n")
    assert got[0].startswith("read_name\tstatus\t") and got[-1] == ""
    assert got[1:-1] == E.tsv_lines(names, reads, status, ro, result, seen)
    for ext in (".fa", ".log", ".stats_basics.txt"):
        fa, fp = tmp_path / ("ed" + ext), tmp_path / ("plain" + ext)
        assert fa.exists() == fp.exists() and (not fa.exists() or fa.read_bytes() == fp.read_bytes()), ext
    assert (tmp_path / "ed.config.txt").read_bytes().replace(b"ed", b"plain") == (tmp_path / "plain.config.txt").read_bytes().replace(b"ed", b"plain")
    assert not (tmp_path / "plain.edits.tsv").exists() and not (tmp_path / "ed.map.tsv").exists()
    ok = np.asarray(status) == 0
    rows = result[2]
    line = "[TALC]: edits: %d matches, %d mismatches, %d insertions, %d deletions in %d corrected reads (%d segments not aligned)" % (
        int(rows["n_match"][ok].sum()), int(rows["n_mismatch"][ok].sum()), int(rows["n_ins"][ok].sum()), int(rows["n_del"][ok].sum()), int(ok.sum()),
        int(rows["n_unaligned"].sum()))
    out_a, out_p = a.stdout.decode().splitlines(), p.stdout.decode().splitlines()
    assert line in out_a and [l for l in out_a if l != line] == [l.replace("plain.fa", "ed.fa") for l in out_p]
    # with the other reports: their files are those of a run without --corr-edits, and the edits at the default cap
    m = cli(args + ["--corr-edits", "--soft-mask", "--corr-map", "--solidity", "--split", "-o", "all"], tmp_path)
    q = cli(args + ["--soft-mask", "--corr-map", "--solidity", "--split", "-o", "rest"], tmp_path)
    assert m.returncode == 0 and q.returncode == 0, (m.stderr.decode(), q.stderr.decode())
    for ext in (".fa", ".map.tsv", ".solidity.tsv", ".split.fa", ".log"):
        fa, fq = tmp_path / ("all" + ext), tmp_path / ("rest" + ext)
        assert fa.exists() == fq.exists() and (not fa.exists() or fa.read_bytes() == fq.read_bytes()), ext
    assert (tmp_path / "all.edits.tsv").read_text().split("\n")[1:-1] == E.tsv_lines(names, reads, status, ro, E.edits(reads, segs, so, rec, ro), seen)
