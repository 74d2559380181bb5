"""No result may depend on what device memory held before, and no kernel may write outside its buffers.  The suites' own
references run again under the hooks of talc_devmem.h (lib.poisoned: every device buffer the library hands out, fresh or from
a context's cache, starts as a pattern byte over its whole capacity and sits between red zones that are checked when it is
given back; the search scratch, the edge boxes and a retry stage are poisoned before every launch).  "Corrected in one batch"
below means: on an unpoisoned fresh context, which is the result the other suites pin to the references.  Integers and bytes,
tolerance 0.  What the hooks cannot see: a read past a red zone, a stray write inside the same buffer."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import corr_map_ref as M
import dump_cases as DC
import dump_ref as D
import edits_ref as E
import kmer_ref as KR
import oracle_lib as O
import parity_util as PU
import solidity_ref as S
import strand_ref as R
import test_gpu_edits as GE
from memcheck_util import BACKWARD, PATTERNS, TEXT_PATTERNS, everything, fetch_all, first_difference, guards_checked, per_read
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ids = lambda b: "0x%02X" % b


# ---------------------------------------------------------------- 1. the instrument
@pytest.mark.parametrize("byte", PATTERNS, ids=ids)
@pytest.mark.parametrize("guard", [256, 1024])
def test_the_self_test_reads_its_fills_back_and_finds_its_two_writes(byte, guard):
    before = T.guard_report()
    with T.poisoned(byte, guard):
        r = T.guard_selftest()
    assert r["fills"] == 15, r                       # both buffers: every byte the poison (the cached one's slack too), every guard byte ~poison
    assert r["violations"] == 2, r
    assert r["behind"] == (1, 0), r                  # one byte just past the end of the first buffer
    assert r["in_front"] == (0, guard - 1), r        # ... and one just before the start of the second
    assert T.guard_report() == before                # the planted writes are the self test's own, not the product's


def test_with_the_setting_off_the_report_does_not_move_and_the_self_test_refuses(gpu_pair):
    before = T.guard_report()
    assert T.poison_setting() == (-1, 0)
    ctx = T.Context(gpu_pair.ttab, gpu_pair.p, 0)
    try:
        for _ in range(2):                           # (the second batch takes the first one's buffers from the cache)
            ctx.correct(*gpu_pair.reads(0, 20))
    finally:
        ctx.close()
    assert T.guard_report() == before
    with pytest.raises(T.TalcError):
        T.guard_selftest()
    with T.poisoned(0xA5, 0):                        # poison without red zones: nothing to check, nothing to plant
        with pytest.raises(T.TalcError):
            T.guard_selftest()
    assert T.guard_report() == before


def test_a_buffer_made_under_one_setting_is_given_back_under_another(gpu_pair):
    with guards_checked():
        with T.poisoned(0xA5, 512):
            ctx = T.Context(gpu_pair.ttab, gpu_pair.p, 0)
            b = ctx.batch(*gpu_pair.reads(0, 20))
        try:
            b.correct()                              # setting off: the batch's later buffers are plain ones, from the same cache
            got = b.fetch_corrected()
            with T.poisoned(0x00, 256):
                b2 = ctx.batch(*gpu_pair.reads(0, 20))
                b2.correct()
                got2 = b2.fetch_corrected()
                b2.close()
        finally:
            b.close()
            ctx.close()
        want = gpu_pair.ctx.correct(*gpu_pair.reads(0, 20))
        for g in (got, got2):
            assert all(np.array_equal(x, y) for x, y in zip(g, want))


# ---------------------------------------------------------------- 2. whole pipeline, every output
# The three sets of the issue, and the no-structure set of test_gpu_solidity.py beside them: under the three sets' parameters
# the reference cannot leave a read without a structure (findINRegions finds a region wherever reCoverage found an IN k-mer,
# analyzeINRegions keeps its input when it drops every region, and the structure of unchanged regions always adds up to the
# read), so READ_NO_STRUCTURE is asserted where the reference produces it: SR_ERROR_RATE 1.5.
PIPE_SETS = {
    "default": M.SETS["default"][:5], "k31": M.SETS["k31"][:5], "paralog-maxb4": M.SETS["paralog-maxb4"][:5],
    "no-structure": (60_000, 22, 403, dict(paralog_frac=0.4, paralog_div=0.03), dict(sr_error_rate=1.5, alpha=0.5, min_count=5)),
}
_pipe = {}


def oracle_runs(pair, k, kw, bases, offs):
    """[(records, status)] of the oracle with reverse = 0 and 1."""
    runs = []
    for reverse in (0, 1):
        p, q = PU.both_params(k=k, reverse=reverse, **kw)
        ot = O.OracleTable(q, O.OracleTable.FLAT)
        ot.insert_packed(pair.keys, pair.counts)
        ot.decolour()
        out, oo, st = ot.correct_batch(bases, offs, nthreads=16)
        runs.append((PU.seqs_of(out, oo), np.asarray(st).tolist()))
        ot.close()
    return runs


def pipe_set(name):
    """Reads (200 of the generator, every second one reverse complemented, and hand reads), the oracle's records in both
    orientations, the orientation strand_ref chooses, and everything an unpoisoned fresh context gives, plain and auto
    strand (computed once, shared, left unchanged)."""
    if name not in _pipe:
        target, k, seed, synth_kw, kw = PIPE_SETS[name]
        pair = PU.Pair(target_kmers=target, k=k, seed=seed, synth_kw=synth_kw, **kw)
        pair.ttab.upload(0)
        r = PU.seqs_of(*pair.reads(0, 200))
        reads = [PU.revcomp(s) if i % 2 else s for i, s in enumerate(r)]
        reads += ["", r[0][:k], r[2][:k + 1], "ACGT" * 200, "N" * 80, "".join(random.Random(5).choice("ACGT") for _ in range(900))]
        bases, offs = PU.pack_reads(reads)
        runs = oracle_runs(pair, k, kw, bases, offs)
        rows = R.rows(reads, k, pair.p.min_count, S.host_lookup(pair.ttab))
        fresh = {}
        for auto in (False, True):
            ctx = T.Context(pair.ttab, pair.p, 0)
            ctx.auto_strand(auto)
            try:
                fresh[auto] = everything(ctx, reads)
            finally:
                ctx.close()
        _pipe[name] = dict(pair=pair, k=k, reads=reads, runs=runs, rows=rows, fresh=fresh)
    return _pipe[name]


@pytest.mark.parametrize("name", list(PIPE_SETS))
def test_the_pipeline_sets_reach_every_status_by_the_oracle_alone(name):
    s = pipe_set(name)
    k, lens = s["k"], [len(x) for x in s["reads"]]
    st = s["runs"][0][1]
    assert st.count(T.READ_CORRECTED) >= 50, np.bincount(st, minlength=5).tolist()
    assert st.count(T.READ_SKIPPED_SHORT) >= 1 and st.count(T.READ_NO_SOLID_KMER) >= 1
    assert lens.count(0) == 1 and lens.count(k) == 1 and st[lens.index(0)] == st[lens.index(k)] == T.READ_SKIPPED_SHORT
    both = st + s["runs"][1][1]
    if name == "no-structure":
        assert both.count(T.READ_NO_STRUCTURE) >= 1
    nrev = int(s["rows"]["reverse"].sum())
    assert nrev >= 50 and len(lens) - nrev >= 50      # the auto-strand context turns a quarter of the reads at least


def test_some_pipeline_set_has_reads_without_a_structure():
    s = pipe_set("no-structure")
    n = [run[1].count(T.READ_NO_STRUCTURE) for run in s["runs"]]
    assert min(n) >= 1, n
    chosen = [s["runs"][int(rv)][1][i] for i, rv in enumerate(s["rows"]["reverse"])]
    assert chosen.count(T.READ_NO_STRUCTURE) >= 1


@pytest.mark.parametrize("byte", PATTERNS, ids=ids)
@pytest.mark.parametrize("name", list(PIPE_SETS))
def test_every_output_of_a_poisoned_context_equals_the_oracle_and_a_fresh_context(name, byte):
    s = pipe_set(name)
    reads, n = s["reads"], len(s["reads"])
    with guards_checked():
        for auto in (False, True):
            with T.poisoned(byte):
                ctx = T.Context(s["pair"].ttab, s["pair"].p, 0)
                ctx.auto_strand(auto)
                try:
                    per, work, rows = everything(ctx, reads)
                finally:
                    ctx.close()
            for i in range(n):                        # records and status: the oracle's, in the orientation strand_ref chooses
                recs, st = s["runs"][int(s["rows"]["reverse"][i]) if auto else 0]
                assert per[i][0].decode() == recs[i] and per[i][1] == st[i], (name, byte, auto, i)
            want, want_work, want_rows = s["fresh"][auto]
            assert first_difference(per, want) is None, (name, byte, auto, first_difference(per, want))
            assert work[0] == want_work[0] and work[3:] == want_work[3:], (name, byte, auto, work, want_work)   # (return code, k-mers, bases, retried, failed)
            if auto:
                assert np.array_equal(rows, s["rows"]) and np.array_equal(want_rows, s["rows"])


# ---------------------------------------------------------------- 3. one context, recycled buffers
_recycle = {}


def recycle_inputs():
    if not _recycle:
        pair = PU.Pair(target_kmers=250_000, k=21, seed=77, synth_kw=dict(paralog_frac=0.6, paralog_div=0.04))
        pair.ttab.upload(0)
        seqs = PU.seqs_of(*pair.reads(0, 240))
        hand = ["", seqs[0][:20], seqs[1][:21], seqs[2][:22], "ACGT" * 5, "N" * 12, seqs[3][:7], "A"]
        reads = seqs + hand
        ctx = T.Context(pair.ttab, pair.p, 0)
        try:
            want = everything(ctx, reads, batch_free=True)[0]
        finally:
            ctx.close()
        # K = 31: one read of 15 to 20 kb among 30 short ones, a table and a context of its own
        big = PU.Pair(target_kmers=600_000, k=31, seed=43, synth_kw=dict(mixed_lengths=1))
        big.ttab.upload(0)
        cand = PU.seqs_of(*big.reads(0, 200))
        order = sorted(range(len(cand)), key=lambda i: len(cand[i]))
        big_reads = [cand[i] for i in order[:15]] + [cand[order[-1]]] + [cand[i] for i in order[15:30]]
        assert len(cand[order[-1]]) >= 15000 and len(cand[order[29]]) < 2000
        ctx = T.Context(big.ttab, big.p, 0)
        try:
            big_want = everything(ctx, big_reads, batch_free=True)[0]
        finally:
            ctx.close()
        _recycle.update(pair=pair, reads=reads, want=want, nset=len(seqs), big=big, big_reads=big_reads, big_want=big_want)
    return _recycle


@pytest.mark.parametrize("byte", PATTERNS, ids=ids)
def test_one_poisoned_context_over_batches_that_take_each_others_buffers(byte):
    s = recycle_inputs()
    reads, want, nset = s["reads"], s["want"], s["nset"]
    order = sorted(range(nset), key=lambda i: len(reads[i]))
    below_k = [i for i in range(len(reads)) if len(reads[i]) < 21]
    assert len(below_k) >= 5 and 0 in [len(reads[i]) for i in below_k]

    def same(got, idx, what):
        d = first_difference(got, [want[i] for i in idx])
        assert d is None, (byte, what, d, None if d is None else idx[d[0]] if d[0] < len(idx) else None)

    def whole(ctx, idx, what, order_=None):
        kw = dict(order=order_) if order_ else {}
        same(everything(ctx, [reads[i] for i in idx], batch_free=True, **kw)[0], idx, what)

    with guards_checked() as before:
        with T.poisoned(byte):
            ctx = T.Context(s["pair"].ttab, s["pair"].p, 0)
            big_ctx = T.Context(s["big"].ttab, s["big"].p, 0)
            try:
                for rep in range(2):
                    whole(ctx, order[:60], (rep, "the 60 shortest"))
                    whole(ctx, order[-60:], (rep, "the 60 longest"))
                    whole(ctx, [order[100]], (rep, "one read"))
                    whole(ctx, [], (rep, "no read"))
                    whole(ctx, below_k, (rep, "every read shorter than K"))
                    d = first_difference(everything(big_ctx, s["big_reads"], batch_free=True)[0], s["big_want"])
                    assert d is None, (byte, rep, "K = 31, one long read among short ones", d)
                    # two live batches, as the command line's workers have them
                    ia, ib, ic = order[60:90], order[150:200], order[90:120]
                    ctx.record_map(True)
                    a = ctx.batch(*PU.pack_reads([reads[i] for i in ia]))
                    b = ctx.batch(*PU.pack_reads([reads[i] for i in ib]))
                    c = None
                    try:
                        b.correct()
                        a.correct()
                        fa = per_read(fetch_all(a), len(ia), batch_free=True)
                        a.close()
                        c = ctx.batch(*PU.pack_reads([reads[i] for i in ic]))       # (gets a's buffers)
                        fb = per_read(fetch_all(b), len(ib), batch_free=True)
                        c.correct()
                        fc = per_read(fetch_all(c), len(ic), batch_free=True)
                    finally:
                        for x in (a, b, c):
                            if x is not None:
                                x.close()
                    same(fa, ia, (rep, "batch A of two"))
                    same(fb, ib, (rep, "batch B of two"))
                    same(fc, ic, (rep, "batch C in A's buffers"))
                    # corrected twice (the record buffer is kept), outputs asked for backwards
                    idx = order[120:150]
                    b = ctx.batch(*PU.pack_reads([reads[i] for i in idx]))
                    try:
                        b.correct()
                        b.fetch_corrected()
                        b.correct()
                        same(per_read(fetch_all(b, BACKWARD), len(idx), batch_free=True), idx, (rep, "corrected twice, fetched backwards"))
                    finally:
                        b.close()
                    whole(ctx, order[200:240], (rep, "fetched backwards"), BACKWARD)
                    # the map off, then on again; auto strand toggled between coverage() and correct()
                    idx = order[30:80]
                    ctx.record_map(False)
                    out, oo, st = ctx.correct(*PU.pack_reads([reads[i] for i in idx]))
                    out = bytes(out)
                    for j, i in enumerate(idx):
                        assert (out[int(oo[j]):int(oo[j + 1])], int(st[j])) == want[i][:2], (byte, rep, "map off", i)
                    ctx.record_map(True)
                    b = ctx.batch(*PU.pack_reads([reads[i] for i in idx]))
                    try:
                        ctx.auto_strand(True)
                        b.coverage()
                        ctx.auto_strand(False)
                        b.correct()
                        same(per_read(fetch_all(b), len(idx), batch_free=True), idx, (rep, "auto strand on for the coverage only"))
                    finally:
                        b.close()
                        ctx.auto_strand(False)
                        ctx.record_map(False)
            finally:
                ctx.close()
                big_ctx.close()
        # reuse really happened: the caches served requests with buffers used before (a batch with every output asks for more
        # than 40 buffers, and the second pass over the sequence finds the first one's)
        reused = T.guard_report()["reused"] - before["reused"]
        print("requests served from the caches:", reused)
        assert reused >= 50, reused


# ---------------------------------------------------------------- 4. the search under every switch that changes what it allocates
SWITCHES = {
    "retry-stage": dict(TALC_TEST_TINY_CAPS="1"),
    "edge-boxes": dict(TALC_EDGE_TASKS="1"),
    "edge-redo": dict(TALC_EDGE_TASKS="1", TALC_EDGE_TASK_MIN="0", TALC_TEST_EDGE_REDO="1"),
    "no-walk-tables": dict(TALC_WALK="0"),
    "no-edge-lane": dict(TALC_TEST_EDGE_LANE="0"),
    "three-slots": dict(TALC_SEARCH_SLOTS="3"),
}
_search = {}


def search_inputs():
    if not _search:
        pair = PU.Pair(target_kmers=250_000, k=21, seed=77, synth_kw=dict(paralog_frac=0.6, paralog_div=0.04))
        pair.ttab.upload(0)
        bases, offs = pair.reads(0, 200)
        out, oo, st = pair.otab.correct_batch(bases, offs, nthreads=16)
        _search.update(pair=pair, bases=bases, offs=offs, want=PU.seqs_of(out, oo), st=np.asarray(st))
    return _search


@pytest.mark.parametrize("byte", PATTERNS, ids=ids)
@pytest.mark.parametrize("case", list(SWITCHES))
def test_the_search_under_a_switch_equals_the_oracle(case, byte, monkeypatch):
    s = search_inputs()
    pair = s["pair"]
    for name, value in SWITCHES[case].items():
        monkeypatch.setenv(name, value)
    with guards_checked():
        with T.poisoned(byte):
            table = pair.ttab
            if case == "no-walk-tables":             # (a table switch: read by the upload)
                table = T.Table.from_arrays(pair.keys, pair.counts, pair.p)
                table.decolour_repeats()
                table.upload(0)
                assert 0 < table.device_bytes < pair.ttab.device_bytes
            ctx = T.Context(table, pair.p, 0)
            try:
                for rep in range(2):                 # (the second launch finds the first one's scratch, poisoned again)
                    out, oo, st = ctx.correct(s["bases"], s["offs"])
                    t = ctx.timing()
                    assert t.n_failed == 0
                    assert PU.seqs_of(out, oo) == s["want"] and np.array_equal(st, s["st"]), (case, byte, rep)
                    if case == "retry-stage":
                        assert t.n_retried >= 1
            finally:
                ctx.close()
                if table is not pair.ttab:
                    table.close()


# ---------------------------------------------------------------- 5. DP primitives
def dp_pairs():
    """(mode, a, b, p0 .. p3, what the oracle or the routine itself expects) as the four tests of test_gpu_parity.py make
    their pairs, ten of each."""
    L = O.lib()
    cases = []
    rnd = random.Random(97)                          # rows continued (mode 7): the kept row against the alignment from scratch
    for n in [30, 64, 65, 129, 260, 770, 2047, 2048, 4096, 8191]:
        ref = [rnd.choice("ACGT") for _ in range(n)]
        cand = []
        for ch in ref[: min(n, 700)]:
            x = rnd.random()
            if x < 0.05:
                cand.append(rnd.choice("ACGT"))
            elif x < 0.10:
                cand += [ch, rnd.choice("ACGT")]
            elif x >= 0.15:
                cand.append(ch)
        cand += [rnd.choice("ACGT") for _ in range(15)]
        step = rnd.choice([1, 3, 6, 6, 9]) if n <= 260 else rnd.choice([6, 9, 17])
        first = 21 if len(cand) < 70 else rnd.choice([21, 70])
        cases.append(("rows", 7, "".join(ref), "".join(cand), (first, 0, step, rnd.choice([5, 10, 15])), None))
    rnd = random.Random(44)                          # seed and extension beyond x = 255 (mode 1)
    for it in range(5):
        n = rnd.choice([400, 700, 1000, 1300, 1700])
        ref = [rnd.choice("ACGT") for _ in range(n)]
        cand = list(ref[: rnd.randint(300, min(n, 1300))])
        for _ in range(rnd.choice([0, 1, 3, 10, 40])):
            p = rnd.randrange(len(cand))
            x = rnd.random()
            if x < 0.4:
                cand[p] = rnd.choice("ACGT")
            elif x < 0.7:
                cand.insert(p, rnd.choice("ACGT"))
            elif len(cand) > 25:
                del cand[p]
        ref, cand = "".join(ref), "".join(cand)
        xdrop = rnd.randint(256, 511) if it else rnd.randint(512, 700)
        for direction in (0, 1):
            out = np.zeros(3, dtype=np.int64)
            stop = C.c_int32()
            sc = L.orc_seed_and_extension(ref.encode(), cand.encode(), xdrop, direction, 21, out.ctypes.data, C.byref(stop))
            a, b = (ref, cand) if direction else (ref[::-1], cand[::-1])
            cases.append(("xdrop", 1, a, b, (xdrop, direction, 0, 0), (int(out[0]), int(out[1]), int(out[2]), int(sc), stop.value)))
    rnd = random.Random(17)                          # kept wavefront (mode 8): every scoring against the extension from level 0
    for it in range(5):
        n = rnd.randint(120, 700)
        ref = "".join(rnd.choice("ACGT") for _ in range(n))
        cand = "".join(ch if rnd.random() > (0.1 if it % 2 else 0.02) else rnd.choice("ACGT") for ch in ref)
        cand = (ref[:21] + cand[21:])[:600]
        step = rnd.choice([1, 3, 6, 11])
        for dir_right in (1, 0):
            cases.append(("wavefront", 8, ref, cand, (21 + step, dir_right, step, rnd.choice([2, 3, 5])), None))
    rnd = random.Random(131)                         # edit distance and LCS beyond 4096 columns (mode 4)
    for n, m in [(4096, 4096), (4097, 4096), (8193, 5000), (9000, 9400), (13001, 700)]:
        a = "".join(rnd.choice("ACGTN" if rnd.random() < 0.05 else "ACGT") for _ in range(n))
        b = "".join(ch if rnd.random() > 0.15 else rnd.choice("ACGT") for ch in a)
        b = (b + "".join(rnd.choice("ACGT") for _ in range(max(0, m - len(b)))))[:m]
        exp_e = L.orc_global_alignment(a.encode(), b.encode(), 0, -1, -1, 0, 0, 0, 0)
        exp_l = L.orc_global_alignment(a.encode(), b.encode(), 1, 0, 0, 0, 0, 0, 0)
        cases += [("blocks", 4, a, b, (0, 0, 0, 0), (exp_e, exp_l)), ("blocks", 4, b, a, (0, 0, 0, 0), (exp_e, exp_l))]
    return cases


_dp = []


@pytest.mark.parametrize("byte", PATTERNS, ids=ids)
def test_dp_primitives_on_a_poisoned_context(gpu_pair, byte):
    if not _dp:
        _dp.extend(dp_pairs())
    assert [sum(1 for c in _dp if c[0] == w) for w in ("rows", "xdrop", "wavefront", "blocks")] == [10, 10, 10, 10]
    with guards_checked():
        with T.poisoned(byte):
            ctx = T.Context(gpu_pair.ttab, gpu_pair.p, 0)
            try:
                for what, mode, a, b, (p0, p1, p2, p3), want in _dp:
                    got = ctx.test_dp(mode, a, b, p0, p1, p2, p3)
                    where = (what, byte, len(a), len(b), p0, p1, p2, p3, got[:6].tolist())
                    if what == "rows":
                        assert got[5] == 0 and got[0] > 0 and got[1] == 0, where
                    elif what == "xdrop":
                        assert got[5] == 0 and tuple(got[:5].tolist()) == want, where
                    elif what == "wavefront":
                        assert got[0] > 0 and got[1] == 0, where
                    else:
                        assert got[5] == 0 and (got[0], got[1]) == want, where
            finally:
                ctx.close()


# ---------------------------------------------------------------- 6. edit scripts through the global scratch
_edits = {}


def edit_inputs():
    if not _edits:
        s = M.map_set("k31")
        if s.pair.ctx is None:
            s.pair.upload(0)
        with GE.corrected(s.pair.ctx, *s.packed()) as b:
            args = GE.args_of(b, s.reads)
            args = (args[0], args[1].copy(), args[2].copy(), args[3].copy(), args[4].copy())
        _, nglob, biggest = GE.plan_of(args[1], E.DEFAULT_MAX_CELLS, 1 << 27)
        budget = 8 * biggest
        rounds = GE.plan_of(args[1], E.DEFAULT_MAX_CELLS, budget // 8)[0]
        assert 2 <= rounds <= nglob
        rng = np.random.default_rng(23)
        pairs = [GE.pair_of(content, la, lb, rng) for content in ("edits", "one-N") for la in (127, 128, 129) for lb in (127, 128, 129)]
        a = GE.rnd(rng, 3000)
        pairs.append((a, (GE.mutated(rng, a) + GE.rnd(rng, 2900))[:2900]))
        assert (len(pairs[-1][0]), len(pairs[-1][1])) == (3000, 2900)
        _edits.update(set=s, args=args, want=E.edits(*args), budget=budget, pairs=pairs, ops=[E.pair_ops(x, y) for x, y in pairs])
    return _edits


@pytest.mark.parametrize("byte", PATTERNS, ids=ids)
def test_edit_scripts_in_several_rounds_and_around_the_lds_limit(byte):
    e = edit_inputs()
    s = e["set"]
    with guards_checked():
        with T.poisoned(byte):
            ctx = T.Context(s.pair.ttab, s.pair.p, 0)
            try:
                with GE.corrected(ctx, *s.packed()) as b:
                    got = GE.args_of(b, s.reads)
                    for g, w in zip(got[1:], e["args"][1:]):          # the map and the records the reference was fed with
                        assert np.array_equal(g, w), byte
                    GE.same(b.edits(0, scratch_bytes=e["budget"]), e["want"], ("rounds", byte))
                    GE.same(b.edits(0), e["want"], ("one round", byte))
                for (x, y), want in zip(e["pairs"], e["ops"]):
                    ops, dist = ctx.test_edit_script(x, y)
                    assert np.array_equal(ops, want), (byte, len(x), len(y), T.cigar_text(ops)[:80], E.cigar_text(want)[:80])
                    assert dist == int((want[(want & 15) != E.OP_EQ] >> 4).sum()), (byte, len(x), len(y))
            finally:
                ctx.close()


# ---------------------------------------------------------------- 7. tables
def image_of(t):
    """Both bucket tables as exported (a staged or an uploaded image), host copies."""
    img = PU.DeviceImage(t)
    img.free()
    return img.right, img.left


def derived_of(t):
    """After an upload: both walk tables.  (The presence filter has no fetch hook: it is cleared before it is built, and
    every pipeline test of this file reads it through k_coverage.)"""
    return t.fetch_walk(0), t.fetch_walk(1)


def canonical(records):
    """The records of a table as a sorted multiset.  The device builder's claim kernel gives a slot to whichever thread's CAS
    comes first, so two builds of one dump may place the keys of a probe chain in another order: which buckets exist and what
    they hold is compared byte for byte, where they sit is pinned by the lookups against the oracle."""
    flat = np.ascontiguousarray(records).view(np.dtype((np.void, records.dtype.itemsize)))
    return np.sort(flat).tobytes()


def same_table(t, ref, what, uploaded=True):
    r, l = image_of(t)
    assert canonical(r) == canonical(ref["right"]) and canonical(l) == canonical(ref["left"]), (what, "buckets")
    if uploaded:
        w0, w1 = derived_of(t)
        assert canonical(w0) == canonical(ref["walk"][0]) and canonical(w1) == canonical(ref["walk"][1]), (what, "walk tables")


def snapshot(t, uploaded=True):
    r, l = image_of(t)
    return dict(right=r, left=l, walk=derived_of(t) if uploaded else None)


def queries(keys, k, n_absent=1000):
    rng = np.random.default_rng(3)
    absent = rng.integers(0, 1 << (2 * k), n_absent, dtype=np.uint64)
    return np.concatenate([np.asarray(keys, dtype=np.uint64), absent])


def oracle_answers(otab, keys, k):
    """The oracle's lookup and successor counts of every stored key and 1000 absent ones (computed once per table)."""
    q = queries(keys, k)
    nxt = []
    for direction in (0, 1):
        rows = [otab.next_counts(KR.unpack(x, k), direction) for x in q.tolist()]
        nxt.append((np.array([r[0] for r in rows], dtype=np.uint32), np.array([r[1] for r in rows], dtype=np.uint32)))
    return dict(q=q, lookup=otab.lookup_packed(q), next=nxt)


def against_the_oracle(t, ans, what):
    gc, gj = t.lookup(ans["q"])
    assert np.array_equal(ans["lookup"][0], gc) and np.array_equal(ans["lookup"][1], gj), (what, "lookup")
    for direction in (0, 1):
        gc, gj = t.next_counts(ans["q"], direction)
        assert np.array_equal(ans["next"][direction][0], gc) and np.array_equal(ans["next"][direction][1], gj), (what, "next_counts", direction)


_tab = {}


def table_inputs():
    """A 60 k-k-mer dump with junction lines at, above and below the colour threshold; the oracle's table and the unpoisoned
    device builds of it, before and after the upload."""
    if not _tab:
        k = 21
        syn = Synth(target_kmers=60_000, k=k, seed=9)
        keys, counts = syn.dump_arrays()
        p, q = PU.both_params(k=k, use_junctions=1)
        rng = np.random.default_rng(12)
        jk = rng.choice(keys, 300, replace=False)
        thr = p.coloured_count_thr
        jc = rng.choice(np.asarray([thr - 1, thr, thr + 1, 1, 5 * thr], dtype=np.int64), 300)
        otab = O.OracleTable(q, O.OracleTable.FLAT)
        otab.insert_packed(keys, counts)
        otab.colour_packed(jk, jc)
        otab.decolour()
        t = T.Table.from_arrays(keys, counts, p, device=0)
        plain = snapshot(t, uploaded=False)
        t.colour(jk, jc)
        coloured = snapshot(t, uploaded=False)
        t.decolour_repeats()
        t.upload(0)
        ans = oracle_answers(otab, keys, k)
        assert int((ans["lookup"][0] >= p.min_count).sum()) > 50_000 and int((ans["lookup"][0] == 0).sum()) >= 1000
        assert int((ans["lookup"][1] > 0).sum()) >= 100          # coloured k-mers
        otab.close()
        _tab.update(k=k, p=p, keys=keys, counts=counts, jk=jk, jc=jc, ans=ans, plain=plain, coloured=coloured, final=snapshot(t), table=t)
    return _tab


@pytest.mark.parametrize("byte", TEXT_PATTERNS, ids=ids)
def test_the_device_builder_colouring_and_export_import_under_poison(byte):
    s = table_inputs()
    k, p = s["k"], s["p"]
    with guards_checked():
        with T.poisoned(byte):
            t = T.Table.from_arrays(s["keys"], s["counts"], p, device=0)
            same_table(t, s["plain"], (byte, "built"), uploaded=False)
            t.colour(s["jk"], s["jc"])
            same_table(t, s["coloured"], (byte, "coloured"), uploaded=False)
            t.decolour_repeats()
            t.upload(0)
            same_table(t, s["final"], (byte, "uploaded"))
            against_the_oracle(t, s["ans"], (byte, "uploaded"))
            # export, then import: a second table from the first one's image
            img = PU.DeviceImage(t)
            try:
                t2 = T.Table.import_device(p, t.capacity, len(t), img.right_ptr.value, img.left_ptr.value, 0)
            finally:
                img.free()
            t2.upload(0)
            same_table(t2, s["final"], (byte, "imported"))
            against_the_oracle(t2, s["ans"], (byte, "imported"))
            t2.close()
            t.close()


_dumps = {}


def dump_inputs(tmp):
    """The files of dump_cases' case D whose sizes are 64 n, 16384 n and 16384 n + 1 bytes, and the one-line file: the lines by
    the reference parser, the oracle's answers, and the unpoisoned build."""
    if not _dumps:
        k = 21
        p, q = PU.both_params(k=k)
        lays = DC.case_d(k)
        assert [len(lays[n].data) % m for n, m in (("multiple-of-64", 64), ("multiple-of-tile", 16384), ("tile-plus-one", 16384))] == [0, 0, 1]
        for name in ("one-line", "multiple-of-64", "multiple-of-tile", "tile-plus-one"):
            data = lays[name].data
            path = DC.write(tmp / (name + ".txt"), data)
            km, ct, flagged = D.parse(data, k)
            assert not flagged
            otab = O.OracleTable(q, O.OracleTable.FLAT)
            otab.insert_packed(km, ct)
            otab.decolour()
            ans = oracle_answers(otab, np.unique(km), k)
            otab.close()
            ref = T.Table.from_files(path, None, p, device=0)
            ref.upload(0)
            _dumps[name] = dict(path=path, size=len(data), km=km, ct=ct, ans=ans, want=snapshot(ref))
            ref.close()
        _dumps["params"] = p
    return _dumps


@pytest.mark.parametrize("byte", TEXT_PATTERNS, ids=ids)
def test_dump_files_parsed_and_built_under_poison(byte, tmp_path_factory):
    s = dump_inputs(tmp_path_factory.mktemp("poison_dumps") if not _dumps else None)
    p, k = s["params"], 21
    with guards_checked():
        with T.poisoned(byte):
            for name, c in s.items():
                if name == "params":
                    continue
                km, ct = c["km"], c["ct"]
                for chunk in sorted({4096, max(c["size"] - 1, 1)}):
                    r = T.parse_text_hook(c["path"], k, p.min_count, where=1, device=0, chunk_bytes=chunk, reader_threads=3)
                    assert r["flags"] == 0 and r["n_lines"] == len(km) and r["kept"] == int((ct >= p.min_count).sum()), (byte, name, chunk)
                    assert np.array_equal(r["kmers"], km) and np.array_equal(r["counts"], ct), (byte, name, chunk)
                t = T.Table.from_files(c["path"], None, p, device=0)
                t.upload(0)
                same_table(t, c["want"], (byte, name))
                against_the_oracle(t, c["ans"], (byte, name))
                t.close()


_counted = {}


def counter_inputs():
    if not _counted:
        k = 21
        rng = np.random.default_rng(31)
        text = "".join(rng.choice(list("ACGT"), size=200))
        small = {}
        for total in (1, 63, 64, 65):                # the whole text of the add: the records and one separator after each
            recs = [text[:total - 1]] if total < 40 else [text[:30], text[40:40 + total - 32]]
            assert sum(len(x) + 1 for x in recs) == total
            small[total] = recs
        grow = [["".join(rng.choice(list("ACGT"), size=150)) for _ in range(300)] for _ in range(3)]   # 39 000 windows per add
        _counted.update(k=k, small=small, grow=grow)
    return _counted


@pytest.mark.parametrize("byte", TEXT_PATTERNS, ids=ids)
def test_the_kmer_counter_under_poison(byte):
    s = counter_inputs()
    k = s["k"]
    p = T.default_params(k=k)

    def check(counter, recs, what):
        want_k, want_c = KR.count(*KR.records_to_arrays(recs), k)
        gk, gc = counter.fetch(1)
        o = np.argsort(gk)
        assert np.array_equal(gk[o], want_k) and np.array_equal(gc[o], want_c), (byte, what, len(gk), len(want_k))
        st = counter.stats()
        assert st[0] == int(want_c.sum()) and st[1] == len(want_k), (byte, what, st)

    with guards_checked():
        with T.poisoned(byte):
            for total, recs in s["small"].items():
                c = T.KmerCounter(p, 0)
                try:
                    c.add(*KR.records_to_arrays(recs))
                    check(c, recs, ("text of", total, "bytes"))
                finally:
                    c.close()
            c = T.KmerCounter(p, 0)
            try:
                seen = []
                for recs in s["grow"]:               # 2^16 slots hold 45 875 k-mers at load 0.7: the second and the third add rehash
                    c.add(*KR.records_to_arrays(recs))
                    seen += recs
                    check(c, seen, ("after", len(seen), "reads"))
                assert c.stats()[1] > 0.7 * (1 << 17)
            finally:
                c.close()


# ---------------------------------------------------------------- 8. the command line
CLI_OPTIONS = ["--batch-reads", "37", "--corr-map", "--soft-mask", "--solidity", "--trim", "--split", "--corr-edits", "--fastq", "--auto-strand", "--read-stats"]


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    """BASELINE config 1's table (5 M k-mers, K = 21; the dump goes the device parser's way), its first 600 reads, and the two
    runs without the variable."""
    d = tmp_path_factory.mktemp("poison_cli")
    syn = Synth(target_kmers=5_000_000, k=21, seed=1)
    syn.write_dump(str(d / "sr.dump"))
    syn.write_fasta(str(d / "reads.fa"), 0, 600)
    syn.close()
    return dict(dir=d, base={})


def run_cli(inputs, fake, poison):
    d = inputs["dir"]
    out = d / ("run_%d_%s" % (fake, (poison or "off").replace(",", "_")))
    out.mkdir()
    env = {k: v for k, v in os.environ.items() if k not in ("TALC_TEST_POISON", "TALC_FAKE_GPUS")}
    args = [TALC, str(d / "reads.fa"), "-k", "21", "-SR", str(d / "sr.dump"), "-o", "o"] + CLI_OPTIONS
    if fake:
        env["TALC_FAKE_GPUS"] = str(fake)
        args += ["--gpus", str(fake)]
    if poison:
        env["TALC_TEST_POISON"] = poison
    r = subprocess.run(args, cwd=out, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r, {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}


@pytest.mark.parametrize("poison", ["165,256", "255,256"])
@pytest.mark.parametrize("fake", [0, 2], ids=["one-gpu", "two-logical-gpus"])
def test_cli_files_are_byte_identical_under_poison(cli_inputs, fake, poison):
    if fake not in cli_inputs["base"]:
        cli_inputs["base"][fake] = run_cli(cli_inputs, fake, None)
    base, base_files = cli_inputs["base"][fake]
    assert base.returncode == 0 and b"[talc-poison]" not in base.stderr, base.stderr.decode()[-800:]
    assert {"o.fa", "o.fq", "o.map.tsv", "o.solidity.tsv", "o.trim.fa", "o.split.fa", "o.edits.tsv", "o.strand.tsv"} <= set(base_files), sorted(base_files)
    assert base_files["o.fa"].count(b">") == 600
    r, files = run_cli(cli_inputs, fake, poison)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-800:]
    lines = [x for x in err.splitlines() if x.startswith("[talc-poison]")]
    byte, guard = poison.split(",")
    assert len(lines) == 1 and lines[0].startswith("[talc-poison] byte %s, red zones of %s bytes: " % (byte, guard)), err[-800:]
    checked, violations = [int(x) for x in lines[0].split(": ")[1].replace(" buffers checked, ", " ").replace(" violations", "").split()]
    assert checked > 100 and violations == 0, lines[0]
    assert sorted(files) == sorted(base_files)
    for f in files:
        assert files[f] == base_files[f], (f, fake, poison)
    if fake:
        assert b"correcting on 2 GPU(s)" in r.stdout
