"""The out-of-memory contract (docs/out_of_memory.md): every allocation request of a scenario fails once, by the test hook
of talc_devmem.h (lib.failing_allocs).  A failed request that the call cannot work around is TALC_ERR_NOMEM (-3), never -4
and never a success with other data; a documented fallback gives the very outputs of the run without a failure; with the
hook off the same call on the same object succeeds and gives the baseline; after the objects are closed the library holds
as many device buffers as before; no red zone is written.  Baselines come from runs with the hook off, which the other
suites pin to the references (memcheck_util.everything: test_gpu_poison.py; kmer_ref.count; dump_ref; the oracle's tables
of test_gpu_table_lifecycle.py).  Single-threaded; integers and bytes, tolerance 0.

A scenario is a list of steps (name, call, makes an object).  One run plays the steps on fresh objects with requests
skip .. skip + count - 1 failing; at the first -3 the hook goes off and the failed step and the rest are played again on the
same objects.  A run without a -3 plays the steps behind the constructors a second time, hook off, on the same objects."""
import numpy as np
import pytest

import dump_cases as DC
import dump_ref as D
import ends_ref as R
import kmer_ref as KR
import parity_util as PU
import prep_ref as P
import test_gpu_chimera as GC
import test_gpu_prep_chain as PC
import test_gpu_table_lifecycle as TL
from memcheck_util import FORWARD, everything, fetch_all, first_difference, guards_checked, per_read
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

DEVICE, PINNED, BOTH = T.KIND_DEVICE, T.KIND_PINNED, T.KIND_DEVICE | T.KIND_PINNED
HIP_OUT_OF_MEMORY = 2            # hipErrorOutOfMemory
POISON = 0xA5                    # the one pattern byte of memcheck_util.PATTERNS the count = 1 sweeps run under


# ---------------------------------------------------------------- the engine
class Scenario:
    """steps: [(name, call(env), makes_an_object)]; again: the first step a run without a failure plays a second time;
    result(env): what is compared; close(env): gives every object back; failed_step(env, i): after a -3 of step i, hook off,
    before the step is played again (what the object must still say)."""

    def __init__(self, steps, again, result, close, failed_step=None):
        self.steps, self.again, self.result, self.close, self.failed_step = steps, again, result, close, failed_step


def work_of(ctx, rc):
    t = ctx.timing()
    return (rc, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)


def count_requests(sc, kinds):
    """N of the scenario: the requests of `kinds` one run makes when none fails."""
    env = {}
    try:
        with T.failing_allocs(kinds, 0, 0):
            for _, call, _ in sc.steps:
                call(env)
        rep = T.alloc_report()
    finally:
        sc.close(env)
    assert rep["injected"] == 0
    return (rep["device"] if kinds & DEVICE else 0) + (rep["pinned"] if kinds & PINNED else 0), rep


def play(sc, kinds, skip, count, real=False):
    """One run.  Returns (report of the hook, the failed step or None, result of the run under the hook or None, result after
    the steps were played again with the hook off)."""
    env, failed, first = {}, None, None
    live0 = T.alloc_report()["live"]
    try:
        with T.failing_allocs(kinds, skip, count, real):
            for i, (name, call, makes) in enumerate(sc.steps):
                live = T.alloc_report()["live"]
                try:
                    call(env)
                except T.TalcError as e:
                    failed = (i, name, e.code, str(e))
                    if makes:                         # a constructor that failed left no object and no buffer behind
                        assert T.alloc_report()["live"] == live, (failed, live)
                    break
        rep = T.alloc_report()
        assert rep["kinds"] == 0
        if failed is not None:
            assert failed[2] == T.ERR_NOMEM and len(failed[3]) > len("libtalc_hip error -3: "), (skip, count, failed, rep)
            if sc.failed_step:
                sc.failed_step(env, failed[0])
            start = failed[0]
        else:
            first = sc.result(env)
            start = sc.again
        for _, call, _ in sc.steps[start:]:           # hook off: the same calls on the same objects
            call(env)
        after = sc.result(env)
    finally:
        sc.close(env)
    assert T.alloc_report()["live"] == live0, (skip, count, failed, live0, T.alloc_report())
    return rep, failed, first, after


def sweep(sc, kinds, count, same, survivable=None, poison=None):
    """Every request of the scenario fails once (count = 1) or twice in a row (count = 2).  same(result, what): asserts the
    baseline.  survivable: how many DevBuf requests a count = 1 run gets over (the test's list, from the code).  Returns the
    tally for the results log."""
    n, _ = count_requests(sc, kinds)
    assert n > 0
    tally = dict(N=n, nomem={}, survived={})
    before = T.guard_report()
    for skip in range(n):
        if poison is None:
            rep, failed, first, after = play(sc, kinds, skip, count)
        else:
            with T.poisoned(poison):
                rep, failed, first, after = play(sc, kinds, skip, count)
        what = (skip, count, rep["owner"], rep["bytes"], failed)
        assert rep["injected"] >= 1, what                       # (a)
        owner = rep["owner"]
        if failed is None:                                       # (b) success: every output is the baseline's
            same(first, what + ("under the hook",))
            tally["survived"][owner] = tally["survived"].get(owner, 0) + 1
        else:
            tally["nomem"][owner] = tally["nomem"].get(owner, 0) + 1
        same(after, what + ("hook off, same objects",))          # (c)
        if count == 1:
            if owner in (T.OWNER_DEVCACHE, T.OWNER_HOST_BLOCK):  # the cache tries again; a host block is pageable instead
                assert failed is None, what
    assert T.guard_report()["violations"] == before["violations"], T.guard_report()       # (e)
    if count == 1 and survivable is not None:
        assert tally["survived"].get(T.OWNER_DEVBUF, 0) == survivable, (tally, survivable)
    print("alloc-failure sweep: kinds %d count %d N %d, -3 by owner %s, survived by owner %s" % (kinds, count, n, tally["nomem"], tally["survived"]))
    return tally


# ---------------------------------------------------------------- the instrument
_pipe = {}


def pipe():
    """The default set of test_gpu_poison.py (250 k k-mers, K = 21, seed 77): its table, uploaded once with the hook off, 26
    generator reads and the four hand reads; everything a fresh context gives for them, plain and auto strand."""
    if not _pipe:
        assert T.alloc_report()["kinds"] == 0
        pair = PU.Pair(target_kmers=250_000, k=21, seed=77)
        pair.ttab.upload(0)
        r = PU.seqs_of(*pair.reads(0, 26))
        reads = [PU.revcomp(s) if i % 2 else s for i, s in enumerate(r)] + ["", r[0][:21], r[2][:22], "N" * 80]
        fresh = {}
        for auto in (False, True):
            ctx = T.Context(pair.ttab, pair.p, 0)
            ctx.auto_strand(auto)
            try:
                fresh[auto] = everything(ctx, reads)
            finally:
                ctx.close()
        _pipe.update(pair=pair, reads=reads, packed=PU.pack_reads(reads), fresh=fresh)
    return _pipe


def test_the_request_count_of_a_fresh_context_is_the_same_twice_and_a_second_batch_asks_for_less(gpu_pair):
    bases, offs = gpu_pair.reads(0, 20)
    counts = []
    for _ in range(2):
        with T.failing_allocs(DEVICE, 0, 0):
            ctx = T.Context(gpu_pair.ttab, gpu_pair.p, 0)
            try:
                ctx.correct(bases, offs)
                one = T.alloc_report()["device"]
                ctx.correct(bases, offs)
                both = T.alloc_report()["device"]
            finally:
                ctx.close()
        rep = T.alloc_report()
        assert rep["injected"] == 0 and rep["kinds"] == 0 and rep["owner"] == 0
        counts.append((one, both - one))
    print("device requests of a fresh context's first and second batch of 20 reads:", counts)
    assert counts[0] == counts[1] and counts[0][0] > 10
    assert counts[0][1] < counts[0][0]                           # the second batch's buffers come from the cache


def test_a_refused_pinned_array_is_minus_3_and_leaves_nothing():
    live = T.alloc_report()["live"]
    with T.failing_allocs(PINNED, 0, 1):
        with pytest.raises(T.TalcError) as e:
            T.PinnedArray(4096)
    rep = T.alloc_report()
    assert e.value.code == -3 and "pinned" in str(e.value)
    assert (rep["injected"], rep["owner"], rep["bytes"], rep["pinned"], rep["device"]) == (1, T.OWNER_PINNED, 4096, 1, 0), rep
    assert rep["live"] == live and rep["kinds"] == 0
    a = T.PinnedArray(4096)                                      # hook off: the same call succeeds
    a.array[:] = 7
    a.close()
    with T.failing_allocs(DEVICE, 0, 1):                         # the other kind selected: a pinned request is seen, not numbered
        a = T.PinnedArray(64)
        a.close()
    rep = T.alloc_report()
    assert (rep["injected"], rep["pinned"]) == (0, 1), rep


_runtime = {}


def runtime_code(gpu_pair):
    """What the runtime answers to a request for 2^60 bytes of device memory (real = 1), once per session."""
    if not _runtime:
        live = T.alloc_report()["live"]
        with T.failing_allocs(DEVICE, 0, 1, real=True):
            with pytest.raises(T.TalcError) as e:
                T.Context(gpu_pair.ttab, gpu_pair.p, 0)
        rep = T.alloc_report()
        assert rep["injected"] == 1 and rep["owner"] == T.OWNER_DEVBUF and rep["live"] == live, rep
        _runtime.update(code=rep["runtime_code"], rc=e.value.code, text=str(e.value))
        print("the runtime's code for a request of 2^60 bytes: %d; the call returned %d (%s)" % (rep["runtime_code"], e.value.code, str(e.value)))
    return _runtime


def test_a_real_refusal_is_recorded_with_the_runtimes_code(gpu_pair):
    r = runtime_code(gpu_pair)
    assert r["code"] != 0                                        # the runtime refused, by an error return
    if r["code"] == HIP_OUT_OF_MEMORY:
        assert r["rc"] == -3, r
    ctx = T.Context(gpu_pair.ttab, gpu_pair.p, 0)                # the call after the failed one does not fail on it
    try:
        out = ctx.correct(*gpu_pair.reads(0, 5))
        want = gpu_pair.ctx.correct(*gpu_pair.reads(0, 5))
        assert all(np.array_equal(x, y) for x, y in zip(out, want))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 1. context and batch, 2. retry passes
def batch_steps(make_ctx, packed, auto, whats=FORWARD):
    def ctx_step(e):
        e["ctx"] = make_ctx()

    def batch_step(e):
        if e.get("b") is not None:
            e["b"].close()
        e["b"], e["f"] = None, {}
        e["b"] = e["ctx"].batch(*packed)

    def correct_step(e):
        e["work"] = work_of(e["ctx"], e["b"].correct())

    def fetch_step(what):
        return lambda e: e["f"].update(fetch_all(e["b"], (what,)))

    def strand_step(e):
        e["rows"] = e["b"].strand() if auto else None

    # (a batch that failed to build has given its buffers back to its context's cache: they are counted when the context closes)
    steps = [("context", ctx_step, True), ("batch", batch_step, False), ("correct", correct_step, False)]
    steps += [(w, fetch_step(w), False) for w in whats] + [("strand", strand_step, False)]
    return steps


def close_batch(e):
    for name in ("b", "ctx"):
        if e.get(name) is not None:
            e[name].close()


def pipe_scenario(auto):
    s = pipe()

    def make_ctx():
        ctx = T.Context(s["pair"].ttab, s["pair"].p, 0)
        ctx.auto_strand(auto)
        ctx.record_map(True)
        return ctx

    n = len(s["reads"])
    return Scenario(batch_steps(make_ctx, s["packed"], auto), 1, lambda e: (per_read(e["f"], n), e["work"], e["rows"]), close_batch)


# what a count = 1 run of the correction gets over although the request's owner is a DevBuf: the search scratch's first
# attempt (ensure_stage tries once more) and the edge boxes (the search runs without)
SURVIVABLE_CORRECTION = 2


@pytest.mark.parametrize("count", [1, 2])
@pytest.mark.parametrize("auto", [False, True], ids=["plain", "auto-strand"])
def test_context_and_batch_with_every_request_failing(auto, count):
    s = pipe()
    want, want_work, want_rows = s["fresh"][auto]

    def same(got, what):
        per, work, rows = got
        assert first_difference(per, want) is None, (what, first_difference(per, want))
        assert work == (want_work[0],) + want_work[3:], (what, work, want_work)
        if auto:
            assert np.array_equal(rows, want_rows), what

    assert want_work[0] == 0 and [t[1] for t in want].count(T.READ_CORRECTED) >= 10 and [t[1] for t in want].count(T.READ_SKIPPED_SHORT) >= 2
    if count == 1:
        with guards_checked():
            tally = sweep(pipe_scenario(auto), BOTH, 1, same, SURVIVABLE_CORRECTION, poison=POISON)
        assert tally["survived"].get(T.OWNER_DEVCACHE, 0) >= 30 and tally["survived"].get(T.OWNER_HOST_BLOCK, 0) >= 3, tally
        assert tally["nomem"].get(T.OWNER_DEVBUF, 0) >= 4, tally   # the context's own four buffers at least
    else:
        tally = sweep(pipe_scenario(auto), BOTH, 2, same)
        assert tally["nomem"].get(T.OWNER_DEVCACHE, 0) >= 30, tally   # both attempts of the cache fail: -3


def test_retry_passes_with_every_request_failing(monkeypatch):
    """TALC_TEST_TINY_CAPS: reads overflow their first-pass scratch, the x 8 stage and d_retry are asked for.  A refused
    retry stage or d_retry leaves the reads still flagged as the first pass left them: their tuples are those of a run whose
    retry stage TALC_TEST_FAIL_RETRY_ALLOC refuses (test_gpu_solidity.py), everybody else's the baseline's.

    The x 64 stage: the hook at level 1 shrinks the capacities of the first pass only; the x 8 stage has eight times the
    ordinary capacities, which hold every read this suite has, so no read is still flagged behind it and exactly one stage
    is sized here.  A x 64 stage refused behind a x 8 pass that ran is the test below (level 2)."""
    s = pipe()
    reads, n = s["reads"], len(s["reads"])
    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "1")

    def make_ctx():
        ctx = T.Context(s["pair"].ttab, s["pair"].p, 0)
        ctx.record_map(True)
        return ctx

    ctx = make_ctx()
    try:
        want, want_work, _ = everything(ctx, reads)
    finally:
        ctx.close()
    monkeypatch.setenv("TALC_TEST_FAIL_RETRY_ALLOC", "1")
    ctx = make_ctx()
    try:
        refused, refused_work, _ = everything(ctx, reads)
    finally:
        ctx.close()
    monkeypatch.delenv("TALC_TEST_FAIL_RETRY_ALLOC")
    assert want_work[0] == 0 and want_work[5] >= 1 and want_work[6] == 0, want_work          # reads were retried, none failed
    assert refused_work[0] == T.WARN_READ_ERRORS and refused_work[6] == refused_work[5] == want_work[5], (refused_work, want_work)
    warned = []

    def same(got, what):
        per, work, _ = got
        flagged = [i for i in range(n) if per[i][1] == T.READ_ERROR]
        if work[0] == T.WARN_READ_ERRORS:
            assert flagged and work[4] == len(flagged) and all(refused[i][1] == T.READ_ERROR for i in flagged), (what, work, flagged)
            warned.append(what)
        else:
            assert work[0] == 0 and not flagged and work[4] == 0, (what, work)
        mixed = [refused[i] if i in flagged else want[i] for i in range(n)]
        assert first_difference(per, mixed) is None, (what, first_difference(per, mixed))
        assert work[1:3] == (want_work[3], want_work[4]), (what, work)

    sc = Scenario(batch_steps(make_ctx, s["packed"], False), 1, lambda e: (per_read(e["f"], n), e["work"], None), close_batch)
    with guards_checked():
        tally = sweep(sc, DEVICE, 1, same, poison=POISON)
    # DevBuf requests a count = 1 run gets over: scratch (first attempt) and boxes of the first pass; per retry stage S its
    # scratch (first attempt; no outputs change) and d_retry (the reads stay flagged: a warning)
    under_hook = [w for w in warned if w[-1] == "under the hook"]
    stages = len(under_hook)
    assert stages == 1, warned                        # one d_retry: the x 8 stage alone (the docstring says why)
    assert all(w[2] == T.OWNER_DEVBUF and w[1] == 1 for w in under_hook)
    assert tally["survived"].get(T.OWNER_DEVBUF, 0) == SURVIVABLE_CORRECTION + 2 * stages, (tally, stages)
    warned.clear()
    tally = sweep(sc, DEVICE, 2, same)
    assert len([w for w in warned if w[-1] == "under the hook"]) >= stages, warned     # both attempts of a retry stage refused


def test_a_refused_x64_stage_behind_an_x8_pass_that_ran(monkeypatch):
    """TALC_TEST_TINY_CAPS=2: the x 8 stage is as small as the first pass, every read it searched is flagged again and the
    x 64 stage and its d_retry are asked for.  The sweep finds two stages; a refused d_retry of either — for the x 64 stage:
    behind a x 8 pass that ran and rewrote the states — leaves exactly the reads flagged before it, passed through as the
    first pass passed them (the tuples of a run whose retry stage TALC_TEST_FAIL_RETRY_ALLOC refuses), and the call returns
    the warning; a refused scratch is asked for once more and changes nothing."""
    s = pipe()
    reads, n = s["reads"], len(s["reads"])
    monkeypatch.setenv("TALC_SEARCH_SLOTS", "8")
    want = s["fresh"][False][0]

    def make_ctx():
        ctx = T.Context(s["pair"].ttab, s["pair"].p, 0)
        ctx.record_map(True)
        return ctx

    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "1")
    monkeypatch.setenv("TALC_TEST_FAIL_RETRY_ALLOC", "1")
    ctx = make_ctx()
    try:
        refused, refused_work, _ = everything(ctx, reads)
    finally:
        ctx.close()
    monkeypatch.delenv("TALC_TEST_FAIL_RETRY_ALLOC")
    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "2")
    ctx = make_ctx()
    try:
        got, got_work, _ = everything(ctx, reads)
        rep = ctx.retry_report()
    finally:
        ctx.close()
    first_flagged = [i for i in range(n) if refused[i][1] == T.READ_ERROR]
    assert first_difference(got, want) is None and got_work[0] == 0 and got_work[6] == 0
    assert rep == dict(x8=len(first_flagged), x64=len(first_flagged), left=0, refused=0) and first_flagged, (rep, first_flagged)
    warned = []

    def same(got, what):
        per, work, _ = got
        flagged = [i for i in range(n) if per[i][1] == T.READ_ERROR]
        if work[0] == T.WARN_READ_ERRORS:
            assert flagged == first_flagged and work[4] == len(flagged), (what, work, flagged)
            warned.append(what)
        else:
            assert work[0] == 0 and not flagged and work[4] == 0, (what, work)
        mixed = [refused[i] if i in flagged else want[i] for i in range(n)]
        assert first_difference(per, mixed) is None, (what, first_difference(per, mixed))
        assert work[3] == len(first_flagged), (what, work)
        assert work[1:3] == (got_work[3], got_work[4]), (what, work)
        if what[2] == T.OWNER_DEVBUF and what[-1] == "under the hook":
            requested.append(what[3])

    def result(e):
        per, work, rep = per_read(e["f"], n), e["work"], e["ctx"].retry_report()
        # the report of the correction whose outputs these are: a warning is one stage refused, the reads before it left
        if work[0] == T.WARN_READ_ERRORS:
            assert rep["refused"] == 1 and rep["left"] == work[4] == len(first_flagged) and rep["x64"] == 0 and rep["x8"] in (0, rep["left"]), (rep, work)
        else:
            assert rep == dict(x8=len(first_flagged), x64=len(first_flagged), left=0, refused=0), (rep, work)
        return per, work, None

    requested = []
    sc = Scenario(batch_steps(make_ctx, s["packed"], False), 1, result, close_batch)
    with guards_checked():
        tally = sweep(sc, DEVICE, 1, same, poison=POISON)
    under_hook = [w for w in warned if w[-1] == "under the hook"]
    stages = len(under_hook)
    assert stages == 2, warned                        # the d_retry of the x 8 stage and that of the x 64 stage
    # the largest request a run got over is the x 64 stage's scratch (its first attempt)
    print("x 64 stage of %d flagged reads, longest read %d bases, TALC_SEARCH_SLOTS=8: scratch of %d bytes" % (len(first_flagged), max(map(len, reads)), max(requested)))
    assert all(w[2] == T.OWNER_DEVBUF and w[1] == 1 for w in under_hook)
    assert tally["survived"].get(T.OWNER_DEVBUF, 0) == SURVIVABLE_CORRECTION + 2 * stages, (tally, stages)


# ---------------------------------------------------------------- 3. preparation
@pytest.mark.parametrize("count", [1, 2])
def test_preparation_with_every_request_failing(count):
    s = PC.inputs()
    c, reads = s["c"], s["small"]
    assert len(reads) == 44
    packed = R.batch(reads)

    def make_ctx():
        ctx = PC.fresh(c, "plain")
        try:
            ctx.set_ends(**P.ENDS_KW)
            ctx.set_chimera(*P.CHIMERA)
            ctx.set_demux(*P.DEMUX)
            ctx.set_umi(*P.UMI)
            ctx.record_map(True)
        except T.TalcError:
            ctx.close()
            raise
        return ctx

    def ctx_step(e):
        e["ctx"] = make_ctx()

    def batch_step(e):
        if e.get("b") is not None:
            e["b"].close()
        e["b"], e["f"], e["r"] = None, {}, {}
        e["b"] = e["ctx"].batch(*packed, clip=True, split=True)

    def cov_step(e):
        e["b"].coverage()
        e["r"]["cov"] = [x.tobytes() for x in e["b"].fetch_coverage()]

    def struct_step(e):
        e["b"].structure()
        e["r"]["struct"] = {k: v.tobytes() for k, v in e["b"].fetch_structure().items()}

    def correct_step(e):
        e["r"]["work"] = work_of(e["ctx"], e["b"].correct())

    def report_step(name, call):
        def step(e):
            got = call(e["b"])
            e["r"][name] = tuple(np.asarray(x).tobytes() for x in got) if isinstance(got, tuple) else np.asarray(got).tobytes()
        return step

    steps = [("context", ctx_step, True), ("batch", batch_step, False), ("coverage", cov_step, False), ("structure", struct_step, False),
             ("correct", correct_step, False)]
    steps += [(w, (lambda w: lambda e: e["f"].update(fetch_all(e["b"], (w,))))(w), False) for w in FORWARD]
    steps += [(name, report_step(name, call), False) for name, call in (("ends", lambda b: b.ends()), ("chimera", lambda b: b.chimera()),
                                                                         ("pieces", lambda b: b.split_pieces()), ("demux", lambda b: b.demux()),
                                                                         ("umi", lambda b: b.umi()))]

    def result(e):
        return dict(e["r"], per=per_read(e["f"], e["b"].n_reads), n=e["b"].n_reads)

    sc = Scenario(steps, 1, result, close_batch)
    # the baseline: the same calls with the hook off, held to test_gpu_chimera.everything_of on a context that never failed
    env = {}
    try:
        for _, call, _ in steps:
            call(env)
        want = result(env)
    finally:
        close_batch(env)
    ctx = make_ctx()
    try:
        ref = GC.everything_of(ctx, *packed, clip=True, split=True, ends=True)
    finally:
        ctx.close()
    assert ref["n"] == want["n"] and ref["cov"] == want["cov"] and ref["struct"] == want["struct"] and first_difference(want["per"], ref["per"]) is None
    assert np.asarray(ref["rows"]).tobytes() == want["ends"] and tuple(np.asarray(x).tobytes() for x in (ref["hits"], ref["hit_off"])) == want["chimera"]
    assert (ref["work"][0],) + ref["work"][3:] == want["work"] and want["n"] > len(reads)        # some read was split

    def same(got, what):
        for k in want:
            if k == "per":
                assert first_difference(got["per"], want["per"]) is None, (what, first_difference(got["per"], want["per"]))
            else:
                assert got[k] == want[k], (what, k)

    if count == 1:
        with guards_checked():
            tally = sweep(sc, DEVICE, 1, same, SURVIVABLE_CORRECTION, poison=POISON)
    else:
        tally = sweep(sc, DEVICE, 2, same)
    assert tally["N"] > 40, tally                   # the context's 5, the split batch's 20 and more, every report's


# ---------------------------------------------------------------- 4. tables
_tables = {}


def table_specs():
    if not _tables:
        _tables.update(plain=TL.Spec(False, 71), coloured=TL.Spec(True, 72))
    return _tables


@pytest.mark.parametrize("count", [1, 2])
@pytest.mark.parametrize("walk", [None, "1"], ids=["walk-unset", "walk-1"])
@pytest.mark.parametrize("name", ["plain", "coloured"])
def test_tables_with_every_request_failing(name, walk, count, monkeypatch):
    spec = table_specs()[name]
    if walk is None:
        monkeypatch.delenv("TALC_WALK", raising=False)
    else:
        monkeypatch.setenv("TALC_WALK", walk)
    qs, few = spec.qs, spec.qs[:600]

    def close(e):
        for k in ("t2", "t"):
            if e.get(k) is not None:
                e[k].close()

    def build(e):
        e["t"] = T.Table.from_arrays(spec.keys, spec.counts, spec.p, device=0)

    def move(e):
        if e.get("t2") is not None:
            e["t2"].close()
            e["t2"] = None
        t = e["t"]
        with TL.device_buffers(t.image_bytes) as (r, l):
            t.export_device(0, r, l)
            e["t2"] = T.Table.import_device(spec.p, t.capacity, len(t), r, l, 0)

    def canonical(records):
        """A walk table as a sorted multiset of records: two device builds of one dump may place the keys of a probe chain in
        another order (test_gpu_poison.py: canonical); where the buckets sit is pinned by the look-ups."""
        flat = np.ascontiguousarray(records).view(np.dtype((np.void, 32))).ravel()
        return np.sort(flat).tobytes()

    def walks(t):
        try:
            return (canonical(t.fetch_walk(0)), canonical(t.fetch_walk(1)))
        except T.TalcError as err:
            assert err.code == -6, err                            # uploaded without walk tables
            return None

    steps = [("from_arrays", build, True), ("colour", lambda e: e["t"].colour(spec.jk, spec.jc), False),
             ("decolour", lambda e: e["t"].decolour_repeats(), False), ("upload", lambda e: e["t"].upload(0), False),
             ("lookup", lambda e: e.__setitem__("lk", e["t"].lookup(qs)), False),
             ("next_counts", lambda e: e.__setitem__("nx", [e["t"].next_counts(few, d) for d in (0, 1)]), False),
             ("export-import", move, False), ("upload-2", lambda e: e["t2"].upload(0), False),
             ("lookup-2", lambda e: e.__setitem__("lk2", e["t2"].lookup(qs)), False)]

    def result(e):
        return dict(lk=e["lk"], lk2=e["lk2"], nx=e["nx"], walks=(walks(e["t"]), walks(e["t2"])), size=(len(e["t"]), len(e["t2"])))

    # successor counts and walk tables: those of a table built with the hook off; lookups: the oracle's
    env = {}
    try:
        for _, call, _ in steps:
            call(env)
        base = result(env)
    finally:
        close(env)
    spec.same(base["lk"], "final")
    spec.same(base["lk2"], "final")
    has_walk = base["walks"][0] is not None
    assert walk is None or has_walk
    assert base["walks"][0] == base["walks"][1] and base["size"] == (spec.size, spec.size)

    def same(got, what):
        spec.same(got["lk"], "final", what)
        spec.same(got["lk2"], "final", what)
        for d in (0, 1):
            assert np.array_equal(got["nx"][d][0], base["nx"][d][0]) and np.array_equal(got["nx"][d][1], base["nx"][d][1]), (what, d)
        assert got["size"] == base["size"], what
        for w, bw in zip(got["walks"], base["walks"]):            # walk tables that did not fit are absent, never different
            assert w is None or w == bw, what
        if walk == "1":
            assert got["walks"] == base["walks"], what

    sc = Scenario(steps, 4, result, close)        # (an uploaded table is immutable: a run without a failure asks its questions again)
    # TALC_WALK unset: the two walk tables of either upload are done without; TALC_WALK=1: they are mandatory
    survivable = 4 if (walk is None and has_walk) else 0
    if count == 1:
        with guards_checked():
            tally = sweep(sc, DEVICE, 1, same, survivable, poison=POISON)
        assert tally["nomem"].get(T.OWNER_DEVBUF, 0) >= 15, tally
    else:
        sweep(sc, DEVICE, 2, same)


# ---------------------------------------------------------------- 5. the text route
@pytest.mark.parametrize("kinds", [DEVICE, PINNED, BOTH])
def test_text_route_with_every_request_failing(kinds, tmp_path):
    k = 21
    data = DC.case_d(k)["tile-plus-one"].data
    path = DC.write(tmp_path / "dump.txt", data)
    km, ct, flagged = D.parse(data, k)
    assert not flagged and len(km) > 100
    p = T.default_params(k=k)

    def parse(e):
        e["r"] = T.parse_text_hook(path, k, p.min_count, where=1, device=0, chunk_bytes=4096, reader_threads=1)

    def same(r, what):
        assert r["flags"] == 0 and r["n_lines"] == len(km) and r["kept"] == int((ct >= p.min_count).sum()), what
        assert np.array_equal(r["kmers"], km) and np.array_equal(r["counts"], ct), what

    sc = Scenario([("parse", parse, True)], 0, lambda e: e["r"], lambda e: None)
    for count in (1, 2):
        if count == 1:
            with guards_checked():
                tally = sweep(sc, kinds, count, same, 0, poison=POISON)
        else:
            tally = sweep(sc, kinds, count, same)
        # the hook has no host parser to fall back to: every refused request of the device parser is -3 there
        assert not tally["survived"] and sum(tally["nomem"].values()) == tally["N"], tally
        assert tally["N"] >= (12 if kinds & DEVICE else 0) + (2 if kinds & PINNED else 0), tally


# ---------------------------------------------------------------- 6. the k-mer counter
_counter = {}


def counter_inputs():
    if not _counter:
        k = 21
        rng = np.random.default_rng(41)
        adds = [["".join(rng.choice(list("ACGT"), size=150)) for _ in range(1000)] for _ in range(3)]
        arrays = [KR.records_to_arrays(a) for a in adds]
        refs = {}
        for both in (False, True):
            seen, steps = [], []
            for a in adds:
                seen = seen + a
                steps.append(fold(*KR.count(*KR.records_to_arrays(seen), k), k, both))
            ek = np.concatenate([steps[-1][0][:500], rng.integers(0, 1 << (2 * k), 500, dtype=np.uint64)])
            ec = rng.integers(1, 5, 1000).astype(np.uint32)
            final = merged(np.concatenate([steps[-1][0], canon(ek, k) if both else ek]), np.concatenate([steps[-1][1].astype(np.uint64), ec.astype(np.uint64)]))
            refs[both] = dict(steps=steps, extra=(ek, ec), final=final)
        # enough distinct k-mers to grow the 64 K-slot hash (load 0.7) at least once
        assert len(refs[False]["steps"][0][0]) > 0.7 * (1 << 16) and len(refs[True]["steps"][0][0]) > 0.7 * (1 << 16)
        _counter.update(k=k, arrays=arrays, refs=refs)
    return _counter


def canon(km, k):
    return np.minimum(km, PU.revcomp_packed(km, k))


def merged(keys, counts):
    """(sorted distinct keys, summed counts), entries whose sum is 0 dropped."""
    u, inv = np.unique(keys, return_inverse=True)
    c = np.zeros(len(u), dtype=np.uint64)
    np.add.at(c, inv, counts.astype(np.uint64))
    return u[c > 0], c[c > 0].astype(np.uint32)


def fold(km, ct, k, both):
    return merged(canon(km, k), ct) if both else (km, ct)


# build_table first builds beside the hash and only then as the memory asks for it: the two kept arrays and the builder's
# five buffers of the first way are got over (TALC_WALK=0: the table's upload asks for no walk tables, which it would do without)
SURVIVABLE_BUILD_TABLE = 7


@pytest.mark.parametrize("count", [1, 2])
@pytest.mark.parametrize("variant", ["directional", "both-strands", "filtered"])
def test_kmer_counter_with_every_request_failing(variant, count, monkeypatch):
    monkeypatch.setenv("TALC_WALK", "0")
    s = counter_inputs()
    k, both, filtered = s["k"], variant == "both-strands", variant == "filtered"
    ref = s["refs"][both]
    p = T.default_params(k=k)
    fk, fc = ref["final"]
    minc = p.min_count
    want_hist = np.zeros(52, dtype=np.uint64)
    np.add.at(want_hist, np.minimum(fc, 51), 1)
    want_table = (fk[fc >= minc], fc[fc >= minc])
    assert len(want_table[0]) > 100 and int((fc == 1).sum()) > 1000

    def create(e):
        c = T.KmerCounter(p, 0, expected_distinct=1, both_strands=both)
        try:
            if filtered:                              # a quality floor no base is below: the filter's buffers, the same counts
                c.set_filter(min_qual=20)
        except T.TalcError:
            c.close()
            raise
        e["c"], e["added"] = c, 0

    def add(i):
        def step(e):
            bases, offs = s["arrays"][i]
            e["c"].add(bases, offs, np.full(len(bases), ord("I"), dtype=np.uint8) if filtered else None)
            e["added"] = i + 1
        return step

    def add_counts(e):
        e["c"].add_counts(*ref["extra"])
        e["added"] = 4

    def build(e):
        if e.get("t") is not None:
            e["t"].close()
            e["t"] = None
        e["t"] = e["c"].build_table()

    def look(e):
        e["t"].upload(0)
        q = want_table[0]
        e["lk"] = [e["t"].lookup(q)[0]] + ([e["t"].lookup(PU.revcomp_packed(q, k))[0]] if both else [])

    steps = [("create", create, True)] + [("add-%d" % i, add(i), False) for i in range(3)]
    steps += [("add_counts", add_counts, False), ("fetch", lambda e: e.__setitem__("fetch", e["c"].fetch(1)), False),
              ("histo", lambda e: e.__setitem__("histo", e["c"].histo(50)), False), ("build_table", build, False), ("lookup", look, False)]

    def failed_step(e, i):
        """A failed add or add_counts has counted nothing: stats() is the reference's after the adds that succeeded."""
        name = steps[i][0]
        if name.startswith("add"):
            done = e["added"]
            st = e["c"].stats()
            if done == 0:
                assert st[:2] == (0, 0), (name, st)
            else:
                rk, rc_ = ref["steps"][done - 1]
                assert st[:2] == (int(rc_.astype(np.uint64).sum()), len(rk)), (name, done, st)

    def close(e):
        for name in ("t", "c"):
            if e.get(name) is not None:
                e[name].close()

    def result(e):
        gk, gc = e["fetch"]
        o = np.argsort(gk)
        return dict(fetch=(gk[o], gc[o]), histo=e["histo"], lk=e["lk"], size=len(e["t"]))

    def same(got, what):
        assert np.array_equal(got["fetch"][0], fk) and np.array_equal(got["fetch"][1], fc), (what, len(got["fetch"][0]), len(fk))
        hist, st = got["histo"]
        assert np.array_equal(hist, want_hist) and st == (len(fk), int((fc == 1).sum()), int(fc.astype(np.uint64).sum()), int(fc.max())), (what, st)
        for lk in got["lk"]:
            assert np.array_equal(lk, want_table[1]), what
        palindromes = int((PU.revcomp_packed(want_table[0], k) == want_table[0]).sum())
        assert got["size"] == (2 * len(want_table[0]) - palindromes if both else len(want_table[0])), (what, got["size"])

    # (a run without a failure has spent its counter: only the look-ups are played again)
    sc = Scenario(steps, len(steps) - 1, result, close, failed_step)
    if count == 1:
        with guards_checked():
            tally = sweep(sc, BOTH, 1, same, SURVIVABLE_BUILD_TABLE, poison=POISON)
        assert tally["nomem"].get(T.OWNER_PINNED, 0) >= 2 and tally["nomem"].get(T.OWNER_DEVBUF, 0) >= 12, tally
    else:
        sweep(sc, BOTH, 2, same)


# ---------------------------------------------------------------- clean state
def test_the_call_after_a_real_refusal_does_not_fail_on_it(gpu_pair):
    """real = 1: the runtime itself refuses a DevBuf request of batch.correct() — the search scratch, and with count = 2,
    because one refusal of the scratch is got over by its second attempt and the call would not fail at all; then a second
    batch on the same context.  What is asserted is that every later call succeeds (0, the baseline's records, and three more
    calls that launch kernels and read the runtime's last error behind them): talc_last_error() keeps the text of the last
    failure of the thread until the next one, by its contract (include/talc_hip.h: a message for a call that failed), so
    "no text mentions the earlier failure" can only be said of calls that fail, and none does.  (Where the runtime does not
    answer a request of 2^60 bytes with hipErrorOutOfMemory the library's own refusal is used: the runtime's error state
    is then not covered.)"""
    s = pipe()
    real = runtime_code(gpu_pair)["code"] == HIP_OUT_OF_MEMORY
    print("clean state with real =", int(real), "" if real else "(the runtime's state is NOT covered)")
    want = s["fresh"][False][0]
    n = len(s["reads"])
    ctx = T.Context(s["pair"].ttab, s["pair"].p, 0)
    ctx.record_map(True)
    try:
        with T.failing_allocs(DEVICE, 0, 0):
            b = ctx.batch(*s["packed"])
            made = T.alloc_report()["device"]
            b.correct()
            done = T.alloc_report()["device"]
            b.close()
        ctx.close()
        hit = None
        for skip in range(made, done):                # the DevBuf requests of correct(): the first one that two refusals turn into -3
            ctx = T.Context(s["pair"].ttab, s["pair"].p, 0)
            ctx.record_map(True)
            b = ctx.batch(*s["packed"])
            # (requests are numbered from the arming call: the batch exists already)
            with T.failing_allocs(DEVICE, skip - made, 2, real=real):
                try:
                    b.correct()
                except T.TalcError as e:
                    hit = (skip, e.code, str(e))
            rep = T.alloc_report()
            b.close()
            if hit and rep["owner"] == T.OWNER_DEVBUF:
                break
            hit = None
            ctx.close()
        assert hit is not None and hit[1] == -3, hit
        assert rep["injected"] == 2 and (not real or rep["runtime_code"] == HIP_OUT_OF_MEMORY), rep
        b2 = ctx.batch(*s["packed"])                   # the same context, a second batch
        try:
            assert b2.correct() == 0
            per = per_read(fetch_all(b2), n)
            assert first_difference(per, want) is None, first_difference(per, want)
            for call in (b2.coverage, b2.structure, b2.solidity):   # every later call launches kernels and checks the runtime's last error
                call()
        finally:
            b2.close()
    finally:
        ctx.close()
