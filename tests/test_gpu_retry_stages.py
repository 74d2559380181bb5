"""The retry stages of the correction as they really run (search_retry_passes): TALC_TEST_TINY_CAPS=2 leaves the first pass
and the x 8 stage with three positions and one bridge per search, so that flagged reads are served by a real x 64 stage;
=3 shrinks that one too, so that reads are searched in all three stages, overflow in each and leave as they came.
Ctx.retry_report() says which stages ran.  The reference of every comparison is a plain context on the same table (whose
records compare_correction holds to the oracle here); integers and bytes, tolerance 0.  Inputs: tests/retry_cases.py.
Also here: the trace hook on a read that ends in x 64, the executable under the hook, and the constructed read that needs
the x 64 stage without a hook, its record and map against the oracle's.

TALC_SEARCH_SLOTS=8 everywhere but in the slot-choice test: the x 64 stage of the 8 kb reads is then 8 slots of 12.6 MB."""
import numpy as np
import pytest

import os
import subprocess

import corr_map_ref as CM
import long_gap_cases as LG
import oracle_lib as O
import parity_util as PU
import retry_cases as RC
import test_gpu_param_limits as PLT
import test_gpu_prep_chain as PC
import test_gpu_solidity as G
from memcheck_util import F_RECORD, F_SEGS, F_SPLIT_TEXTS, F_STATUS, everything, guards_checked
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

SLOTS = "8"
POISON_BYTES = (0xFF, 0xA5)
HOOKS = ("TALC_TEST_TINY_CAPS", "TALC_TEST_FAIL_RETRY_ALLOC", "TALC_SEARCH_SLOTS", "TALC_TRACE_STEPS")
_cases = {}


class Case:
    """pair (tables on both sides, uploaded, .ctx a plain context), reads, plain: everything() of the plain context."""


def case(name, gpu_pair):
    if name not in _cases:
        c = Case()
        if name == "default-k21":
            _, first, n = RC.GENERATOR_SETS[name]
            c.pair, c.reads = gpu_pair, PU.seqs_of(*gpu_pair.reads(first, n))
        elif name in RC.GENERATOR_SETS:
            kw, first, n = RC.GENERATOR_SETS[name]
            c.pair = PU.Pair(**kw)
            c.pair.upload(0)
            c.reads = PU.seqs_of(*c.pair.reads(first, n))
        elif name == "tandem-k21":
            transcripts, c.reads = RC.tandem_set()
            c.pair = PU.CustomPair(transcripts, k=21, depth=20)
            c.pair.upload(0)
        elif name == "long-gap":
            g, params, _ = LG.case(RC.LONG_GAP)
            c.pair = PU.CustomPair(g.transcripts, k=g.k, depth=20, **params)
            c.pair.upload(0)
            c.reads = [g.read, g.read[:len(g.read) // 2], PU.revcomp(g.read)]
        else:
            raise KeyError(name)
        bad, _, _ = PU.compare_correction(c.pair, *PU.pack_reads(c.reads), nthreads=16, verbose=False)
        assert not bad, (name, bad[:8])
        c.plain = everything(c.pair.ctx, c.reads, batch_free=True)
        _cases[name] = c
    return _cases[name]


def context(pair, monkeypatch, level=None, slots=SLOTS, refuse=False, p=None, steps=False):
    """A context of the pair's table made under the hook (a context reads the switches when it is created)."""
    for name, value in zip(HOOKS, (level, "1" if refuse else None, slots, "1" if steps else None)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    try:
        return T.Context(pair.ttab, p or pair.p, 0)
    finally:
        for name in HOOKS:
            monkeypatch.delenv(name, raising=False)


def run(pair, reads, monkeypatch, **kw):
    """(per-read tuples, work, retry report) of a fresh context under the hook."""
    ctx = context(pair, monkeypatch, **kw)
    try:
        per, work, _ = everything(ctx, reads, batch_free=True)
        return per, work, ctx.retry_report()
    finally:
        ctx.close()


def reached_x64(work, rep, what):
    """Level 2: reads went to x 8, the same reads to x 64, none is left."""
    rc, n_retried, n_failed = work[0], work[5], work[6]
    print("retry stages %s: retried %d, report %s" % (what, n_retried, rep))
    assert rc == 0 and n_retried > 0 and n_failed == 0, (what, work)
    assert rep == dict(x8=n_retried, x64=n_retried, left=0, refused=0), (what, rep, n_retried)


# ---------------------------------------------------------------- level 2
@pytest.mark.parametrize("name", RC.HOOK_INPUTS)
def test_reads_served_by_the_x64_stage_equal_the_plain_context(name, gpu_pair, monkeypatch):
    """Records, offsets, statuses, read stats, map segments, masked records, pieces, edits, solidity and base support."""
    c = case(name, gpu_pair)
    want, want_work, _ = c.plain
    assert want_work[0] == 0 and want_work[5] == 0                 # the plain context retries nothing
    per, work, rep = run(c.pair, c.reads, monkeypatch, level=2)
    reached_x64(work, rep, name)
    assert per == want, (name, [i for i in range(len(want)) if per[i] != want[i]][:8])
    assert work[3:5] == want_work[3:5]


@pytest.mark.parametrize("setting", ["rev", "auto-strand"])
def test_x64_stage_under_rev_and_auto_strand(setting, gpu_pair, monkeypatch):
    c = case("default-k21", gpu_pair)
    reads = [PU.revcomp(s) if (setting == "rev" or i % 2) else s for i, s in enumerate(c.reads[:80])]
    p = T.default_params(k=21, reverse=1 if setting == "rev" else 0)
    got = []
    for level in (None, 2):
        ctx = context(c.pair, monkeypatch, level=level, p=p)
        try:
            if setting == "auto-strand":
                ctx.auto_strand(True)
            per, work, rows = everything(ctx, reads, batch_free=True)
            got.append((per, work, rows, ctx.retry_report()))
        finally:
            ctx.close()
    (want, want_work, want_rows, _), (per, work, rows, rep) = got
    assert [t[F_STATUS] for t in want].count(T.READ_CORRECTED) >= 60
    reached_x64(work, rep, setting)
    assert per == want
    if setting == "auto-strand":
        assert np.array_equal(rows, want_rows) and 20 <= int(rows["reverse"].sum()) <= 60


@pytest.mark.parametrize("byte", POISON_BYTES, ids=lambda b: "0x%02X" % b)
@pytest.mark.parametrize("level", [2, 3])
def test_stages_under_poison(level, byte, gpu_pair, monkeypatch):
    """Every launch finds its stage poisoned, the x 64 stage a fresh allocation; no red zone is written."""
    c = case("paralogs-k21", gpu_pair)
    want = c.plain[0]
    with guards_checked():
        with T.poisoned(byte):
            per, work, rep = run(c.pair, c.reads, monkeypatch, level=level)
    if level == 2:
        reached_x64(work, rep, "poison 0x%02X" % byte)
        assert per == want
    else:
        clean, _, _ = run(c.pair, c.reads, monkeypatch, level=3)
        assert per == clean and work[0] == T.WARN_READ_ERRORS and rep["left"] == work[6] > 0


def test_one_context_over_batches_that_end_in_different_stages(gpu_pair, monkeypatch):
    """No retry, x 64, another longest read, x 64 again, and — a second context at level 1 on the same table — a batch the
    x 8 stage cures: each batch equals the plain context's tuples of its reads."""
    c = case("default-k21", gpu_pair)
    want = c.plain[0]
    order = sorted(range(len(c.reads)), key=lambda i: len(c.reads[i]))
    ctx = context(c.pair, monkeypatch, level=2)
    try:
        per, work, _ = everything(ctx, ["", "N" * 80, c.reads[0][:21]], batch_free=True)
        assert work[5] == 0 and ctx.retry_report() == dict(x8=0, x64=0, left=0, refused=0) and [t[F_STATUS] for t in per].count(T.READ_CORRECTED) == 0
        for what, idx in (("short", order[:40]), ("longest", order[-30:]), ("mixed", order[::5]), ("short again", order[:40])):
            per, work, _ = everything(ctx, [c.reads[i] for i in idx], batch_free=True)
            reached_x64(work, ctx.retry_report(), what)
            assert per == [want[i] for i in idx], what
    finally:
        ctx.close()
    ctx = context(c.pair, monkeypatch, level=1)
    try:
        for idx in (order[-30:], order[:40]):
            per, work, _ = everything(ctx, [c.reads[i] for i in idx], batch_free=True)
            rep = ctx.retry_report()
            assert work[0] == 0 and rep == dict(x8=work[5], x64=0, left=0, refused=0) and work[5] > 0, (work, rep)
            assert per == [want[i] for i in idx]
    finally:
        ctx.close()


def test_ensure_stage_picks_the_slots_of_the_x64_stage(gpu_pair, monkeypatch):
    """TALC_SEARCH_SLOTS unset: one slot per CU at x 64, at most one per read — twelve short reads."""
    c = case("default-k21", gpu_pair)
    reads = [s[:2000] for s in c.reads[:12]]
    want, _, _ = everything(c.pair.ctx, reads, batch_free=True)
    per, work, rep = run(c.pair, reads, monkeypatch, level=2, slots=None)
    reached_x64(work, rep, "slots by the device")
    assert per == want


def search_lines(trace):
    """The lines the search writes (searches, anchors, results, steps); the structure's lines and STATUS / OUT apart."""
    lines = trace.splitlines()
    return [l for l in lines if l[:2] in ("3 ", "4 ", "5 ", "6 ")], [l for l in lines if l[:2] not in ("3 ", "4 ", "5 ", "6 ")]


def test_trace_of_a_read_that_ends_in_the_x64_stage(gpu_pair, monkeypatch):
    """talc_batch_trace_read corrects the read as a batch of one, every pass writing into the one trace: the tiny first pass
    (the oracle's trace up to the step on which the oracle records its second bridge: the pinning of
    test_gpu_param_limits.trace_diff), the tiny x 8 pass, and last the x 64 pass, whose lines are the oracle's whole search
    trace; STATUS, the structure's lines and OUT are the oracle's."""
    c = case("long-gap", gpu_pair)
    read = c.reads[0]
    assert PLT.records_two_bridges(c.pair.otab.trace(read, steps=True))
    ctx = context(c.pair, monkeypatch, level=2, steps=True)
    try:
        assert PLT.trace_diff(c.pair.otab, ctx, read, tiny=True) == "overflow"
        assert ctx.retry_report() == dict(x8=1, x64=1, left=0, refused=0)       # (the report is the one-read correction's)
        b = ctx.batch(*PU.pack_reads([read]))
        try:
            got = b.trace(0)
        finally:
            b.close()
        assert ctx.retry_report() == dict(x8=1, x64=1, left=0, refused=0)
    finally:
        ctx.close()
    want_search, want_rest = search_lines(c.pair.otab.trace(read, steps=True))
    got_search, got_rest = search_lines(got)
    print("trace: oracle %d search lines, three passes %d" % (len(want_search), len(got_search)))
    assert got_rest == want_rest                                              # STATUS, threshold and regions, OUT
    assert len(got_search) > len(want_search) > 100
    assert got_search[-len(want_search):] == want_search                      # the last pass: the whole trace


def test_cli_under_the_hook_writes_the_files_of_the_run_without(tmp_path, monkeypatch):
    """The executable with every report option, TALC_TEST_TINY_CAPS=2 in its environment: every output file is the plain
    run's.  That the hook sends these reads to the x 64 stage is seen on a context over the same table."""
    c = G.gen_set("default")
    reads = c.reads[:60]
    ctx = context(c, monkeypatch, level=2)
    try:
        ctx.correct(*PU.pack_reads(reads))
        rep = ctx.retry_report()
        assert rep["x64"] == rep["x8"] > 0 and rep["left"] == 0, rep
    finally:
        ctx.close()
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    (tmp_path / "lr.fa").write_text("".join(">read%d\n%s\n" % (i, x) for i, x in enumerate(reads)))
    args = [PC.TALC, str(tmp_path / "lr.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "25", "-o", "o"] + PC.REPORT_OPTIONS
    plain_env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    for d, env in (("plain", plain_env), ("hook", dict(plain_env, TALC_TEST_TINY_CAPS="2", TALC_SEARCH_SLOTS=SLOTS))):
        (tmp_path / d).mkdir()
        r = subprocess.run(args, cwd=tmp_path / d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, (d, r.stderr.decode()[-800:])
    files = {d: sorted(f for f in os.listdir(tmp_path / d) if f.startswith("o.") and f != "o.log") for d in ("plain", "hook")}
    assert files["plain"] == files["hook"] and PC.REPORT_FILES <= {f[1:] for f in files["plain"]}, files
    for f in files["plain"]:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "hook" / f).read_bytes(), f


# ---------------------------------------------------------------- level 3
@pytest.mark.parametrize("name", ["default-k21", "paralogs-k21", "tandem-k21", "long-gap"])
def test_reads_that_exhaust_every_stage_leave_as_they_came(name, gpu_pair, monkeypatch):
    c = case(name, gpu_pair)
    want = c.plain[0]
    n = len(c.reads)
    refused, refused_work, refused_rep = run(c.pair, c.reads, monkeypatch, level=1, refuse=True)     # (what the other suites pin a failed read to)
    assert refused_rep == dict(x8=0, x64=0, left=refused_work[5], refused=1) and refused_work[6] == refused_work[5] > 0, (refused_rep, refused_work)
    per, work, rep = run(c.pair, c.reads, monkeypatch, level=3)
    print("retry stages %s, level 3: work %s, report %s" % (name, work, rep))
    flagged = [i for i in range(n) if per[i][F_STATUS] == T.READ_ERROR]
    assert work[0] == T.WARN_READ_ERRORS and 0 < work[6] == rep["left"] == len(flagged) <= work[5], (work, rep, len(flagged))
    assert rep["x8"] == work[5] and 0 < rep["x64"] <= rep["x8"] and rep["left"] <= rep["x64"] and rep["refused"] == 0, rep
    refused_set = {i for i in range(n) if refused[i][F_STATUS] == T.READ_ERROR}
    assert set(flagged) <= refused_set and refused_work[6] == len(refused_set)
    for i in range(n):
        if i in flagged:
            assert per[i][F_RECORD] == c.reads[i].encode(), i                 # byte-identical to its input
            seg = np.frombuffer(per[i][F_SEGS], dtype=T.SEGMENT_DTYPE)
            L = len(c.reads[i])
            assert seg.tolist() == [(T.SEG_RAW, 0, L, 0, L)] and per[i][F_SPLIT_TEXTS] == (), (i, seg.tolist())
            assert per[i] == refused[i], i                                    # one RAW segment, no piece, all '=', the raw rows
        else:
            assert per[i] == want[i], i


# ---------------------------------------------------------------- no hook
def test_constructed_read_is_served_by_the_x64_stage_without_a_hook(monkeypatch):
    """Position lists of 2600 entries: beyond the 2048 of the first pass and of the x 8 stage."""
    c = RC.constructed()
    p, q = PU.both_params(k=c.k)
    ot = O.OracleTable(q, O.OracleTable.FLAT)
    ot.insert_packed(c.keys, c.counts)
    ot.decolour()
    tt = T.Table.from_arrays(c.keys, c.counts, p)
    tt.decolour_repeats()
    tt.upload(0)
    o_out, o_off, o_st = ot.correct_batch(*PU.pack_reads([c.read]))
    monkeypatch.setenv("TALC_SEARCH_SLOTS", SLOTS)
    ctx = T.Context(tt, p, 0)
    monkeypatch.delenv("TALC_SEARCH_SLOTS")
    try:
        ctx.record_map(True)
        b = ctx.batch(*PU.pack_reads([c.read]))
        try:
            assert b.correct() == 0
            out, oo, st = b.fetch_corrected()
            segs, so = b.fetch_map()
        finally:
            b.close()
        t, rep = ctx.timing(), ctx.retry_report()
        print("constructed read: retried %d, report %s" % (t.n_retried, rep))
        assert rep == dict(x8=1, x64=1, left=0, refused=0) and t.n_failed == 0, rep
        assert int(st[0]) == int(o_st[0]) == T.READ_CORRECTED and bytes(out) == bytes(o_out) != c.read.encode()
        e = CM.expected(ot, c.read)
        assert e["status"] == 0 and e["out"].encode() == bytes(out) and len(e["segs"]) == 5         # head, region, weak stretch, region, tail
        assert np.array_equal(segs, CM.as_array(e["segs"])), (segs.tolist(), e["segs"])
        assert [s[0] for s in e["segs"]] == [T.SEG_CORRECTED, T.SEG_SOLID, T.SEG_RAW, T.SEG_SOLID, T.SEG_CORRECTED]
    finally:
        ctx.close()
        tt.close()
