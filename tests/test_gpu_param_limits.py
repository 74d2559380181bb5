"""-m gpu: the path search at the upper ends of its parameter ranges (tests/param_limit_cases.py; that the cases get there is
asserted from the oracle alone in tests/test_param_limits_reference.py).  k_search runs one wavefront per read, and the
values the C ABI accepts — 64 competing paths, 60 inner paths, 64 start anchors, any border limit, any check interval —
lead to Trail sets of two and three passes of 64, to gardening with MAXB = 64 over 81 and 192 candidates, and to anchor
lists cut at exactly 64.  Every read is compared with the oracle: record and status, and for the ladders and the
heaviest reads of every row the whole step trace, which pins the size of the set after every step and every gardening.
Under TALC_TEST_TINY_CAPS the trace hook shows the tiny first pass alone, so there the trace is pinned up to the step on
which the oracle records its second bridge and the retried read by record and status; the three ladders whose search
goes on after its cut, and the bush, are the ones that record one and so reach the retry pass (asserted)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
import param_limit_cases as PL
import parity_util as PU
from memcheck_util import guards_checked
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

SWITCHES = ("TALC_WALK", "TALC_TEST_EDGE_LANE", "TALC_TEST_TINY_CAPS", "TALC_TRACE_STEPS")


def trace_diff(otab, ctx, seq, tiny=False):
    """None, or the first line at which the HIP path's step trace of `seq` (a context made under TALC_TRACE_STEPS=1) and
    the oracle's differ, with the lines before it.  tiny: the context was made under TALC_TEST_TINY_CAPS=1, whose first
    pass holds one recorded bridge per start anchor; the trace hook shows that pass alone (the retry passes are the
    batch's), so the traces may part where the oracle records its second bridge, on a step line that agrees in step and
    set size — and nowhere before.  Returns "overflow" then."""
    to = otab.trace(seq, steps=True).splitlines()
    b = ctx.batch(*PU.pack_reads([seq]))
    try:
        tg = b.trace(0).splitlines()
    finally:
        b.close()
    assert sum(l.startswith("6 ") for l in to) > 0          # (a trace with its step lines)
    for i in range(min(len(to), len(tg))):
        if to[i] != tg[i]:
            fo, fg = to[i].split(" "), tg[i].split(" ")
            if tiny and fo[0] == fg[0] == "6" and fo[1:3] == fg[1:3] and int(fo[3]) > 1 and int(fg[3]) == 1:
                return "overflow"
            return dict(line=i, oracle=[l[:60] for l in to[max(0, i - 3):i + 2]], hip=[l[:60] for l in tg[max(0, i - 3):i + 2]])
    if len(to) != len(tg):
        n = min(len(to), len(tg))
        return dict(line=n, oracle=[l[:60] for l in to[n - 2:n + 2]], hip=[l[:60] for l in tg[n - 2:n + 2]], lines=(len(to), len(tg)))
    return None


def records_two_bridges(trace_text):
    """A start anchor of the oracle's trace records more than one bridge (the `6` line's third figure): more than a first
    pass under TALC_TEST_TINY_CAPS=1 holds, so the read goes to the retry pass."""
    inner = False
    for l in trace_text.splitlines():
        f = l.split(" ")
        if f[0] == "3":
            inner = int(f[1]) == PL.INNER
        elif f[0] == "6" and inner and int(f[3]) > 1:
            return True
    return False


def corrected(ctx, otab, reads, what):
    """The reads through one batch of ctx: 0 returned (no TALC_WARN_READ_ERRORS: no read fell to TALC_READ_ERROR), every
    record and status the oracle's.  Returns the oracle's (records, status)."""
    bases, offs = PU.pack_reads(reads)
    o_out, o_off, o_st = otab.correct_batch(bases, offs, nthreads=16)
    b = ctx.batch(bases, offs)
    try:
        rc = b.correct()
        g_out, g_off, g_st = b.fetch_corrected()
    finally:
        b.close()
    so, sg = PU.seqs_of(o_out, o_off), PU.seqs_of(g_out, g_off)
    bad = [i for i in range(len(so)) if so[i] != sg[i] or int(o_st[i]) != int(g_st[i])]
    if bad:
        class _P:
            pass
        pair = _P()
        pair.otab, pair.ctx = otab, ctx
        d = PU.first_trace_diff(pair, bases, offs, bad[0])
        raise AssertionError("%s: reads %s differ (of %d); status oracle / HIP of the first %d / %d; first trace difference of read %d: %s"
                             % (what, bad[:8], len(so), int(o_st[bad[0]]), int(g_st[bad[0]]), bad[0], d))
    assert rc == 0 and ctx.timing().n_failed == 0, (what, rc)
    assert not (np.asarray(g_st) == T.READ_ERROR).any()
    return so, np.asarray(o_st)


def clean_env(monkeypatch, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------- the synthetic rows
@pytest.mark.parametrize("case", list(PL.SYNTHETIC), ids=lambda c: PL.SYNTHETIC[c][0])
def test_row_at_the_limits_matches_oracle(case, monkeypatch):
    kw, pkw, n = PL.synthetic_row(case)
    clean_env(monkeypatch)
    pair = PU.Pair(**kw, **pkw)
    pair.upload(0)
    reads = PL.row_reads(pair.synth, case)
    assert len(reads) == n
    so, o_st = corrected(pair.ctx, pair.otab, reads, "row %d" % case)
    assert int((o_st == 0).sum()) > 0.85 * n                 # the draw really is corrected reads
    pair.ctx.close()
    # the three reads with the largest Trail set, and for the anchor rows the three with the longest anchor list: step by step
    clean_env(monkeypatch, TALC_TRACE_STEPS="1")
    ctx = T.Context(pair.ttab, pair.p, 0)
    first = reads[:32]
    with ThreadPoolExecutor(16) as ex:
        traces = list(ex.map(lambda s: pair.otab.trace(s, steps=True), first))
    picks = set(sorted(range(len(first)), key=lambda i: max(PL.largest_sets(traces[i]).values()))[-3:])
    if "anchors" in PL.SYNTHETIC[case][1]:
        picks |= set(sorted(range(len(first)), key=lambda i: PL.max_anchors(traces[i]))[-3:])
        assert max(PL.max_anchors(traces[i]) for i in picks) > 32
    try:
        for i in sorted(picks):
            d = trace_diff(pair.otab, ctx, first[i])
            assert d is None, ("row %d read %d" % (case, i), PL.largest_sets(traces[i]), PL.max_anchors(traces[i]), d)
    finally:
        ctx.close()
        pair.ttab.close()


# ---------------------------------------------------------------- the ladders
CONFIGS = {
    "walk-records": dict(TALC_WALK="1"),
    "no-walk-records": dict(TALC_WALK="0"),
    "edge-lane": dict(TALC_TEST_EDGE_LANE="1"),
    "no-edge-lane": dict(TALC_TEST_EDGE_LANE="0"),
    "retry-pass": dict(TALC_TEST_TINY_CAPS="1"),
    "poisoned": dict(),
}


def _ladder_run(name, config, monkeypatch):
    lad, pkw, why = PL.ladder_case(name)
    clean_env(monkeypatch, TALC_TRACE_STEPS="1", **CONFIGS[config])     # (the table's switch is read by the upload, the others by the context)
    pair = PU.CustomPair(lad.transcripts, k=lad.k, **pkw)
    pair.upload(0)
    try:
        what = "%s [%s]" % (name, config)
        top = PL.largest_sets(pair.otab.trace(lad.read, steps=True))
        assert top[why["location"]] == why.get("visible", why.get("scored", top[why["location"]])), (what, top)
        tiny = config == "retry-pass"
        overflows = tiny and records_two_bridges(pair.otab.trace(lad.read, steps=True))
        d = trace_diff(pair.otab, pair.ctx, lad.read, tiny)
        assert d == ("overflow" if overflows else None), (what, top, d)
        # the read three times in one batch (three waves at once on the same graph), record and status
        corrected(pair.ctx, pair.otab, [lad.read] * 3, what)
        if tiny:
            # (a ladder whose searches end above max_nb_inner_paths before they record a second bridge fits the tiny first pass)
            assert (pair.ctx.timing().n_retried > 0) == overflows, what
        return bool(overflows)
    finally:
        pair.ctx.close()
        pair.ttab.close()


@pytest.mark.parametrize("name", list(PL.LADDERS))
def test_ladder_step_by_step_under_every_switch(name, monkeypatch):
    """One ladder: the whole step trace (Batch.trace against OracleTable.trace(steps=True), line by line) and the record,
    with and without the walk records, with and without the fused edge lane, under TALC_TEST_TINY_CAPS (the retry pass
    for the ladders that record a second bridge: see the header), and on poisoned device memory between checked red
    zones (192 of TCAP = 320 slots of a Trail set; the bush's test fills them further)."""
    for config in CONFIGS:
        if config == "poisoned":
            with guards_checked():
                with T.poisoned(0xA5, 512):
                    _ladder_run(name, config, monkeypatch)
        else:
            retried = _ladder_run(name, config, monkeypatch)
            if config == "retry-pass":
                assert retried == ("cut" in PL.LADDERS[name][2] and PL.LADDERS[name][2]["location"] == PL.INNER), name


# ---------------------------------------------------------------- ladder reads between ordinary reads
class MixedPair:
    """Set 301's dump with the k-mers of the K = 21 ladders added (no k-mer in common), on both sides."""

    def __init__(self, ladders, **pkw):
        kw, _, _ = PL.synthetic_row(406)
        base = PU.Pair(**kw, **pkw)
        code = str.maketrans("ACGT", "0123")
        extra = {}
        for lad in ladders:
            assert lad.k == kw["k"]
            for km, c in PL.kmer_counts(lad.transcripts, lad.k).items():
                extra[int(km.translate(code), 4)] = extra.get(int(km.translate(code), 4), 0) + 20 * c
        ek = np.fromiter(extra.keys(), dtype=np.uint64, count=len(extra))
        assert not np.isin(ek, base.keys).any() and len(ek) == sum(len(PL.kmer_counts(l.transcripts, l.k)) for l in ladders)
        self.keys = np.concatenate([base.keys, ek])
        self.counts = np.concatenate([base.counts, np.fromiter(extra.values(), dtype=np.uint32, count=len(extra))])
        self.p, self.synth = base.p, base.synth
        base.ttab.close()
        self.otab = O.OracleTable(base.q, O.OracleTable.FLAT)
        self.otab.insert_packed(self.keys, self.counts)
        self.otab.decolour()
        self.ttab = T.Table.from_arrays(self.keys, self.counts, self.p)
        self.ttab.decolour_repeats()
        self.ttab.upload(0)


def test_ladder_reads_between_ordinary_reads_in_one_batch(monkeypatch):
    """A wave with 192 Trails in its scratch beside waves with ordinary reads: 60 reads of set 301 with four ladder reads
    (bridge 4-4-3-4-4 and 3-3-3-3-3, head and tail 4-4-3-4-4) between them, in the order given and in a permuted one, on
    one table.  Every record is the oracle's — the ladder reads' as much as their neighbours'."""
    clean_env(monkeypatch)
    names = ("bridge-k21-44344-ci5", "bridge-k21-33333-ci5", "tail-k21-44344", "head-k21-44344")
    ladders = [PL.ladder_case(n)[0] for n in names]
    pair = MixedPair(ladders, max_nb_competing_paths=64, max_nb_inner_paths=60, check_interval=5)
    reads = PU.seqs_of(*pair.synth.reads(0, 60))
    for at, lad in zip((3, 20, 21, 59), ladders):
        reads.insert(at, lad.read)
    where = [reads.index(l.read) for l in ladders]
    tops = [max(PL.largest_sets(pair.otab.trace(l.read, steps=True)).values()) for l in ladders]
    assert tops == [192, 81, 192, 192], tops                 # on the joint table the ladders are what they are alone
    ctx = T.Context(pair.ttab, pair.p, 0)
    try:
        so, _ = corrected(ctx, pair.otab, reads, "mixed batch")
        order = np.random.default_rng(4).permutation(len(reads)).tolist()
        so2, _ = corrected(ctx, pair.otab, [reads[i] for i in order], "mixed batch, permuted")
        assert so2 == [so[i] for i in order] and where == [3, 20, 21, 59]
    finally:
        ctx.close()
        pair.ttab.close()


# ---------------------------------------------------------------- more survivors than candidates
def test_bush_300_survivors_of_240_candidates(monkeypatch):
    """Gardening's "complex" branch keeps MAXB + n' of n candidates (param_limit_cases.bush: 64 + 236 of 240).  With 288
    slots per Trail set the HIP path raised OVF_TRAILS there, in the retry passes too, and the read came back as
    TALC_READ_ERROR where the reference goes on to its next attempt.  The oracle's step counts are asserted, then the
    whole trace and the record: on the first pass, through the retry pass, and on poisoned device memory between checked
    red zones — 300 of TCAP = 320 slots of a Trail set, 300 of the kept list's and 240 of the gardening workspace's TCAP + 64
    entries, 540 of NBUF = 576 sequence buffers: the furthest any accepted input fills them but for three more Trails."""
    B = PL.bush()
    for env in ({}, dict(TALC_TEST_TINY_CAPS="1"), "poisoned"):
        if env == "poisoned":
            with guards_checked():
                with T.poisoned(0xA5, 512):
                    _bush_run(B, {}, monkeypatch)
        else:
            _bush_run(B, env, monkeypatch)


def _bush_run(B, env, monkeypatch):
    clean_env(monkeypatch, TALC_TRACE_STEPS="1", **env)
    p, q = PU.both_params(k=B.k, **PL.BUSH_PARAMS)
    otab = O.OracleTable(q, O.OracleTable.FLAT)
    otab.insert_packed(B.keys, B.counts)
    otab.decolour()
    first = PL.searches(otab.trace(B.read, steps=True))[0]
    assert first["sizes"][0][-5:] == [60, 60, 60, 60, 300] and first["steps"][0][-1] == 61
    ttab = T.Table.from_arrays(B.keys, B.counts, p)
    ttab.decolour_repeats()
    ttab.upload(0)
    ctx = T.Context(ttab, p, 0)
    try:
        d = trace_diff(otab, ctx, B.read, bool(env))
        assert d == ("overflow" if env else None), (env, d)
        corrected(ctx, otab, [B.read, B.backbone, B.read], "bush %s" % env)
        assert (ctx.timing().n_retried > 0) == bool(env)
    finally:
        ctx.close()
        ttab.close()
