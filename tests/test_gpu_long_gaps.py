"""-m gpu: the path search across the sizes at which k_search changes what it does, and reads beyond 65 535 bases, against
the live oracle (tests/long_gap_cases.py; that every case crosses the switch point it is named after is asserted from
the oracle alone in tests/test_long_gap_reference.py).  Per case: the record and the status, and the whole step trace —
which pins the Trails after every step, so every gardening after every scoring of the two-Trail cases — under the default
switches, without the walk records (no wide cycle filter: the LDS one serves the same path), without the fused edge
lane, and on poisoned device memory between checked red zones.  Then what only a sequence of batches or a mixed batch
shows: the row arena and the wide filter are never reset between batches and the wave slots move when the longest read
changes; long reads beside short ones; the reverse strand and the correction map of records of 8 kb and more.

The oracle's half of a case is made once per process (long_gap_cases.oracle_side) and shared by every test here."""
import numpy as np
import pytest

import corr_map_ref as M
import long_gap_cases as LG
import oracle_lib as O
import parity_util as PU
from memcheck_util import guards_checked
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

SWITCHES = ("TALC_WALK", "TALC_TEST_EDGE_LANE", "TALC_TEST_TINY_CAPS", "TALC_TRACE_STEPS", "TALC_SEQ_ARENA")
SETTINGS = {"defaults": {}, "no-walk-records": dict(TALC_WALK="0"), "no-edge-lane": dict(TALC_TEST_EDGE_LANE="0")}


def clean_env(monkeypatch, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class Product:
    """The product's table of a dump, uploaded, and a context on it (the switches are read by the upload and by the
    context: set them before)."""

    def __init__(self, keys, counts, k, **pkw):
        self.p, _ = PU.both_params(k=k, **pkw)
        self.ttab = T.Table.from_arrays(keys, counts, self.p)
        self.ttab.decolour_repeats()
        self.ttab.upload(0)
        self.ctx = T.Context(self.ttab, self.p, 0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()
        self.ttab.close()


def product_of(side):
    return Product(*LG.packed_kmers(side.g.transcripts, side.g.k), side.g.k, **side.params)


def first_difference(want, got):
    """None, or where two trace texts part (parity_util.first_line_diff), the lines cut to their first 70 characters: a
    line of a long read's trace can hold a record."""
    d = PU.first_line_diff(want.splitlines(), got.splitlines())
    return d if d is None else (d[0], [l[:70] for l in d[1]], [l[:70] for l in d[2]])


def corrected(ctx, reads):
    """One batch: (records, statuses, return code, timing)."""
    b = ctx.batch(*PU.pack_reads(reads))
    try:
        rc = b.correct()
        out, off, st = b.fetch_corrected()
        return PU.seqs_of(out, off), [int(x) for x in st], rc, ctx.timing()
    finally:
        b.close()


def device_trace(ctx, read):
    b = ctx.batch(*PU.pack_reads([read]))
    try:
        return b.trace(0)
    finally:
        b.close()


def check_case(side, ctx, what, trace=True):
    """The case's read alone in a batch of ctx: record, status, counters and (a context made under TALC_TRACE_STEPS=1)
    the step trace, against the oracle's."""
    recs, st, rc, t = corrected(ctx, [side.g.read])
    print("%s: search %.1f ms, retry %.1f ms, %d trail steps, %d DP cells, retried %d" % (what, t.search_ms, t.retry_ms, t.n_trail_steps, t.n_dp_cells, t.n_retried))
    d = None
    if recs[0] != side.out or st[0] != side.status:
        d = first_difference(side.trace, device_trace(ctx, side.g.read))
    assert recs[0] == side.out and st[0] == side.status, (what, st[0], side.status, len(recs[0]), len(side.out), d)
    assert rc == 0 and t.n_failed == 0, (what, rc, t.n_failed)
    if side.why.get("retry"):
        assert t.n_retried >= 1, what
    else:
        assert t.n_retried == 0, what
        if trace:   # (the trace hook shows the first pass alone: a retried read's trace ends where that pass gave up)
            d = first_difference(side.trace, device_trace(ctx, side.g.read))
            assert d is None, (what, d)
    return t


# ---------------------------------------------------------------- every case under every switch
@pytest.mark.parametrize("name", list(LG.CASES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_case_matches_oracle(setting, name, monkeypatch):
    side = LG.oracle_side(name)
    clean_env(monkeypatch, TALC_TRACE_STEPS="1", **SETTINGS[setting])
    with product_of(side) as prod:
        check_case(side, prod.ctx, "%s [%s]" % (name, setting))


@pytest.mark.parametrize("name", LG.BOUNDARY + ["retry-for-real"])
def test_boundary_case_on_poisoned_memory(name, monkeypatch):
    """Two fills of every device buffer, red zones checked: a search that read a row record, a filter word or a Trail
    buffer it had not written would differ between the fills or from the oracle."""
    side = LG.oracle_side(name)
    for byte in (0xA5, 0xFF):
        with guards_checked():
            with T.poisoned(byte, 512):
                clean_env(monkeypatch, TALC_TRACE_STEPS="1")
                with product_of(side) as prod:   # (record, status and counters: the step trace is compared above)
                    check_case(side, prod.ctx, "%s [poison %02x]" % (name, byte), trace=False)


# ---------------------------------------------------------------- joint tables
class Joint:
    """One table over several dumps (no k-mer in common), on both sides."""

    def __init__(self, dumps, k=LG.K_DEFAULT, **pkw):
        keys = np.concatenate([d[0] for d in dumps])
        counts = np.concatenate([d[1] for d in dumps])
        assert len(np.unique(keys)) == sum(len(np.unique(d[0])) for d in dumps)
        self.k, self.pkw = k, pkw
        _, q = PU.both_params(k=k, **pkw)
        self.otab = O.OracleTable(q, O.OracleTable.FLAT)
        self.otab.insert_packed(keys, counts)
        self.otab.decolour()
        self.keys, self.counts = keys, counts

    def product(self):
        return Product(self.keys, self.counts, self.k, **self.pkw)

    def oracle(self, reads):
        out, off, st = self.otab.correct_batch(*PU.pack_reads(reads), nthreads=16)
        return PU.seqs_of(out, off), [int(x) for x in st]


def short_reads(n, seed=5):
    synth = Synth(target_kmers=60_000, k=LG.K_DEFAULT, seed=seed)
    return synth.dump_arrays(), PU.seqs_of(*synth.reads(0, n))


def test_one_context_over_batches_of_changing_shape(monkeypatch):
    """A long gap, 60 short reads, three gaps in one read, a reference of 8192 — twice over, on one context.  The row arena
    and the wide filter keep what the batch before left in them (a record is this search's only by its stamps, a filter
    is cleared by the search that uses it), and the slots are laid out again when the longest read changes."""
    clean_env(monkeypatch)
    cases = [LG.case(n)[0] for n in ("ref-8191", "two-long-gaps", "ref-8192")]
    dump, shorts = short_reads(60)
    # (one context, one set of parameters: the two-Trail cases' limit, and a check interval that scores each of them a few times)
    joint = Joint([LG.packed_kmers(g.transcripts, g.k) for g in cases] + [dump], **dict(LG.TWO, check_interval=250))
    batches = [[cases[0].read], shorts, [cases[1].read], [cases[2].read]]
    recs, st = joint.oracle([r for b in batches for r in b])
    want, at = [], 0
    for b in batches:
        want.append((recs[at:at + len(b)], st[at:at + len(b)]))
        at += len(b)
    assert all(s == 0 for s in st[:1] + st[-2:])
    with joint.product() as prod:
        for rnd in range(2):
            for i, (b, w) in enumerate(zip(batches, want)):
                recs, st, rc, t = corrected(prod.ctx, b)
                assert (recs, st) == w, ("round %d batch %d" % (rnd, i), [j for j in range(len(b)) if recs[j] != w[0][j]][:5])
                assert rc == 0 and t.n_failed == 0 and t.n_retried == 0


# ---------------------------------------------------------------- reads beyond 65 535 bases
_long = {}


def long_side(k):
    """The long reads of one K on a table of their transcript and of 200 short reads' generator, with the oracle's
    record and status of every read."""
    if k not in _long:
        L = LG.long_reads(k)
        synth = Synth(target_kmers=60_000, k=k, seed=5)
        L.joint = Joint([LG.packed_kmers(L.transcripts, k), synth.dump_arrays()], k=k)
        L.shorts = PU.seqs_of(*synth.reads(0, 200))
        L.names = list(L.reads)
        L.all = [L.reads[n] for n in L.names] + L.shorts
        L.want = L.joint.oracle(L.all)
        _long[k] = L
    return _long[k]


@pytest.mark.parametrize("k", [21, 18, 31])
def test_long_reads_alone_and_between_short_reads(k, monkeypatch):
    """65 535 + K, 65 537 + K and 140 000 bases, one of them with an 8.3 kb comb: each alone in a batch (8 arena buffers of
    the longest stride, regCap in the tens of thousands), then all four between 200 short reads in one permuted batch —
    every record the oracle's, and the same as alone."""
    clean_env(monkeypatch)
    L = long_side(k)
    wrec, wst = L.want
    assert all(s == 0 for s in wst[:4])
    with L.joint.product() as prod:
        for i, n in enumerate(L.names):
            recs, st, rc, t = corrected(prod.ctx, [L.all[i]])
            print("K = %d %s alone: search %.1f ms, retry %.1f ms, retried %d" % (k, n, t.search_ms, t.retry_ms, t.n_retried))
            assert recs[0] == wrec[i] and st[0] == wst[i], (k, n, len(recs[0]), len(wrec[i]))
            assert rc == 0 and t.n_failed == 0
        order = np.random.default_rng(6).permutation(len(L.all)).tolist()
        recs, st, rc, t = corrected(prod.ctx, [L.all[i] for i in order])
        bad = [i for j, i in enumerate(order) if recs[j] != wrec[i] or st[j] != wst[i]]
        assert not bad, (k, bad[:8])
        assert rc == 0 and t.n_failed == 0


def test_comb_gap_of_the_140k_read_step_by_step(monkeypatch):
    """The trace of the 140 kb read with the comb: all of it, the search of the 8.3 kb gap among 1800 others."""
    clean_env(monkeypatch, TALC_TRACE_STEPS="1")
    L = long_side(LG.K_DEFAULT)
    read = L.reads["140k-comb"]
    want = LG.traced(L.joint.otab, read)[0]
    longest = max(len(r["steps"]) for s in LG.runs(want) for r in s["runs"])
    assert longest >= LG.LONG_COMB                               # the comb's search is in it
    with L.joint.product() as prod:
        d = first_difference(want, device_trace(prod.ctx, read))
        assert d is None, d


# ---------------------------------------------------------------- the reverse strand and the correction map
def reverse_and_map_inputs():
    """(name, transcripts, read, parameters) of the three cases run under reverse = 1 and with the map, and of the fourth
    that is run with the map alone."""
    L = LG.long_reads(LG.K_DEFAULT)
    out = []
    for n in ("ref-8192", "trail-past-8191"):
        g, pkw, _ = LG.case(n)
        out.append((n, g.transcripts, g.read, pkw))
    out.append(("140k-comb", L.transcripts, L.reads["140k-comb"], {}))
    out.append(("65537+K", L.transcripts, L.reads["65537+K"], {}))
    return out


@pytest.mark.parametrize("which", range(3), ids=["ref-8192", "trail-past-8191", "140k-comb"])
def test_reverse_strand_of_a_long_record(which, monkeypatch):
    """reverse = 1: the context corrects the reverse complement of what it is given and k_pack turns the record back, 8 kb
    and more of it through its word path."""
    clean_env(monkeypatch)
    name, transcripts, read, pkw = reverse_and_map_inputs()[which]
    pkw = dict(pkw, reverse=1)
    given = PU.revcomp(read)
    keys, counts = LG.packed_kmers(transcripts, LG.K_DEFAULT)
    otab = LG.oracle_table(transcripts, LG.K_DEFAULT, **pkw)
    _, status, out, _, _ = LG.traced(otab, given)
    assert status == 0 and len(out) >= 8000
    with Product(keys, counts, LG.K_DEFAULT, **pkw) as prod:
        recs, st, rc, t = corrected(prod.ctx, [given])
        assert recs[0] == out and st[0] == status, (name, len(recs[0]), len(out))
        assert rc == 0 and t.n_failed == 0


@pytest.mark.parametrize("which", range(4), ids=["ref-8192", "trail-past-8191", "140k-comb", "65537+K"])
def test_correction_map_of_a_long_record(which, monkeypatch):
    """The map against corr_map_ref.expected: one CORRECTED segment whose out_len is a whole long gap, and for the long
    reads many passes of 64 segments in k_pack_map."""
    clean_env(monkeypatch)
    name, transcripts, read, pkw = reverse_and_map_inputs()[which]
    keys, counts = LG.packed_kmers(transcripts, LG.K_DEFAULT)
    e = M.expected(LG.oracle_table(transcripts, LG.K_DEFAULT, **pkw), read)
    longest = max(s[4] for s in e["segs"] if s[0] == M.CORRECTED)
    assert e["status"] == 0 and (longest >= 7700 if which < 3 else len(e["segs"]) > 64 * 8), (name, longest, len(e["segs"]))
    with Product(keys, counts, LG.K_DEFAULT, **pkw) as prod:
        prod.ctx.record_map(True)
        b = prod.ctx.batch(*PU.pack_reads([read]))
        try:
            rc = b.correct()
            out, off, st = b.fetch_corrected()
            segs, so = b.fetch_map()
        finally:
            b.close()
            prod.ctx.record_map(False)
        w = M.as_array(e["segs"])
        assert rc == 0 and int(st[0]) == e["status"] and PU.seqs_of(out, off)[0] == e["out"], name
        assert len(segs) == len(w) == int(so[-1]) and (segs == w).all(), (name, len(segs), len(w), np.nonzero(segs != w)[0][:4].tolist() if len(segs) == len(w) else None)
