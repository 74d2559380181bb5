"""The C ABI's threading contract (include/talc_hip.h, docs/threading.md): contexts and counters used from concurrent host
threads, one owner thread each, over tables they share.

The harness starts N Python threads (calls through ctypes.CDLL release the GIL, so the library calls run side by side),
lets them go together through a threading.Barrier at the start of every round, and records the time.perf_counter() interval
of every library call a thread makes (TimedLib stands in for lib.lib() while the threads run).  A thread asserts nothing: it
returns what it got, the main thread joins all of them and compares.  That the calls really overlapped is a condition of
every test, computed from the intervals: in every round every thread has a call that intersects a call of another thread.

Wanted values: the same helper run on one thread on a fresh context before any thread starts (memcheck_util.everything, whose
outputs the per-feature files hold to the oracle and the numpy contracts; prep_ref.chain; kmer_ref, fold_ref, spectrum_ref;
the oracle table's lookup and next_counts), and every thread's records and status directly against the oracle's
correct_batch of its reads.  Integers and bytes, tolerance 0.

Nine roles are asked for and at most eight threads: the table reader's calls are made by the two counter threads (they own
no context), one per table, after their counter's own calls of the round."""
import contextlib
import json
import os
import subprocess
import threading
import time
import traceback

import numpy as np
import pytest

import corr_map_ref as M
import demux_ref as DR
import ends_ref as R
import fold_ref as F
import kmer_ref as KR
import memcheck_util as MU
import oracle_lib as O
import parity_util as PU
import prep_ref as P
import solidity_ref as S
import spectrum_ref as SP
import strand_ref as SR
import test_gpu_prep_chain as GP
import test_gpu_solidity as G
import umi_ref as U
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

ROUNDS = 3
BARRIER_TIMEOUT = 120          # seconds; a thread that fails aborts the barrier, so nobody waits this long
JOIN_TIMEOUT = 300
ERR_INVALID, ERR_STATE = -1, -6
HISTO_HIGH = 50


# ---------------------------------------------------------------- the harness
class TimedLib:
    """Stands in for the loaded library: every call made by a thread that has a log (begin()) is recorded there as
    (name, t0, t1) of time.perf_counter()."""

    def __init__(self, real):
        self._real = real
        self._tls = threading.local()

    def begin(self, log):
        self._tls.log = log

    def mark(self):
        """How many calls the calling thread's log holds."""
        return len(self._tls.log)

    def __getattr__(self, name):
        f = getattr(self._real, name)
        tls = self._tls

        def call(*args):
            log = getattr(tls, "log", None)
            if log is None:
                return f(*args)
            t0 = time.perf_counter()
            try:
                return f(*args)
            finally:
                log.append((name, t0, time.perf_counter()))
        return call


@contextlib.contextmanager
def timed_library():
    real = T.lib()
    timed = TimedLib(real)
    T._LIB = timed
    try:
        yield timed
    finally:
        T._LIB = real


def run_threads(bodies, rounds=ROUNDS):
    """bodies: [(name, fn(round) -> result)].  Every thread waits at the barrier, then runs its fn, `rounds` times over.
    Returns {name: dict(rounds=[(result, log)], error=None or the traceback)} once every thread has been joined."""
    assert len(bodies) <= 8
    barrier = threading.Barrier(len(bodies))
    out = {name: dict(rounds=[], error=None) for name, _ in bodies}
    assert len(out) == len(bodies)

    with timed_library() as timed:
        def main(name, fn):
            res = out[name]
            try:
                for r in range(rounds):
                    barrier.wait(BARRIER_TIMEOUT)
                    log = []
                    timed.begin(log)
                    try:
                        res["rounds"].append((fn(r), log))
                    finally:
                        timed.begin(None)
            except BaseException:
                res["error"] = traceback.format_exc()
                barrier.abort()

        threads = [threading.Thread(target=main, args=b, name=b[0], daemon=True) for b in bodies]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_TIMEOUT)
        alive = [t.name for t in threads if t.is_alive()]
    assert not alive, ("threads still running", alive)
    errors = {n: r["error"] for n, r in out.items() if r["error"]}
    own = {n: e for n, e in errors.items() if "BrokenBarrierError" not in e}      # (the others only met the aborted barrier)
    assert not errors, "\n".join("%s:\n%s" % kv for kv in (own or errors).items())
    return out


def overlaps(logs):
    """(pairs of calls of two different threads whose intervals intersect, the threads without any) of {thread: log}."""
    events = sorted((t0, t1, th) for th, log in logs.items() for _, t0, t1 in log)
    active, pairs, hit = [], 0, set()
    for t0, t1, th in events:
        active = [(e, o) for e, o in active if e > t0]
        for _, o in active:
            if o != th:
                pairs += 1
                hit.update((o, th))
        active.append((t1, th))
    return pairs, sorted(th for th in logs if th not in hit)


def check_overlap(results, what):
    """The stated condition: in every round every thread has a library call that intersects a call of another thread."""
    rounds = len(next(iter(results.values()))["rounds"])
    for r in range(rounds):
        logs = {name: res["rounds"][r][1] for name, res in results.items()}
        pairs, lonely = overlaps(logs)
        long_ones = {name: [c for c in log if c[0] in ("talc_batch_correct", "talc_correct_batch", "talc_counter_add", "talc_batch_create_split")]
                     for name, log in logs.items()}
        print("%s, round %d: %d overlapping call pairs between %d threads (%d between corrections / counter adds), %s calls" % (
            what, r, pairs, len(logs), overlaps(long_ones)[0], [len(log) for log in logs.values()]))
        assert not lonely, (what, r, "no call of these threads overlapped another thread's", lonely)


# ---------------------------------------------------------------- the helpers both sides run: one thread before, N threads after
def plain_everything(ctx, reads, order):
    per, work, rows = MU.everything(ctx, reads, order)
    return per, work, None if rows is None else rows.tobytes()


def prepared_everything(ctx, reads):
    """A split and clipped batch of `reads` on a context with the four preparation settings: every report, then everything
    the corrected batch gives."""
    ctx.record_map(True)
    b = ctx.batch(*R.batch(reads), clip=True, split=True)
    try:
        rep = dict(n=b.n_reads, n_bases=b.n_bases, demux=b.demux(), umi=b.umi(), ends=b.ends())
        rep["hits"], rep["hit_off"] = b.chimera()
        rep["pieces"], rep["piece_off"] = b.split_pieces()
        rc = b.correct()
        t = ctx.timing()
        work = (rc, t.n_trail_steps, t.n_dp_cells, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)
        return MU.per_read(MU.fetch_all(b), b.n_reads), work, rep
    finally:
        b.close()
        ctx.record_map(False)


def counted(params, chunks, both):
    """A counter of its own that starts at the smallest hash and grows: the adds, then stats, fetch and histo."""
    c = T.KmerCounter(params, 0, expected_distinct=1, both_strands=both)
    try:
        for bases, offs in chunks:
            c.add(bases, offs)
        st = c.stats()
        km, ct = c.fetch(1)
        o = np.argsort(km, kind="stable")
        hist, hstats = c.histo(HISTO_HIGH)
        return km[o].tobytes(), ct[o].tobytes(), st, hist.tobytes(), hstats
    finally:
        c.close()


def table_reads(tab, q):
    c, j = tab.lookup(q)
    n0, n1 = tab.next_counts(q, 0), tab.next_counts(q, 1)
    hist, hstats = tab.histo(0, HISTO_HIGH)
    return c.tobytes(), j.tobytes(), n0[0].tobytes(), n0[1].tobytes(), n1[0].tobytes(), n1[1].tobytes(), hist.tobytes(), hstats


def fresh(pair, fn, *args, auto=False):
    """fn(ctx, *args) on a context made for this one call."""
    ctx = T.Context(pair.ttab, pair.p, 0)
    try:
        if auto:
            ctx.auto_strand(True)
        return fn(ctx, *args)
    finally:
        ctx.close()


# ---------------------------------------------------------------- the inputs: disjoint slices of the sets the suite builds
# the second preparation kit: other primers (a template-switch oligo and a sequencing adapter, both published), 12 barcodes
# of 16 letters (one pass of the demux kernel, where the first kit's 96 take three) and a shorter UMI pattern
SSP_B, VNP_B = "AAGCAGTGGTATCAACGCAGAGT", "CTACACGACGCTCTTCCGATCT"
UMI_B = "CAGNNNNNNNNNNNNACG"
KIT_B = dict(ends=dict(adapters=[SSP_B, VNP_B], max_error_pct=15, poly_min=10, window=256), chimera=(True, 15, 60), umi=(UMI_B, 10, 128))
KIT_A = dict(ends=P.ENDS_KW, chimera=P.CHIMERA, demux=P.DEMUX, umi=P.UMI)


def dressed_b(bodies, rng, barcodes):
    """prep_ref.reads_of with the second kit's parts: barcode' . junk . SSP . umi' . body . A{15..39} . revcomp(VNP) . junk .
    revcomp(barcode''), or the reverse complement of all of it; every ninth body bare, every tenth read joined to the next."""
    junk = lambda: R.random_seq(rng, int(rng.integers(0, 11)))

    def dress(body):
        bc = barcodes[int(rng.integers(len(barcodes)))]
        copy = lambda: R.mutate(rng, bc, int(rng.integers(0, 3)), "SID")
        umi = R.mutate(rng, U.instance(rng, UMI_B), int(rng.integers(0, 2)), "SID")
        s = copy() + junk() + SSP_B + umi + body + "A" * int(rng.integers(15, 40)) + R.revcomp(VNP_B).decode() + junk() + R.revcomp(copy()).decode()
        return s if rng.integers(2) else R.revcomp(s).decode()

    one = [b if i % 9 == 4 else dress(b) for i, b in enumerate(bodies)]
    reads, i = [], 0
    while i < len(one):
        if i % 10 == 9 and i + 1 < len(one):
            joint = "A" * 30 + R.mutate(rng, R.revcomp(VNP_B).decode(), int(rng.integers(0, 3))) + R.mutate(rng, SSP_B, int(rng.integers(0, 3)))
            reads.append(one[i] + joint + one[i + 1])
            i += 2
        else:
            reads.append(one[i])
            i += 1
    return reads + ["", "ACGT", SSP_B + U.instance(rng, UMI_B), barcodes[0]]


def set_kit(ctx, kit):
    ctx.set_ends(**kit["ends"])
    ctx.set_chimera(*kit["chimera"])
    ctx.set_demux(*kit["demux"])
    ctx.set_umi(*kit["umi"])


def oracle_records(otab, reads):
    out, oo, st = otab.correct_batch(*PU.pack_reads(reads), nthreads=16)
    return [x.encode() for x in PU.seqs_of(out, oo)], np.asarray(st).tolist()


def queries(pair, seed):
    """2000 k-mers the table was built from and 2000 random ones (absent: 4^K is far above the table's size)."""
    rng = np.random.default_rng(seed)
    stored = rng.choice(pair.keys[pair.counts >= pair.p.min_count], 2000, replace=False)
    absent = rng.integers(0, 1 << (2 * int(pair.p.k)), 2000, dtype=np.uint64)
    return np.concatenate([stored, absent]).astype(np.uint64)


def oracle_table_reads(pair, q):
    """What table_reads must give, from the oracle's table and spectrum_ref."""
    k = int(pair.p.k)
    c, j = pair.otab.lookup_packed(q)
    out = [c.tobytes(), j.tobytes()]
    for direction in (0, 1):
        rows = [pair.otab.next_counts(KR.unpack(x, k), direction) for x in q.tolist()]
        out += [np.array([r[0] for r in rows], np.uint32).tobytes(), np.array([r[1] for r in rows], np.uint32).tobytes()]
    stored = pair.otab.lookup_packed(np.unique(pair.keys))[0]          # (the generator's dump names a few k-mers twice)
    hist, hstats = SP.histo(stored[stored >= pair.p.min_count], HISTO_HIGH)
    return tuple(out) + (hist.tobytes(), hstats)


_in = {}


def inputs():
    """Everything the tests share, computed once on the main thread and left unchanged: per role its reads, what the same
    helper gives on a fresh context of one thread, and what the oracle and the numpy contracts say."""
    if _in:
        return _in
    s21, s31 = M.map_set("default"), M.map_set("k31")
    for s in (s21, s31):
        s.pair.ttab.upload(0)
    r21, r31 = s21.reads, s31.reads
    p21 = s21.pair
    role = {}

    def corrected(name, pair, reads, order, env=None, auto=False):
        """A role that runs everything() on plain batches: reads per round, the single-thread run, the oracle's records."""
        rounds = reads if isinstance(reads[0], list) else [reads]
        for key, value in (env or {}).items():
            os.environ[key] = value
        try:
            want = [fresh(pair, plain_everything, x, order, auto=auto) for x in rounds]
        finally:
            for key in env or {}:
                del os.environ[key]
        role[name] = dict(pair=pair, reads=rounds, order=order, env=env, auto=auto, want=want, oracle=[oracle_records(pair.otab, x) for x in rounds])

    corrected("plain", p21, r21[0:40], MU.FORWARD)
    auto_reads = r21[40:70] + [M.revcomp(x) for x in r21[70:72]]
    corrected("auto strand", p21, auto_reads, MU.BACKWARD, auto=True)
    corrected("retry stage", p21, r21[72:112], MU.FORWARD, env=dict(TALC_TEST_TINY_CAPS="1"))
    # changing shape: the longest read of each round differs; round 1 carries one read of about 20 kb, built from the set's
    # own reads joined end to end (so the K = 31 table it shares with nobody else has its k-mers, and the oracle corrects it)
    long_read, i = "", 100
    while len(long_read) < 20_000:
        long_read += r31[i]
        i += 1
    by_len = sorted(r31[0:90], key=len)
    shape = [by_len[0:30], by_len[30:50] + [long_read], by_len[50:90]]
    corrected("changing shape", s31.pair, shape, MU.FORWARD)

    # the auto-strand role against the oracle in the orientation strand_ref chooses
    rows = SR.rows(auto_reads, int(p21.p.k), p21.p.min_count, S.host_lookup(p21.ttab))
    _, q = PU.both_params(k=int(p21.p.k), reverse=1)
    rev = O.OracleTable(q, O.OracleTable.FLAT)
    rev.insert_packed(p21.keys, p21.counts)
    rev.decolour()
    both = (role["auto strand"]["oracle"][0], oracle_records(rev, auto_reads))
    rev.close()
    role["auto strand"]["oracle"] = [([both[int(v)][0][i] for i, v in enumerate(rows["reverse"])], [both[int(v)][1][i] for i, v in enumerate(rows["reverse"])])]
    role["auto strand"]["rows"] = rows.tobytes()

    # prepared: two kits on disjoint bodies
    KIT_B["demux"] = (DR.barcode_set(12, 16, seed=23, min_dist=6), 20, 2)
    prepared = {"prepared A": (KIT_A, P.reads_of(r21[112:152], np.random.default_rng(41))),
                "prepared B": (KIT_B, dressed_b(r21[152:192], np.random.default_rng(42), KIT_B["demux"][0]))}
    for name, (kit, reads) in prepared.items():
        ref = P.chain(reads, kit["ends"], kit["chimera"], kit["demux"], kit["umi"], clip=True, split=True)
        want = fresh(p21, lambda ctx: (set_kit(ctx, kit), prepared_everything(ctx, reads))[1])
        role[name] = dict(pair=p21, kit=kit, reads=reads, ref=ref, want=want, base=fresh(p21, plain_everything, ref["texts"], MU.FORWARD),
                          oracle=oracle_records(p21.otab, ref["texts"]))

    # counters: 4000 short reads each in four adds; table readers: one per table
    syn = Synth(target_kmers=150_000, k=21, seed=77)
    params = T.default_params(k=21)
    for name, both_strands, first, pair in (("counter", False, 0, p21), ("counter, both strands", True, 4000, s31.pair)):
        bases, offs = syn.short_reads(first, 4000, length=150, sub_rate=0.01, n_rate=0.002)
        chunks = [(bases[int(offs[a]):int(offs[b])].copy(), (offs[a:b + 1] - offs[a]).copy()) for a, b in ((0, 1000), (1000, 2000), (2000, 2001), (2001, 4000))]
        if both_strands:
            km, ct = F.fold_records(bases, offs, 21)
            assert int(ct.max()) < 1 << 32
        else:
            km, ct = KR.count(bases, offs, 21)
        hist, hstats = SP.histo(ct, HISTO_HIGH)
        ref = (km.tobytes(), ct.astype(np.uint32).tobytes(), (int(ct.sum()), len(km), int((ct >= params.min_count).sum())), hist.tobytes(), hstats)
        q = queries(pair, 5 + first)
        role[name] = dict(params=params, chunks=chunks, both=both_strands, ref=ref, want=counted(params, chunks, both_strands), distinct=len(km),
                          pair=pair, q=q, table_ref=oracle_table_reads(pair, q), table_want=table_reads(pair.ttab, q))
    syn.close()
    _in.update(s21=s21, s31=s31, role=role)
    return _in


def test_the_inputs_do_what_they_are_there_for():
    """The single-thread runs against the oracle and the numpy contracts, and each role's reason to be there."""
    role = inputs()["role"]
    for name in ("plain", "auto strand", "retry stage", "changing shape"):
        ro = role[name]
        for reads, (per, work, rows), (recs, st) in zip(ro["reads"], ro["want"], ro["oracle"]):
            assert [t[MU.F_RECORD] for t in per] == recs and [t[MU.F_STATUS] for t in per] == st, name
            assert work[0] == 0 and work[6] == 0 and work[1] > 0 and work[2] > 0, (name, work)
            assert st.count(T.READ_CORRECTED) >= len(reads) // 2, (name, st)
    assert 40 <= len(role["plain"]["reads"][0]) <= 60
    assert role["auto strand"]["want"][0][2] == role["auto strand"]["rows"]
    assert np.frombuffer(role["auto strand"]["rows"], SR.DTYPE)["reverse"][-2:].tolist() == [1, 1]
    assert role["retry stage"]["want"][0][1][5] > 0                                  # n_retried, n_failed == 0 above
    assert role["plain"]["want"][0][1][5] == 0
    longest = [max(len(x) for x in reads) for reads in role["changing shape"]["reads"]]
    assert len(set(longest)) == 3 and 20_000 <= longest[1] < 24_000 and max(longest[0], longest[2]) < 5000, longest
    works = [w for name in ("plain", "auto strand", "retry stage", "changing shape", "prepared A", "prepared B") for w in
             ([x[1] for x in role[name]["want"]] if isinstance(role[name]["want"], list) else [role[name]["want"][1]])]
    assert len(set(works)) == len(works), works                                      # a context that saw another's counters would show
    for name in ("prepared A", "prepared B"):
        ro = role[name]
        per, work, rep = ro["want"]
        check_prepared(name, ro, per, work, rep)
        ref = ro["ref"]
        assert 35 <= len(ro["reads"]) <= 45 and len(ref["pieces"]) > len(ro["reads"]) and len(ref["hits"]) >= 3, (name, len(ro["reads"]), len(ref["pieces"]))
        seen = np.bincount(ref["demux"]["status"], minlength=5)
        assert seen[DR.BOTH] >= 10 and seen[DR.NONE] >= 3, (name, seen)
        assert (ref["umi"]["end"] != 0).sum() >= 10 and (ref["ends"]["kept_len"] < [len(x) for x in ref["came"]]).sum() >= 20, name
        assert work[1] > 0
    a, b = role["prepared A"]["kit"], role["prepared B"]["kit"]
    assert not set(a["ends"]["adapters"]) & set(b["ends"]["adapters"]) and a["umi"][0] != b["umi"][0] and len(a["demux"][0]) != len(b["demux"][0])
    for name in ("counter", "counter, both strands"):
        ro = role[name]
        assert ro["want"] == ro["ref"], (name, [i for i, (x, y) in enumerate(zip(ro["want"], ro["ref"])) if x != y])
        assert ro["distinct"] > 2 * 0.7 * (1 << 16)                                  # the smallest hash holds 45 875: it grew, twice
        assert ro["table_want"] == ro["table_ref"], (name, [i for i, (x, y) in enumerate(zip(ro["table_want"], ro["table_ref"])) if x != y])
        c = np.frombuffer(ro["table_ref"][0], np.uint32)
        assert (c[:2000] >= ro["pair"].p.min_count).all() and not c[2000:].any()
    assert role["counter"]["pair"] is not role["counter, both strands"]["pair"]


def check_prepared(name, ro, per, work, rep):
    """One prepared run against chain(), against plain batches of the host-cut texts, and against the oracle."""
    ref, (base_per, base_work, _) = ro["ref"], ro["base"]
    assert rep["n"] == len(ref["texts"]) and rep["n_bases"] == sum(len(x) for x in ref["texts"]), name
    for key in GP.REPORTS:
        assert rep[key].dtype == ref[key].dtype and len(rep[key]) == len(ref[key]), (name, key)
        bad = np.flatnonzero(rep[key] != ref[key])
        assert len(bad) == 0, (name, key, len(bad), int(bad[0]), rep[key][bad[0]].tolist(), ref[key][bad[0]].tolist())
    d = MU.first_difference(per, base_per)
    assert d is None, (name, "against plain batches of the texts", d)
    assert work == base_work, (name, work, base_work)
    recs, st = ro["oracle"]
    assert [t[MU.F_RECORD] for t in per] == recs and [t[MU.F_STATUS] for t in per] == st, (name, "against the oracle")


# ---------------------------------------------------------------- 1. and 2. every role at once
def every_role_at_once():
    """The eight threads over three rounds; contexts made and closed here, on the main thread (the retry stage's while
    TALC_TEST_TINY_CAPS is set: a context keeps its own copy of the switches).  Returns the threads' results."""
    role = inputs()["role"]
    ctxs = {}
    try:
        for name in ("retry stage", "plain", "auto strand", "changing shape", "prepared A", "prepared B"):
            ro = role[name]
            for key, value in (ro.get("env") or {}).items():
                os.environ[key] = value
            try:
                ctxs[name] = T.Context(ro["pair"].ttab, ro["pair"].p, 0)
            finally:
                for key in ro.get("env") or {}:
                    del os.environ[key]
            if ro.get("auto"):
                ctxs[name].auto_strand(True)
            if "kit" in ro:
                set_kit(ctxs[name], ro["kit"])
        assert "TALC_TEST_TINY_CAPS" not in os.environ

        def corrector(name):
            ro, ctx = role[name], ctxs[name]
            return lambda r: (plain_everything(ctx, ro["reads"][r % len(ro["reads"])], ro["order"]), T.poison_setting())

        def preparer(name):
            ro, ctx = role[name], ctxs[name]
            return lambda r: (prepared_everything(ctx, ro["reads"]), T.poison_setting())

        def counter(name):
            ro = role[name]
            return lambda r: (counted(ro["params"], ro["chunks"], ro["both"]), [table_reads(ro["pair"].ttab, ro["q"]) for _ in range(3)], T.poison_setting())

        bodies = [(n, corrector(n)) for n in ("plain", "auto strand", "retry stage", "changing shape")]
        bodies += [(n, preparer(n)) for n in ("prepared A", "prepared B")] + [(n, counter(n)) for n in ("counter", "counter, both strands")]
        return run_threads(bodies)
    finally:
        for ctx in ctxs.values():
            ctx.close()


def check_every_role(results, what, setting=(-1, 0)):
    role = inputs()["role"]
    check_overlap(results, what)
    for name, res in results.items():
        ro = role[name]
        assert len(res["rounds"]) == ROUNDS, (what, name)
        for r, (got, _) in enumerate(res["rounds"]):
            where = (what, name, "round %d" % r)
            assert got[-1] == setting, (where, "the poison setting as this thread sees it", got[-1])
            if "chunks" in ro:
                assert got[0] == ro["want"] == ro["ref"], (where, [i for i, (x, y) in enumerate(zip(got[0], ro["ref"])) if x != y])
                for t in got[1]:
                    assert t == ro["table_want"] == ro["table_ref"], (where, [i for i, (x, y) in enumerate(zip(t, ro["table_ref"])) if x != y])
                continue
            per, work, extra = got[0]
            if "kit" in ro:
                want_per, want_work, _ = ro["want"]
                check_prepared(where, ro, per, work, extra)
            else:
                (want_per, want_work, want_rows), (recs, st) = ro["want"][r % len(ro["want"])], ro["oracle"][r % len(ro["oracle"])]
                assert extra == want_rows, (where, "strand rows")
                assert [t[MU.F_RECORD] for t in per] == recs and [t[MU.F_STATUS] for t in per] == st, (where, "against the oracle")
            d = MU.first_difference(per, want_per)
            assert d is None, (where, "read and fields that differ from the single-thread run", d)
            print("%s: rc, n_trail_steps, n_dp_cells, n_kmers, n_bases, n_retried, n_failed %s (one thread: %s)" % (where, work, want_work))
            assert work == want_work, (where, work, want_work)
            if name == "retry stage":
                assert work[5] > 0 and work[6] == 0, (where, work)


def test_every_role_at_once():
    check_every_role(every_role_at_once(), "every role")


@pytest.mark.parametrize("byte", [0xA5, 0xFF], ids=lambda b: "0x%02X" % b)
def test_every_role_at_once_on_poisoned_memory_between_red_zones(byte):
    inputs()                                                          # (the wanted values, made before the poison is on)
    with MU.guards_checked() as before:
        with T.poisoned(byte):
            results = every_role_at_once()
    after = T.guard_report()
    print("red zones checked: %d, violations: %d, requests served from the caches: %d" % (
        after["checked"] - before["checked"], after["violations"], after["reused"] - before["reused"]))
    # every buffer of the concurrent phase sat between red zones: six contexts with every output, three times over, hand
    # back some hundreds of buffers, and from the second round on their caches serve requests with buffers used before
    assert after["checked"] - before["checked"] >= 500 and after["reused"] - before["reused"] >= 100
    check_every_role(results, "poisoned %#x" % byte, setting=(byte, 256))


# ---------------------------------------------------------------- 3. lifecycle under load
def test_contexts_created_and_destroyed_while_others_correct():
    """Two steady threads keep correcting while a third makes a context, corrects one batch, fetches and destroys the context,
    ten times over, on short and long reads in turn.  Under poison, so that every buffer that comes and goes is fenced and
    talc_test_cache_reuses() counts (it counts while the setting is on)."""
    s = inputs()["s21"]
    pair, reads = s.pair, s.reads
    by_len = sorted(reads[80:200], key=len)
    sets = dict(a=reads[0:40], b=reads[40:80], short=by_len[:15], long=by_len[-15:])
    assert max(len(x) for x in sets["short"]) * 2 < min(len(x) for x in sets["long"])
    want = {k: fresh(pair, plain_everything, v, MU.FORWARD) for k, v in sets.items()}
    for k, v in sets.items():
        recs, st = oracle_records(pair.otab, v)
        assert [t[MU.F_RECORD] for t in want[k][0]] == recs and [t[MU.F_STATUS] for t in want[k][0]] == st, k
    stop = threading.Event()
    reuses = lambda: (time.perf_counter(), T.guard_report()["reused"], time.perf_counter())
    L = T.lib()
    kinds = ["short", "long"] * 5

    def steady(key):
        def body(r):
            ctx = T.Context(pair.ttab, pair.p, 0)
            got = []
            try:
                while not stop.is_set() and len(got) < 400:
                    got.append((plain_everything(ctx, sets[key], MU.FORWARD), reuses()))
            finally:
                ctx.close()
            return got
        return body

    def short_lived(r):
        got = []
        try:
            for kind in kinds:
                n0 = T.lib().mark()
                got.append((fresh(pair, plain_everything, sets[kind], MU.FORWARD), reuses(), (n0, T.lib().mark())))
        finally:
            stop.set()
        return got

    with MU.guards_checked():
        with T.poisoned(0xA5):
            results = run_threads([("steady a", steady("a")), ("steady b", steady("b")), ("short-lived", short_lived)], rounds=1)
    assert T.lib() is L
    check_overlap(results, "lifecycle")
    logs = {name: res["rounds"][0][1] for name, res in results.items()}
    samples = []
    for name, key in (("steady a", "a"), ("steady b", "b")):
        got = results[name]["rounds"][0][0]
        print("lifecycle: %s corrected %d batches" % (name, len(got)))
        assert len(got) >= 3, (name, len(got))
        for i, (x, sample) in enumerate(got):
            assert x[1:] == want[key][1:] and MU.first_difference(x[0], want[key][0]) is None, (name, i, MU.first_difference(x[0], want[key][0]), x[1], want[key][1])
            samples.append(sample)
    got = results["short-lived"]["rounds"][0][0]
    assert len(got) == 10
    for i, (x, sample, (n0, n1)) in enumerate(got):
        assert x[1:] == want[kinds[i]][1:] and MU.first_difference(x[0], want[kinds[i]][0]) is None, ("short-lived", i, kinds[i], MU.first_difference(x[0], want[kinds[i]][0]))
        samples.append(sample)
        life = logs["short-lived"][n0:n1]
        assert {"talc_ctx_create", "talc_batch_correct", "talc_ctx_destroy"} <= {c[0] for c in life}, i
        pairs, lonely = overlaps({"life": life, "steady": logs["steady a"] + logs["steady b"]})
        print("lifecycle: context %d (%s reads): %d of its calls' pairs overlap the steady threads'" % (i, kinds[i], pairs))
        assert not lonely, ("short-lived context %d ran while no steady thread was in a call" % i)
    # talc_test_cache_reuses() only ever grows: of two reads of it of which one ended before the other began, in any threads
    samples.sort()
    for i, (t0, v, t1) in enumerate(samples):
        later = [w for s0, w, _ in samples[i + 1:] if s0 > t1]
        assert not later or min(later) >= v, ("the count of reuses went back", v, min(later))
    assert samples[-1][1] > samples[0][1]


# ---------------------------------------------------------------- 4. talc_last_error answers for the calling thread
def refusals_a(L, ctx, b):
    """A fetch before talc_batch_correct (TALC_ERR_STATE), then a setting out of range (TALC_ERR_INVALID)."""
    rc1 = L.talc_batch_fetch_corrected(ctx._h, b._h, None, 0, None, None)
    m1 = L.talc_last_error()
    rc2 = L.talc_ctx_set_chimera(ctx._h, 1, 31, 0)
    m2 = L.talc_last_error()
    return (rc1, m1), (rc2, m2)


BAD_BARCODES = b"ACGTTGCAACGTTGCAACGTTGCA,ACGTTGCAACGTTGCAACGTTGC"


def refusals_b(L, ctx, b):
    """The chimera scan asked of a context that has it off (TALC_ERR_STATE), then barcodes of two lengths (TALC_ERR_INVALID)."""
    rc1 = L.talc_batch_chimera(ctx._h, b._h)
    m1 = L.talc_last_error()
    rc2 = L.talc_ctx_set_demux(ctx._h, BAD_BARCODES, 20, 2, 256, 0)
    m2 = L.talc_last_error()
    return (rc1, m1), (rc2, m2)


def test_last_error_answers_for_the_calling_thread():
    s = inputs()["s21"]
    pair, reads = s.pair, s.reads[0:40]
    bases, offs = PU.pack_reads(reads)
    recs, st = oracle_records(pair.otab, reads)
    ctxs = [T.Context(pair.ttab, pair.p, 0) for _ in range(3)]
    batches = [c.batch(bases, offs) for c in ctxs[:2]]
    stop = threading.Event()
    try:
        want = dict(a=refusals_a(T.lib(), ctxs[0], batches[0]), b=refusals_b(T.lib(), ctxs[1], batches[1]))
        # the codes and texts the single-thread error tests assert (test_gpu_corr_map, test_gpu_chimera, test_gpu_demux)
        assert [x[0] for x in want["a"]] == [ERR_STATE, ERR_INVALID] and [x[0] for x in want["b"]] == [ERR_STATE, ERR_INVALID]
        assert b"talc_batch_correct has not run" in want["a"][0][1] and b"max_error_pct=31" in want["a"][1][1]
        assert b"off" in want["b"][0][1] and b"barcode 2 has 23 letters" in want["b"][1][1]
        assert len({m for v in want.values() for _, m in v}) == 4

        def refused(fn, ctx, b):
            def body(r):
                seen, n = {}, 0
                while (not stop.is_set() or n < 200) and n < 30_000:
                    got = fn(T.lib(), ctx, b)
                    seen[got] = seen.get(got, 0) + 1
                    n += 1
                return seen
            return body

        def corrects(r):
            try:
                return [tuple(bytes(x) if i == 0 else np.asarray(x).tolist() for i, x in enumerate(ctxs[2].correct(bases, offs))) for _ in range(6)]
            finally:
                stop.set()

        results = run_threads([("A", refused(refusals_a, ctxs[0], batches[0])), ("B", refused(refusals_b, ctxs[1], batches[1])), ("C", corrects)], rounds=1)
    finally:
        for x in batches + ctxs:
            x.close()
    check_overlap(results, "last error")
    for name in ("A", "B"):
        seen = results[name]["rounds"][0][0]
        print("last error: thread %s made %d rounds of refused calls" % (name, sum(seen.values())))
        assert list(seen) == [want[name.lower()]], (name, "read another thread's message, or none", [k for k in seen if k != want[name.lower()]][:3])
        assert sum(seen.values()) >= 200
    a_calls = [c for c in results["A"]["rounds"][0][1] if c[0] != "talc_last_error"]
    b_calls = [c for c in results["B"]["rounds"][0][1] if c[0] == "talc_last_error"]
    between = overlaps_in_order(a_calls, b_calls)
    print("last error: %d refused calls of A had B read its message right after them" % between)
    for out, oo, st_ in results["C"]["rounds"][0][0]:                # C's calls returned 0 (Context.correct raises otherwise)
        assert [out[int(oo[i]):int(oo[i + 1])] for i in range(len(reads))] == recs and st_ == st


def overlaps_in_order(calls, reads_of_other):
    """How many of `calls` (one thread's failing calls) were followed by a talc_last_error of the other thread before the
    thread's own next call: the interleaving under which a process-wide message would be the wrong one."""
    ends = sorted(t1 for _, _, t1 in calls)
    starts = sorted(t0 for _, t0, _ in reads_of_other)
    n = j = 0
    for i, e in enumerate(ends):
        nxt = ends[i + 1] if i + 1 < len(ends) else float("inf")
        while j < len(starts) and starts[j] <= e:
            j += 1
        n += j < len(starts) and starts[j] < nxt
    return n


# ---------------------------------------------------------------- 5. same settings, same reads, N contexts
def test_four_contexts_correct_the_same_batch():
    """The command line's situation without its I/O: every result byte-identical to the others and to the oracle."""
    s = inputs()["s21"]
    pair, reads = s.pair, s.reads[0:60]
    bases, offs = PU.pack_reads(reads)
    out, oo, st = pair.otab.correct_batch(bases, offs, nthreads=16)
    want = (bytes(out), np.asarray(oo, np.uint64).tobytes(), np.asarray(st, np.int32).tobytes())
    ctxs = [T.Context(pair.ttab, pair.p, 0) for _ in range(4)]
    try:
        body = lambda ctx: lambda r: tuple(bytes(x) if i == 0 else x.tobytes() for i, x in enumerate(ctx.correct(bases, offs)))
        results = run_threads([("context %d" % i, body(c)) for i, c in enumerate(ctxs)])
    finally:
        for c in ctxs:
            c.close()
    check_overlap(results, "same batch")
    for name, res in results.items():
        for r, (got, _) in enumerate(res["rounds"]):
            assert got == want, (name, r, [i for i in range(3) if got[i] != want[i]])


# ---------------------------------------------------------------- 6. the command line: many batches dealt to two workers against one batch
def test_cli_two_workers_over_many_batches_equal_one_batch(tmp_path):
    c = G.gen_set("default")
    reads = P.reads_of(c.reads[:60], np.random.default_rng(34))
    names = ["read%d/x" % i for i in range(len(reads))]
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    fasta = lambda nms, seqs: "".join(">%s\n%s\n" % (nm, x) for nm, x in zip(nms, seqs))
    (tmp_path / "dressed.fa").write_text(fasta(names, reads))
    (tmp_path / "bc.fa").write_text(fasta(["bc%02d" % (i + 1) for i in range(96)], P.BC24))
    lr = ["--LRBarcodes", str(tmp_path / "bc.fa"), "--LRDemuxOut", "--LRAdapter", P.SSP23, "--LRAdapter", P.VNP, "--LRPolyA", "12", "--LRSplit", "--LRClip",
          "--LRUmi", P.UMI[0]]
    files, timing = {}, {}
    for d, batch_reads in (("many", 3), ("one", len(reads))):
        (tmp_path / d).mkdir()
        args = [GP.TALC, str(tmp_path / "dressed.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", str(batch_reads), "-o", "o"] + GP.REPORT_OPTIONS + lr
        run = subprocess.run(args, cwd=tmp_path / d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert run.returncode == 0, (d, run.stderr.decode()[-800:])
        line = [x for x in run.stderr.decode().splitlines() if x.startswith("[talc-timing] ")]
        timing[d] = json.loads(line[0][len("[talc-timing] "):])
        files[d] = {f: (tmp_path / d / f).read_bytes() for f in sorted(os.listdir(tmp_path / d))}
    # the batches are dealt as the workers come free: 20 batches for two workers, at least 6 each when neither is more than
    # twice as fast as the other (the tally is summed over the workers, so the share of each is not in the report)
    assert timing["many"]["workers"] == 2 and timing["many"]["batches"] == 20 and timing["one"]["batches"] == 1, timing
    assert len(reads) == 59 and timing["many"]["reads"] == 59
    want = {"o" + x for x in GP.REPORT_FILES | GP.LR_FILES | {".config.txt", ".bc01.fa", ".unclassified.fa"}}
    assert want <= set(files["one"]) and sorted(files["many"]) == sorted(files["one"]), sorted(set(files["many"]) ^ set(files["one"]))
    assert files["one"]["o.fa"].count(b">") > len(reads) and len(files["one"]["o.edits.tsv"].splitlines()) > len(reads)
    for f in files["one"]:
        assert files["many"][f] == files["one"][f], f
