"""What a batch holds and what drops it, across the features and through the C ABI itself: after every step of
a walk over correct / structure / auto strand, every fetch whose result that step dropped answers TALC_ERR_STATE and every
count 0, whatever the Python class remembers; and the device buffers a batch keeps or grows from call to call (pieces,
support, edit scripts, records) give the right bytes between red zones.

Wanted values: memcheck_util.everything() of a fresh batch on a fresh context, plain and auto strand (the per-feature tests
hold that function's outputs to the oracle and the numpy contracts), and the oracle's own records where the set has them."""
import ctypes as C

import numpy as np
import pytest

import corr_map_ref as M
import parity_util as PU
import pieces_ref as P
import memcheck_util as MU
from memcheck_util import everything, fetch_all, first_difference, guards_checked, per_read
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

ERR_STATE = -6
N_SET = 20
_in = {}


def inputs():
    """The first 20 reads of the default map set, "", one read of exactly k bases, and two reads of the set reverse
    complemented (plain, they have no solid k-mer and pass through; auto strand turns and corrects them, so the two
    orientations' records differ in length).  Computed once, shared, left unchanged."""
    if not _in:
        s = M.map_set("default")
        s.pair.ttab.upload(0)
        k = int(s.pair.p.k)
        reads = s.reads[:N_SET] + ["", s.reads[N_SET][:k]] + [M.revcomp(x) for x in s.reads[N_SET:N_SET + 2]]
        want = {}
        for auto in (False, True):
            ctx = T.Context(s.pair.ttab, s.pair.p, 0)
            ctx.auto_strand(auto)
            try:
                want[auto] = everything(ctx, reads)
            finally:
                ctx.close()
        for i in range(N_SET):                        # records and status: the oracle's
            assert want[False][0][i][MU.F_RECORD].decode() == s.exp[i]["out"] and want[False][0][i][MU.F_STATUS] == s.exp[i]["status"], i
        ctx = T.Context(s.pair.ttab, s.pair.p, 0)     # the edit scripts with max_cells = 1, of a fresh batch
        ctx.record_map(True)
        b = ctx.batch(*PU.pack_reads(reads))
        try:
            b.correct()
            ops, eo, rows = b.edits(max_cells=1)
            edits1 = (ops.copy(), eo.copy(), rows.copy())
        finally:
            b.close()
            ctx.close()
        _in.update(s=s, k=k, reads=reads, want=want, edits1=edits1)
    return _in


def record_total(per):
    return sum(len(t[MU.F_RECORD]) for t in per)


def test_the_inputs_do_what_they_are_there_for():
    s = inputs()
    assert MU._field_layout_holds()                              # the F_ constants name what per_read puts there
    reads, plain, auto = s["reads"], s["want"][False][0], s["want"][True][0]
    assert [len(x) for x in reads].count(0) == 1 and [len(x) for x in reads].count(s["k"]) == 1
    assert sum(len(t[MU.F_SPLIT_TEXTS]) for t in plain) > len(reads)   # SPLIT, min_len 0: more pieces than reads
    assert record_total(plain) != sum(len(x) for x in reads)     # the two support sources' totals
    assert record_total(plain) != record_total(auto)             # the two orientations' record totals
    assert int(s["want"][True][2]["reverse"].sum()) >= 2 and s["want"][False][2] is None


# ---------------------------------------------------------------- 1. the state walk, through T.lib()
def probe(L, h, n):
    """({fetch: return code}, {count: value}) of the batch as it stands.  The fetches are asked without buffers (the state
    check comes before anything is copied, and nothing is made: the masked records are made for a buffer only); the work
    queue needs its two."""
    order, bucket = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint32)
    codes = dict(
        corrected=L.talc_batch_fetch_corrected(*h, None, 0, None, None),
        masked=L.talc_batch_fetch_corrected_masked(*h, None, 0, None, None),
        map=L.talc_batch_fetch_map(*h, None, 0, None),
        pieces=L.talc_batch_fetch_pieces(*h, None, 0, None, None, 0, None),
        edits=L.talc_batch_fetch_edits(*h, None, 0, None, None),
        support=L.talc_batch_fetch_support(*h, None, 0, None),
        solidity=L.talc_batch_fetch_solidity(*h, None, None),
        structure=L.talc_batch_fetch_structure(*h, None, None, None, None, None, None, None, 0, None),
        order=L.talc_batch_order(*h, order.ctypes.data, bucket.ctypes.data),
        coverage=L.talc_batch_fetch_coverage(*h, None, None, None, None),
        strand=L.talc_batch_fetch_strand(*h, None))
    b = h[1]
    counts = dict(
        corrected_bytes=L.talc_batch_corrected_bytes(b), segments=L.talc_batch_num_segments(b), pieces=L.talc_batch_num_pieces(b),
        pieces_bytes=L.talc_batch_pieces_bytes(b), edit_ops=L.talc_batch_num_edit_ops(b), support_bytes=L.talc_batch_support_bytes(b))
    return codes, counts


def holds(L, h, n, step, fetches=(), counts=()):
    """The fetches named succeed and the counts named are not 0; every other fetch is TALC_ERR_STATE, every other count 0."""
    codes, cnt = probe(L, h, n)
    want = {name: (0 if name in fetches else ERR_STATE) for name in codes}
    assert codes == want, (step, {x: (codes[x], want[x]) for x in codes if codes[x] != want[x]})
    for name, v in cnt.items():
        assert (v != 0) == (name in counts), (step, name, v)


EVERY_OUTPUT = ("corrected", "masked", "map", "pieces", "edits", "support", "solidity", "coverage")
EVERY_COUNT = ("corrected_bytes", "segments", "pieces", "pieces_bytes", "edit_ops", "support_bytes")


def make_everything(b):
    """fetch_all of a batch the walk has corrected through the ABI.  fetch_all goes through the Batch methods; of the class's
    own memory they use one thing, whether solidity() asks for corrected rows, so that is set to what the library must hold
    by now.  What the library holds is asked of the library, by probe()."""
    b._corrected, b._enc_auto = True, b.ctx._auto
    return per_read(fetch_all(b), b.n_reads)


def test_every_step_drops_what_was_made_from_what_it_replaces():
    s = inputs()
    reads, n = s["reads"], len(s["reads"])
    plain, auto, auto_rows = s["want"][False][0], s["want"][True][0], s["want"][True][2]
    L = T.lib()
    ctx = T.Context(s["s"].pair.ttab, s["s"].pair.p, 0)
    ctx.record_map(True)
    b = ctx.batch(*PU.pack_reads(reads))
    h = (ctx._h, b._h)
    raw_support = T.SupportParams(T.SUPPORT_RAW, 0, 0, 0)
    try:
        holds(L, h, n, "1: a fresh batch")
        assert L.talc_batch_correct(*h) == 0
        holds(L, h, n, "2: corrected, nothing made yet", ("corrected", "masked", "map", "coverage"), ("corrected_bytes", "segments"))
        d = first_difference(make_everything(b), plain)
        assert d is None, ("2: every output", d)
        holds(L, h, n, "2: every output made", EVERY_OUTPUT, EVERY_COUNT)

        assert L.talc_batch_structure(*h) == 0
        holds(L, h, n, "3: talc_batch_structure", ("structure", "order", "coverage"))

        assert L.talc_batch_correct(*h) == 0
        holds(L, h, n, "4: corrected again, nothing made yet", ("corrected", "masked", "map", "coverage"), ("corrected_bytes", "segments"))
        d = first_difference(make_everything(b), plain)
        assert d is None, ("4: every output", d)
        assert L.talc_batch_support(*h, C.byref(raw_support)) == 0       # (the last support of the batch is of its codes alone)
        holds(L, h, n, "4: every output made", EVERY_OUTPUT, EVERY_COUNT)

        ctx.auto_strand(True)
        assert L.talc_batch_coverage(*h) == 0
        holds(L, h, n, "5: auto strand on, talc_batch_coverage", ("coverage", "strand"))
        rows = np.zeros(n, dtype=T.STRAND_DTYPE)
        assert L.talc_batch_fetch_strand(*h, rows.ctypes.data) == 0 and np.array_equal(rows, auto_rows)
        assert L.talc_batch_correct(*h) == 0
        holds(L, h, n, "5: corrected, nothing made yet", ("corrected", "masked", "map", "coverage", "strand"), ("corrected_bytes", "segments"))
        d = first_difference(make_everything(b), auto)
        assert d is None, ("5: every output under auto strand", d)
        holds(L, h, n, "5: every output made", EVERY_OUTPUT + ("strand",), EVERY_COUNT)

        ctx.auto_strand(False)
        assert L.talc_batch_solidity(*h) == 0
        holds(L, h, n, "6: auto strand off, talc_batch_solidity", ("solidity", "strand"))
        raw, cor = np.zeros(n, dtype=T.SOLIDITY_DTYPE), np.zeros(n, dtype=T.SOLIDITY_DTYPE)
        assert L.talc_batch_fetch_solidity(*h, raw.ctypes.data, None) == 0
        assert [raw[r].tolist() for r in range(n)] == [t[MU.F_SOLIDITY_RAW] for t in plain]
        assert L.talc_batch_fetch_solidity(*h, raw.ctypes.data, cor.ctypes.data) == ERR_STATE
        rows[:] = 0
        assert L.talc_batch_fetch_strand(*h, rows.ctypes.data) == 0 and np.array_equal(rows, auto_rows)   # the vote is never dropped
    finally:
        b.close()
        ctx.close()


# ---------------------------------------------------------------- 1b. the device times of the reports
def report_times(ctx):
    """Every device time the context's getters report, by the kernel(s) it is the time of."""
    (pack_map, mask_case), (sol_raw, sol_records) = ctx.map_timing(), ctx.solidity_timing()
    (piece_count, piece_pack), (edit_align, edit_pack) = ctx.pieces_timing(), ctx.edits_timing()
    return dict(pack_map=pack_map, mask_case=mask_case, sol_raw=sol_raw, sol_records=sol_records, piece_count=piece_count,
                piece_pack=piece_pack, edit_align=edit_align, edit_pack=edit_pack, support=ctx.support_timing(), vote=ctx.strand_timing())


def test_every_report_keeps_its_own_time_and_a_pending_one_is_read_by_the_next_wait():
    """Each call sets the times of its own kernels and of no other's: what was read after an earlier call reads the same
    after every later one, and what has not run yet reads exactly 0.  A time is > 0 where a kernel ran over the 24 reads
    between its two events; the pieces' and the edit scripts' are held to >= 0, as their own tests hold them.  A vote that
    auto strand launches inside another call is timed by that call, and an uncorrected batch's solidity has no time for
    the records' rows, whatever an earlier batch of the context left."""
    s = inputs()
    table, p = s["s"].pair.ttab, s["s"].pair.p
    packed = PU.pack_reads(s["reads"])
    ctx = T.Context(table, p, 0)
    ctx.record_map(True)
    b = ctx.batch(*packed)
    try:
        steps = [(b.correct, ("pack_map",), ()),
                 (b.solidity, ("sol_raw", "sol_records"), ()),
                 (lambda: b.pieces(T.PIECES_TRIM, soft_mask=True), ("mask_case",), ("piece_count", "piece_pack")),
                 (b.edits, (), ("edit_align", "edit_pack")),
                 (b.support, ("support",), ()),
                 (b.strand, ("vote",), ())]
        seen = {}
        assert report_times(ctx) == dict.fromkeys(report_times(ctx), 0.0)
        for i, (call, positive, not_negative) in enumerate(steps):
            call()
            now = report_times(ctx)
            print("step", i, {k: now[k] for k in positive + not_negative})
            for name in positive:
                assert now[name] > 0, (i, name, now[name])
            for name in not_negative:
                assert now[name] >= 0, (i, name, now[name])
            for name, v in now.items():
                if name not in positive + not_negative:
                    assert v == seen.get(name, 0.0), (i, name, v, seen.get(name, 0.0))
            seen.update((name, now[name]) for name in positive + not_negative)
        fresh = ctx.batch(*packed)          # not corrected, on a context whose last solidity had records
        try:
            fresh.solidity()
            assert ctx.solidity_timing()[0] > 0 and ctx.solidity_timing()[1] == 0.0
        finally:
            fresh.close()
    finally:
        b.close()
        ctx.close()
    for first in ("solidity", "correct"):   # auto strand, no strand(): the vote runs inside the call and is timed by it
        ctx = T.Context(table, p, 0)
        ctx.auto_strand(True)
        b = ctx.batch(*packed)
        try:
            assert ctx.strand_timing() == 0.0
            getattr(b, first)()
            print(first, "vote", ctx.strand_timing())
            assert ctx.strand_timing() > 0, first
            if first == "solidity":
                assert ctx.solidity_timing()[1] == 0.0
        finally:
            b.close()
            ctx.close()


# ---------------------------------------------------------------- 2. the buffers a batch keeps or grows
def same_pieces(got, want, what):
    for name, g, w in zip(("bytes", "piece offsets", "pieces", "read offsets"), got, want):
        assert np.array_equal(g, w), (what, name)


def per_read_bytes(buf, offs, n):
    buf = bytes(buf)
    return [buf[int(offs[r]):int(offs[r + 1])] for r in range(n)]


def test_kept_and_grown_buffers_hold_every_result():
    s = inputs()
    reads, n = s["reads"], len(s["reads"])
    plain, auto = s["want"][False][0], s["want"][True][0]
    bases, offs = PU.pack_reads(reads)
    with guards_checked():
        with T.poisoned(0xA5):
            ctx = T.Context(s["s"].pair.ttab, s["s"].pair.p, 0)
            b = ctx.batch(bases, offs)
            try:
                # records without the map, then with it: the segment buffers' first allocation on a batch that has records
                assert b.correct() == 0
                out, oo, st = b.fetch_corrected()
                assert [(x, int(c)) for x, c in zip(per_read_bytes(out, oo, n), st)] == [(t[MU.F_RECORD], t[MU.F_STATUS]) for t in plain]
                ctx.record_map(True)
                assert b.correct() == 0
                out, oo, st = b.fetch_corrected()
                segs, so = b.fetch_map()
                assert [(x, int(c)) for x, c in zip(per_read_bytes(out, oo, n), st)] == [(t[MU.F_RECORD], t[MU.F_STATUS]) for t in plain]

                # pieces: none (buffers of one element), more than reads (they grow), none (the larger ones are kept), more again
                far = 1 << 20
                assert far > max(len(t[MU.F_RECORD]) for t in plain)
                for i, (mode, min_len) in enumerate([(T.PIECES_TRIM, far), (T.PIECES_SPLIT, 0)] * 2):
                    got = b.pieces(mode, min_len)
                    assert len(got[2]) == 0 if min_len else len(got[2]) > n, (i, len(got[2]))
                    same_pieces(got, P.pieces(segs, so, out, oo, mode, min_len), ("pieces", i, mode, min_len))

                # support: the smaller source, the larger, the smaller again
                totals = dict(raw=int(offs[n]), record=int(oo[n]))
                assert totals["raw"] != totals["record"]
                small, large = sorted(totals, key=totals.get)
                for i, source in enumerate((small, large, small)):
                    sb, sof = b.support(source)
                    assert len(sb) == totals[source]
                    assert per_read_bytes(sb, sof, n) == [t[MU.F_SUPPORT[source]] for t in plain], ("support", i, source)

                # edit scripts: next to no op, the default's, next to none again
                ops1, eo1, rows1 = s["edits1"]
                want_default = ([t[MU.F_OPS] for t in plain], [t[MU.F_EDIT_ROW] for t in plain])
                assert len(ops1) < sum(len(x) for x in want_default[0]) // 4      # fewer ops than the default has: the buffer has to grow
                for i, cells in enumerate((1, 0, 1)):
                    ops, eo, rows = b.edits(max_cells=cells)
                    if cells:
                        assert np.array_equal(ops, ops1) and np.array_equal(eo, eo1) and np.array_equal(rows, rows1), ("edits", i)
                    else:
                        got = ([ops[int(eo[r]):int(eo[r + 1])].tobytes() for r in range(n)], [rows[r].tolist() for r in range(n)])
                        assert got == want_default, ("edits", i)

                # every output of the plain correction, then of auto strand: the record total differs, d_dense is kept or grown
                d = first_difference(per_read(fetch_all(b), n), plain)
                assert d is None, ("plain", d)
                ctx.auto_strand(True)
                assert b.correct() == 0
                assert b.corrected_bytes == record_total(auto) != int(oo[n])
                d = first_difference(per_read(fetch_all(b), n), auto)
                assert d is None, ("auto strand", d)
            finally:
                b.close()
                ctx.close()


# ---------------------------------------------------------------- 3. the preparation reports: what a batch holds of them, what rescans
def prep_probe(L, ctx, b):
    """({fetch: return code}, {fetch: what it wrote}, {count: value}) of the five preparation reports of the batch as it
    stands; the buffers have the sizes the batch's own counts give."""
    h = (ctx._h, b._h)
    n, src = b.n_reads, b.n_source_reads
    nh, npc = int(L.talc_batch_num_chimera_hits(b._h)), int(L.talc_batch_num_split_pieces(b._h))
    ends, demux, umi = np.zeros(max(n, 1), T.ENDS_DTYPE), np.zeros(max(src, 1), T.DEMUX_DTYPE), np.zeros(max(n, 1), T.UMI_DTYPE)
    hits, hit_off = np.zeros(max(nh, 1), T.CHIMERA_DTYPE), np.zeros(src + 1, np.uint64)
    pieces, piece_off = np.zeros(max(npc, 1), T.SPLIT_PIECE_DTYPE), np.zeros(src + 1, np.uint64)
    codes = dict(ends=L.talc_batch_fetch_ends(*h, ends.ctypes.data), chimera=L.talc_batch_fetch_chimera(*h, hits.ctypes.data, nh, hit_off.ctypes.data),
                 split=L.talc_batch_fetch_split(*h, pieces.ctypes.data, piece_off.ctypes.data), demux=L.talc_batch_fetch_demux(*h, demux.ctypes.data),
                 umi=L.talc_batch_fetch_umi(*h, umi.ctypes.data))
    wrote = dict(ends=(ends[:n],), chimera=(hits[:nh], hit_off), split=(pieces[:npc], piece_off), demux=(demux[:src],), umi=(umi[:n],))
    return codes, wrote, dict(hits=nh, pieces=npc)


def prep_holds(L, ctx, b, step, want):
    """The fetches named in `want` succeed and give those arrays; every other fetch is TALC_ERR_STATE; the two counts are
    those of the wanted hits and pieces, else 0."""
    codes, wrote, counts = prep_probe(L, ctx, b)
    expect = {name: (0 if name in want else ERR_STATE) for name in codes}
    assert codes == expect, (step, {x: (codes[x], expect[x]) for x in codes if codes[x] != expect[x]})
    assert counts == dict(hits=len(want["chimera"][0]) if "chimera" in want else 0, pieces=len(want["split"][0]) if "split" in want else 0), (step, counts)
    for name, arrays in want.items():
        for i, (g, w) in enumerate(zip(wrote[name], arrays)):
            assert g.dtype == w.dtype and len(g) == len(w), (step, name, i, len(g), len(w))
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (step, name, i, len(bad), int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist())


def held(k, *names):
    """prep_holds' `want` from a prep_ref.chain result."""
    every = dict(ends=(k["ends"],), chimera=(k["hits"], k["hit_off"]), split=(k["pieces"], k["piece_off"]), demux=(k["demux"],), umi=(k["umi"],))
    return {name: every[name] for name in names}


def scan_times(ctx):
    return dict(ends=ctx.ends_timing()[0], chimera=ctx.chimera_timing()[0], demux=ctx.demux_timing(), umi=ctx.umi_timing())


def test_the_preparation_reports_rescan_only_under_their_own_setting_and_remade_batches_keep_theirs():
    """The walk of test_every_step_drops_what_was_made_from_what_it_replaces over the four preparation settings.  What the
    times say: docs/demux.md and docs/umi.md promise 0 after a call that found its rows made.  docs/read_ends.md and
    docs/chimeras.md promise only "the context's last k_read_ends / k_read_chimera": talc_batch_ends and talc_batch_chimera
    that find their rows made launch nothing and leave the span as it was, so the time reads exactly what it read before."""
    import chimera_ref as CR
    import demux_ref as DR
    import ends_ref as R
    import prep_ref as PR
    import test_gpu_prep_chain as PC
    import umi_ref as U
    s = PC.inputs()
    reads = s["reads"][:26] + s["reads"][-4:]
    n = len(reads)
    assert n == 30
    ENDS_B = dict(PR.ENDS_KW, adapters=PR.ENDS_KW["adapters"][::-1])
    CHIMERA_B, DEMUX_B, UMI_B = (True, 0, 100), (PR.BC24, 10, 0), (PR.UMI[0], 5, 256)
    A = (PR.ENDS_KW, PR.CHIMERA, PR.DEMUX, PR.UMI)
    a = PR.chain(reads, *A)
    a_swapped = PR.chain(reads, ENDS_B, PR.CHIMERA, PR.DEMUX, PR.UMI)                 # step 3: the adapters in the other order
    b_all = PR.chain(reads, ENDS_B, CHIMERA_B, DEMUX_B, UMI_B)
    differ = lambda x, y: len(x) != len(y) or bool((x != y).any())
    assert differ(a["ends"], a_swapped["ends"]) and differ(a["hits"], a_swapped["hits"]) and len(a["hits"]) >= 10       # from the reference alone: each step is seen
    assert differ(a["demux"], b_all["demux"]) and differ(a["umi"], b_all["umi"]) and differ(a_swapped["hits"], b_all["hits"])
    L = T.lib()
    ctx = T.Context(s["c"].ttab, s["c"].p, 0)
    bases, offs = R.batch(reads)
    plain = ctx.batch(bases, offs)
    h = (ctx._h, plain._h)
    SCAN = dict(ends=L.talc_batch_ends, chimera=L.talc_batch_chimera, demux=L.talc_batch_demux, umi=L.talc_batch_umi)
    made = []

    def no_scan(b, names, step):
        """The scans named answer TALC_OK on batch b and launch nothing."""
        for name in names:
            before = scan_times(ctx)
            assert SCAN[name](ctx._h, b._h) == 0, (step, name, L.talc_last_error())
            after = scan_times(ctx)
            assert after[name] == (0.0 if name in ("demux", "umi") else before[name]), (step, name, before, after)
            assert {k: v for k, v in after.items() if k != name} == {k: v for k, v in before.items() if k != name}, (step, name)

    def rescans(b, name, step):
        assert SCAN[name](ctx._h, b._h) == 0, (step, name, L.talc_last_error())
        assert scan_times(ctx)[name] > 0, (step, name)

    try:
        # 1. everything off
        prep_holds(L, ctx, plain, "1: a fresh batch, every setting off", {})
        for name in SCAN:
            assert SCAN[name](*h) == ERR_STATE and b"off" in L.talc_last_error(), name
        assert scan_times(ctx) == dict(ends=0.0, chimera=0.0, demux=0.0, umi=0.0)
        prep_holds(L, ctx, plain, "1: after the refused scans", {})

        # 2. all four on: each scan runs once
        ctx.set_ends(**PR.ENDS_KW)
        ctx.set_chimera(*PR.CHIMERA)
        ctx.set_demux(*PR.DEMUX)
        ctx.set_umi(*PR.UMI)
        prep_holds(L, ctx, plain, "2: the settings alone make nothing", {})
        done = []
        for name in ("ends", "chimera", "demux", "umi"):
            rescans(plain, name, "2: first call")
            done.append(name)
            prep_holds(L, ctx, plain, "2: after " + name, held(a, *done))
        no_scan(plain, ("ends", "chimera", "demux", "umi"), "2: the same call again")
        prep_holds(L, ctx, plain, "2: every report made", held(a, "ends", "chimera", "demux", "umi"))

        # 3. the adapters in the other order: the ends and, through chimeraEndsGen, the hits; neither demux nor UMI
        ctx.set_ends(**ENDS_B)
        no_scan(plain, ("demux", "umi"), "3")
        rescans(plain, "ends", "3")
        rescans(plain, "chimera", "3")
        prep_holds(L, ctx, plain, "3: a new ends setting", held(a_swapped, "ends", "chimera", "demux", "umi"))
        no_scan(plain, ("ends", "chimera", "demux", "umi"), "3: again")

        # 4. a new demux setting: demux alone; a new UMI setting: the UMI alone
        ctx.set_demux(*DEMUX_B)
        no_scan(plain, ("ends", "chimera", "umi"), "4: demux")
        rescans(plain, "demux", "4: demux")
        want = dict(held(a_swapped, "ends", "chimera", "umi"), demux=(b_all["demux"],))
        prep_holds(L, ctx, plain, "4: a new demux setting", want)
        ctx.set_umi(*UMI_B)
        no_scan(plain, ("ends", "chimera", "demux"), "4: umi")
        rescans(plain, "umi", "4: umi")
        want["umi"] = (b_all["umi"],)
        prep_holds(L, ctx, plain, "4: a new UMI setting", want)
        no_scan(plain, ("ends", "chimera", "demux", "umi"), "4: again")

        # 5. four remade batches under A
        ctx.set_ends(**PR.ENDS_KW)
        ctx.set_chimera(*PR.CHIMERA)
        ctx.set_demux(*PR.DEMUX)
        ctx.set_umi(*PR.UMI)
        kinds = {}
        for name, clip, split in PR.KINDS[1:]:
            k = PR.chain(reads, *A, clip=clip, split=split)
            b = ctx.batch(bases, offs, clip=clip, split=split)
            made.append(b)
            # (a split batch made without clip has no end rows of its own: like a plain batch it would scan its pieces when asked)
            kinds[name] = (b, held(k, *(("ends",) if clip else ()) + (("chimera", "split") if split else ()) + ("demux", "umi")),
                           (("ends",) if clip else ()) + (("chimera",) if split else ()) + ("demux", "umi"))
        ctx.set_ends()
        k = PR.chain(reads, None, None, PR.DEMUX, PR.UMI, clip=True)
        b = ctx.batch(bases, offs, clip=True)
        made.append(b)
        kinds["clip, the UMI alone"] = (b, held(k, "demux", "umi"), ("demux", "umi"))
        assert differ(k["umi"], kinds["clip"][1]["umi"][0])                           # (the claims of the ends are in the one, not in the other)

        def remade_keep(step):
            for name, (b, want, scans) in kinds.items():
                prep_holds(L, ctx, b, "%s: %s" % (step, name), want)
                no_scan(b, scans, "%s: %s" % (step, name))
                prep_holds(L, ctx, b, "%s: %s, after the calls" % (step, name), want)
            for name in ("clip", "clip, the UMI alone"):                              # no longer the reads as they came
                assert L.talc_batch_chimera(ctx._h, kinds[name][0]._h) == ERR_STATE, (step, name)
            assert L.talc_batch_ends(ctx._h, kinds["clip, the UMI alone"][0]._h) == ERR_STATE, step
            assert L.talc_batch_fetch_ends(ctx._h, kinds["clip, the UMI alone"][0]._h, None) == ERR_STATE, step

        remade_keep("5: as they were made")
        ctx.set_ends(**ENDS_B)
        ctx.set_chimera(*CHIMERA_B)
        ctx.set_demux(*DEMUX_B)
        ctx.set_umi(*UMI_B)
        remade_keep("5: every setting changed to B")
        for name in SCAN:                                                             # the plain batch follows the new settings
            rescans(plain, name, "5: B")
        prep_holds(L, ctx, plain, "5: the plain batch under B", held(b_all, "ends", "chimera", "demux", "umi"))
        ctx.set_ends()
        ctx.set_chimera(False)
        ctx.set_demux()
        ctx.set_umi()
        remade_keep("5: every setting off")
        for name in SCAN:
            assert SCAN[name](*h) == ERR_STATE, name
        prep_holds(L, ctx, plain, "5: the plain batch keeps the rows of its last scans", held(b_all, "ends", "chimera", "demux", "umi"))
        assert L.talc_batch_ends(ctx._h, kinds["split"][0]._h) == ERR_STATE                # (nothing to scan its pieces under)

        # 6. made while demux and the UMI were off: never, even once they are on
        ctx.set_ends(**PR.ENDS_KW)
        ctx.set_chimera(*PR.CHIMERA)
        late = []
        for name, clip, split in PR.KINDS[1:]:
            b = ctx.batch(bases, offs, clip=clip, split=split)
            made.append(b)
            k = PR.chain(reads, PR.ENDS_KW, PR.CHIMERA, None, None, clip=clip, split=split)
            late.append((name, b, held(k, *(("ends",) if clip else ()) + (("chimera", "split") if split else ()))))
        ctx.set_demux(*PR.DEMUX)
        ctx.set_umi(*PR.UMI)
        for name, b, want in late:
            before = scan_times(ctx)
            assert L.talc_batch_demux(ctx._h, b._h) == ERR_STATE and L.talc_batch_umi(ctx._h, b._h) == ERR_STATE, name
            assert scan_times(ctx) == before, name
            prep_holds(L, ctx, b, "6: " + name, want)
    finally:
        for b in made:
            b.close()
        plain.close()
        ctx.close()
