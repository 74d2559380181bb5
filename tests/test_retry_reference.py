"""tests/retry_cases.py from the oracle alone (no GPU): every case is what its name says, and make_caps — the scratch layout
of a search stage, reached through the pure library — against the same formulas in Python integers."""
import ctypes as C
import os

import numpy as np
import pytest

import long_gap_cases as LG
import oracle_lib as O
import parity_util as PU
import retry_cases as RC
from talc_amd import build as B

_pure = None


def pure():
    global _pure
    if _pure is None:
        L = C.CDLL(os.path.join(B.OUT, "libtalc_pure.so"))
        L.talc_pure_make_caps.restype = None
        L.talc_pure_make_caps.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        L.pure_is_expected_by_last_node.restype = C.c_int
        L.pure_is_expected_by_last_node.argtypes = [C.c_double, C.c_uint32, C.c_uint32]
        _pure = L
    return _pure


# ---------------------------------------------------------------- the hook inputs
@pytest.mark.parametrize("name", list(RC.GENERATOR_SETS))
def test_generator_sets_are_small_and_mostly_corrected(name):
    kw, first, n = RC.GENERATOR_SETS[name]
    pair = PU.Pair(**kw)
    bases, offs = pair.reads(first, n)
    lens = np.diff(offs.astype(np.int64))
    assert len(lens) == n <= 200 and lens.max() <= RC.MAX_READ, (n, int(lens.max()))
    out, oo, st = pair.otab.correct_batch(bases, offs, nthreads=8)
    corrected = int((st == 0).sum())
    print(name, "reads", n, "longest", int(lens.max()), "corrected", corrected)
    assert corrected >= 0.8 * n, (name, corrected)


def test_tandem_set_has_repeats_and_is_mostly_corrected():
    transcripts, reads = RC.tandem_set()
    assert len(reads) == 90 and max(map(len, reads)) <= RC.MAX_READ
    ot = LG.oracle_table(transcripts, 21)
    out, oo, st = ot.correct_batch(*PU.pack_reads(reads), nthreads=8)
    assert int((st == 0).sum()) >= 60, np.bincount(st).tolist()


def test_long_gap_read_records_a_second_bridge():
    """Under the hook fullCap is 1: a search that records two bridges is flagged (OVF_FULLPATHS)."""
    s = LG.oracle_side(RC.LONG_GAP)
    assert s.status == 0 and len(s.g.read) <= RC.MAX_READ
    assert max(max(r["full"], default=0) for search in s.runs for r in search["runs"]) >= 2


# ---------------------------------------------------------------- the constructed read
def test_constructed_read_has_two_long_regions_and_position_lists_beyond_2048():
    """What the reference makes of the constructed read: its structure step accepts the two regions as built, every position
    of a region is recorded (2600 per side, between the 2048 the first pass and the x 8 stage hold and the 16 384 of the
    x 64 stage), and the read is corrected: head and tail are rewritten to the truth.  The bridge over the weak stretch is
    not found from either side (the trace's two `5 1 0` lines), so that stretch stays as it came: both sides' lists are
    built all the same, which is what the case is for.  Forks inside the regions (FORK_EVERY > 0: some thirty anchors per
    side, the anchor sort beyond 16) make the reference search edges of 2.6 kb from anchors deep inside a region, 25
    minutes for the one read: left out."""
    c = RC.constructed()
    p, q = PU.both_params(k=c.k)
    assert all(p.min_count <= x < p.max_in_count for x in c.levels + (RC.BETWEEN,))
    L = pure()
    expected = lambda nxt, cur: bool(L.pure_is_expected_by_last_node(p.alpha, nxt, cur))
    lo, hi = c.levels
    assert not expected(hi, lo) and not expected(lo, hi) and expected(RC.BETWEEN, lo) and expected(RC.BETWEEN, hi)
    ot = O.OracleTable(q, O.OracleTable.FLAT)
    ot.insert_packed(c.keys, c.counts)
    ot.decolour()
    reg, thr, ok = ot.structure(c.read)
    assert ok and reg.tolist() == [list(r) for r in c.regions], reg.tolist()
    cov, _, nin = ot.coverage(c.read)
    for first, last in c.regions:
        assert last - first + 1 == RC.REGION
        for side in (0, 1):
            n = len(RC.position_list(cov, first, last, side, expected, p.min_count, p.max_in_count))
            assert RC.ANCH_CAP_FLOOR < n < RC.ANCH_CAP_X64 and n == RC.REGION, (side, n)
            assert n < len(c.read) + 8                       # anchCap at x 64: min(16 384, L + 8)
    text, status, out, _, _ = LG.traced(ot, c.read)
    assert status == 0 and out != c.read, status
    a0, b1 = c.regions[0][0], c.regions[1][1] + c.k
    assert out[:a0] == c.truth[:a0] != c.read[:a0] and out[b1:] == c.truth[b1:] != c.read[b1:]
    found = [l.split(" ")[1:3] for l in text.splitlines() if l.startswith("5 ")]
    assert found == [["1", "0"], ["1", "0"], ["0", "1"], ["2", "1"]], found


# ---------------------------------------------------------------- make_caps
MAX_LENS = (0, 1, None, 200, 2040, 2041, 7000, 140_000, 14_000_000, 112_000_000, 0x7fffff00)     # None: K


def caps_of(max_len, k, scale, tiny=False):
    w = np.zeros(36, dtype=np.uint64)
    pure().talc_pure_make_caps(max_len, k, scale, 0, int(tiny), w.ctypes.data)
    w = [int(x) for x in w]
    return dict(zip(RC.FIELDS, w[:10])), w[10], w[11:34], w[34]


def holds_read(max_len, k, scale):
    """caps_hold_read: what ensure_stage asks before it sizes a stage."""
    w = np.zeros(36, dtype=np.uint64)
    pure().talc_pure_make_caps(max_len, k, scale, 0, 0, w.ctypes.data)
    return bool(w[35])


@pytest.mark.parametrize("k", [18, 21, 31])
def test_make_caps_layout_and_capacities(k):
    """The regions of a slot are in order and disjoint, every offset is 16-aligned, slotBytes covers the last region,
    dpCap >= 2048, the capacities are the formulas' in unbounded integers with every 32-bit field saturating at 0xFFFFFF00,
    and without the hook no capacity is smaller at a larger scale (fullPool wrapped at x 64 from reads of 14 Mb, at x 8 from
    112 Mb, edgeCap from 1.95 Gb, weakPool from 1 Gb: a larger stage then had the smaller pool)."""
    for max_len in MAX_LENS:
        max_len = k if max_len is None else max_len
        before = None
        for scale in (1, 8, 64):
            for tiny in (False, True):
                caps, slot, offs, end = caps_of(max_len, k, scale, tiny)
                want, sizes = RC.caps_reference(max_len, k, scale, tiny)
                what = (max_len, k, scale, tiny)
                assert caps == want, (what, {f: (caps[f], want[f]) for f in caps if caps[f] != want[f]})
                assert all(v < 1 << 32 for v in want.values()) and caps["dpCap"] >= 2048, what
                assert offs[0] == 0 and all(o % 16 == 0 for o in offs), what
                for i, (o, size) in enumerate(zip(offs, sizes)):
                    nxt = offs[i + 1] if i + 1 < len(offs) else end
                    assert o + size <= nxt and (i + 1 == len(offs) or nxt - (o + size) < 16), (what, RC.REGIONS[i], o, size, nxt)
                assert slot >= end and slot % 256 == 0 and slot - end < 256, what
            if before is not None:
                assert all(caps_of(max_len, k, scale)[0][f] >= before[f] for f in RC.FIELDS), (max_len, k, scale)
            before = caps_of(max_len, k, scale)[0]


@pytest.mark.parametrize("k", [18, 21, 31])
def test_a_stage_whose_read_sized_buffers_saturated_is_refused(k):
    """The edge buffers, the DP arrays and the weak pool are filled by the read's length without a count: where one of them
    saturated (weakPool from reads beyond 2^30 - 320 bases, edgeCap from 1.95 Gb) caps_hold_read is false and ensure_stage
    refuses the stage; everywhere below it is true, at every scale."""
    for scale in (1, 8, 64):
        for max_len in (0, 1, k, 7000, 14_000_000, 112_000_000, (1 << 30) - 320):
            assert holds_read(max_len, k, scale), (max_len, scale)
            c, _ = RC.caps_reference(max_len, k, scale)
            assert c["edgeCap"] >= c["seqCap"] + c["refCap"] and c["dpCap"] >= max(c["edgeCap"], c["seqCap"]) + 8 and c["weakPool"] >= 4 * max_len + 1024
        for max_len in ((1 << 30) - 319, 1_950_000_000, 0x7fffff00):
            assert not holds_read(max_len, k, scale), (max_len, scale)


def test_the_hook_leaves_a_stage_with_three_positions_and_one_bridge():
    for scale in (1, 8, 64):
        caps = caps_of(7000, 21, scale, True)[0]
        assert (caps["anchCap"], caps["fullCap"], caps["fullPool"]) == (3, 1, caps["seqCap"]), (scale, caps)
