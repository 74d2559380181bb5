"""CPU checks of the references the -m gpu tests of the structure kernel and of the derived device tables compare
against (tests/test_gpu_structure.py, tests/test_gpu_derived_tables.py): a reference that is wrong in the kernel's own
way proves nothing, so each one is pinned here to answers worked out by hand — and the conditions the GPU cases state
about their inputs (how many raw regions, how many reads the oracle edits beyond the 512th) are evaluated with the
oracle alone, so that a drift of the generator shows without a GPU."""
import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
from talc_amd.synth import Synth


def test_runs_are_the_maximal_stretches():
    assert PU.runs(np.array([], bool)).shape == (0, 2)
    assert PU.runs(np.array([0, 0, 0], bool)).tolist() == []
    assert PU.runs(np.array([1, 1, 0, 1, 0, 0, 1], bool)).tolist() == [[0, 1], [3, 3], [6, 6]]
    assert PU.runs(np.array([0, 1, 1, 1], bool)).tolist() == [[1, 3]]


def test_region_words_on_hand_made_hit_vectors():
    """Hit index of a region's start = its tile's base + the hits of that tile below it; clean = one tile, every
    position from start to end a hit."""
    hit = np.zeros(1300, bool)
    hit[[3, 4, 5]] = True            # hits 0, 1, 2 of tile 0
    hit[10:20] = True                # hits 3 .. 12
    hit[500:530] = True              # 12 hits in tile 0 (500 .. 511), 18 in tile 1
    hit[600:610] = True
    hit[1024] = True
    hit[1299] = True
    C = PU.REG_CLEAN
    regs = [(3, 5), (10, 19), (500, 529), (500, 511), (512, 529), (600, 609), (1024, 1024), (1299, 1299),
            (10, 25),      # its end is no hit (defineStructure2 leaves such ends)
            (7, 19),       # its start is no hit: the index counts the hits below it all the same
            (3, 19)]       # a hole inside
    w = PU.region_words_reference(hit, regs)
    assert w.tolist() == [0 | C, 3 | C, 13, 13 | C, 512 | C, (512 + 18) | C, 1024 | C, (1024 + 1) | C, 3, 3, 0]
    # a tile's last position and the next tile's first are never one clean region, full of hits or not
    assert PU.region_words_reference(np.ones(1024, bool), [(511, 512), (0, 511), (512, 1023)]).tolist() == [511, 0 | C, 512 | C]


def test_head_counts_and_span_reference():
    assert PU.head_counts_reference(np.arange(1, 40, dtype=np.uint32)).tolist() == list(range(1, 17))
    assert PU.head_counts_reference(np.array([7, 0, 9], np.uint32)).tolist() == [7, 0, 9] + [0] * 13
    assert PU.in_span_reference(np.array([[3, 5], [10, 10]])) == 4 and PU.in_span_reference(np.zeros((0, 2))) == 0


def _hand_table(transcripts, k, depth=9):
    q = O.params(k=k)
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    cnt = {}
    for t in transcripts:
        for i in range(len(t) - k + 1):
            v = 0
            for ch in t[i:i + k]:
                v = (v << 2) | code[ch]
            cnt[v] = depth
    tab = O.OracleTable(q, O.OracleTable.FLAT)
    tab.insert_packed(np.fromiter(cnt.keys(), np.uint64, len(cnt)), np.fromiter(cnt.values(), np.uint32, len(cnt)))
    return tab


def test_oracle_out_degrees_on_a_hand_graph():
    """A fork and two dead ends: P + A + S1 and P + C + S2 (random text, K = 18: no (K-1)-mer repeats)."""
    import random
    rnd = random.Random(77)
    k = 18
    P, S1, S2 = ("".join(rnd.choice("ACGT") for _ in range(n)) for n in (40, 30, 30))
    t1, t2 = P + "A" + S1, P + "C" + S2
    tab = _hand_table([t1, t2], k)
    left, right = tab.out_degrees(t1)
    n = len(t1) - k + 1
    fork = len(P) - k                      # the last k-mer that lies in P alone: two successors
    assert len(left) == len(right) == n
    assert right.tolist() == [2 if i == fork else (0 if i == n - 1 else 1) for i in range(n)]
    assert left.tolist() == [0] + [1] * (n - 1)
    # walking LEFT out of the branch, the k-mers up to the join have one predecessor each; seen from t2 the same
    l2, r2 = tab.out_degrees(t2)
    assert l2.tolist() == left.tolist() and r2.tolist() == right.tolist()
    # a k-mer that is not in the table still has the degrees of its neighbours in the graph; one with an N has none
    mixed = t1[:50] + "N" + t1[51:]
    lm, rm = tab.out_degrees(mixed)
    for i in range(n):
        if i <= 50 < i + k:
            assert (lm[i], rm[i]) == (0, 0), i
        else:
            assert (lm[i], rm[i]) == (left[i], right[i]), i
    assert tab.out_degrees("ACGT")[0].shape == (0,) and tab.out_degrees(t1[:k])[1].tolist() == [1]
    # degrees agree with the successor counts they are defined by
    for i in (0, fork, n - 1):
        for d, got in ((0, left[i]), (1, right[i])):
            c, _ = tab.next_counts(t1[i:i + k], d)
            assert int((c >= 2).sum()) == got


def test_python_walk_on_a_five_kmer_graph():
    """K = 3, MIN_COUNT 2: ACG 5, CGT 7, GTA 3, GTC 9, TCA 9000 — every level word worked out by hand."""
    k, minc = 3, 2
    enc = lambda s: int("".join("%d%d" % divmod("ACGT".index(c), 2) for c in s), 2)
    keys = np.array([enc(x) for x in ("ACG", "CGT", "GTA", "GTC", "TCA")], np.uint64)
    counts = np.array([5, 7, 3, 9, 9000], np.uint32)
    right, left = PU.bucket_dicts(keys, counts, k, minc)
    assert right == {enc("AC"): [0, 0, 5, 0], enc("CG"): [0, 0, 0, 7], enc("GT"): [3, 9, 0, 0], enc("TC"): [9000, 0, 0, 0]}
    assert left == {enc("CG"): [5, 0, 0, 0], enc("GT"): [0, 7, 0, 0], enc("TA"): [0, 0, 3, 0], enc("TC"): [0, 0, 9, 0], enc("CA"): [0, 0, 0, 9000]}
    succ = lambda key, d: (right if d else left).get(key)
    S, B = PU.WALK_SINGLE, PU.WALK_BASE_SHIFT
    # RIGHT from AC: G (single), then CG: T (single), then GT: C with 9 beside A with 3 (a fork: not single), then TC: 9000 does not fit
    lv, why = PU.walk_reference(succ, enc("AC"), 1, k, minc)
    assert lv == [5 | S | (2 << B), 7 | S | (3 << B), 9 | (1 << B), 0x1FFF] + [0] * 8 and why == "clamp"
    # LEFT from TA: G (GTA), then GT: C (CGT), then CG: A (ACG), then AC: no k-mer ends with AC
    lv, why = PU.walk_reference(succ, enc("TA"), 0, k, minc)
    assert lv == [3 | S | (2 << B), 7 | S | (1 << B), 5 | S] + [0] * 9 and why == "missing"
    # a count that equals MIN_COUNT beside the top one: not single; below it: single
    assert PU.walk_reference(lambda key, d: [9, 2, 0, 0] if key == 0 else None, 0, 1, k, minc)[0][0] == 9
    assert PU.walk_reference(lambda key, d: [9, 1, 0, 0] if key == 0 else None, 0, 1, k, minc)[0][0] == 9 | S
    # a tie goes to the first base; a cycle runs through all twelve levels
    lv, why = PU.walk_reference(lambda key, d: [4, 4, 0, 0], 0, 1, k, minc)
    assert lv == [4] * 12 and why == "last"
    assert PU.walk_reference(lambda key, d: [0, 0, 0, 0], 0, 1, k, minc) == ([0] * 12, "count0")


def test_comb_generator_is_the_stated_one():
    rng = np.random.default_rng(5)
    s = "ACGT" * 40
    n = PU.comb(s, 21, "N", rng)
    pos = [i for i, c in enumerate(n) if c == "N"]
    assert len(n) == len(s) and pos and pos[0] < 21 and all(22 <= b - a <= 26 and (b - a - 21) in (1, 2, 3, 5) for a, b in zip(pos, pos[1:]))
    assert all(a == b for i, (a, b) in enumerate(zip(s, n)) if i not in pos)
    m = PU.comb(s, 21, "sub", np.random.default_rng(5))
    diff = [i for i in range(len(s)) if s[i] != m[i]]
    assert "N" not in m and len(diff) >= 5 and all(b - a >= 22 for a, b in zip(diff, diff[1:]))


@pytest.mark.parametrize("graph", list(PU.COMB_GRAPHS))
def test_comb_reads_reach_the_paths_beyond_512_regions(graph):
    """The reach conditions of the comb cases of tests/test_gpu_structure.py, from the oracle alone (measured when the
    cases were written: 19 and more of 24 reads beyond 512 raw regions at K = 21; the oracle edits the regions beyond the
    512th in 17 and more reads of a substituted set, in none of an N set; 2-3 reads beyond 512 at K = 31)."""
    k, seed, kw = PU.comb_synth_kw(graph)
    S = Synth(target_kmers=600_000, k=k, seed=seed, **kw)
    keys, counts = S.dump_arrays()
    q = O.params(k=k)
    tab = O.OracleTable(q, O.OracleTable.FLAT)
    tab.insert_packed(keys, counts)
    tab.decolour()
    sets = PU.comb_reads(S, k)
    assert all(len(v) == 24 for v in sets.values())
    print("read lengths", sorted(len(s) for s in sets["N"]))
    for how, reads in sets.items():
        facts = [PU.structure_facts(tab, s, q.min_count) for s in reads]
        PU.assert_comb_reach(graph, how, facts)
