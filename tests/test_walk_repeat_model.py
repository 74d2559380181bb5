"""walk_repeat_possible (talc_pure.h) — the test walk_record makes before its in-record cycle chain — against direct
comparison of the k-mers of a record.

A case is K + 12 bases in growth order (oldest first): the tip and the twelve bases a walk record would append.  The
brute force (pure_walk_repeat_check in pure_capi.cpp, on plain base arrays, no packing) forms the twelve tips after
levels 0..11 and compares every pair; bit p of `pair` says that two of them p levels apart are equal.  Bit p of `pred`
is the predicate for period p on the packed tip, as the kernel holds it in that direction.  The predicate has to be
NECESSARY: a pair at distance p without its bit would be a cycle the walk runs through.

Random cases (10^6 per K, both directions) and constructed ones: every period p in 1..11 and every level a in 0..11-p at
which the first fully periodic k-mer can fall (its repeat is level a + p), the run broken one base before it, so it
begins inside the tip — at K = 12 the later k-mers are made of new bases alone — and runs that start at the tip's oldest
base.  Random cases hold next to no true pair (a pair costs K equalities), so the constructed ones must show theirs in
the brute force: the comparison is not vacuous.

Rarity (what makes the predicate worth its instructions): at K = 21 it fires on fewer than 1 tip in 10^4 of random
sequence; 11 x 4^-9 = 4.2e-5 is expected."""
import ctypes as C

import numpy as np
import pytest

from talc_amd import build as B

LEVELS = 12
KS = (12, 13, 14, 18, 21, 30, 31)
ALL_P = sum(1 << p for p in range(1, LEVELS))
N_RANDOM = 1_000_000


@pytest.fixture(scope="module")
def check():
    L = C.CDLL(B.build_pure())
    f = L.pure_walk_repeat_check
    f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    f.restype = None

    def run(g, k, dir_right):
        g = np.ascontiguousarray(g, dtype=np.uint8)
        assert g.ndim == 2 and g.shape[1] == k + LEVELS and int(g.max(initial=0)) < 4
        pair, pred = np.zeros(len(g), np.uint32), np.zeros(len(g), np.uint32)
        f(g.ctypes.data, len(g), k, int(dir_right), pair.ctypes.data, pred.ctypes.data)
        return pair, pred
    return run


@pytest.fixture(scope="module")
def random_cases():
    """One array per K, shared by both directions and every test (never written to)."""
    rng = np.random.default_rng(20)
    out = {}
    for k in KS:
        g = rng.integers(0, 4, (N_RANDOM, k + LEVELS), dtype=np.uint8)
        g.setflags(write=False)
        out[k] = g
    return out


def constructed(k, rng, fills=6):
    """(cases, period of each): G[t] = G[t - p] for t in [a + 1 + p, a + K + p], so the tips after levels a and a + p are
    equal; where there is room G[a + p] != G[a], so that level a's is the first such k-mer.  Also runs from base 0 on and
    runs that cover the whole case."""
    gs, ps = [], []
    n = k + LEVELS
    for p in range(1, LEVELS):
        for a in range(0, LEVELS - p):
            for _ in range(fills):
                g = rng.integers(0, 4, n, dtype=np.uint8)
                g[a + p] = (g[a] + 1 + rng.integers(0, 3)) % 4
                for t in range(a + 1 + p, a + k + p + 1):
                    g[t] = g[t - p]
                gs.append(g)
                ps.append(p)
        for start in (0, 1):                       # the run begins at the tip's oldest base / covers everything
            g = rng.integers(0, 4, n, dtype=np.uint8)
            for t in range(start + p, n):
                g[t] = g[t - p]
            gs.append(g)
            ps.append(p)
    return np.stack(gs), np.array(ps)


@pytest.mark.parametrize("dir_right", [1, 0], ids=["RIGHT", "LEFT"])
@pytest.mark.parametrize("k", KS)
def test_predicate_is_necessary_on_random_cases(check, random_cases, k, dir_right):
    pair, pred = check(random_cases[k], k, dir_right)
    assert (pair & ~np.uint32(ALL_P)).max() == 0 and (pred & ~np.uint32(ALL_P)).max() == 0
    missed = np.nonzero(pair & ~pred)[0]
    print("K=%d dir=%d: cases %d, with a pair %d, predicate fires on %d" % (k, dir_right, len(pair), int((pair != 0).sum()), int((pred != 0).sum())))
    assert len(missed) == 0, (k, dir_right, missed[:5], pair[missed[:5]], pred[missed[:5]])
    if k == 12:
        assert (pred == ALL_P).all()


@pytest.mark.parametrize("dir_right", [1, 0], ids=["RIGHT", "LEFT"])
@pytest.mark.parametrize("k", KS)
def test_predicate_is_necessary_on_constructed_repeats(check, k, dir_right):
    g, ps = constructed(k, np.random.default_rng(100 + k))
    pair, pred = check(g, k, dir_right)
    bit = (np.uint32(1) << ps.astype(np.uint32))
    assert ((pair & bit) != 0).all(), np.nonzero((pair & bit) == 0)[0][:5]      # the case holds the pair it was built for
    missed = np.nonzero(pair & ~pred)[0]
    assert len(missed) == 0, (k, dir_right, missed[:5], ps[missed[:5]], pair[missed[:5]], pred[missed[:5]])
    assert sorted(set(ps.tolist())) == list(range(1, LEVELS))
    if k == 12:
        assert (pred == ALL_P).all()


def test_both_directions_agree_on_a_case(check, random_cases):
    """The predicate is a statement about the bases in growth order, so the two packings must give the same answer."""
    for k in (13, 21, 31):
        g = random_cases[k][:200_000]
        assert np.array_equal(check(g, k, 1)[1], check(g, k, 0)[1])


@pytest.mark.parametrize("dir_right", [1, 0], ids=["RIGHT", "LEFT"])
def test_predicate_is_rare_at_k21(check, random_cases, dir_right):
    _, pred = check(random_cases[21], 21, dir_right)
    fired = int((pred != 0).sum())
    print("K=21 dir=%d: predicate fires on %d of %d tips (expected %.0f)" % (dir_right, fired, N_RANDOM, N_RANDOM * 11 * 4.0 ** -9))
    assert fired * 10_000 < N_RANDOM
