"""Inputs for the retry stages of the correction (search_retry_passes: the first pass, a stage with capacities x 8, one
with x 64).  Nothing here needs a GPU: tests/test_retry_reference.py asserts from the oracle alone that every case is what
its name says, tests/test_gpu_retry_stages.py runs them through the HIP path under TALC_TEST_TINY_CAPS = 2 and 3 and, the
constructed read, under no hook at all.

Hook inputs.  Under the hook a stage has anchCap = 3, fullCap = 1 and a bridge pool of one Trail (make_caps): a read is
flagged when a side of a search records more than three positions or a search records a second bridge.  The sets are the
ones the other retry tests use: the generator's default graph at K = 21 (the session's pair, reads 7000 .. 7199), a
branching graph (paralog families), tandem repeats (cycles), K = 18 and K = 31, and one read of long_gap_cases.py whose two
Trails tie to the end of a gap, so that its search records two bridges.

The constructed read needs the x 64 stage without a hook.  anchCap is min(max(256 * scale, 2048), L + 8): 2048 in the first
pass and in the x 8 stage, L + 8 at x 64 for a read below 16 376 bases.  The position list of a side (Explorer.cpp:427-447;
build_anchors_body: anchorPos) takes the pivot and then every position whose count is not expected after the last one
taken while both are IN counts.  The read has two solid regions of REGION k-mers around a short weak stretch, and the table
counts of a region's k-mers alternate between two levels neither of which is expected after the other
(is_expected_by_last_node): every position of the region is taken, the list has REGION entries, more than 2048.  With
FORK_EVERY > 0 every FORK_EVERY-th k-mer of a region has a second successor and a second predecessor in the table and
some thirty positions become anchors (the anchor sort beyond 16 elements); it is 0, test_retry_reference.py says why.
"""
import random

import numpy as np

import long_gap_cases as LG
import parity_util as PU

ANCH_CAP_FLOOR = 2048            # make_caps: anchCap below x 64
ANCH_CAP_X64 = 256 * 64
HEAD_COV = PU.HEAD_COV

# name -> (pair keywords, first read, reads)
GENERATOR_SETS = {
    "default-k21": (dict(target_kmers=400_000, k=21, seed=11), 7000, 200),            # conftest.gpu_pair
    "paralogs-k21": (dict(target_kmers=250_000, k=21, seed=77, synth_kw=dict(paralog_frac=0.5, paralog_div=0.03)), 0, 120),
    "k18": (dict(target_kmers=250_000, k=18, seed=38), 0, 100),
    "k31": (dict(target_kmers=250_000, k=31, seed=51), 0, 100),
}
LONG_GAP = "instance-8-ref-512"
HOOK_INPUTS = tuple(GENERATOR_SETS) + ("tandem-k21", "long-gap")
MAX_READ = 7000 + 1000           # the generator's reads are "7 kb" before their insertions


def _noisy(rnd, seq, rate):
    out = []
    for ch in seq:
        x = rnd.random()
        if x < rate * 0.4:
            out.append(rnd.choice("ACGT"))
        elif x < rate * 0.7:
            continue
        elif x < rate:
            out.append(ch + rnd.choice("ACGT"))
        else:
            out.append(ch)
    return "".join(out)


def tandem_set(k=21, seed=1234, n_transcripts=30, per=3):
    """(transcripts, reads): tandem repeats with a unit of K + 2 .. 3 K bases, 2 - 6 copies, a diverged copy in some, and
    reads with 8 - 14 % errors across them (the construction of test_gpu_parity's tandem-repeat test, half its size)."""
    rnd = random.Random(seed)
    transcripts = []
    for _ in range(n_transcripts):
        parts = ["".join(rnd.choice("ACGT") for _ in range(rnd.randint(150, 400)))]
        for _ in range(rnd.randint(1, 3)):
            unit = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(k + 2, 3 * k)))
            for _ in range(rnd.randint(2, 6)):
                u = unit
                if rnd.random() < 0.3:
                    i = rnd.randrange(len(u))
                    u = u[:i] + rnd.choice("ACGT".replace(u[i], "")) + u[i + 1:]
                parts.append(u)
            parts.append("".join(rnd.choice("ACGT") for _ in range(rnd.randint(100, 350))))
        transcripts.append("".join(parts))
    reads = []
    for t in transcripts:
        for _ in range(per):
            reads.append(_noisy(rnd, t[rnd.randint(0, 60):len(t) - rnd.randint(0, 60)], rnd.choice([0.08, 0.11, 0.14])))
    return transcripts, reads


# ---------------------------------------------------------------- the constructed read
REGION = 2600                    # k-mers per solid region
WEAK = 31                        # bases of the weak stretch between them
HEAD = TAIL = 45                 # noisy bases before the first and after the last region
LEVELS = (20, 50)                # alpha = 2.57: after 20 a count is expected in [11, 34], after 50 in [34, 72]
BETWEEN = 34                     # ... and 34 after either: the count of the true k-mers outside the regions
FORK_EVERY = 0                   # (0: no forks, see test_retry_reference.py)


class Constructed:
    """k, truth, read, keys / counts (the table's dump), regions ((first, last) k-mer position of the two regions in the
    read), levels."""


def _code(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def _other(b, rng):
    return [c for c in "ACGT" if c != b][int(rng.integers(0, 3))]


def constructed(k=21, seed=5):
    rng = np.random.default_rng(seed)
    span = REGION + k - 1                                    # bases of a region
    n = HEAD + span + WEAK + span + TAIL
    t = "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    a0, b0 = HEAD, HEAD + span + WEAK                        # first k-mer of either region
    read = list(t)
    noisy = list(range(0, HEAD, 6)) + [HEAD - 1] + [a0 + span + i for i in range(0, WEAK, 10)] + [b0 - 1]
    noisy += list(range(b0 + span, n, 6))
    for p in set(noisy):
        read[p] = _other(t[p], rng)
    cnt = {}
    for p in range(n - k + 1):
        in_a, in_b = a0 <= p < a0 + REGION, b0 <= p < b0 + REGION
        c = LEVELS[(p - (a0 if in_a else b0)) % 2] if (in_a or in_b) else BETWEEN
        cnt.setdefault(_code(t[p:p + k]), c)
    assert len(cnt) == n - k + 1                             # (no k-mer twice: the counts are what the positions say)
    for r0 in (a0, b0) if FORK_EVERY else ():
        for p in range(r0 + FORK_EVERY // 2, r0 + REGION - 1, FORK_EVERY):
            km = t[p:p + k]
            cnt.setdefault(_code(km[1:] + _other(t[p + k], rng)), LEVELS[0])       # a second successor
            cnt.setdefault(_code(_other(t[p - 1], rng) + km[:-1]), LEVELS[0])      # a second predecessor
    c = Constructed()
    c.k, c.truth, c.read = k, t, "".join(read)
    c.keys = np.fromiter(cnt.keys(), dtype=np.uint64, count=len(cnt))
    c.counts = np.fromiter(cnt.values(), dtype=np.uint32, count=len(cnt))
    c.regions = ((a0, a0 + REGION - 1), (b0, b0 + REGION - 1))
    c.levels = LEVELS
    return c


def position_list(cov, first, last, side, expected, minc, max_in):
    """The positions a side's walk records (Explorer.cpp:427-447 / 493-513) over the region [first, last] of a read whose
    counts are `cov`: side 0 walks from `last` down, side 1 from `first` up; expected(next, current) is
    isExpectedbyLastNode."""
    pivot, step, end = (last, -1, first) if side == 0 else (first, 1, last)
    out, cur = [pivot], int(cov[pivot])
    p = pivot
    while p != end:
        p += step
        c = int(cov[p])
        if c >= minc and c < max_in and expected(c, cur):
            continue
        if cur >= minc and c >= minc and c < max_in:
            out.append(p)
            cur = c
        else:
            break
    return out


# ---------------------------------------------------------------- make_caps in Python integers
NBUF, TCAP, ROW_ARENA_INTS, WIDE_BLOOM_WORDS = 576, 320, 448 * 1024, 16384
SAT = 0xFFFFFF00
FIELDS = ("seqCap", "seqArena", "refCap", "edgeCap", "anchCap", "fullCap", "fullPool", "dpCap", "regCap", "weakPool")
REGIONS = ("setA", "setB", "seqPool", "ref", "ancL", "ancR", "ancPos", "fullMeta", "fullPoolB", "edgeLong", "edgeShort", "edgeTmp", "dp",
           "gard", "regS", "regE", "wOff", "wLen", "weak", "wideBloom", "rowPool", "regH", "trace")
ANCHOR_REC, FULL_META = 24, 24   # sizeof(AnchorRec), sizeof(FullMeta)
TRAIL_SET = (8 + 8 + 8 + 4 + 4 + 4 + 4 + 4 + 4) * TCAP


def _up(x, a):
    return (x + a - 1) // a * a


def _sat(x, a):
    return _up(min(x, SAT), a)


def caps_reference(max_len, k, scale, tiny=False):
    """make_caps (talc_kernels_search.h) with unbounded integers: (capacities by name, region sizes in layout order)."""
    c = {}
    c["seqCap"] = _up(int(1.2 * float(max_len)) + 4 * k + 64, 16)
    arena = NBUF * c["seqCap"]
    if scale == 1:
        arena = min(arena, max(1 << 20, 8 * c["seqCap"]))
    c["seqArena"] = _sat(arena, 16)
    c["refCap"] = _sat(max_len + 2 * k + 64, 16)
    c["edgeCap"] = _sat(c["seqCap"] + c["refCap"], 16)
    c["anchCap"] = max(8, min(max(256 * scale, 2048), max_len + 8))
    c["fullCap"] = 128 * scale
    c["fullPool"] = _sat(max(65536, 4 * c["seqCap"]) * scale, 16)
    c["dpCap"] = max(2048, _sat(max(c["edgeCap"], c["seqCap"]) + 8, 4))
    if tiny:
        c["anchCap"], c["fullCap"], c["fullPool"] = 3, 1, _up(c["seqCap"], 16)
    c["regCap"] = max_len // 2 + 4
    c["weakPool"] = _sat(4 * max_len + 1024, 16)
    sizes = [TRAIL_SET, TRAIL_SET, c["seqArena"], c["refCap"], c["anchCap"] * ANCHOR_REC, c["anchCap"] * ANCHOR_REC, c["anchCap"] * 4,
             c["fullCap"] * FULL_META, c["fullPool"], c["edgeCap"], c["edgeCap"], c["edgeCap"], 3 * c["dpCap"] * 4,
             (TCAP + 64) * (8 + 8 + 16 + 32 + 4), c["regCap"] * 4, c["regCap"] * 4, c["regCap"] * 4, c["regCap"] * 4, c["weakPool"],
             WIDE_BLOOM_WORDS * 8, ROW_ARENA_INTS * 4, c["regCap"] * 4, 64]
    return c, sizes
