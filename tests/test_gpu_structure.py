"""-m gpu: what sits between coverage and search, compared with the oracle directly instead of through the records it
leads to — the structure kernel (regions, threshold, status, the hit index and clean flag of every region, head counts,
span) and the degree bits the coverage kernel leaves beside every hit.

References: OracleTable.structure for regions, threshold and ok; numpy over OracleTable.coverage for the region words,
the head counts and the span (parity_util.region_words_reference, checked by hand in test_structure_reference.py);
OracleTable.out_degrees for the degree bits.  Every comparison is exact: integers equal, the threshold equal as a bit
pattern (the same IEEE operations in the same order on both sides).

Regions and threshold are compared for the reads with a structure AND for those without one (NO_STRUCTURE): the oracle's
defineStructure2 sets both before setInitialStructure's length check fails, and keeps the original list when no region
qualified (Read.cpp:599).  Reads of K bases or fewer and reads without a solid k-mer never reach the structure stage on
either side: for them the status and "no regions" are compared, nothing else exists.

Every read of a case goes through ONE batch (a read's region, k-mer and bitmap-word offsets depend on its neighbours),
then through a permuted batch.  Each case states, from the oracle's data alone, what its inputs must reach."""
import random
import struct
import time

import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
from stress_cases import CASES
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

DEG_KNOWN = 0x40   # talc_batch_fetch_coverage_degrees: right degree | left degree << 3 | known << 6


def _oracle_facts(pair, seq, degrees):
    """`seq` as the device works on it."""
    k = pair.p.k
    f = PU.structure_facts(pair.otab, seq, pair.p.min_count)
    f["status"] = (T.READ_SKIPPED_SHORT if len(seq) <= k else T.READ_NO_SOLID_KMER if f["nin"] <= 0
                   else T.READ_CORRECTED if f["ok"] else T.READ_NO_STRUCTURE)
    if degrees:
        f["deg"] = pair.otab.out_degrees(seq)
    return f


def _compare_batch(pair, seqs, facts, order, degrees, label):
    bases, offs = PU.pack_reads([seqs[i] for i in order])
    b = pair.ctx.batch(bases, offs)
    b.structure()
    g = b.fetch_structure()
    if degrees:
        gdeg = b.fetch_coverage_degrees()
        _, _, ko, _ = b.fetch_coverage()
    b.close()
    ro = g["region_offsets"].astype(np.int64)
    compared = 0
    for j, i in enumerate(order):
        f, where = facts[i], (label, "read", i, "slot", j)
        assert int(g["status"][j]) == f["status"], (where, int(g["status"][j]), f["status"])
        greg = g["regions"][ro[j]:ro[j + 1]].astype(np.int64)
        assert int(g["n_regions"][j]) == len(greg)
        if f["status"] in (T.READ_SKIPPED_SHORT, T.READ_NO_SOLID_KMER):
            assert len(greg) == 0, where
        else:
            compared += 1
            assert len(greg) == len(f["reg"]) and (greg == f["reg"]).all(), (where, len(greg), len(f["reg"]))
            assert struct.pack("<d", float(g["lam"][j])) == struct.pack("<d", f["thr"]), (where, float(g["lam"][j]), f["thr"])
            hit = f["cov"] > 0
            want = PU.region_words_reference(hit, f["reg"])
            got = g["region_hits"][ro[j]:ro[j + 1]]
            assert (got == want).all(), (where, np.nonzero(got != want)[0][:5], got[got != want][:5], want[got != want][:5])
            assert g["head_counts"][j].tolist() == PU.head_counts_reference(f["cov"]).tolist(), where
            assert int(g["in_span"][j]) == PU.in_span_reference(f["reg"]), where
        if degrees:
            d = gdeg[int(ko[j]):int(ko[j + 1])]
            assert len(d) == len(f["cov"]), where
            hit = f["cov"] > 0
            left, right = f["deg"]
            want = np.where(hit, DEG_KNOWN | right | (left << 3), 0).astype(np.uint8)
            assert (d == want).all(), (where, np.nonzero(d != want)[0][:5], d[d != want][:5], want[d != want][:5])
    return compared


def _compare_case(pair, seqs, label, degrees=True, oracle_seqs=None):
    """Every read in one batch, then in a permuted batch; returns the oracle's facts per read."""
    t0 = time.time()
    facts = [_oracle_facts(pair, s, degrees) for s in (oracle_seqs or seqs)]
    t1 = time.time()
    n = len(seqs)
    c1 = _compare_batch(pair, seqs, facts, list(range(n)), degrees, label)
    c2 = _compare_batch(pair, seqs, facts, np.random.default_rng(17).permutation(n).tolist(), degrees, label + " permuted")
    # no read is left out: only those of K bases or fewer and those without a solid k-mer have no region comparison
    assert c1 == c2 == sum(1 for s, f in zip(oracle_seqs or seqs, facts) if len(s) > pair.p.k and f["nin"] > 0)
    st = np.bincount([f["status"] for f in facts], minlength=4).tolist()
    print("%s: %d reads, status %s, raw regions up to %d, edited by analyzeINRegions %d; oracle %.1f s, device + compare %.1f s"
          % (label, n, st, max([len(f["raw"]) for f in facts] + [0]), sum(f["changed"] for f in facts), t1 - t0, time.time() - t1))
    return facts


def _reads(pair, first, n):
    return PU.seqs_of(*pair.reads(first, n))


def _clean_reads(pair, first, n, rate):
    """Reads of the pair's own transcriptome with `rate` substitutions / insertions / deletions each instead of 4 %."""
    from talc_amd.synth import Synth
    S = Synth(target_kmers=int(pair.synth.spec.target_kmers), k=pair.synth.k, seed=int(pair.synth.spec.seed),
              sub_rate=rate, ins_rate=rate, del_rate=rate)
    return PU.seqs_of(*S.reads(first, n))


def _stress_pair(case):
    kw, pkw = CASES[case]
    pair = PU.Pair(**kw, **pkw)
    pair.upload(0)
    return pair


# ---------------------------------------------------------------- 1. the suite's own inputs
def test_structure_of_the_session_pair(gpu_pair):
    facts = _compare_case(gpu_pair, _reads(gpu_pair, 1000, 600), "session pair")
    assert 4 * sum(f["changed"] for f in facts) >= len(facts)      # (264 of 598 when written: the walks and fix-ups run)


def test_structure_on_a_branching_graph():
    pair = _stress_pair(103)
    _compare_case(pair, _reads(pair, 0, 600), "set 103")


def test_structure_of_the_read_whose_region_ends_on_no_hit():
    """Set 103, reads 1300 .. 1399: a region whose last position is not a hit must not be flagged clean (the one parity
    bug of the history, test_region_whose_last_position_is_not_a_hit) — here seen in the flag itself."""
    pair = _stress_pair(103)
    facts = _compare_case(pair, _reads(pair, 1300, 100), "set 103 from 1300")
    # a region that passes every other term of `clean` (one tile, every position before the end a hit) but ends on no hit
    n = 0
    for f in facts:
        hit = f["cov"] > 0
        n += sum(1 for s, e in f["reg"].tolist() if e > s and s // PU.COV_TILE == e // PU.COV_TILE and hit[s:e].all() and not hit[e])
    assert n >= 1


def test_structure_of_long_reads_with_few_solid_kmers():
    pair = _stress_pair(105)
    facts = _compare_case(pair, _reads(pair, 0, 200), "set 105")
    minc = pair.p.min_count
    assert sum(1 for f in facts if f["nin"] > 0 and 0 < int((f["cov"] >= minc).sum()) <= 10) >= 8      # (16 when written: no trimming)
    assert max(len(f["raw"]) for f in facts) > 48


def test_structure_with_counts_beyond_the_histogram():
    """Counts x 700: every read has a count of 1024 or more, so the threshold comes from the bisection
    (trimmed_prefix_sum), not from the LDS histogram."""
    pair = PU.Pair(target_kmers=200_000, k=21, seed=23, count_scale=700, min_count=2 * 700)
    pair.upload(0)
    facts = _compare_case(pair, _reads(pair, 0, 150), "counts x 700")
    reached = [f for f in facts if f["status"] in (T.READ_CORRECTED, T.READ_NO_STRUCTURE)]
    assert len(reached) >= 140 and all(int(f["cov"].max()) >= 1024 for f in reached)


def test_structure_of_reads_without_one():
    pair = _stress_pair(403)
    facts = _compare_case(pair, _reads(pair, 0, 300), "set 403")
    assert sum(f["status"] == T.READ_NO_STRUCTURE for f in facts) >= 10       # (19 when written)


# ---------------------------------------------------------------- 2. hand reads
def test_structure_of_edge_inputs(gpu_pair):
    r = _reads(gpu_pair, 5000, 8)
    q = _reads(gpu_pair, 12000, 2)
    reads = ["", r[0][:21], r[0][:22], r[1].lower(), r[2][:400] + "N" + r[2][400:],
             r[3][:300] + "N" * 10 + r[3][300:900] + "RYKM" + r[3][900:], "ACGT" * 300, "A" * 500,
             "".join(random.Random(1).choice("ACGT") for _ in range(1500)), r[4], r[5][:60], r[6] + r[7],
             q[0][:21], q[1][:22], "ACGT" * 200, "N" * 80, "".join(random.Random(5).choice("ACGT") for _ in range(900))]
    facts = _compare_case(gpu_pair, reads, "hand reads")
    st = [f["status"] for f in facts]
    assert st[0] == st[1] == T.READ_SKIPPED_SHORT and T.READ_NO_SOLID_KMER in st and T.READ_CORRECTED in st


# ---------------------------------------------------------------- 3. parameters
@pytest.mark.parametrize("kw", [dict(k=18), dict(k=25), dict(k=31), dict(min_count=3, window_size=6, max_nb_competing_paths=5)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_structure_parameter_variants(kw):
    kw = dict(kw)
    k = kw.pop("k", 21)
    pair = PU.Pair(target_kmers=250_000, k=k, seed=20 + k, **kw)
    pair.upload(0)
    _compare_case(pair, _reads(pair, 0, 160), "k=%d %s" % (k, kw), degrees=False)


def test_structure_with_junction_colours():
    pair = PU.Pair(target_kmers=300_000, k=21, seed=31, junctions=True)
    pair.upload(0)
    _compare_case(pair, _reads(pair, 0, 300), "junction colours", degrees=False)


def test_structure_in_reverse_mode():
    """-rev: the device works on the reverse complement (main.cpp:253), so the oracle is given it."""
    pair = PU.Pair(target_kmers=300_000, k=21, seed=32, reverse=1)
    pair.upload(0)
    reads = [PU.revcomp(s) for s in _reads(pair, 0, 200)]
    facts = _compare_case(pair, reads, "reverse", degrees=True, oracle_seqs=[PU.revcomp(s) for s in reads])
    assert sum(f["status"] == T.READ_CORRECTED for f in facts) > 150


# ---------------------------------------------------------------- 4. long regions
def test_structure_of_nearly_clean_reads(gpu_pair):
    """Error-free and 0.3 %-error reads: regions of a thousand k-mers cross the tiles of 512 positions, so their clean flag
    must be off, and on for the short ones."""
    reads = _clean_reads(gpu_pair, 200, 12, 0.0) + _clean_reads(gpu_pair, 200, 80, 0.003)
    facts = _compare_case(gpu_pair, reads, "nearly clean")
    words = np.concatenate([PU.region_words_reference(f["cov"] > 0, f["reg"]) for f in facts if len(f["reg"])])
    spans = np.concatenate([f["reg"][:, 1] - f["reg"][:, 0] + 1 for f in facts if len(f["reg"])])
    clean = (words & PU.REG_CLEAN) != 0
    assert clean.sum() >= 20 and (~clean).sum() >= 20 and int(spans[~clean].max()) >= 1000 and int(spans.max()) >= 1000


# ---------------------------------------------------------------- 5. comb reads: hundreds of regions per read
@pytest.fixture(scope="module", params=list(PU.COMB_GRAPHS))
def comb_pair(request):
    k, seed, kw = PU.comb_synth_kw(request.param)
    pair = PU.Pair(target_kmers=600_000, k=k, seed=seed, synth_kw=kw)
    pair.upload(0)
    pair.graph = request.param
    pair.comb = PU.comb_reads(pair.synth, k)
    return pair


@pytest.mark.parametrize("how", ["N", "sub"])
def test_structure_of_comb_reads(comb_pair, how):
    """An error-free read of 12-20 kb with one base every K + g positions replaced by N, or substituted: 560-890 raw IN
    regions per read.  The structure kernel keeps the region-end degrees of its first 512 regions in LDS and reads the
    coverage word per position beyond them; every loop over regions takes more than one 64-region pass.  The N combs keep
    every region (the degree reads beyond the 512th), the substituted ones have ends of degree 0 there (the per-position
    walks and span fix-ups beyond the 512th)."""
    facts = _compare_case(comb_pair, comb_pair.comb[how], "comb %s %s" % (comb_pair.graph, how))
    PU.assert_comb_reach(comb_pair.graph, how, facts)
    if comb_pair.graph == "branching-k21" and how == "sub":
        # degrees 0, 1 and >= 2 all occur in both directions among the compared (hit) positions
        for d in (0, 1):
            v = np.concatenate([f["deg"][d][f["cov"] > 0] for f in facts if len(f["cov"])])
            assert (v == 0).sum() >= 50 and (v == 1).sum() >= 1000 and (v >= 2).sum() >= 50, (d, np.bincount(v).tolist())


@pytest.mark.parametrize("how", ["N", "sub"])
def test_correction_of_comb_reads(comb_pair, how):
    """The search has never seen a read with more than 64 regions either: the whole correction against the oracle."""
    bases, offs = PU.pack_reads(comb_pair.comb[how])
    t0 = time.time()
    bad, (so, ost), (sg, gst) = PU.compare_correction(comb_pair, bases, offs, nthreads=16, verbose=False)
    print("comb %s %s corrected: status %s, oracle %.1f s, device %.1f s, %.1f s in all"
          % (comb_pair.graph, how, np.bincount(ost, minlength=4).tolist(), *comb_pair.last_times, time.time() - t0))
    if bad:
        raise AssertionError("comb reads %s differ; first trace difference of read %d: %s"
                             % (bad[:8], bad[0], PU.first_trace_diff(comb_pair, bases, offs, bad[0])))
    assert comb_pair.ctx.timing().n_failed == 0


# ---------------------------------------------------------------- coverage degrees at the tile and read edges
def test_coverage_degrees_where_nobody_publishes_the_right_degree(gpu_pair):
    """A hit's right degree is published through LDS by the NEXT position's lookup of the same tile; a hit at a tile's last
    position (511, 1023), at the read's last position, or before a k-mer that holds an N has no such neighbour and is
    probed.  Error-free reads, so that the positions in question are hits."""
    k = gpu_pair.p.k
    r = [s for s in _clean_reads(gpu_pair, 0, 12, 0.0) if len(s) > 1100][:3]
    assert len(r) == 3
    reads = [r[0], r[0][:511 + k], r[0][:512 + k], r[0][:513 + k], r[1][:1023 + k], r[1][:1024 + k], r[1][:1025 + k], r[1],
             r[2][:300] + "N" + r[2][301:], r[2][:511 + k] + "N" + r[2][512 + k:], r[0][:k], r[0][:k + 1], r[1][:700].lower()]
    facts = _compare_case(gpu_pair, reads, "degree edges")
    cov = [f["cov"] for f in facts]
    for i, p in ((0, 511), (0, 512), (0, 1023), (1, 510), (1, 511), (2, 511), (2, 512), (3, 512), (3, 513), (4, 1022), (4, 1023),
                 (5, 1023), (5, 1024), (6, 1024), (6, 1025), (8, 279), (8, 301), (9, 511), (9, 512 + k), (10, 0), (11, 0), (11, 1)):
        assert cov[i][p] > 0, (i, p)                       # a hit
    for i in (1, 2, 3, 4, 5, 6, 10, 11):
        assert len(cov[i]) - 1 in (511, 512, 513, 1023, 1024, 1025, 0, 1)         # ... at the read's last position
    assert cov[8][280] == 0 and cov[8][300] == 0 and cov[9][512] == 0      # the k-mers with the N are none
