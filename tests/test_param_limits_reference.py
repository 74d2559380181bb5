"""From the oracle alone: every case of tests/param_limit_cases.py reaches what it is there for.  The HIP path is compared
with the oracle on these cases in tests/test_gpu_param_limits.py; here the oracle's own trace says that the comparison is
one of Trail sets beyond a wave, of gardening over more than 64 candidates, and of full anchor lists.  The thresholds are
conditions on the inputs (the figures measured when the cases were made are in the messages' neighbourhood: 149 of 200
reads, 72 / 117 / 74 Trails in head / inner / tail searches of row 406; 192 and 81 Trails on the ladders)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
import param_limit_cases as PL
import parity_util as PU
from talc_amd.synth import Synth

_rows = {}


def oracle_table(keys, counts, k, **pkw):
    p, q = PU.both_params(k=k, **pkw)
    ot = O.OracleTable(q, O.OracleTable.FLAT)
    ot.insert_packed(keys, counts)
    ot.decolour()
    return ot


def packed_kmers(transcripts, k, depth=20):
    """(keys, counts) as parity_util.CustomPair stores a list of transcripts."""
    cnt = PL.kmer_counts(transcripts, k)
    keys = np.array([int(km.translate(str.maketrans("ACGT", "0123")), 4) for km in cnt], dtype=np.uint64)
    return keys, np.array([c * depth for c in cnt.values()], dtype=np.uint32)


def row_traces(case, n=None):
    """The oracle's step traces of a row's reads (the first n), made once."""
    if case not in _rows:
        kw, pkw, n_reads = PL.synthetic_row(case)
        synth = Synth(target_kmers=kw["target_kmers"], k=kw["k"], seed=kw["seed"], **kw.get("synth_kw", {}))
        _rows[case] = dict(ot=oracle_table(*synth.dump_arrays(), kw["k"], **pkw), seqs=PL.row_reads(synth, case), traces={})
    r = _rows[case]
    want = range(len(r["seqs"]) if n is None else n)
    todo = [i for i in want if i not in r["traces"]]
    with ThreadPoolExecutor(16) as ex:
        for i, t in zip(todo, ex.map(lambda i: r["ot"].trace(r["seqs"][i], steps=True), todo)):
            r["traces"][i] = t
    return [r["traces"][i] for i in want]


# ---------------------------------------------------------------- the synthetic rows
def test_the_rows_are_the_ones_the_c_abi_accepts_at_its_limits():
    rows = {c: PL.synthetic_row(c)[1] for c in PL.SYNTHETIC}
    assert (rows[406]["max_nb_competing_paths"], rows[406]["max_nb_inner_paths"]) == (64, 60)
    assert (rows[407]["max_nb_competing_paths"], rows[407]["max_nb_inner_paths"]) == (63, 59)
    assert rows[408]["check_interval"] == 1 and rows[409]["check_interval"] == 40 and rows[409]["max_nb_border_paths"] == 300
    assert (rows[410]["max_start_anchors"], rows[410]["min_start_anchors"]) == (64, 64)
    assert (rows[411]["max_start_anchors"], rows[411]["min_start_anchors"]) == (1, 63)
    assert rows[412]["max_nb_border_paths"] == 1 and rows[415]["reverse"] == 1
    ks = {c: PL.synthetic_row(c)[0]["k"] for c in PL.SYNTHETIC}
    assert ks[413] == 31 and PL.synthetic_row(413)[0]["synth_kw"]["mixed_lengths"] == 1 and ks[414] == 18
    for c in (406, 407, 408, 409, 410, 411, 413, 414, 415):
        assert rows[c]["max_nb_competing_paths"] >= 63 and rows[c]["max_nb_inner_paths"] >= 59


@pytest.mark.parametrize("case", [c for c, v in PL.SYNTHETIC.items() if "sets" in v[1]], ids=lambda c: PL.SYNTHETIC[c][0])
def test_row_has_sets_beyond_a_wave_in_every_location(case):
    traces = row_traces(case)
    big = [PL.largest_sets(t) for t in traces]
    reads = sum(max(b.values()) > PL.WAVE for b in big)
    top = {loc: max(b[loc] for b in big) for loc in (PL.HEAD, PL.INNER, PL.TAIL)}
    print("row %d: %d of %d reads with a set above 64; largest head / inner / tail %s" % (case, reads, len(traces), top))
    assert len(traces) == 200 and reads >= 100, (case, reads)
    assert all(v > PL.WAVE for v in top.values()), (case, top)


@pytest.mark.parametrize("case", [c for c, v in PL.SYNTHETIC.items() if "garden" in v[1]], ids=lambda c: PL.SYNTHETIC[c][0])
def test_row_gardens_more_than_a_wave_of_candidates_with_maxb_64(case):
    """With check_interval = 1 every step is a check step, so no set above MAXB = 64 is ever left for the trace to show; the
    twin row (the same reads, check_interval 6) shows it.  Where the two traces of a read part, on the step of an inner
    search after which the twin has more than 64 Trails and this row fewer, gardening was handed the twin's number of
    candidates with MAXB = 64."""
    assert PL.synthetic_row(case)[1]["max_nb_competing_paths"] == 64
    n = 40
    cuts = []
    for a, b in zip(row_traces(case, n), row_traces(PL.GARDEN_TWIN[case], n)):
        cuts += PL.cuts_against_twin(a, b)
    print("row %d: %d of the first %d reads part from row %d's trace at a cut of more than 64 candidates: %s" % (case, len(cuts), n, PL.GARDEN_TWIN[case], cuts[:6]))
    assert len(cuts) >= 1 and all(c[3] > 64 and c[4] < c[3] for c in cuts)
    assert any(c[5] for c in cuts)                      # ... and somewhere the search went on with what was kept


@pytest.mark.parametrize("case", [c for c, v in PL.SYNTHETIC.items() if "anchors" in v[1]], ids=lambda c: PL.SYNTHETIC[c][0])
def test_row_has_a_search_with_a_full_anchor_list(case):
    most = sorted(PL.max_anchors(t) for t in row_traces(case))
    print("row %d: most anchors on a side of one search, the top five reads: %s" % (case, most[-5:]))
    assert most[-1] >= 64 and sum(m > 32 for m in most) >= 3, most[-5:]


# ---------------------------------------------------------------- the ladders
_ladders = {}


def ladder_trace(name):
    if name not in _ladders:
        lad, pkw, why = PL.ladder_case(name)
        ot = oracle_table(*packed_kmers(lad.transcripts, lad.k), lad.k, **pkw)
        _ladders[name] = (lad, why, ot.trace(lad.read, steps=True))
    return _ladders[name]


def first_beyond(ways, limit):
    n = 1
    for w in ways:
        n *= w
        if n > limit:
            break
    return n


@pytest.mark.parametrize("name", list(PL.LADDERS))
def test_builder_self_checks(name):
    lad = PL.ladder_case(name)[0]
    k = lad.k
    counts = PL.kmer_counts(lad.transcripts, k)
    assert set(counts.values()) == {1}                                   # allele counts are equal: every k-mer stored once
    spans = PL.sites_spanned(lad)
    assert set(spans.values()) == {0, 1}                                 # every stored k-mer spans at most one site
    assert sum(v == 1 for v in spans.values()) == k * sum(lad.ways)      # ... and every allele of every site has its k k-mers
    assert lad.transcripts[0] == lad.backbone and len(lad.read) == len(lad.backbone)
    lo, hi = lad.noisy
    if lad.form in ("bridge", "tail"):
        assert lad.read[:300] == lad.backbone[:300] and lo >= 300
    if lad.form in ("bridge", "head"):
        assert lad.read[-300:] == lad.backbone[-300:] and hi <= len(lad.read) - 300
    assert (lad.form == "tail") == (hi == len(lad.read)) and (lad.form == "head") == (lo == 0)
    assert all(lad.read[s] == lad.backbone[s] == al[0] for s, al in zip(lad.sites, lad.alleles))
    # no k-mer of the noisy stretch is solid: the ladder is walked by one search, from the k-mer beside the stretch
    assert not any(lad.read[i:i + k] in counts for i in range(max(lo - k + 1, 0), min(hi, len(lad.read) - k + 1)))
    diff = [i for i in range(len(lad.read)) if lad.read[i] != lad.backbone[i]]
    assert lo <= diff[0] and diff[-1] < hi and 0.10 * (hi - lo) < len(diff) < 0.25 * (hi - lo)


@pytest.mark.parametrize("name", list(PL.LADDERS))
def test_ladder_reaches_the_set_it_is_named_after(name):
    lad, why, trace = ladder_trace(name)
    sizes = PL.set_sizes(trace)
    top = PL.largest_sets(trace)
    print(name, "largest sets head / inner / tail", top, "searches", [(s["location"], s["direction"], [len(r) for r in s["sizes"]]) for s in PL.searches(trace)])
    loc = why["location"]
    assert all(v == 0 for l, v in top.items() if l != loc), top          # the search the form was made for walks it, no other
    if "visible" in why:
        # the set is multiplied at every site until it is above max_nb_inner_paths, which ends the search; a bridge is tried
        # from the left anchor and, failing that, from the right one, an edge search walks from its one anchor
        ways = list(PL.LADDERS[name][0]["ways"])
        orders = [ways, ways[::-1]] if lad.form == "bridge" else [ways]
        assert top[loc] == why["visible"] == max(first_beyond(o, 60) for o in orders) and top[loc] > PL.WAVE
    if "cut" in why:
        twin = ladder_trace(why["twin"])[2]
        cuts = PL.cuts_against_twin(trace, twin, maxb=PL.ladder_case(name)[1]["max_nb_competing_paths"])
        print(name, "parts from", why["twin"], "at", cuts)
        assert len(cuts) == 1 and cuts[0][0] == loc and cuts[0][3] == why["cut"] and cuts[0][4] <= 60 and cuts[0][5], cuts
    if "scored" in why:
        twin = ladder_trace(why["twin"])[2]
        assert top[loc] == why["scored"] and trace != twin


def test_ladders_cover_two_and_three_passes_and_a_used_three_pass_set():
    tops = {name: max(PL.largest_sets(ladder_trace(name)[2]).values()) for name in PL.LADDERS}
    whys = {name: PL.LADDERS[name][2] for name in PL.LADDERS}
    assert any(64 < t <= 128 for t in tops.values()) and any(t >= 129 for t in tops.values()), tops
    for loc in (PL.HEAD, PL.INNER, PL.TAIL):          # two passes and three in a head, an inner and a tail search
        assert any(64 < whys[n].get("visible", 0) <= 128 and whys[n]["location"] == loc for n in tops), loc
        assert any(whys[n].get("visible", 0) >= 129 and whys[n]["location"] == loc for n in tops), loc
    assert {PL.LADDERS[n][0]["k"] for n in tops} == {18, 21, 31}
    # the step after a three-pass set continues the same search: a ladder whose 192 candidates are cut on the step that
    # makes them (asserted per ladder above against its twin), with steps of the same run after it
    assert any(whys[n].get("cut", 0) >= 129 for n in tops)


# ---------------------------------------------------------------- more survivors than candidates
def test_bush_keeps_300_of_240_candidates():
    """Gardening's "complex" branch returns MAXB + n' indices, n' the candidates that tie for the best score: on the bush
    the oracle's set after the step that makes 240 candidates is 300 — more than the children of any step, and what a
    Trail set of the HIP path must hold (TCAP, talc_kernels_search.h; 288 slots until this case was made)."""
    B = PL.bush()
    assert len(B.leaves) == len(set(B.leaves)) == 240 and B.read.count("N") == 4
    trace = oracle_table(B.keys, B.counts, B.k, **PL.BUSH_PARAMS).trace(B.read, steps=True)
    first = PL.searches(trace)[0]
    sizes = first["sizes"][0]
    changes = [(st, n) for i, (st, n) in enumerate(zip(first["steps"][0], sizes)) if i == 0 or n != sizes[i - 1]]
    print("bush:", changes)
    assert (first["location"], first["direction"]) == (PL.INNER, 1)
    assert changes == [(1, 1), (41, 4), (46, 16), (51, 59), (56, 60), (61, 300)] and len(sizes) == 61
    assert max(sizes) == 64 + 240 - 4 and max(sizes) > 288
