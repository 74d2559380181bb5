"""From the oracle alone: every case of tests/long_gap_cases.py gets where its name says.  The HIP path is compared with
the oracle on these cases in tests/test_gpu_long_gaps.py; here the oracle's structure and step trace say that the
comparison is one across a switch point of k_search: the reference length on either side of 8191 with two
Trails really scored and a cut of four Trails to two that the scores decide, a Trail beyond 8191 bases under a shorter
reference, every score_bridges_rows instance, 192 candidates scored with 175 row records, a cycle met under every size
of the cycle filter, three searches of one wave, more Trails than a
first-pass arena has buffers, reads beyond 65 535 bases.  The formulas of the case file (refLen, pathMax) are checked
against the oracle's regions and against the steps a search walks.

The cap — the oracle corrects every case in at most 10 s of one thread — is a condition on the inputs, so that the GPU
file stays affordable; it says nothing about the code under test.  One scoring at 8 kb costs the oracle 0.25 s per Trail
(it aligns from scratch, 60 M cells), which is what sets the check intervals of the cases; each test prints its figure."""
import numpy as np
import pytest

import long_gap_cases as LG

RIGHT, INNER = 1, 1
CAP_SECONDS = 10.0


def right_runs(side):
    """The first start anchor's run of every inner search towards RIGHT: one per gap, in read order."""
    return [s["runs"][0] for s in side.runs if s["location"] == INNER and s["direction"] == RIGHT]


@pytest.mark.parametrize("name", list(LG.CASES))
def test_case_is_what_its_facts_say(name):
    side = LG.oracle_side(name)
    g, k, why = side.g, side.g.k, side.why
    reg, thr, ok = side.otab.structure(g.read)
    print(name, "oracle %.2f s, scoreBridges calls %d" % (side.seconds, side.score_calls),
          [(G.read_gap, G.true_len, G.ref_len, G.path_max) for G in g.gaps], [LG.size_changes(r)[:8] for r in right_runs(side)])
    assert side.seconds <= CAP_SECONDS, (name, side.seconds)
    assert side.status == 0 and ok
    # the structure is the flanks and nothing else, and the case file's formulas give what the search will compute from it
    assert [tuple(x) for x in reg.tolist()] == g.regions and len(g.regions) == len(g.gaps) + 1
    assert len(g.gaps) == 1 or name == "two-long-gaps"
    rr = right_runs(side)
    assert len(rr) == len(g.gaps)
    ci, maxb = side.params.get("check_interval", 6), side.params.get("max_nb_competing_paths", 7)
    for G, (ls, le), (rs, re), run in zip(g.gaps, g.regions, g.regions[1:], rr):
        which_start = le
        assert rs - (which_start + k) == G.read_gap and re + k - which_start == G.ref_len
        assert G.path_max == int(1.2 * (rs - (which_start + k)) + 3 * k)
        assert run["steps"] == list(range(1, len(run["steps"]) + 1)) and run["steps"][-1] <= G.path_max
        if run["sizes"][-1] > 0 and run["sizes"][-1] <= side.params.get("max_nb_inner_paths", 50):
            assert run["steps"][-1] == G.path_max                       # Trails left when the search ends: it walked pathMax steps
        # every site doubles the Trails on the step that adds its base
        want, n = [(1, 1)], 1
        for s in G.sites:
            n *= 2
            want.append((s + 1, n))
        got = [c for c in LG.size_changes(run) if c[1] > 0]
        assert got[:len(want)] == want, (name, got[:8], want)
        if why.get("two_trails"):
            # ... both live on, tied at every check, and have been scored when the decisive site doubles them; the next
            # check keeps the two that have the read's allele there: the one change of the set that a score decides
            # (on a later check than the next where the site is not yet inside what the truncated reference aligns: the
            # Trail of an insertion comb is shorter than the read it follows, and a site 2-3 steps old lies in the window)
            (d,) = G.decisive
            assert any(G.sites[0] + 1 < s <= d for s in LG.check_steps(run, ci, maxb)), (name, d)
            assert got[:-1] == want + [(d + 1, 4)] and got[-1][1] == 2, (name, got, want, d)
            cut = got[-1][0]
            assert cut > d + 1 and cut % ci == 0, (name, got)
    # what was scored: the check steps with more Trails than max_nb_competing_paths, over every run of every search
    checks = [LG.check_steps(r, ci, maxb) for s in side.runs for r in s["runs"]]
    if why.get("cut"):
        assert side.score_calls >= 1                                    # (the set after the cut is what the trace shows)
    else:
        assert side.score_calls == sum(len(c) for c in checks), (name, side.score_calls, checks)
    if why.get("two_trails"):
        for G, run in zip(g.gaps, rr):
            scored = LG.check_steps(run, ci, maxb)
            # a first scoring and ones that go on from kept rows (beyond ROW_MAX_REF there are none to go on from: two scorings)
            assert len(scored) >= (2 if why.get("trail_below") else 4), (name, scored)
            assert LG.last_step_with(run, 2) >= scored[-1]
            assert sum(s > G.decisive[0] + 1 for s in scored) >= 1
    # no search needs more Trail buffers than the first pass has, but the one that is there for it
    most = max(max(r["sizes"]) for s in side.runs for r in s["runs"])
    buffers = min(LG.first_pass_buffers(G.path_max, k, len(g.read)) for G in g.gaps)
    assert (most > buffers) == bool(why.get("retry")), (name, most, buffers)


@pytest.mark.parametrize("name", ["ref-8190", "ref-8191", "ref-8192"])
def test_reference_length_on_either_side_of_row_max_ref(name):
    side = LG.oracle_side(name)
    ref = side.why["ref"]
    assert side.g.ref_len == ref == int(name[4:]) and side.g.comb == "sub"
    assert LG.row_records(ref) == side.why["records"] and (LG.row_records(ref) > 0) == (ref <= LG.ROW_MAX_REF)
    assert LG.row_records(8191) == 55 and LG.row_records(8192) == 0
    run = right_runs(side)[0]
    # two Trails from ~300 bases before the gap's end, scored while every Trail is still below 8192 bases
    assert side.g.read_gap - side.g.sites[0] in range(300, 316)
    scored = LG.check_steps(run, side.params["check_interval"], 1)
    assert len(scored) == (7 if ref <= LG.ROW_MAX_REF else 4) and max(scored) + side.g.k + 1 < LG.ROW_COV_LIMIT


def test_trail_passes_8191_under_a_shorter_reference():
    side = LG.oracle_side("trail-past-8191")
    g, k = side.g, side.g.k
    assert g.comb == "del" and g.ref_len <= LG.ROW_MAX_REF and LG.row_records(g.ref_len) > 0 and g.true_len + 2 * k >= LG.ROW_COV_LIMIT
    run = right_runs(side)[0]
    scored = LG.check_steps(run, side.params["check_interval"], 1)
    # score_bridges is handed len + 1 = K + step rows: with kept rows below 8192, from scratch from there on — and two
    # scorings beyond it, so that a count that wrapped in 13 bits on the first would be read by the second
    below = [s for s in scored if k + s < LG.ROW_COV_LIMIT]
    beyond = [s for s in scored if k + s >= LG.ROW_COV_LIMIT]
    print("trail-past-8191: scored with two Trails at steps", scored, "last step with two", LG.last_step_with(run, 2))
    assert len(below) >= 2 and len(beyond) >= 2, scored
    assert LG.last_step_with(run, 2) + k >= LG.ROW_COV_LIMIT


def test_reference_beyond_8191_with_every_trail_below():
    side = LG.oracle_side("ref-past-8191-trail-below")
    g, k = side.g, side.g.k
    assert g.comb == "ins" and g.ref_len > LG.ROW_MAX_REF and LG.row_records(g.ref_len) == 0
    assert max(max(r["steps"]) for s in side.runs for r in s["runs"]) + k + 1 < LG.ROW_COV_LIMIT
    assert right_runs(side)[0]["full"][-1] >= 2                       # the Trails reached the aim


def test_every_instance_and_both_sides_of_its_boundaries():
    refs = {n: LG.CASES[n][2]["ref"] for n in LG.CASES if n.startswith("instance-") or n.startswith("ref-81")}
    for n, ref in refs.items():
        assert LG.oracle_side(n).g.ref_len == ref
        if n.startswith("instance-"):
            assert LG.CASES[n][2]["instance"] == LG.instance_of(ref) == int(n.split("-")[1])
    have = {LG.instance_of(r) for r in refs.values() if r <= LG.ROW_MAX_REF}
    assert have == set(LG.INSTANCES)
    assert LG.instance_of(128) == 2 and LG.instance_of(129) == 4 and LG.instance_of(8191) == 128 and LG.instance_of(8192) == 0
    values = set(refs.values())
    for n in (2, 4, 6, 96):                                            # the first three boundaries and the last
        assert {64 * n, 64 * n + 1} <= values
    assert {8191, 8192} <= values
    for n in LG.INSTANCES[:-1]:                                        # the widest reference of every instance
        assert 64 * n in values


def test_row_arena_has_fewer_records_than_trails():
    side = LG.oracle_side("row-arena")
    assert side.g.ref_len == 8000 and LG.row_records(8000) == 57
    run = right_runs(side)[0]
    assert max(run["sizes"]) == 64 and run["steps"][-1] == side.g.sites[-1] + 1
    assert side.g.read_gap - side.g.sites[0] <= 185                    # (six sites at least K apart on the comb's teeth: 5 x 30 bases)
    # Under the 64 / 60 limits nothing is scored here: a set is scored only above max_nb_competing_paths Trails, and the
    # search ends above 60.  This case is the copies with a destination at or above rowAvail; the scoring with both kinds
    # of buffer is row-arena-scored, below.
    assert side.score_calls == 0


def test_row_arena_scores_more_candidates_than_it_has_records():
    """One scoring of 192 candidates with 175 records: the trace of the twin (no check on that step) shows the 192 after
    the step on which this case's set is cut to the few the scores leave, and the search goes on with them."""
    import param_limit_cases as PL
    side, twin = LG.oracle_side("row-arena-scored"), LG.oracle_side("row-arena-scored-twin")
    records = LG.row_records(side.g.ref_len)
    assert side.g.ref_len == 2617 and records == side.why["records"] == 175 and side.g.read == twin.g.read
    cuts = PL.cuts_against_twin(side.trace, twin.trace, maxb=64)
    print("row-arena-scored parts from its twin at", cuts, "scoreBridges calls", side.score_calls, "oracle %.2f s" % side.seconds)
    assert len(cuts) == 1 and side.score_calls == 1 and twin.score_calls == 0
    loc, direction, step, before, after, goes_on = cuts[0]
    assert (loc, direction) == (INNER, RIGHT) and before == side.why["candidates"] == 192 and before > records
    assert before - records >= 17 and 1 <= after < 48 and goes_on
    assert step == side.g.ladder_sites[3] + 1 and step % side.params["check_interval"] == 0
    inner = [s for s in side.runs if s["location"] == INNER]
    assert inner[0]["found"] == 1


@pytest.mark.parametrize("name", [n for n in LG.CASES if n.startswith("bloom-")])
def test_cycle_filter_size_and_the_repeat_met(name):
    side = LG.oracle_side(name)
    g, k, why = side.g, side.g.k, side.why
    assert LG.wide_bloom_words(g.path_max) == why["words"]
    run = right_runs(side)[0]
    if why["repeat"]:
        (a, b), = g.repeats
        assert g.truth[g.true_start + a:g.true_start + a + k + 20] == g.truth[g.true_start + b:g.true_start + b + k + 20]
        ch = LG.size_changes(run)
        # the Trail forks where the first copy ends, and the one that walks on meets its own k-mers in the second copy
        assert any(n == 2 and abs(s - (a + k + 20 + 1)) <= 1 for s, n in ch), ch
        drop = [s for (s, n), (_, before) in zip(ch[1:], ch) if n < before and abs(s - (b + k)) <= 1]
        assert drop, (name, ch, b + k)
    else:
        assert max(run["sizes"]) == 1 and run["full"][-1] == 1


def test_cycle_filter_cases_sit_on_both_sides_of_every_size():
    pm = {n: LG.oracle_side(n).g.path_max for n in LG.CASES if n.startswith("bloom-")}
    assert (pm["bloom-600"], pm["bloom-601"]) == (600, 601)
    assert LG.wide_bloom_words(600) == 0 and LG.wide_bloom_words(601) == 1024
    for w in (1024, 2048, 4096, 8192, 16384):
        lo, hi = pm["bloom-sizes-%d-below" % w], pm["bloom-sizes-%d-above" % w]
        assert lo // 2 == w and hi // 2 == w + 1 and lo == 2 * w + 1 and hi == 2 * w + 2
        assert LG.wide_bloom_words(lo) == w and LG.wide_bloom_words(hi) == min(2 * w, LG.WIDE_BLOOM_WORDS)
    repeats = [n for n in pm if LG.CASES[n][2]["repeat"]]
    assert len(repeats) >= len(pm) // 2
    far = [n for n in repeats if LG.oracle_side(n).g.repeats[0][1] - LG.oracle_side(n).g.repeats[0][0] > 500]
    assert len(far) >= 3 and len(repeats) - len(far) >= 3


def test_two_long_gaps_have_the_same_reference_length():
    side = LG.oracle_side("two-long-gaps")
    refs = tuple(G.ref_len for G in side.g.gaps)
    assert refs == side.why["refs"] and refs[0] == refs[1] != refs[2] and max(refs) <= LG.ROW_MAX_REF
    inner = [s for s in side.runs if s["location"] == INNER]
    assert [s["direction"] for s in inner] == [RIGHT] * 3 and all(s["found"] == 1 for s in inner)


def test_retry_case_outgrows_the_first_pass_arena():
    side = LG.oracle_side("retry-for-real")
    g = side.g
    buffers = LG.first_pass_buffers(g.path_max, g.k, len(g.read))
    assert buffers == 62 and max(right_runs(side)[0]["sizes"]) == 64
    assert LG.first_pass_buffers(LG.path_max(12000, g.k), g.k, 12800) == 72        # (a 12 kb gap would be held)


# ---------------------------------------------------------------- reads beyond 65 535 bases
@pytest.mark.parametrize("k", [21, 18, 31])
def test_long_reads(k):
    L = LG.long_reads(k)
    assert len(L.reads["65535+K"]) == 65535 + k and len(L.reads["65537+K"]) == 65537 + k
    assert 139_990 <= len(L.reads["140k"]) <= 140_000 and abs(len(L.reads["140k-comb"]) - 140_000) < 200
    otab = LG.oracle_table(L.transcripts, k)
    for name, read in L.reads.items():
        text, status, out, seconds, _ = LG.traced(otab, read)
        reg, thr, ok = otab.structure(read)
        print("K = %d %s: %d bases, %d regions, oracle %.2f s, record %d bases" % (k, name, len(read), len(reg), seconds, len(out)))
        assert status == 0 and ok and seconds <= CAP_SECONDS
        assert len(reg) >= (100 if k == 31 else 500) and len(reg) <= len(read) // 2 + 4        # (regCap = L / 2 + 4)
        assert len(read) // 2 + 4 > 30_000
        if name == "140k-comb":
            G = L.comb
            ends = [int(e) + k for s, e in reg.tolist()]
            starts = [int(s) for s, e in reg.tolist()]
            assert G.start in ends and G.start + G.read_gap in starts       # the comb is one gap between two regions
            i = ends.index(G.start)
            assert starts[i + 1] == G.start + G.read_gap and G.path_max == LG.path_max(8300, k)
            assert LG.first_pass_buffers(G.path_max, k, len(read)) >= 100
    # 8 buffers of the longest stride: the first pass's arena of a batch with a 140 kb read
    seq_cap = (int(1.2 * 140_000) + 4 * k + 64 + 15) & ~15
    assert 8 * seq_cap > 1 << 20 and LG.first_pass_buffers(int(1.2 * 140_000) + 3 * k, k, 140_000) == 8
