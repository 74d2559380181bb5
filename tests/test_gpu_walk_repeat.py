"""-m gpu: cycles of period <= 11 that close INSIDE one walk record.

walk_record (talc_kernels_search.h) asks the search's filter about the twelve k-mers of a record before it enters any of
them, so a k-mer that repeats a lower level of the same record is seen only by the record's own hash chain — and that
chain runs only where walk_repeat_possible (talc_pure.h) says a repeat can exist.  The tandem repeats of
test_gpu_parity.py have units longer than K: there the filter decides.  Here the transcripts begin and end with a run of
a primitive unit of 1..11 bases, K + 30 bases or more: the run's k-mers form a closed cycle of single successors with no
exit at the transcript's end, a head search walks LEFT into it and a tail search RIGHT, and the first fully periodic
k-mer and its repeat p steps later fall into one record whenever the record's alignment allows ((12 - p) / 12 of the
time).  Reads: four per transcript, 8-14 % errors, ending 0-40 bases inside the runs.

Every K: records and statuses equal the oracle's, and TALC_TEST_EDGE_LANE=0 and TALC_WALK=0 give the same records and
the same Trail-step and DP-cell counts (tolerance 0: bytes and integers).  The profile build's counters say that the
chain did run on this set (`#ffdup chain` > 0) and that it ran on fewer than 1 % of the records of an ordinary set."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import parity_util as PU
from talc_amd import build as B
from talc_amd import lib as T

pytestmark = pytest.mark.gpu


def primitive_unit(rnd, p):
    """p random bases that are not a repetition of a shorter unit."""
    while True:
        u = "".join(rnd.choice("ACGT") for _ in range(p))
        if all(u != u[:d] * (p // d) for d in range(1, p) if p % d == 0):
            return u


def noisy(rnd, seq, rate):
    out = []
    for ch in seq:
        x = rnd.random()
        if x < rate * 0.4:
            out.append(rnd.choice("ACGT"))          # substitution
        elif x < rate * 0.7:
            continue                                # deletion
        elif x < rate:
            out.append(ch)
            out.append(rnd.choice("ACGT"))          # insertion
        else:
            out.append(ch)
    return "".join(out)


def cycle_set(k, seed=77, n_transcripts=44):
    """(transcripts, reads): run of unit A (p bases) + random core of 200-300 bases + run of unit B (p' bases), p and p'
    cycling through 1..11 (four times each at either end); runs of K + 30 .. K + 41 bases."""
    rnd = random.Random(seed + k)
    transcripts, reads = [], []
    for t in range(n_transcripts):
        pa, pb = 1 + t % 11, 1 + (t * 3 + 5) % 11
        la, lb = k + 30 + rnd.randint(0, 11), k + 30 + rnd.randint(0, 11)
        ua, ub = primitive_unit(rnd, pa), primitive_unit(rnd, pb)
        core = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(200, 300)))
        # (the run at the start ends on a whole unit next to the core, the run at the end starts on one)
        head = (ua * (la // pa + 2))[-la:]
        tail = (ub * (lb // pb + 2))[:lb]
        tr = head + core + tail
        transcripts.append(tr)
        for _ in range(4):
            a = la - rnd.randint(0, 40)
            b = len(tr) - lb + rnd.randint(0, 40)
            reads.append(noisy(rnd, tr[a:b], rnd.choice([0.08, 0.11, 0.14])))
    return transcripts, reads


def run_product(pair, bases, offs):
    ctx = T.Context(pair.ttab, pair.p, 0)   # (a context reads the switches when it is created)
    g_out, g_off, g_st = ctx.correct(bases, offs)
    t = ctx.timing().as_dict()
    ctx.close()
    return PU.seqs_of(g_out, g_off), [int(x) for x in g_st], (int(t["n_trail_steps"]), int(t["n_dp_cells"]))


@pytest.mark.parametrize("k", [18, 21, 31])
def test_cycles_that_close_inside_a_record(k, monkeypatch):
    transcripts, reads = cycle_set(k)
    bases, offs = PU.pack_reads(reads)
    pair = PU.CustomPair(transcripts, k=k, depth=20)
    o_out, o_off, o_st = pair.otab.correct_batch(bases, offs, nthreads=16)
    want, want_st = PU.seqs_of(o_out, o_off), [int(x) for x in o_st]
    print("K=%d: reads %d, oracle statuses %s" % (k, len(reads), np.bincount(o_st, minlength=5).tolist()))
    assert sum(s == 0 for s in want_st) > len(reads) // 2          # the oracle alone corrects more than half of them
    counts = {}
    for what, env in (("default", {}), ("TALC_TEST_EDGE_LANE=0", {"TALC_TEST_EDGE_LANE": "0"}), ("TALC_WALK=0", {"TALC_WALK": "0"})):
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        if what != "default":                                       # (an upload reads TALC_WALK: a table of its own)
            pair = PU.CustomPair(transcripts, k=k, depth=20)
        pair.ttab.upload(0)
        got, got_st, counts[what] = run_product(pair, bases, offs)
        for name in env:
            monkeypatch.delenv(name)
        bad = [i for i in range(len(want)) if want[i] != got[i] or want_st[i] != got_st[i]]
        print("K=%d %s: mismatches %d, trail steps %d, dp cells %d" % ((k, what, len(bad)) + counts[what]))
        assert not bad, (k, what, bad[:8])
    assert counts["default"] == counts["TALC_TEST_EDGE_LANE=0"] == counts["TALC_WALK=0"], counts
    assert counts["default"][0] > 0


# ---------------------------------------------------------------- the profile build's counters (child processes)
def _profile_child(which):
    """(run in a child process whose library is the profile build)"""
    if which == "cycles":
        transcripts, reads = cycle_set(21)
        pair = PU.CustomPair(transcripts, k=21, depth=20)
        bases, offs = PU.pack_reads(reads)
    else:
        pair = PU.Pair(target_kmers=200_000, k=21, seed=11)
        bases, offs = pair.reads(0, 2000)
    pair.ttab.upload(0)
    ctx = T.Context(pair.ttab, pair.p, 0)
    ctx.correct(bases, offs)
    ctx.close()


def _profile_counters(which):
    env = dict(os.environ, TALC_LIB=B.build_hip_prof(), TALC_PROF_PRINT="1")
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_walk_repeat as M; M._profile_child(%r)" % (
        os.path.dirname(here), here, which)
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    out = {}
    for m in re.finditer(r"^\[prof\] (.+?)\s+(\d+) cycles", r.stderr.decode(), re.M):
        out[m.group(1)] = out.get(m.group(1), 0) + int(m.group(2))   # (one block per launch: first pass, retry)
    assert "#ffrecords" in out and "#ffdup chain" in out, sorted(out)
    return out


def test_profile_build_shows_where_the_chain_runs():
    cyc = _profile_counters("cycles")
    plain = _profile_counters("plain")
    print({k: (cyc[k], plain[k]) for k in ("#ffrecords", "#ffdup chain", "#ffsteps")})
    assert cyc["#ffdup chain"] > 0
    assert plain["#ffrecords"] > 10_000
    assert plain["#ffdup chain"] * 100 < plain["#ffrecords"]
