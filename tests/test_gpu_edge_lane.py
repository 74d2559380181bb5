"""-m gpu: the edge lane (talc_kernels_search.h: edge_lane — an edge search's lone Trail walked and scored in one loop)
against the separate fast-forward / score_edges calls (TALC_TEST_EDGE_LANE=0) and against the oracle.

The reads are built for edge searches: an error-free stretch of a transcript whose two ends (the edges, 10 to 600
bases) carry an edit every few bases, closer together than K, so that no k-mer of an edge is solid and the only solid
region is the middle.  A Trail then runs the length of its edge, is scored every CHECK_INTERVAL steps with an x-drop that
grows with its edit distance, and on the long edges the band passes 63 diagonals: the lane hands the scoring over to the
phased instances mid-edge, which take or refuse the wavefront it kept.

Every case: records and statuses equal the oracle's with the lane on and with it off, and the two runs count the same
Trail steps and DP cells (tolerance 0: bytes and integers).  Equal outputs alone would also hold with a dead hook, so
test_profile_build_shows_where_the_lane_runs reads the profile build's category counters: the lane's own category is
entered with the hook on and never with it off or without walk records, with the same number of x-drop calls and
levels every time, and more levels per call on average than the lane's own instance can run (so scorings were handed
over to the phased instances)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import parity_util as PU
from stress_cases import CASES
from talc_amd import build as B
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

EDGE_LENS = (20, 45, 90, 150, 250, 400, 600, 10)   # (10: an edge shorter than any K used here)


def edge_reads(synth, n, k, seed, n_in_edge=False):
    """n reads whose head and tail edges (EDGE_LENS in turn) are mutated: an edit every 5 .. K-2 bases."""
    rng = np.random.default_rng(seed)
    bases, offs = synth.short_reads(0, n, length=1600, sub_rate=0.0)
    clean = PU.seqs_of(bases, offs)
    out = []
    for i, s in enumerate(clean):
        e = EDGE_LENS[i % len(EDGE_LENS)]
        if len(s) < 2 * e + 4 * k:
            e = max(0, (len(s) - 4 * k) // 2)

        def garble(seg):
            r, p = [], 0
            while True:
                p2 = p + int(rng.integers(5, max(6, k - 1)))
                if p2 >= len(seg):
                    r.append(seg[p:])
                    break
                r.append(seg[p:p2])
                op = rng.random()
                if op < 0.7:
                    r.append("ACGT"[("ACGT".index(seg[p2]) + int(rng.integers(1, 4))) % 4])   # substitution
                elif op < 0.85:
                    r.append(seg[p2] + "ACGT"[int(rng.integers(0, 4))])                          # insertion
                p = p2 + 1                                                                      # (else: deletion)
            return "".join(r)

        head, mid, tail = s[:e], s[e:len(s) - e], s[len(s) - e:]
        head, tail = garble(head[::-1])[::-1], garble(tail)   # (edits start next to the solid middle on both sides)
        if n_in_edge and e >= 40:
            head = head[:len(head) // 2] + "N" + head[len(head) // 2 + 1:]
            tail = tail[:len(tail) // 3] + "NN" + tail[len(tail) // 3 + 2:]
        out.append(head + mid + tail)
    nb = np.frombuffer("".join(out).encode(), dtype=np.uint8)
    no = np.zeros(len(out) + 1, dtype=np.uint64)
    no[1:] = np.cumsum([len(x) for x in out])
    return nb, no


def lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, what):
    o_out, o_off, o_st = pair.otab.correct_batch(bases, offs, nthreads=16)
    so = PU.seqs_of(o_out, o_off)
    counts = {}
    for lane in ("1", "0"):
        monkeypatch.setenv("TALC_TEST_EDGE_LANE", lane)
        ctx = T.Context(pair.ttab, pair.p, 0)   # (a context reads the switches when it is created)
        g_out, g_off, g_st = ctx.correct(bases, offs)
        t = ctx.timing().as_dict()
        ctx.close()
        sg = PU.seqs_of(g_out, g_off)
        bad = [i for i in range(len(so)) if so[i] != sg[i] or int(o_st[i]) != int(g_st[i])]
        print("%s lane=%s: reads %d, mismatches %d, trail steps %d, dp cells %d, retried %d"
              % (what, lane, len(so), len(bad), t["n_trail_steps"], t["n_dp_cells"], t["n_retried"]))
        assert not bad, (what, "TALC_TEST_EDGE_LANE=" + lane, bad[:5])
        counts[lane] = (int(t["n_trail_steps"]), int(t["n_dp_cells"]), int(t["n_retried"]))
    monkeypatch.delenv("TALC_TEST_EDGE_LANE")
    assert counts["1"] == counts["0"], (what, counts)
    assert counts["1"][0] > 0
    return counts["1"], so


def _pair(k=21, seed=11, target_kmers=200_000, **params_kw):
    pair = PU.Pair(target_kmers=target_kmers, k=k, seed=seed, **params_kw)
    pair.ttab.upload(0)
    return pair


@pytest.mark.parametrize("k", [18, 21, 31])
def test_edges_of_10_to_600_bases(k, monkeypatch):
    """Edges from shorter than K to 600 bases, K = 18, 21 and 31, default parameters."""
    pair = _pair(k=k, seed=500 + k)
    bases, offs = edge_reads(pair.synth, 320, k, seed=k)
    (steps, cells, _), so = lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, "K=%d" % k)
    # the searches really do walk the edges: more Trail steps than a third of the garbled bases
    assert steps > sum(2 * e for e in EDGE_LENS) * (320 // len(EDGE_LENS)) // 3


@pytest.mark.parametrize("ci", [1, 4, 6, 7, 13])
def test_check_intervals(ci, monkeypatch):
    """CHECK_INTERVAL 1, 4, 6, 7 and 13 (13: a round spans two walk records)."""
    pair = _pair(seed=520 + ci, check_interval=ci)
    bases, offs = edge_reads(pair.synth, 240, 21, seed=100 + ci)
    lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, "CHECK_INTERVAL=%d" % ci)


@pytest.mark.parametrize("params", [dict(allowed_failure_rate=0.1), dict(allowed_failure_rate=0.5),
                                    dict(max_nb_border_failures=0), dict(max_nb_border_failures=3),
                                    dict(max_border_length=100), dict(max_border_length=1000)],
                         ids=["AFR0.1", "AFR0.5", "MAXFAIL0", "MAXFAIL3", "MAXBORDER100", "MAXBORDER1000"])
def test_scoring_parameters(params, monkeypatch):
    """The parameters that decide when a Trail fails its scoring, and edges on both sides of MAX_BORDER_LENGTH."""
    pair = _pair(seed=540, **params)
    bases, offs = edge_reads(pair.synth, 240, 21, seed=7)
    lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, str(params))


def test_n_bases_inside_edges(monkeypatch):
    pair = _pair(seed=560)
    bases, offs = edge_reads(pair.synth, 240, 21, seed=8, n_in_edge=True)
    assert b"N" in bytes(bases)
    lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, "N in edges")


def test_paralog_graph_forks_and_dead_ends_inside_edges(monkeypatch):
    """The branching graph of stress set 103 (80 % paralogs, CHECK_INTERVAL 4): forks, dead ends and filter hits inside
    the edges, so the lane hands back at every kind of step it does not take; the generator's own reads and edge reads."""
    kw, pkw = CASES[103]
    pair = PU.Pair(**kw, **pkw)
    pair.ttab.upload(0)
    bases, offs = pair.reads(0, 600)
    lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, "set 103, generator reads")
    bases, offs = edge_reads(pair.synth, 240, kw["k"], seed=9)
    lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, "set 103, edge reads")


def test_retry_pass(monkeypatch):
    """TALC_TEST_TINY_CAPS=1: the first pass's scratch overflows and the reads go through the retry launch."""
    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "1")
    pair = _pair(seed=580)
    bases, offs = edge_reads(pair.synth, 160, 21, seed=10)
    (_, _, retried), _ = lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, "tiny caps")
    assert retried > 0


def test_without_walk_records(monkeypatch):
    """TALC_WALK=0: no walk records, the lane is never entered; the results are the same."""
    monkeypatch.setenv("TALC_WALK", "0")
    pair = _pair(seed=590)
    bases, offs = edge_reads(pair.synth, 160, 21, seed=11)
    lane_on_off_vs_oracle(pair, bases, offs, monkeypatch, "TALC_WALK=0")


def _profile_child():
    """(run in a child process whose library is the profile build: one batch of edge reads)"""
    pair = _pair(seed=600)
    bases, offs = edge_reads(pair.synth, 160, 21, seed=12)
    ctx = T.Context(pair.ttab, pair.p, 0)
    ctx.correct(bases, offs)
    ctx.close()


def _profile_counters(extra_env):
    """{category: value} the profile build prints (TALC_PROF_PRINT) for _profile_child under extra_env."""
    env = dict(os.environ, TALC_LIB=B.build_hip_prof(), TALC_PROF_PRINT="1", **extra_env)
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_edge_lane as M; M._profile_child()" % (
        os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    out = {}
    for m in re.finditer(r"^\[prof\] (.+?)\s+(\d+) cycles", r.stderr.decode(), re.M):
        out[m.group(1)] = out.get(m.group(1), 0) + int(m.group(2))   # (one block per launch: first pass, retry)
    assert "edgelane*" in out and "#xdrop calls" in out, sorted(out)
    return out


def test_profile_build_shows_where_the_lane_runs():
    """The lane's category (edgelane*) holds cycles with the hook on, none with TALC_TEST_EDGE_LANE=0 and none with
    TALC_WALK=0; x-drop calls and levels are the same three times, fast-forward steps the same with the hook on and off;
    with the lane on, fewer cycles go to the fast-forward's entry (ff.entry: the lane enters once per call, not per round);
    and the mean number of levels per x-drop is beyond what one diagonal per lane can run, so the phased instances did
    take over from the lane on the long edges."""
    on = _profile_counters({})
    off = _profile_counters({"TALC_TEST_EDGE_LANE": "0"})
    nowalk = _profile_counters({"TALC_WALK": "0"})
    print({k: (on[k], off[k], nowalk[k]) for k in ("edgelane*", "#xdrop calls", "#xdrop levels", "#ffsteps", "x.stage", "ff.entry")})
    assert on["edgelane*"] > 0 and off["edgelane*"] == 0 and nowalk["edgelane*"] == 0
    assert on["#xdrop calls"] == off["#xdrop calls"] == nowalk["#xdrop calls"] > 1000
    assert on["#xdrop levels"] == off["#xdrop levels"] == nowalk["#xdrop levels"]
    assert on["#ffsteps"] == off["#ffsteps"] > 0
    assert on["ff.entry"] < off["ff.entry"]
    # a run of one diagonal per lane (the only kind the lane scores itself) has at most 31 levels: a mean beyond that says
    # that scorings of these edges went to the phased instances, i.e. that the lane handed over mid-edge
    assert on["#xdrop levels"] > 40 * on["#xdrop calls"]
