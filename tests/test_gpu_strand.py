"""Auto strand on the device (docs/auto_strand.md; k_strand_vote, talc_ctx_set_auto_strand) against the contract in numpy
(tests/strand_ref.py, from the host image of the table: never from a device result), and an auto-strand context against the
two fixed contexts, plain and -rev, read by read.  Integers and bytes, tolerance 0."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
import solidity_ref as S
import strand_ref as R
import test_gpu_solidity as G
from memcheck_util import everything   # (every output of a corrected batch, per read; shared with test_gpu_poison.py)
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
TILE = 256        # VOTE_TILE (talc_kernels_strand.h): positions per pass of a wave
ERR_INVALID, ERR_STATE = -1, -6


def same_rows(got, want, what=""):
    assert got.dtype == R.DTYPE and len(got) == len(want)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def rnd(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n).tolist())


def solid_runs(c, minc):
    """[(first, last)] of the maximal runs of c >= minc."""
    return [tuple(x) for x in PU.runs(np.asarray(c) >= minc).tolist()]


# ---------------------------------------------------------------- 1. hand-made tables
def hand_made(k, minc=2):
    """X and Y: two unrelated sequences of 3 000 bases; the table holds the k-mers of both, those that start in the first
    1 000 positions with count MIN, in the next 1 000 with MIN + 1, the rest with 50 (and, K = 18, one palindromic 18-mer).
    The reads: noise with stretches of X (solid forward) and of revcomp(Y) (solid in the reverse complement) at chosen
    k-mer positions; the noise base next to a stretch never continues it.  Returns (keys, counts, reads, plans, at):
    plans[i] = ([(first, last)] forward runs, [...] rc runs), in the read's coordinates, or None where the read has no plan."""
    rng = np.random.default_rng(2000 + k)
    X, Y = rnd(rng, 3000), rnd(rng, 3000)
    table = {}
    for seq in (X, Y):
        for i in range(len(seq) - k + 1):
            table.setdefault(S.pack(seq[i:i + k]), minc if i < 1000 else minc + 1 if i < 2000 else 50)
    half = rnd(rng, 9)
    pal = half + S.revcomp(half)
    if k == 18:
        table[S.pack(pal)] = 30
    n = 3 * TILE - 70                                   # k-mer positions of a read: three passes, the last word partial
    cursor = {"f": 2100, "r": 2100}                     # planted stretches without a place of their own: from the count-50 part
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}

    def splice(parts):
        """parts: ("f" | "r", npos, at or None) a stretch of npos k-mer positions of X from `at`, or the reverse complement
        of one of Y; ("n", bases) noise.  The noise bases beside a stretch differ from the base that would continue it."""
        out, ban_next = [], None
        for i, part in enumerate(parts):
            if part[0] == "n":
                m = part[1]
                if m == 0:
                    continue
                t = list(rnd(rng, m))
                ban_last = None
                if i + 1 < len(parts) and parts[i + 1][0] != "n":
                    ban_last = before(parts[i + 1])
                if ban_next and (m > 1 or not ban_last):
                    t[0] = next(ch for ch in "ACGT" if ch != ban_next)
                if ban_last:
                    t[-1] = next(ch for ch in "ACGT" if ch != ban_last and (m > 1 or ch != ban_next))
                out.append("".join(t))
                ban_next = None
            else:
                o, npos, at = part
                if at is None:
                    if cursor[o] + npos + k > 2990:
                        cursor[o] = 2100
                    at = cursor[o]
                    cursor[o] = at + npos + k
                    parts[i] = (o, npos, at)
                m = npos + k - 1
                assert 1 <= at and at + m < 3000
                out.append(X[at:at + m] if o == "f" else S.revcomp(Y[at:at + m]))
                ban_next = X[at + m] if o == "f" else comp[Y[at - 1]]
        return "".join(out)

    def before(part):
        """The base that, in front of the stretch, would continue it (its place is settled on first use)."""
        o, npos, at = part
        if at is None:
            at = 2100 if cursor[o] + npos + k > 2990 else cursor[o]
        return X[at - 1] if o == "f" else comp[Y[at + npos + k - 1]]

    reads, plans = [], []

    def add(plants):
        """plants: [(first, last, "f" | "r")] k-mer positions of a read of n positions, disjoint in bases, in order."""
        parts, pos = [], 0
        for first, last, o in plants:
            assert first >= pos
            parts += [("n", first - pos), (o, last - first + 1, None)]
            pos = last + k
        parts.append(("n", n + k - 1 - pos))
        r = splice(parts)
        assert len(r) == n + k - 1
        reads.append(r)
        plans.append((sorted((a, b) for a, b, o in plants if o == "f"), sorted((a, b) for a, b, o in plants if o == "r")))

    add([])
    for bnd in (64, TILE, TILE + 1):
        for o in "fr":
            add([(bnd - 40, bnd - 1, o)])                # a run ends at bnd - 1
            add([(bnd, bnd + 39, o)])                    # ... starts at bnd
            add([(bnd - 20, bnd + 19, o)])               # ... straddles bnd - 1 / bnd
            add([(bnd - 1, bnd - 1, o)])                 # ... is position bnd - 1 alone
        add([(0, 5, "f"), (bnd - 20, bnd + 19, "r"), (n - 31, n - 1, "f")])
        add([(0, 5, "r"), (bnd - 20, bnd + 19, "f"), (n - 31, n - 1, "r")])
    for o in "fr":
        add([(0, 9, o)])                                 # the read's two ends
        add([(n - 10, n - 1, o)])
        add([(0, 0, o), (n - 1, n - 1, o)])
        add([(0, n - 1, o)])
    # an N inside a window, lower case, other letters: made from a planted read; the reference says what they are
    base = len(reads)
    add([(30, 120, "f"), (300, 420, "r")])
    r = reads[-1]
    reads += [r[:60] + "N" + r[61:], r[:350] + "n" + r[351:], r.lower(), r[:100].lower() + r[100:], r[:70] + "R" + r[71:330] + "-" + r[331:]]
    plans += [None] * 5
    if k == 18:
        add([(100, 130, "f")])
        r = reads[-1]
        reads.append(r[:400] + pal + r[400 + k:])
        plans.append(None)
    # L = 0, K - 1, K, K + 1
    reads += ["", X[2500:2500 + k - 1], X[2500:2500 + k], X[2500:2500 + k + 1], S.revcomp(Y[2500:2500 + k]), S.revcomp(Y[2500:2500 + k + 1])]
    plans += [None] * 6
    # counts equal to MIN_COUNT in one orientation and above it in the other; the three tie cases (lo: the count-MIN part)
    lo, hi = 100, 2200
    ties = [[("f", 50, lo), ("n", 40), ("r", 50, hi)],            # fwd solid 50 in 0, rc solid 50 in 50: reverse
            [("f", 50, hi), ("n", 40), ("r", 50, lo)],            # the other way round: forward
            [("f", 30, lo), ("n", 40), ("r", 60, lo)],            # rc_in == fwd_in (0) with rc_solid larger: reverse
            [("f", 40, hi), ("n", 40), ("r", 40, hi)],            # all equal: forward
            [("n", 300)],                                         # all equal (0): forward
            [("f", 200, lo), ("n", 40), ("r", 20, hi)]]           # rc_in > fwd_in with rc_solid < fwd_solid: reverse
    reads += [splice(t) for t in ties]
    plans += [None] * len(ties)
    # one 20 kb read: stretches of both strands and noise
    parts = []
    while sum(p[1] for p in parts) < 20000:
        parts += [("f", int(rng.integers(1, 300)), None), ("n", int(rng.integers(1, 60))), ("r", int(rng.integers(1, 300)), None), ("n", int(rng.integers(1, 60)))]
    reads.append(splice(parts)[:20000])
    plans.append(None)
    keys = np.fromiter(table.keys(), dtype=np.uint64, count=len(table))
    counts = np.fromiter(table.values(), dtype=np.uint32, count=len(table))
    return keys, counts, reads, plans, dict(base=base, ties=len(reads) - 1 - len(ties), pal=pal)


@pytest.mark.parametrize("k", [18, 21, 31])
def test_reads_on_a_hand_made_table(k):
    keys, counts, reads, plans, at = hand_made(k)
    c = G.Ctx(keys, counts, k=k)
    minc = c.minc
    want = R.rows(reads, k, minc, c.lookup)
    # the reads are what they were built to be, by the table alone
    for i, (r, plan) in enumerate(zip(reads, plans)):
        if plan is None:
            continue
        f, rc = R.both_counts(r, k, c.lookup)
        assert solid_runs(f, minc) == plan[0] and solid_runs(rc, minc) == plan[1], (k, i, solid_runs(f, minc), solid_runs(rc, minc), plan)
    b0 = at["base"]
    assert want[b0].tolist() == (3 * TILE - 70, 91, 91, 121, 121, 1)
    assert want[b0 + 1]["fwd_solid"] == 91 - min(k, 31) and want[b0 + 2]["rc_solid"] == 121 - k           # the N takes K positions away
    assert want[b0 + 3].tolist() == want[b0].tolist() == want[b0 + 4].tolist()                               # lower case counts
    assert want[b0 + 5]["fwd_solid"] == 91 - k and want[b0 + 5]["rc_solid"] == 121 - k                       # other letters are N
    t0 = at["ties"]
    assert want["n_kmers"][t0 - 6:t0].tolist() == [0, 0, 1, 2, 1, 2] and want["reverse"][t0 - 6:t0].tolist() == [0, 0, 0, 0, 1, 1]
    tie = want[t0:t0 + 6]
    assert tie["reverse"].tolist() == [1, 0, 1, 0, 0, 1], tie.tolist()
    assert tie[0].tolist()[1:5] == (50, 0, 50, 50) and tie[1].tolist()[1:5] == (50, 50, 50, 0)               # MIN_COUNT in one orientation
    assert tie[2]["rc_in"] == tie[2]["fwd_in"] == 0 and tie[2]["rc_solid"] > tie[2]["fwd_solid"] > 0
    assert tie[3].tolist()[1:5] == (40, 40, 40, 40) and tie[4].tolist()[1:5] == (0, 0, 0, 0)
    assert tie[5]["rc_in"] > tie[5]["fwd_in"] and 0 < tie[5]["rc_solid"] < tie[5]["fwd_solid"]
    assert want[-1]["n_kmers"] == 20000 - k + 1 and want[-1]["fwd_solid"] > 3000 and want[-1]["rc_solid"] > 3000
    if k == 18:
        f, rc = R.both_counts(reads[b0 + 7], k, c.lookup)
        assert S.revcomp(at["pal"]) == at["pal"] and f[400] == 30 and rc[400] == 30                          # the palindrome counts in both
    b = c.ctx.batch(*G.pack_reads(reads))
    try:
        got = b.strand()
        same_rows(got, want, "hand-made k=%d" % k)
        assert c.ctx.strand_timing() > 0
        same_rows(b.strand(), want, "a second call finds the rows there")
    finally:
        b.close()
        c.ctx.close()


def test_rc_probes_follow_a_chain_across_the_end_of_the_table():
    """The reverse complements of the zone reads of test_gpu_table_edges (K = 21): the k-mers that live around the end of the
    table are reached through the reverse complement the kernel derives, not through the window."""
    import test_gpu_table_edges as TE
    k, x10 = 21, 20
    synth = Synth(target_kmers=60_000, k=k, seed=700 + k)
    E = PU.end_loaded_table(synth, k, x10, TE.W, TE.F, np.random.default_rng(100 * k + x10))
    TE._upload_with_images(E, "host")
    try:
        reads, _ = TE._zone_reads(E, np.random.default_rng(4))
        rc_reads = [PU.revcomp(r) for r in reads]
        lookup = S.host_lookup(E.ttab)
        minc = E.p.min_count
        want = R.rows(rc_reads, k, minc, lookup)
        # reach, from the image and the homes alone: stored k-mers of the reads' reverse complements whose RIGHT bucket lies
        # below its home (after the wrap)
        slots, keys, home = PU.image_homes(E.after.right, "RIGHT")
        wrapped = set(keys[home > slots].tolist())
        assert len(wrapped) >= 20
        n_wrapped = 0
        for r in rc_reads:
            km, bad = S.kmers_of(S.dna5(r), k)
            rk = R.revcomp_packed(km[~bad], k)
            hit = lookup(rk) >= minc if len(rk) else np.zeros(0, bool)
            n_wrapped += sum(1 for x in (rk[hit] >> np.uint64(2)).tolist() if x in wrapped)
        assert n_wrapped >= 20, n_wrapped
        assert int(want["rc_solid"].sum()) > 10 * int(want["fwd_solid"].sum()) and int((want["reverse"] == 1).sum()) > len(E.fill)
        b = E.ctx.batch(*PU.pack_reads(rc_reads))
        got = b.strand()
        b.close()
        same_rows(got, want, "zone reads, reverse complemented")
        b = E.ctx.batch(*PU.pack_reads(reads))            # ... and as they are: the forward probes
        got = b.strand()
        b.close()
        same_rows(got, R.rows(reads, k, minc, lookup), "zone reads")
    finally:
        E.after.free()
        E.ctx.close()
        E.ttab.close()


# ---------------------------------------------------------------- 2. equivalence with the two fixed contexts
_three = {}


def three_contexts(name):
    """The set's reads with every second one reverse complemented, through a plain, a -rev and an auto-strand context
    over one table (computed once, shared, left unchanged)."""
    if name not in _three:
        c = G.gen_set(name)
        target, k, seed, synth_kw, params_kw = G.SETS[name]
        reads = [S.revcomp(r) if i % 2 else r for i, r in enumerate(c.reads)]
        p_rev = T.default_params(k=k, reverse=1, **params_kw)
        rev, auto = T.Context(c.ttab, p_rev, 0), T.Context(c.ttab, c.p, 0)
        auto.auto_strand()
        try:
            r = dict(c=c, reads=reads, want=R.rows(reads, k, c.minc, c.lookup))
            r["plain"], r["work_plain"], _ = everything(c.ctx, reads)
            r["rev"], _, _ = everything(rev, reads)
            r["auto"], _, r["rows"] = everything(auto, reads)
        finally:
            rev.close()
            auto.close()
        _three[name] = r
    return _three[name]


@pytest.mark.parametrize("name", ["default", "k31", "branching", "min-count-3"])
def test_every_read_equals_the_chosen_fixed_context(name):
    r = three_contexts(name)
    c, want, n = r["c"], r["want"], len(r["reads"])
    nrev = int(want["reverse"].sum())
    assert nrev >= n // 4 and n - nrev >= n // 4, (nrev, n)            # the reference alone puts a quarter on each side
    same_rows(r["rows"], want, name)
    n_corr = [0, 0]
    for i in range(n):
        chosen = r["rev"][i] if want["reverse"][i] else r["plain"][i]
        assert r["auto"][i] == chosen, (name, i, int(want["reverse"][i]), [j for j, (x, y) in enumerate(zip(r["auto"][i], chosen)) if x != y])
        n_corr[int(want["reverse"][i])] += r["auto"][i][1] == T.READ_CORRECTED
    assert min(n_corr) >= 50, n_corr
    # both orientations differ for most reads: the choice is what makes them equal
    assert sum(r["plain"][i] != r["rev"][i] for i in range(n)) >= n // 2
    # a flipped read that is CORRECTED: the reverse complement of the plain context's record of the unflipped read
    run = c.run
    seen = 0
    for i in range(1, n, 2):
        if r["auto"][i][1] == T.READ_CORRECTED and want["reverse"][i] and run["st"][i] == T.READ_CORRECTED:
            assert r["auto"][i][0].decode() == S.revcomp(run["records"][i]), (name, i)
            seen += 1
    assert seen >= 50, seen
    for i in range(0, n, 2):                                            # ... and an unflipped one is that record
        if not want["reverse"][i]:
            assert r["auto"][i][0].decode() == run["records"][i] and r["auto"][i][1] == run["st"][i], (name, i)


def test_passed_through_reads_voted_reverse_come_out_reverse_complemented():
    """The reference's quirk (main.cpp:253): a read passed through under -rev keeps the orientation it was corrected in.  A
    read voted reverse has solid k-mers in its reverse complement, so only NO_STRUCTURE reads (and failed ones) show it."""
    r = three_contexts("no-structure")
    want, n = r["want"], len(r["reads"])
    same_rows(r["rows"], want, "no-structure")
    seen = [0, 0]
    for i in range(n):
        chosen = r["rev"][i] if want["reverse"][i] else r["plain"][i]
        assert r["auto"][i] == chosen, (i, int(want["reverse"][i]))
        if r["auto"][i][1] == T.READ_NO_STRUCTURE:
            rd = S.dna5(r["reads"][i])
            assert r["auto"][i][0].decode() == (S.revcomp(rd) if want["reverse"][i] else rd), i
            seen[int(want["reverse"][i])] += 1
    assert min(seen) >= 2, seen


def test_records_equal_the_oracle_run_in_the_chosen_orientation():
    r = three_contexts("default")
    c = r["c"]
    keys, counts = c.syn.dump_arrays()
    bases, offs = G.pack_reads(r["reads"])
    runs = []
    for reverse in (0, 1):
        p, q = PU.both_params(k=c.k, reverse=reverse)
        ot = O.OracleTable(q, O.OracleTable.FLAT)
        ot.insert_packed(keys, counts)
        ot.decolour()
        out, oo, st = ot.correct_batch(bases, offs, nthreads=8)
        runs.append((G.seqs_of(out, oo), st))
        ot.close()
    for i in range(len(r["reads"])):
        recs, st = runs[int(r["want"]["reverse"][i])]
        assert r["auto"][i][0].decode() == recs[i] and r["auto"][i][1] == int(st[i]), i


# ---------------------------------------------------------------- 3. no behaviour change
def test_a_context_that_never_enabled_it_and_one_that_disabled_it_again():
    r = three_contexts("default")
    c = r["c"]
    other = T.Context(c.ttab, c.p, 0)
    try:
        other.auto_strand(True)
        other.auto_strand(False)
        per, work, rows = everything(other, r["reads"])
        assert rows is None and per == r["plain"] and work == r["work_plain"] and work[1] > 0
    finally:
        other.close()


def test_a_permuted_batch_gives_permuted_rows():
    r = three_contexts("default")
    c = r["c"]
    perm = np.random.default_rng(1).permutation(len(r["reads"]))
    b = c.ctx.batch(*G.pack_reads([r["reads"][i] for i in perm.tolist()]))
    got = b.strand()
    b.close()
    same_rows(got, r["want"][perm], "permuted")


def test_toggling_between_coverage_and_correct_equals_a_fresh_batch():
    r = three_contexts("default")
    c = r["c"]
    reads = r["reads"][:60]
    ctx = T.Context(c.ttab, c.p, 0)
    try:
        def fetched(b):
            out, oo, st = b.fetch_corrected()
            raw, cor = b.solidity()
            return bytes(out), oo.tolist(), st.tolist(), raw.tolist(), cor.tolist()
        fresh = {}
        for on in (False, True):
            ctx.auto_strand(on)
            b = ctx.batch(*G.pack_reads(reads))
            b.correct()
            fresh[on] = fetched(b)
            b.close()
        assert fresh[False] != fresh[True]
        assert [x[0] for x in r["auto"][:60]] == [fresh[True][0][a:e] for a, e in zip(fresh[True][1][:-1], fresh[True][1][1:])]
        for first in (False, True):
            ctx.auto_strand(first)
            b = ctx.batch(*G.pack_reads(reads))
            b.coverage()
            cov_first = b.fetch_coverage()[0].copy()
            ctx.auto_strand(not first)
            b.correct()
            assert fetched(b) == fresh[not first], first
            ctx.auto_strand(first)                       # ... and back: the coverage of the first setting again
            b.coverage()
            assert np.array_equal(b.fetch_coverage()[0], cov_first)
            raw, cor = b.solidity()                      # the batch is as new: no records, so no corrected rows
            assert cor is None and raw.tolist() == fresh[first][3]
            b.close()
    finally:
        ctx.close()


def test_the_two_state_errors():
    c = G.gen_set("default")
    L = T.lib()
    p_rev = T.default_params(k=c.k, reverse=1)
    rev = T.Context(c.ttab, p_rev, 0)
    ctx = T.Context(c.ttab, c.p, 0)
    b = ctx.batch(*G.pack_reads(c.reads[:5]))
    rows = np.zeros(5, R.DTYPE)
    try:
        assert L.talc_ctx_set_auto_strand(rev._h, 1) == ERR_INVALID and b"reverse" in L.talc_last_error()
        assert L.talc_ctx_set_auto_strand(rev._h, 0) == ERR_INVALID
        with pytest.raises(T.TalcError):
            rev.auto_strand()
        assert L.talc_batch_fetch_strand(ctx._h, b._h, rows.ctypes.data) == ERR_STATE and b"vote" in L.talc_last_error()
        b.correct()                                      # auto strand off: a correction runs no vote
        assert L.talc_batch_fetch_strand(ctx._h, b._h, rows.ctypes.data) == ERR_STATE
        assert L.talc_batch_strand(ctx._h, b._h) == 0    # the vote alone, auto strand off
        assert L.talc_batch_fetch_strand(ctx._h, b._h, rows.ctypes.data) == 0
        same_rows(rows, R.rows(c.reads[:5], c.k, c.minc, c.lookup))
        out, oo, st = b.fetch_corrected()                # ... which changes nothing the batch holds
        assert G.seqs_of(out, oo) == c.run["records"][:5]
        assert L.talc_batch_fetch_strand(rev._h, b._h, rows.ctypes.data) == ERR_INVALID          # another context's batch
    finally:
        b.close()
        ctx.close()
        rev.close()


# ---------------------------------------------------------------- 4. the command line
def by_read(path, kind):
    """{read name: the file's text for that read}, names in order of first appearance."""
    out = {}
    if not os.path.exists(path):
        return out
    text = open(path).read()
    if kind == "fasta":          # records; split pieces are name_1, name_2, ...
        for rec in text.split(">")[1:]:
            name = re.sub(r"_\d+$", "", rec.split("\n", 1)[0])
            out[name] = out.get(name, "") + ">" + rec
    elif kind == "log":
        for line in text.splitlines():
            name = re.match(r"\[Read: (.*) \]: ", line).group(1)
            out[name] = out.get(name, "") + line + "\n"
    else:                        # tsv: the name is the first column; "stats": the header's first line has no row
        for line in text.splitlines()[1:]:
            if line:
                name = line.split("\t")[0]
                out[name] = out.get(name, "") + line + "\n"
    return out


FILES = {".fa": "fasta", ".log": "log", ".map.tsv": "tsv0", ".solidity.tsv": "tsv", ".trim.fa": "fasta", ".split.fa": "fasta", ".edits.tsv": "tsv",
         ".stats_basics.txt": "tsv"}


def test_cli_every_line_is_the_line_of_the_run_the_strand_file_names(tmp_path):
    r = three_contexts("default")
    c = r["c"]
    n = 100
    reads, want = r["reads"][:n], r["want"][:n]
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    names = ["read%d/x" % i for i in range(n)]
    (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, reads)))
    base = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7", "-o", "o", "--corr-map", "--soft-mask", "--solidity",
            "--trim", "--split", "--corr-edits", "--read-stats"]
    runs = {}
    for d, extra, env in (("plain", [], None), ("rev", ["-rev"], None), ("auto", ["--auto-strand"], None),
                          ("auto2", ["--auto-strand", "--gpus", "2"], dict(os.environ, TALC_FAKE_GPUS="2"))):
        (tmp_path / d).mkdir()
        runs[d] = subprocess.run([TALC] + base + extra, cwd=tmp_path / d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert runs[d].returncode == 0, (d, runs[d].stderr.decode())
    lines = (tmp_path / "auto" / "o.strand.tsv").read_text().splitlines()
    assert lines[0] == "read_name\tstatus\tn_kmers\tfwd_solid\tfwd_in\trc_solid\trc_in\tstrand"
    st_auto = [x[1] for x in r["auto"][:n]]
    assert lines[1:] == ["\t".join([nm, str(s)] + [str(v) for v in w.tolist()[:5]] + ["-" if w["reverse"] else "+"]) for nm, s, w in zip(names, st_auto, want)]
    nrev = int(want["reverse"].sum())
    assert nrev >= n // 4 and n - nrev >= n // 4
    line = "[TALC]: strand: %d forward, %d reverse of %d reads" % (n - nrev, nrev, n)
    assert runs["auto"].stdout.decode().splitlines().count(line) == 1 and b"strand:" not in runs["plain"].stdout
    differ = 0
    for ext, kind in FILES.items():
        if kind == "tsv0":       # (no header line)
            got, pl, rv = (by_read_headerless(tmp_path / d / ("o" + ext)) for d in ("auto", "plain", "rev"))
        else:
            got, pl, rv = (by_read(str(tmp_path / d / ("o" + ext)), kind) for d in ("auto", "plain", "rev"))
        assert got or ext == ".log", ext
        for nm, w in zip(names, want):
            chosen = rv if w["reverse"] else pl
            assert got.get(nm) == chosen.get(nm), (ext, nm, int(w["reverse"]))
        assert set(got) <= set(names)
        differ += sum(pl.get(nm) != rv.get(nm) for nm in names)
        one, two = tmp_path / "auto" / ("o" + ext), tmp_path / "auto2" / ("o" + ext)
        assert one.exists() == two.exists() and (not one.exists() or one.read_bytes() == two.read_bytes()), ext
    assert differ > 4 * n
    assert (tmp_path / "auto" / "o.strand.tsv").read_bytes() == (tmp_path / "auto2" / "o.strand.tsv").read_bytes()
    assert b"correcting on 2 GPU(s)" in runs["auto2"].stdout
    assert (tmp_path / "auto" / "o.config.txt").read_bytes() == (tmp_path / "plain" / "o.config.txt").read_bytes()
    assert not (tmp_path / "plain" / "o.strand.tsv").exists()
    # a passed-through read voted reverse comes out reverse complemented, and the edits file says so
    ed = by_read(str(tmp_path / "auto" / "o.edits.tsv"), "tsv")
    for nm, s, w in zip(names, st_auto, want):
        assert ed[nm].rstrip("\n").split("\t")[9] == ("-" if (w["reverse"] and s != T.READ_CORRECTED) else "+"), nm


def by_read_headerless(path):
    out = {}
    for line in open(path).read().splitlines():
        name = line.split("\t")[0]
        out[name] = out.get(name, "") + line + "\n"
    return out
