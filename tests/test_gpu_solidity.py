"""The solidity report on the device (docs/solidity.md; k_solidity, talc_batch_solidity) against the contract in numpy
(tests/solidity_ref.py, from the host image of the table: never from a device result).  Integers, tolerance 0."""
import os
import subprocess

import numpy as np
import pytest

import solidity_ref as S
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
TILE = 256        # SOL_TILE (talc_kernels_solidity.h): positions per pass of a wave
ERR_STATE = -6


def seqs_of(buf, offs):
    b = bytes(buf)
    return [b[int(offs[i]):int(offs[i + 1])].decode() for i in range(len(offs) - 1)]


def pack_reads(reads):
    rb = "".join(reads).encode()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in reads])
    return (np.frombuffer(rb, dtype=np.uint8) if rb else np.zeros(0, np.uint8)), offs


def same_rows(got, want, what=""):
    assert got.dtype == S.DTYPE and len(got) == len(want)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


class Ctx:
    """A product table (uploaded) with a context, and the reference's lookup over its host image."""

    def __init__(self, keys=None, counts=None, share=None, **params_kw):
        """share: another Ctx whose table and parameters this one takes, with a context of its own (made now: it reads the
        environment's switches as they are now)."""
        if share is not None:
            self.p, self.ttab, self.lookup = share.p, share.ttab, share.lookup
        else:
            self.p = T.default_params(**params_kw)
            self.ttab = T.Table.from_arrays(keys, counts, self.p)
            self.ttab.decolour_repeats()
            self.lookup = S.host_lookup(self.ttab)
            self.ttab.upload(0)
        self.k, self.minc, self.rev = self.p.k, self.p.min_count, bool(self.p.reverse)
        self.ctx = T.Context(self.ttab, self.p, 0)

    def ref(self, seqs):
        return S.rows(seqs, self.k, self.minc, self.lookup)

    def as_corrected(self, reads):
        """The reads as the correction sees them: Dna5-converted, reverse-complemented under -rev."""
        return [S.revcomp(S.dna5(r)) if self.rev else S.dna5(r) for r in reads]

    def as_probed(self, records, status):
        """The records in that same orientation: a corrected read's record was reverse-complemented on its way out."""
        return [S.revcomp(r) if (self.rev and st == T.READ_CORRECTED) else r for r, st in zip(records, status.tolist())]


SETS = {   # name -> (k-mers of the generator, k, seed, generator settings, parameters)
    "default": (60_000, 21, 7, {}, {}),
    "reverse": (60_000, 21, 7, {}, dict(reverse=1)),
    "k31": (60_000, 31, 7, {}, {}),
    "branching": (60_000, 21, 7, dict(paralog_frac=0.7, paralog_div=0.06), {}),
    "min-count-3": (60_000, 21, 7, {}, dict(min_count=3)),
    "no-structure": (60_000, 22, 403, dict(paralog_frac=0.4, paralog_div=0.03), dict(sr_error_rate=1.5, alpha=0.5, min_count=5)),
    "no-structure-reverse": (60_000, 22, 403, dict(paralog_frac=0.4, paralog_div=0.03), dict(sr_error_rate=1.5, alpha=0.5, min_count=5, reverse=1)),
    # the graph and reads of the correction map's failed-reads case (tests/corr_map_ref.py: SETS["reverse"])
    "map-reverse": (250_000, 21, 77, {}, dict(reverse=1)),
}
_cache = {}


def gen_set(name):
    """One of SETS: the context, the generator's first 200 reads, and everything one correct() + solidity() of them gives
    (computed once, shared, left unchanged)."""
    if name not in _cache:
        target, k, seed, synth_kw, params_kw = SETS[name]
        syn = Synth(target_kmers=target, k=k, seed=seed, **synth_kw)
        c = Ctx(*syn.dump_arrays(), k=k, **params_kw)
        c.syn = syn
        c.reads = seqs_of(*syn.reads(0, 200))
        if c.rev:   # (k-mers are directional: -rev corrects the reads of the opposite strand)
            c.reads = [S.revcomp(r) for r in c.reads]
        c.run = correct_and_report(c, c.reads)
        _cache[name] = c
    return _cache[name]


def correct_and_report(c, reads, before=False):
    bases, offs = pack_reads(reads)
    b = c.ctx.batch(bases, offs)
    try:
        r = {}
        if before:
            r["raw_before"], none = b.solidity()
            assert none is None
        r["rc"] = b.correct()
        t = c.ctx.timing()
        r["work"] = (t.n_trail_steps, t.n_dp_cells, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)
        r["raw"], r["cor"] = b.solidity()
        out, oo, st = b.fetch_corrected()
        r["records"], r["oo"], r["st"], r["out"] = seqs_of(out, oo), oo, st, out.copy()
        return r
    finally:
        b.close()


# ---------------------------------------------------------------- 1. patterned reads on a hand-made table
def patterned(k, minc=2):
    """G: 3 000 random bases with one planted repeat of k - 2 bases (a read that changes copies there has exactly one
    k-mer that is not in the table); the table: every k-mer of G, counts drawn from {MIN, MIN + 1, 50}; the reads:
    substrings of G in which substitutions and changes of place leave weak runs of chosen lengths at chosen positions.
    Returns (keys, counts, reads, wanted weak runs per read as [(first, length)])."""
    rng = np.random.default_rng(1000 + k)
    G = rng.integers(0, 4, 3000).tolist()
    c1, c2 = 700, 2000                                  # the two copies: G[c1 : c1 + k - 2] == G[c2 : c2 + k - 2]
    G[c2:c2 + k - 2] = G[c1:c1 + k - 2]
    G[c2 - 1] = (G[c1 - 1] + 1) % 4                     # ... and no longer: the bases around them differ
    G[c2 + k - 2] = (G[c1 + k - 2] + 2) % 4
    G[2300], G[2299] = (G[1200] + 1) % 4, (G[1199] + 2) % 4   # (the seam 1200 | 2300 of the other change of place: nothing in common)
    G = "".join("ACGT"[x] for x in G)
    table = {}
    for i in range(len(G) - k + 1):
        table.setdefault(S.pack(G[i:i + k]), int(rng.choice([minc, minc + 1, 50])))
    n = 3 * TILE - 70                                   # k-mer positions of a read: three passes, the last word partial
    L = n + k - 1
    reads, want = [], []

    def add(weak, jump=None):
        """weak: [(first, length >= k)] made by substitutions; jump: (first, 1 or k - 1) made by changing place in G."""
        if jump:
            J = jump[0] + k - 1                         # bases of the first part: its last k-mer is position first - 1
            if jump[1] == 1:                            # from the end of copy 1 to the end of copy 2
                r = list(G[c1 + k - 2 - J:c1 + k - 2] + G[c2 + k - 2:c2 + k - 2 + L - J])
            else:                                       # to a place that has nothing in common: k - 1 k-mers span the seam
                r = list(G[1200 - J:1200] + G[2300:2300 + L - J])
        else:
            r = list(G[100:100 + L])
        assert len(r) == L
        for s, w in weak:
            for bpos in list(range(s + k - 1, s + w - 1, k)) + [s + w - 1]:
                r[bpos] = "ACGT"[("ACGT".index(r[bpos]) + 1) % 4]
        reads.append("".join(r))
        want.append(sorted(weak + ([jump] if jump else [])))

    add([])                                             # one run from 0 to n - 1
    for bnd in (64, TILE, TILE + 1):
        add([(bnd, k)])                                 # a solid run ends at bnd - 1
        add([(bnd - k, k)])                             # a solid run starts at bnd
        add([(bnd - 40, k), (bnd + 3, k)])              # a solid run of 43 - k positions straddles bnd - 1 / bnd
        add([(bnd - k, k), (bnd + 1, k)])               # the run is position bnd alone
        add([(bnd - 1 - k, k), (bnd, k)])               # ... position bnd - 1 alone
        for w in (1, k - 1):                            # weak runs shorter than k: the base coverage of the two runs overlaps
            for first in sorted({bnd - 1, bnd, bnd - w // 2, bnd - w + 1}):
                add([], (first, w))
        for w in (k, k + 1, 2 * k + 5):
            for first in sorted({bnd - 1, bnd - w // 2, max(0, bnd - w + 1)}):
                add([(first, w)])
    # the read's two ends: a weak position 0, a weak position n - 1 (one substituted base each), both, and whole words
    add([])
    reads[-1] = "T" + reads[-1][1:] if reads[-1][0] != "T" else "A" + reads[-1][1:]
    want[-1] = [(0, 1)]
    add([])
    reads[-1] = reads[-1][:-1] + ("T" if reads[-1][-1] != "T" else "A")
    want[-1] = [(n - 1, 1)]
    add([(0, k), (n - k, k)])
    add([(0, 64), (n - 64 - (n % 64), 64 + n % 64)])
    add([(0, n)])                                       # none solid
    g0 = G[100:]
    reads += ["", g0[:k - 1], g0[:k], g0[:k + 1], g0[:64 + k - 1], g0[:TILE + k - 1], g0[:TILE + k]]
    want += [[]] * 7
    keys = np.fromiter(table.keys(), dtype=np.uint64, count=len(table))
    counts = np.fromiter(table.values(), dtype=np.uint32, count=len(table))
    return keys, counts, reads, want


@pytest.mark.parametrize("k", [18, 21, 31])
def test_patterned_reads_on_a_hand_made_table(k):
    keys, counts, reads, want = patterned(k)
    c = Ctx(keys, counts, k=k)
    ref = c.ref(reads)
    for i, (r, w) in enumerate(zip(reads, want)):       # the reads are what they were built to be, by the table alone
        weak = S.counts(r, k, c.lookup) < c.minc
        d = np.diff(np.concatenate([[0], weak.astype(np.int8), [0]]))
        runs = list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]).tolist()))
        assert runs == w, (k, i, runs, w)
    assert (ref["n_solid"] != ref["n_in"]).any() and ref["n_regions"].max() >= 3 and ref["longest_weak"].max() == 3 * TILE - 70
    bases, offs = pack_reads(reads)
    b = c.ctx.batch(bases, offs)
    raw, cor = b.solidity()
    b.close()
    assert cor is None
    same_rows(raw, ref, "patterned k=%d" % k)


# ---------------------------------------------------------------- 2. generator sets
@pytest.mark.parametrize("name", ["default", "reverse", "k31", "branching", "min-count-3"])
def test_generator_set(name):
    c = gen_set(name)
    r = c.run
    assert int((r["st"] == T.READ_CORRECTED).sum()) >= 150
    want_raw = c.ref(c.as_corrected(c.reads))
    same_rows(r["raw"], want_raw, name + " raw")
    want_cor = c.ref(c.as_probed(r["records"], r["st"]))
    same_rows(r["cor"], want_cor, name + " corrected")
    assert (want_cor["n_kmers"] == [max(0, len(x) - c.k + 1) for x in r["records"]]).all()
    # the correction is worth something, and the report says so
    assert int(want_cor["solid_bases"].sum()) > int(want_raw["solid_bases"].sum()) and int(want_cor["longest_weak"].max()) > 0
    assert (want_raw["n_solid"] != want_raw["n_in"]).any()
    b = c.ctx.batch(*pack_reads(c.reads))              # Read.cpp:190 as the coverage kernel counts it, on a fresh batch
    b.coverage()
    nin = b.fetch_coverage()[3]
    b.close()
    assert (r["raw"]["n_in"].astype(np.int64) == nin).all()


# ---------------------------------------------------------------- 3. self-consistency
@pytest.mark.parametrize("name", ["default", "k31"])
def test_corrected_rows_are_the_raw_rows_of_the_records(name):
    c = gen_set(name)
    b = c.ctx.batch(*pack_reads(c.run["records"]))
    raw, cor = b.solidity()
    b.close()
    assert cor is None
    same_rows(raw, c.run["cor"], name)


# ---------------------------------------------------------------- 4. long reads
def test_long_reads():
    """20 kb (79 passes of a wave, 313 words) and 64 m + K - 1 bases (the last word is full), raw and corrected."""
    c = gen_set("default")
    cat = "".join(c.reads[:20])
    reads = [cat[:20000], c.reads[3][:64 * 9 + c.k - 1], c.reads[4][:64 * 8 + c.k - 1 + 1], c.reads[5][:TILE * 2 + c.k - 1]]
    assert len(reads[0]) == 20000 and all(len(x) >= 500 for x in reads)
    r = correct_and_report(c, reads)
    same_rows(r["raw"], c.ref(c.as_corrected(reads)), "long raw")
    same_rows(r["cor"], c.ref(c.as_probed(r["records"], r["st"])), "long corrected")
    assert r["raw"]["n_kmers"].tolist() == [20000 - 20, 576, 513, 512] and r["raw"]["n_regions"][0] > 20


# ---------------------------------------------------------------- 5. reads that are passed through
def check_passed_through(c, reads, need):
    r = correct_and_report(c, reads)
    st = r["st"]
    for s in need:
        assert (st == s).any(), (s, np.bincount(st, minlength=5).tolist())
    same_rows(r["raw"], c.ref(c.as_corrected(reads)), "raw")
    same_rows(r["cor"], c.ref(c.as_probed(r["records"], st)), "corrected")
    thru = st != T.READ_CORRECTED
    assert (r["cor"][thru] == r["raw"][thru]).all() and (r["cor"][~thru] != r["raw"][~thru]).any()
    return r


@pytest.mark.parametrize("name", ["no-structure", "no-structure-reverse"])
def test_passed_through_reads_have_equal_rows(name):
    """Too short, no solid k-mer, no structure (14 of the set's 200 reads: they have solid k-mers, so under -rev their
    rows tell whether the record was taken in the orientation it has — as it stands — or flipped like a corrected one)."""
    c = gen_set(name)
    rng = np.random.default_rng(3)
    noise = "".join("ACGT"[x] for x in rng.integers(0, 4, 1500).tolist())
    reads = ["", c.reads[0][:c.k - 1], c.reads[0][:c.k], noise, "ACGT" * 300, "N" * 100, c.reads[1][:400] + "NNNN" + c.reads[1][404:]] + c.reads[:80]
    r = check_passed_through(c, reads, [T.READ_SKIPPED_SHORT, T.READ_NO_SOLID_KMER, T.READ_CORRECTED, T.READ_NO_STRUCTURE])
    assert r["raw"][:2].tolist() == [(0, 0, 0, 0, 0, 0)] * 2 and r["raw"][2]["n_kmers"] == 1 and r["raw"][5].tolist() == (101 - c.k, 0, 0, 0, 0, 101 - c.k)
    ns = r["st"] == T.READ_NO_STRUCTURE
    assert int(ns.sum()) >= 5 and (r["raw"]["n_solid"][ns] > 0).all()


def test_failed_reads_have_equal_rows(monkeypatch):
    """TALC_TEST_TINY_CAPS with TALC_TEST_FAIL_RETRY_ALLOC: reads overflow their scratch, the retry stage is refused, they
    end as TALC_READ_ERROR and are passed through (the means of test_map_survives_the_retry_pass_and_failed_reads)."""
    c = gen_set("map-reverse")
    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "1")
    monkeypatch.setenv("TALC_TEST_FAIL_RETRY_ALLOC", "1")
    c2 = Ctx(share=c)
    try:
        r = check_passed_through(c2, c.reads, [T.READ_ERROR, T.READ_CORRECTED])
        assert r["rc"] == T.WARN_READ_ERRORS
        same_rows(r["raw"], c.run["raw"], "raw rows do not depend on the search")
    finally:
        c2.ctx.close()


# ---------------------------------------------------------------- 6. nothing else moves
@pytest.mark.parametrize("name", ["default", "reverse"])
def test_report_changes_nothing_else(name):
    c = gen_set(name)
    bases, offs = pack_reads(c.reads)
    c.ctx.record_map(True)
    try:
        plain = c.ctx.batch(bases, offs)
        rc0 = plain.correct()
        t = c.ctx.timing()
        work0 = (t.n_trail_steps, t.n_dp_cells, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)
        out0, oo0, st0 = plain.fetch_corrected()
        segs0, so0 = plain.fetch_map()
        plain.close()
        b = c.ctx.batch(bases, offs)
        raw_before, none = b.solidity()                  # before the correction: the raw rows only
        assert none is None
        rc1 = b.correct()
        t = c.ctx.timing()
        work1 = (t.n_trail_steps, t.n_dp_cells, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)
        raw_after, cor = b.solidity()
        out1, oo1, st1 = b.fetch_corrected()
        segs1, so1 = b.fetch_map()
        msk1 = b.fetch_corrected(soft_mask=True)[0]
        assert rc0 == rc1 and work0 == work1 and work0[0] > 0
        assert np.array_equal(out0, out1) and np.array_equal(oo0, oo1) and np.array_equal(st0, st1)
        assert np.array_equal(segs0, segs1) and np.array_equal(so0, so1) and len(segs0) > 200
        assert bytes(msk1).upper() == bytes(out1)
        same_rows(raw_after, raw_before, "raw rows before and after the correction")
        same_rows(raw_after, c.run["raw"], "raw")
        same_rows(cor, c.run["cor"], "corrected")
        b.correct()                                      # a second correction of the batch the report has looked at
        out2, oo2, st2 = b.fetch_corrected()
        assert np.array_equal(out0, out2) and np.array_equal(oo0, oo2) and np.array_equal(st0, st2)
        b.close()
    finally:
        c.ctx.record_map(False)
    assert c.ctx.solidity_timing()[0] > 0 and c.ctx.solidity_timing()[1] > 0


# ---------------------------------------------------------------- 7. errors
def test_fetch_reports_state():
    c = gen_set("default")
    L = T.lib()
    n = 12
    b = c.ctx.batch(*pack_reads(c.reads[:n]))
    raw, cor = np.zeros(n, S.DTYPE), np.zeros(n, S.DTYPE)
    try:
        h = (c.ctx._h, b._h)
        assert L.talc_batch_fetch_solidity(*h, raw.ctypes.data, None) == ERR_STATE             # no talc_batch_solidity yet
        assert L.talc_batch_solidity(*h) == 0
        assert L.talc_batch_fetch_solidity(*h, raw.ctypes.data, cor.ctypes.data) == ERR_STATE  # never corrected
        assert L.talc_batch_fetch_solidity(*h, None, cor.ctypes.data) == ERR_STATE
        assert L.talc_batch_fetch_solidity(*h, raw.ctypes.data, None) == 0
        assert L.talc_batch_fetch_solidity(*h, None, None) == 0
        same_rows(raw, c.run["raw"][:n])
        assert c.ctx.solidity_timing()[1] == 0
        assert b.correct() == 0
        assert L.talc_batch_fetch_solidity(*h, raw.ctypes.data, None) == ERR_STATE             # not since the correction
        assert b"talc_batch_solidity" in L.talc_last_error()
        assert L.talc_batch_solidity(*h) == 0
        raw[:] = 0
        assert L.talc_batch_fetch_solidity(*h, None, cor.ctypes.data) == 0
        assert L.talc_batch_fetch_solidity(*h, raw.ctypes.data, None) == 0
        same_rows(raw, c.run["raw"][:n])
        same_rows(cor, c.run["cor"][:n])
    finally:
        b.close()


# ---------------------------------------------------------------- 8. the command line
def cli(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_cli_solidity_file(tmp_path, rev):
    c = gen_set("reverse" if rev else "default")
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    names = ["read%d/x" % i for i in range(len(c.reads))]
    (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, c.reads)))
    for d in ("with", "without"):
        (tmp_path / d).mkdir()
    args = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "64", "-o", "o"] + (["-rev"] if rev else [])
    a, p = cli(args + ["--solidity"], tmp_path / "with"), cli(args, tmp_path / "without")
    assert a.returncode == 0 and p.returncode == 0, (a.stderr.decode(), p.stderr.decode())
    lines = (tmp_path / "with" / "o.solidity.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["read_name", "status", "raw_length", "corr_length"] + ["raw_" + f for f in S.FIELDS] + ["corr_" + f for f in S.FIELDS]
    r = c.run
    want = ["\t".join([n, str(int(st)), str(len(x)), str(len(y))] + [str(v) for v in a_.tolist()] + [str(v) for v in b_.tolist()])
            for n, st, x, y, a_, b_ in zip(names, r["st"], c.reads, r["records"], r["raw"], r["cor"])]
    assert lines[1:] == want
    for ext in (".fa", ".log", ".config.txt", ".stats_basics.txt"):
        fa, fp = tmp_path / "with" / ("o" + ext), tmp_path / "without" / ("o" + ext)
        assert fa.exists() == fp.exists() and (not fa.exists() or fa.read_bytes() == fp.read_bytes()), ext
    assert (tmp_path / "with" / "o.fa").read_text().replace("\n", "").count(">") == 200 and not (tmp_path / "without" / "o.solidity.tsv").exists()
    cols = np.array([[int(v) for v in l.split("\t")[1:]] for l in lines[1:]], dtype=np.int64)
    A, Bn, Cc, D = int(cols[:, 7].sum()), int(cols[:, 1].sum()), int(cols[:, 13].sum()), int(cols[:, 2].sum())
    line = "[TALC]: solid bases: raw %d of %d (%.2f %%), corrected %d of %d (%.2f %%)" % (A, Bn, 100.0 * A / Bn, Cc, D, 100.0 * Cc / D)
    out = a.stdout.decode().splitlines()
    assert out.count(line) == 1 and Cc > A > 0
    assert [l for l in out if l != line] == p.stdout.decode().splitlines()
