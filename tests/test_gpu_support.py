"""Per-base support on the device (docs/base_support.md; k_base_support, talc_batch_support) against the contract in numpy
(tests/support_ref.py, from the host image of the table: never from a device result).  Bytes, tolerance 0.  Every case
asserts, from the reference alone, that its input reaches what it is there for."""
import os
import subprocess

import numpy as np
import pytest

import solidity_ref as S
import strand_ref as R
import support_ref as P
import test_gpu_solidity as G
from talc_amd import build as B
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
TILE = 256        # SOL_TILE: positions per pass of a wave
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
FORMS = [None, (2, 40), (0, 93)]


def want_bytes(cov, L, k, flip, form):
    """The bytes of one sequence S in the caller's layout, from S's cover: the form, then back to front where S was
    obtained by reverse complement."""
    by = cov.astype(np.uint8) if form is None else P.phred_of(cov, P.span(L, k), *form)
    return by[::-1] if flip else by


def check(got, offs, covers, flips, k, form, what):
    assert len(offs) == len(covers) + 1 and int(offs[-1]) == len(got) == sum(len(c) for c in covers)
    for i, (cov, flip) in enumerate(zip(covers, flips)):
        g, w = got[int(offs[i]):int(offs[i + 1])], want_bytes(cov, len(cov), k, flip, form)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, form, i, len(cov), bool(flip), len(bad), int(bad[0]), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def solid_of(c, seq):
    return S.counts(seq, c.k, c.lookup) >= c.minc


# ---------------------------------------------------------------- 1. hand-made tables, RAW source
_hand = {}


def hand_made(k):
    """test_gpu_solidity.patterned(k) — the table and its reads with weak and solid runs at the word and pass edges — with
    16 reads of 1 .. 16 bases in front (every byte alignment mod 16 of a read's first byte), reads of noise with one k-mer
    of the table alone at an edge, the short lengths, exact multiples of the word and the pass, other letters, and one
    20 kb read.  Returns (Ctx, reads, the cover of every read from the reference): computed once, shared, left unchanged."""
    if k in _hand:
        return _hand[k]
    keys, counts, reads, _ = G.patterned(k)
    c = G.Ctx(keys, counts, k=k)
    rng = np.random.default_rng(77 + k)
    Gs = reads[0]                                        # a substring of the table's sequence: all solid
    n = 3 * TILE - 70
    assert len(Gs) == n + k - 1 and solid_of(c, Gs).all()
    noise = lambda m: "".join("ACGT"[x] for x in rng.integers(0, 4, m).tolist())
    extra, alone = [], []
    for p in (0, 63, 64, 255, 256, 257, n - 1):          # one solid k-mer alone: its k covered bases cross the word or pass edge
        left, right = noise(p), noise(n + k - 1 - p - k)  # (the bases next to it are not those of the table's sequence)
        left = left[:-1] + "ACGT"[("ACGT".index(Gs[4]) + 1) % 4] if p else left
        right = "ACGT"[("ACGT".index(Gs[5 + k]) + 1) % 4] + right[1:] if right else right
        extra.append(left + Gs[5:5 + k] + right)
        alone.append(p)
    shorts = ["", Gs[:k - 1], Gs[:k], Gs[:k + 1], Gs[:2 * k - 2], Gs[:2 * k - 1]]
    exact = [Gs[:64 + k - 1], Gs[:TILE + k - 1], Gs[7:7 + TILE + k - 1]]   # n = 64, 256 (twice: the second starts at another alignment)
    letters = [Gs[:100] + "N" + Gs[101:300], Gs[:200].lower() + "RYK" + Gs[203:420], "n" * 40 + Gs[40:90]]
    front = [Gs[i:i + i + 1] for i in range(16)]         # lengths 1 .. 16
    mine = front + reads + extra + shorts + exact + letters
    # n = 512 exactly and a 20 kb read: concatenations of all-solid stretches (the seams are weak, the rest solid)
    mine.append((Gs + Gs)[:2 * TILE + k - 1])
    mine.append((Gs * 30)[:20000])
    covers = [P.cover(S.dna5(r), k, c.minc, c.lookup) for r in mine]
    # the input is what it is there for, by the table alone
    offs = np.concatenate([[0], np.cumsum([len(r) for r in mine])])
    assert set((offs[:-1] % 16).tolist()) == set(range(16))
    base = len(front) + len(reads)
    for i, p in enumerate(alone):
        sol = solid_of(c, mine[base + i])
        assert np.nonzero(sol)[0].tolist() == [p], (k, p)
        assert covers[base + i].tolist() == [1 if p <= j < p + k else 0 for j in range(n + k - 1)]
    sols = [solid_of(c, r) for r in reads if len(r) == n + k - 1]
    for bnd in (64, TILE, TILE + 1):
        assert any(s[bnd - 1] and not s[bnd] for s in sols) and any(s[bnd] and not s[bnd - 1] for s in sols), bnd    # a run ends, starts
        assert any(s[bnd - 1] and s[bnd] and not s[bnd - 2 - k:bnd + 2 + k].all() for s in sols), bnd                 # ... straddles
        for w in (1, k - 1, k, k + 1, 2 * k + 5):        # a weak run of w positions across the edge
            assert any((not s[bnd - 1] or not s[bnd]) and weak_run_len(s, bnd) == w for s in sols), (k, bnd, w)
    assert any(not s[0] and s[1] for s in sols) and any(not s[-1] and s[-2] for s in sols) and any(s[0] and s[-1] for s in sols)
    lens = [len(r) for r in mine]
    for L in (0, k - 1, k, k + 1, 2 * k - 2, 64 + k - 1, TILE + k - 1, 2 * TILE + k - 1, 20000):
        assert L in lens, L
    assert covers[lens.index(64 + k - 1)].max() == k and covers[lens.index(2 * TILE + k - 1)][-k:].tolist() == list(range(k, 0, -1))
    big = covers[-1]
    assert (big == k).sum() > 15000 and (big < k).sum() > 100
    nn = covers[base + len(extra) + len(shorts) + len(exact)]
    assert nn[100] == 0 and nn[99] == 1 and nn[101] == 1
    _hand[k] = (c, mine, covers)
    return _hand[k]


def weak_run_len(s, bnd):
    """The length of the weak run that holds position bnd - 1 or bnd (0 when both are solid)."""
    i = bnd - 1 if not s[bnd - 1] else bnd
    if s[i]:
        return 0
    a = b = i
    while a > 0 and not s[a - 1]:
        a -= 1
    while b + 1 < len(s) and not s[b + 1]:
        b += 1
    return b - a + 1


def run_raw(ctx, reads, form):
    b = ctx.batch(*G.pack_reads(reads))
    try:
        return b.support("raw", form)
    finally:
        b.close()


@pytest.mark.parametrize("k", [18, 21, 31])
def test_hand_made_table_raw(k):
    c, reads, covers = hand_made(k)
    for form in FORMS:
        got, offs = run_raw(c.ctx, reads, form)
        assert offs.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in reads])]).tolist()
        check(got, offs, covers, [False] * len(reads), k, form, "plain k=%d" % k)


@pytest.mark.parametrize("k", [18, 21, 31])
def test_hand_made_table_reversed_store_path(k):
    """The reverse complements of the same reads through a -rev context (S is the read again, every byte goes to the far
    end), and a mixture through an auto-strand context (the reference's vote says which are turned)."""
    c, reads, covers = hand_made(k)
    rc = [S.revcomp(S.dna5(r)) for r in reads]
    rev = T.Context(c.ttab, T.default_params(k=k, reverse=1), 0)
    auto = T.Context(c.ttab, c.p, 0)
    auto.auto_strand()
    try:
        for form in FORMS:
            got, offs = run_raw(rev, rc, form)
            check(got, offs, covers, [True] * len(reads), k, form, "-rev k=%d" % k)
        mixed = [x if i % 2 else r for i, (r, x) in enumerate(zip(reads, rc))]
        flags = R.rows(mixed, k, c.minc, c.lookup)["reverse"].astype(bool)
        long_ = np.array([len(r) > 600 for r in reads])
        assert (flags & long_).sum() >= 20 and (~flags & long_).sum() >= 20
        # a turned read is seen as its reverse complement: the original read where it was given reverse complemented
        mcov = [P.cover(S.revcomp(S.dna5(m)) if f else S.dna5(m), k, c.minc, c.lookup) for m, f in zip(mixed, flags)]
        assert sum(int(cv.sum()) for cv, f in zip(mcov, flags) if f) > 10000
        for form in FORMS:
            got, offs = run_raw(auto, mixed, form)
            check(got, offs, mcov, flags, k, form, "auto k=%d" % k)
    finally:
        rev.close()
        auto.close()


# ---------------------------------------------------------------- 2. generator sets, RECORD source
SETS = ["default", "reverse", "k31", "branching", "min-count-3", "no-structure", "no-structure-reverse"]
_sets = {}


def set_run(name):
    """One correct() of the set's 200 reads with the support of its records and of its reads, and the reference's covers
    (computed once, shared, left unchanged)."""
    if name not in _sets:
        c = G.gen_set(name)
        b = c.ctx.batch(*G.pack_reads(c.reads))
        try:
            b.correct()
            out, oo, st = b.fetch_corrected()
            r = dict(c=c, records=G.seqs_of(out, oo), oo=oo, st=st)
            r["got"] = {(src, form): b.support(src, form) for src in ("record", "raw") for form in FORMS}
        finally:
            b.close()
        assert r["records"] == c.run["records"]
        r["flip"] = [c.rev and s == T.READ_CORRECTED for s in st.tolist()]
        r["probed"] = c.as_probed(r["records"], st)
        r["cov"] = [P.cover(s, c.k, c.minc, c.lookup) for s in r["probed"]]
        r["raw_cov"] = [P.cover(s, c.k, c.minc, c.lookup) for s in c.as_corrected(c.reads)]
        _sets[name] = r
    return _sets[name]


@pytest.mark.parametrize("name", SETS)
def test_generator_set(name):
    r = set_run(name)
    c = r["c"]
    for form in FORMS:
        got, offs = r["got"][("record", form)]
        assert np.array_equal(offs, r["oo"])
        check(got, offs, r["cov"], r["flip"], c.k, form, name + " record")
        got, offs = r["got"][("raw", form)]
        assert offs.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in c.reads])]).tolist()
        check(got, offs, r["raw_cov"], [c.rev] * len(c.reads), c.k, form, name + " raw")
    rows = c.ref(r["probed"])
    got, offs = r["got"][("record", None)]
    for i, cov in enumerate(r["cov"]):
        g = got[int(offs[i]):int(offs[i + 1])].astype(np.int64)
        assert int(g.sum()) == int(cov.sum()) == c.k * int(rows["n_solid"][i])                  # identity 1
        assert int((g > 0).sum()) == int((cov > 0).sum()) == int(rows["solid_bases"][i])        # identity 2
    allc = np.concatenate(r["cov"])
    alls = np.concatenate([P.span(len(x), c.k) for x in r["cov"]])
    assert ((allc == alls) & (alls > 0)).sum() > 1000 and ((allc > 0) & (allc < alls)).sum() > 100
    if c.rev:
        assert sum(r["flip"]) >= 5


def test_the_sets_together_hold_unsupported_bases():
    assert sum(int((np.concatenate(set_run(n)["cov"]) == 0).sum()) for n in SETS) > 100


# ---------------------------------------------------------------- 3. nothing else moves, state and errors
@pytest.mark.parametrize("name", ["default", "reverse"])
def test_support_changes_nothing_else(name):
    c = G.gen_set(name)
    bases, offs = G.pack_reads(c.reads)
    c.ctx.record_map(True)
    try:
        res = []
        for with_support in (False, True):
            b = c.ctx.batch(bases, offs)
            rc = b.correct()
            t = c.ctx.timing()
            work = (rc, t.n_trail_steps, t.n_dp_cells, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)
            if with_support:
                b.support("record", (2, 40))
                b.support("raw")
            out, oo, st = b.fetch_corrected()
            segs, so = b.fetch_map()
            raw, cor = b.solidity()
            pb, po, pc, rpo = b.pieces(T.PIECES_SPLIT, 0, False)
            ops, eo, erows = b.edits()
            res.append((work, bytes(out), oo.tolist(), st.tolist(), segs.tobytes(), so.tolist(), raw.tobytes(), cor.tobytes(), bytes(pb), pc.tobytes(), ops.tobytes(),
                        erows.tobytes()))
            if with_support:
                b.correct()                                  # a second correction of the batch the pass has looked at
                out2, oo2, st2 = b.fetch_corrected()
                assert bytes(out2) == res[0][1] and st2.tolist() == res[0][3]
            b.close()
        assert res[0] == res[1] and res[0][0][1] > 0 and len(res[0][4]) > 200 * 20
    finally:
        c.ctx.record_map(False)
    assert c.ctx.support_timing() > 0


def test_state_and_errors():
    r = set_run("default")
    c = r["c"]
    L = T.lib()
    n = 12
    b = c.ctx.batch(*G.pack_reads(c.reads[:n]))
    try:
        h = (c.ctx._h, b._h)
        buf, oo = np.zeros(1 << 16, np.uint8), np.zeros(n + 1, np.uint64)

        def params(source, phred=0, qmin=0, qmax=0):
            return T.SupportParams(source, phred, qmin, qmax)

        import ctypes as C
        assert L.talc_batch_fetch_support(*h, buf.ctypes.data, len(buf), oo.ctypes.data) == ERR_STATE      # nothing computed yet
        assert L.talc_batch_support_bytes(b._h) == 0
        assert L.talc_batch_support(*h, C.byref(params(T.SUPPORT_RECORD))) == ERR_STATE                    # no records yet
        for bad in (params(2), params(0, 2), params(0, 1, 5, 4), params(1, 1, 0, 94), params(0, 1, 94, 94)):
            assert L.talc_batch_support(*h, C.byref(bad)) == ERR_INVALID, (bad.source, bad.phred, bad.qmin, bad.qmax)
        assert L.talc_batch_support(*h, None) == ERR_INVALID
        assert L.talc_batch_support(*h, C.byref(params(T.SUPPORT_RAW))) == 0                               # RAW needs no correction
        raw_total = sum(len(x) for x in c.reads[:n])
        assert L.talc_batch_support_bytes(b._h) == raw_total
        assert L.talc_batch_fetch_support(*h, buf.ctypes.data, raw_total - 1, oo.ctypes.data) == ERR_CAPACITY
        assert str(raw_total).encode() in L.talc_last_error()
        assert L.talc_batch_fetch_support(*h, buf.ctypes.data, raw_total, oo.ctypes.data) == 0
        check(buf[:raw_total], oo, r["raw_cov"][:n], [False] * n, c.k, None, "raw before the correction")
        assert L.talc_batch_fetch_support(*h, None, 0, None) == 0
        assert b.correct() == 0
        assert L.talc_batch_fetch_support(*h, buf.ctypes.data, len(buf), oo.ctypes.data) == ERR_STATE      # not since the correction
        assert b"talc_batch_support" in L.talc_last_error() and L.talc_batch_support_bytes(b._h) == 0
        got, offs = b.support("raw")
        check(got, offs, r["raw_cov"][:n], [False] * n, c.k, None, "raw after the correction")
        got, offs = b.support("record", (2, 40))                                                          # ... replaces it
        assert np.array_equal(offs, r["oo"][:n + 1]) and L.talc_batch_support_bytes(b._h) == int(r["oo"][n])
        check(got, offs, r["cov"][:n], [False] * n, c.k, (2, 40), "record replaces raw")
        assert L.talc_batch_fetch_support(*h, buf.ctypes.data, len(buf), oo.ctypes.data) == 0 and np.array_equal(buf[:len(got)], got)
        assert b.correct() == 0
        assert L.talc_batch_fetch_support(*h, buf.ctypes.data, len(buf), oo.ctypes.data) == ERR_STATE      # after a second correct()
    finally:
        b.close()


# ---------------------------------------------------------------- 4. the command line
def cli(args, cwd, env=None):
    return subprocess.run([TALC] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


OTHER = [".fa", ".log", ".config.txt", ".stats_basics.txt", ".trim.fa", ".split.fa", ".strand.tsv"]
CASES = {   # id -> (extra options, generator set, quality range)
    "plain": ([], "default", (2, 40)),
    "soft-mask": (["--soft-mask"], "default", (2, 40)),
    "trim": (["--trim"], "default", (2, 40)),
    "split": (["--split", "--min-piece-len", "50"], "default", (2, 40)),
    "rev": (["-rev"], "reverse", (2, 40)),
    "auto": (["--auto-strand"], "default", (2, 40)),
    "qual-range": (["--qual-range", "0,60"], "default", (0, 60)),
}
N_CLI = 30


@pytest.mark.parametrize("case", list(CASES))
def test_cli_fastq(tmp_path, case):
    extra, name, qr = CASES[case]
    c = G.gen_set(name)
    reads = c.reads[:N_CLI]
    if case == "auto":
        reads = [S.revcomp(x) if i % 2 else x for i, x in enumerate(reads)]
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    names = ["read%d/x" % i for i in range(len(reads))]
    (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (nm, x) for nm, x in zip(names, reads)))
    base = [str(tmp_path / "reads.fa"), "-k", str(c.k), "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7", "-o", "o"]
    plain_extra = [x for x in extra if x not in ("--qual-range", "0,60")]
    runs = [("with", base + extra + ["--fastq"], None), ("without", base + plain_extra, None)]
    if case == "plain":
        runs.append(("two", base + ["--fastq", "--gpus", "2"], dict(os.environ, TALC_FAKE_GPUS="2")))
    out = {}
    for d, args, env in runs:
        (tmp_path / d).mkdir()
        out[d] = cli(args, tmp_path / d, env)
        assert out[d].returncode == 0, (d, out[d].stderr.decode())
    w = tmp_path / "with"
    for ext in OTHER:                                                    # every other file is that of the run without --fastq
        fa, fp = w / ("o" + ext), tmp_path / "without" / ("o" + ext)
        assert fa.exists() == fp.exists() and (not fa.exists() or fa.read_bytes() == fp.read_bytes()), ext
    assert out["with"].stdout == out["without"].stdout and not (tmp_path / "without" / "o.fq").exists()
    # the orientation every record was probed in: the whole file's -rev or the reference's vote, for a CORRECTED read
    turned = [bool(c.rev)] * len(reads)
    ctx = c.ctx
    if case == "auto":
        turned = R.rows(reads, c.k, c.minc, c.lookup)["reverse"].astype(bool).tolist()
        assert 8 <= sum(turned) <= len(reads) - 8
        ctx = T.Context(c.ttab, c.p, 0)
        ctx.auto_strand()
    ctx.record_map(True)
    b = ctx.batch(*G.pack_reads(reads))
    try:
        b.correct()
        st = b.fetch_corrected()[2].tolist()
        pieces = {}
        if case in ("trim", "split"):
            pb, po, pc, rpo = b.pieces(T.PIECES_TRIM if case == "trim" else T.PIECES_SPLIT, 50 if case == "split" else 0, False)
            pieces = {i: pc[int(rpo[i]):int(rpo[i + 1])] for i in range(len(reads))}
    finally:
        b.close()
        ctx.record_map(False)
        if case == "auto":
            ctx.close()
    assert sum(s == T.READ_CORRECTED for s in st) >= 20
    fa = P.parse_fasta((w / "o.fa").read_text())
    fq = P.parse_fastq((w / "o.fq").read_text())
    assert [(nm, s) for nm, s, q in fq] == fa and [nm for nm, s in fa] == names
    if case == "soft-mask":
        assert any(s != s.upper() for nm, s in fa) and any(s != s.lower() for nm, s in fa)
    quals = []
    for (nm, s, q), t, status in zip(fq, turned, st):
        flip = t and status == T.READ_CORRECTED
        rec = s.upper()
        cov = P.cover(S.revcomp(rec) if flip else rec, c.k, c.minc, c.lookup)
        want = want_bytes(cov, len(rec), c.k, flip, qr).tobytes().decode()
        assert q == want, (case, nm, flip)
        quals.append(want)
    allq = "".join(quals)
    assert chr(33 + qr[1]) in allq and chr(33 + qr[0]) in allq and len(set(allq)) > 10            # both ends and what lies between
    if case in ("rev", "auto"):
        assert sum(t and s == T.READ_CORRECTED for t, s in zip(turned, st)) >= 8
    if case in ("trim", "split"):
        pf = P.parse_fasta((w / ("o.%s.fa" % case)).read_text())
        pq = P.parse_fastq((w / ("o.%s.fq" % case)).read_text())
        assert [(nm, s) for nm, s, q in pq] == pf and len(pf) >= 20
        want = []
        for i, nm in enumerate(names):
            for j, pc in enumerate(pieces[i]):
                a, e = int(pc["out_start"]), int(pc["out_start"]) + int(pc["out_len"])
                want.append((nm + ("_%d" % (j + 1) if case == "split" else ""), fa[i][1][a:e], quals[i][a:e]))
        assert pq == want
        assert any(len(s) < len(fa[names.index(nm.rsplit("_", 1)[0] if case == "split" else nm)][1]) for nm, s, q in pq)
    else:
        assert not (w / "o.trim.fq").exists() and not (w / "o.split.fq").exists()
    if case == "plain":
        for f in os.listdir(w):
            assert (tmp_path / "two" / f).read_bytes() == (w / f).read_bytes(), f
        assert b"correcting on 2 GPU(s)" in out["two"].stdout and sorted(os.listdir(w)) == sorted(os.listdir(tmp_path / "two"))
