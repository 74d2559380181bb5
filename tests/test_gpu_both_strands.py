"""Both strands (docs/both_strands.md): the canonical counter, talc_counter_add_counts, the expanding compaction, the
folded builds from arrays and from dumps, and `talc --both-strands`, against the numpy statement of the contract
(tests/fold_ref.py).  Every expected value is made in numpy before the first device call of its test."""
import os
import subprocess

import numpy as np
import pytest

import fold_ref as F
import kmer_ref as R
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ERR_INVALID, ERR_STATE = "error -1:", "error -6:"


def sorted_pairs(kmers, counts):
    o = np.argsort(kmers, kind="stable")
    return kmers[o], counts[o]


def counted(params, chunks, expected_distinct=0, both=True):
    c = T.KmerCounter(params, 0, expected_distinct, both_strands=both)
    for b, o in chunks:
        c.add(b, o)
    st = c.stats()
    k1, c1 = sorted_pairs(*c.fetch(1))
    return c, st, k1, c1


def slices(bases, offsets, cuts):
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(offsets[a]), int(offsets[b])
        out.append((bases[lo:hi], offsets[a:b + 1] - offsets[a]))
    return out


def same_lookups(a, b, q):
    ra, rb = a.lookup(q), b.lookup(q)
    return np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])


@pytest.fixture(scope="module")
def synth():
    return Synth(target_kmers=150_000, k=21, seed=77)


def mixed_reads(synth, n):
    bases, offs = synth.short_reads(0, n, length=150, sub_rate=0.005, n_rate=0.001)
    flipped, _ = F.flip_records(bases, offs, np.random.default_rng(1))
    return flipped, offs


class Mixed:
    """The strand-mixed reads and everything numpy says about them (K = 21, MIN_COUNT = 2)."""

    def __init__(self, synth, n):
        self.bases, self.offs = mixed_reads(synth, n)
        self.dk, self.dc = R.count(self.bases, self.offs, 21)                 # directional
        self.y, self.c = F.fold(self.dk, self.dc, 21)                         # canonical, folded
        self.km, self.ct = F.expand(self.y, self.c, 21, min_count=2)          # what the table stores
        folded_of = self.c[np.searchsorted(self.y, F.canon(self.dk, 21))]
        self.boundary = self.dk[(self.dc < 2) & (folded_of >= 2)]             # half the support on each strand


@pytest.fixture(scope="module")
def mixed(synth):
    return Mixed(synth, 3000)


@pytest.fixture(scope="module")
def deep(synth):
    return Mixed(synth, 200_000)


# ------------------------------------------------------------------ 1. hand cases
@pytest.mark.parametrize("k", [18, 21, 30, 31])
def test_canonical_counter_equals_fold_on_hand_cases(k):
    recs = R.hand_records() + F.palindrome_records(18) + F.palindrome_records(30)
    bases, offs = R.records_to_arrays(recs)
    want_y, want_c = F.fold_records(bases, offs, k)
    want_c = want_c.astype(np.uint32)
    windows = int(R.count(bases, offs, k)[1].sum())
    if k in (18, 30):
        assert F.is_palindrome(want_y, k).any()
    c, st, got_y, got_c = counted(T.default_params(k=k), [(bases, offs)])
    assert (got_y <= F.rc(got_y, k)).all()
    assert np.array_equal(got_y, want_y) and np.array_equal(got_c, want_c)
    assert st == (windows, len(want_y), int((want_c >= 2).sum()))
    y2, c2 = sorted_pairs(*c.fetch(2))
    assert np.array_equal(y2, want_y[want_c >= 2]) and np.array_equal(c2, want_c[want_c >= 2])
    c.close()


# ------------------------------------------------------------------ 2. tile edges, batches, growth
def test_tile_edges_batches_and_growth_give_the_fold(synth):
    k = 21
    rng = np.random.default_rng(21)
    motifs = ["".join(rng.choice(list("ACGT"), size=n)) for n in (23, 37, 41, 64)]
    motifs += [F.revcomp_text(m) for m in motifs]                 # so that reverse complements repeat across tiles too
    long_rec = "".join(motifs[i] for i in rng.integers(0, len(motifs), size=800))
    assert len(long_rec) >= 3 * 8192 + 100
    sb, so = synth.short_reads(200_000, 30_000, length=150, sub_rate=0.01, n_rate=0.002)
    sb, _ = F.flip_records(sb, so, np.random.default_rng(2))
    shorts = [bytes(sb[int(so[i]):int(so[i + 1])]) for i in range(len(so) - 1)]
    recs = shorts[:1001] + [long_rec.encode()] + shorts[1001:9000] + [long_rec[5000:14000].encode(), b"", b"ACGT"] + shorts[9000:]
    bases, offs = R.records_to_arrays(recs)
    want_y, want_c = F.fold_records(bases, offs, k)
    want_c = want_c.astype(np.uint32)
    windows = int(R.count(bases, offs, k)[1].sum())
    assert len(want_y) > 4 * 0.7 * 65536                          # the hash of the last run really grows
    n = len(recs)
    p = T.default_params(k=k)
    cuts = [0, 1, 2, 1000, 1001, 1002, 9001, 9002, 9004, 22000, n]
    one = counted(p, [(bases, offs)])
    many = counted(p, slices(bases, offs, cuts))
    grown = counted(p, slices(bases, offs, cuts), expected_distinct=1)
    for c, st, y1, c1 in (one, many, grown):
        assert st == (windows, len(want_y), int((want_c >= 2).sum()))
        assert np.array_equal(y1, want_y) and np.array_equal(c1, want_c)
        c.close()


# ------------------------------------------------------------------ 3. strand-mixed short reads: the table
def build_both(m, p):
    c = T.KmerCounter(p, 0, both_strands=True)
    c.add(m.bases, m.offs)
    t = c.build_table()
    c.close()
    return t


def table_answers(t, m, rng_seed=3):
    """len, build_stats, and the lookups / next_counts test 3 compares (the queries depend on m alone)."""
    rng = np.random.default_rng(rng_seed)
    absent = rng.integers(0, 1 << 42, size=100_000, dtype=np.uint64)
    q = np.concatenate([m.km, F.rc(m.km, 21), m.dk, F.rc(m.dk, 21), absent])
    sample = rng.choice(m.km, size=20_000)
    t.upload(0)
    out = [len(t), t.lookup(q)]
    for direction in (0, 1):
        out.append(t.next_counts(sample, direction))
    return out


def same_answers(a, b):
    if a[0] != b[0]:
        return False
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a[1:], b[1:]))


def test_table_of_strand_mixed_reads_equals_table_of_the_expanded_fold(mixed):
    m = mixed
    assert len(m.boundary) >= 10_000
    assert len(m.km) == 2 * int((m.c >= 2).sum())                 # K is odd: no palindrome
    p = T.default_params(k=21)
    mine = build_both(m, p)
    ref = T.Table.from_arrays(m.km, m.ct, p, device=0)
    assert len(mine) == len(ref) == len(m.km)
    assert list(mine.build_stats) == [len(m.y), len(m.km), 0]
    got, want = table_answers(mine, m), table_answers(ref, m)
    assert same_answers(got, want)
    # every stored k-mer answers with its folded count, on either strand
    assert np.array_equal(got[1][0][:len(m.km)], m.ct) and np.array_equal(got[1][0][len(m.km):2 * len(m.km)], m.ct)
    # the directional counter's table does not know the k-mers that have half their support on each strand
    cd = T.KmerCounter(p, 0)
    cd.add(m.bases, m.offs)
    plain = cd.build_table()
    cd.close()
    plain.upload(0)
    assert (plain.lookup(m.boundary)[0] == 0).all()
    assert (mine.lookup(m.boundary)[0] >= 2).all()
    assert len(plain) < len(mine)


def test_from_arrays_both_strands_equals_the_counter_route(mixed):
    m = mixed
    p = T.default_params(k=21)
    t = T.Table.from_arrays(m.dk, m.dc, p, device=0, both_strands=True)      # the directional counts, folded
    ref = T.Table.from_arrays(m.km, m.ct, p, device=0)
    assert same_answers(table_answers(t, m), table_answers(ref, m))


# ------------------------------------------------------------------ 4. add_counts
def test_add_counts_folds_sums_and_refuses_overflow():
    k = 30
    rng = np.random.default_rng(30)
    x = rng.integers(0, 1 << 60, size=400, dtype=np.uint64)
    x = x[~F.is_palindrome(x, k)]
    pal = np.uint64(F.pack_text("ACGTTGCAAGGCTTA" + F.revcomp_text("ACGTTGCAAGGCTTA")))
    assert F.is_palindrome(pal, k)
    km = np.concatenate([x, F.rc(x[:200], k), x[:50], [pal, pal], x[300:320]]).astype(np.uint64)
    ct = rng.integers(1, 9, size=len(km)).astype(np.uint32)
    ct[-20:] = 0                                                   # zero counts of k-mers that ARE there ...
    km = np.concatenate([km, rng.integers(0, 1 << 60, size=10, dtype=np.uint64)])
    ct = np.concatenate([ct, np.zeros(10, dtype=np.uint32)])       # ... and of k-mers that are not: no slot
    order = rng.permutation(len(km))
    km, ct = km[order], ct[order]
    want_y, want_c = F.fold(km, ct, k)
    nz = ct > 0
    du, dinv = np.unique(km[nz], return_inverse=True)
    dsum = np.zeros(len(du), dtype=np.uint64)
    np.add.at(dsum, dinv, ct[nz].astype(np.uint64))
    pal_at = int(np.searchsorted(want_y, pal))
    assert want_y[pal_at] == pal and want_c[pal_at] == int(ct[km == pal].sum())
    p = T.default_params(k=k)
    half = len(km) // 3
    for both, wy, wc in ((True, want_y, want_c), (False, du, dsum)):
        c = T.KmerCounter(p, 0, both_strands=both)
        c.add_counts(km[:half], ct[:half])
        c.add_counts(km[half:], ct[half:])
        assert c.stats() == (int(nz.sum()), len(wy), int((wc >= 2).sum()))
        gy, gc = sorted_pairs(*c.fetch(1))
        assert np.array_equal(gy, wy) and np.array_equal(gc, wc.astype(np.uint32))
        if both:                                                   # the table stores the palindrome once
            ek, ec = F.expand(wy, wc, k, min_count=2)
            assert len(ek) == 2 * int((wc >= 2).sum()) - 1
            t = c.build_table()
            assert len(t) == len(ek) and list(t.build_stats) == [len(wy), len(ek), 0]
            t.upload(0)
            assert np.array_equal(t.lookup(ek)[0], ec)
            t.close()
        c.close()
    # windows and entries into one counter
    bases, offs = R.records_to_arrays(F.palindrome_records(30))
    ry, rcnt = F.fold_records(bases, offs, k)
    my, mc = F.fold(np.concatenate([km, ry]), np.concatenate([ct.astype(np.uint64), rcnt]), k)
    c = T.KmerCounter(p, 0, both_strands=True)
    c.add_counts(km[:half], ct[:half])
    c.add(bases, offs)
    with pytest.raises(T.TalcError, match=ERR_STATE):
        c.set_both_strands(False)
    c.add_counts(km[half:], ct[half:])
    gy, gc = sorted_pairs(*c.fetch(1))
    assert np.array_equal(gy, my) and np.array_equal(gc, mc.astype(np.uint32))
    assert c.stats()[0] == int(nz.sum()) + int(R.count(bases, offs, k)[1].sum())
    with pytest.raises(T.TalcError, match=ERR_INVALID):
        c.add_counts(np.array([1 << 60], dtype=np.uint64), np.array([1], dtype=np.uint32))     # wider than 2 K bits
    c.close()
    # 0xFFFFFFFF + 1 over the two strands: refused at every synchronising call, never wrapped
    for order in ((0, 1), (1, 0)):
        pair_k = np.array([x[0], F.rc(x[0], k)], dtype=np.uint64)[list(order)]
        pair_c = np.array([0xFFFFFFFF, 1], dtype=np.uint32)[list(order)]
        c = T.KmerCounter(p, 0, both_strands=True)
        c.add_counts(pair_k, pair_c)
        with pytest.raises(T.TalcError, match=ERR_INVALID):
            c.stats()
        with pytest.raises(T.TalcError, match=ERR_INVALID):
            c.fetch(1)
        with pytest.raises(T.TalcError, match=ERR_INVALID):
            c.build_table()
        c.close()
    c = T.KmerCounter(p, 0)                                        # the same two entries are fine on a directional counter
    c.add_counts(pair_k, pair_c)
    assert c.stats() == (2, 2, 1)
    with pytest.raises(T.TalcError, match=ERR_STATE):
        c.set_both_strands(True)
    c.close()


# ------------------------------------------------------------------ 5. the dump route
def split_dump(n_kmers, k, seed):
    """Lines of a count file whose k-mers come in a random orientation, some with their count split over both: (kmers,
    counts) in file order."""
    rng = np.random.default_rng(seed)
    y = np.unique(F.canon(rng.integers(0, 1 << (2 * k), size=n_kmers, dtype=np.uint64), k))
    c = rng.integers(1, 60, size=len(y)).astype(np.uint32)
    turned = np.where(rng.random(len(y)) < 0.5, y, F.rc(y, k))
    split = (rng.random(len(y)) < 0.1) & (c >= 2)
    first = np.where(split, rng.integers(1, np.maximum(c, 2)), c).astype(np.uint32)      # 1 .. c - 1 where split
    km = np.concatenate([turned, F.rc(turned[split], k)])
    ct = np.concatenate([first, (c - first)[split]])
    o = rng.permutation(len(km))
    return km[o], ct[o]


@pytest.mark.parametrize("n_kmers,big", [(50_000, False), (380_000, True)], ids=["host-tokeniser", "device-parser"])
def test_dump_folded_on_the_device_equals_the_folded_dump(tmp_path, n_kmers, big):
    k = 18
    km, ct = split_dump(n_kmers, k, 18 + n_kmers)
    want_y, want_c = F.fold(km, ct, k)
    assert (ct == 1).any() and len(km) > len(want_y)               # some k-mers reach MIN_COUNT only as a sum
    ek, ec = F.expand(want_y, want_c, k, min_count=1)
    stored = int((ec >= 2).sum())
    rng = np.random.default_rng(5)
    jk = rng.choice(ek[ec >= 2], size=3000, replace=False)
    jc = rng.integers(1, 50, size=len(jk))
    raw, folded, junc = str(tmp_path / "raw.dump"), str(tmp_path / "folded.dump"), str(tmp_path / "junc.dump")
    R.write_dump(raw, km, ct, k)
    R.write_dump(folded, ek, ec, k)
    R.write_dump(junc, jk, jc, k)
    assert (os.path.getsize(raw) > (8 << 20)) == big
    if big:
        assert os.path.getsize(raw) < (9 << 20)
    absent = rng.integers(0, 1 << (2 * k), size=50_000, dtype=np.uint64)
    q = np.concatenate([ek, F.rc(ek, k), jk, F.rc(jk, k), absent])
    p = T.default_params(k=k)
    for j in (None, junc):
        mine = T.Table.from_files(raw, j, p, device=0, both_strands=True)
        ref = T.Table.from_files(folded, j, p, device=0)
        assert len(mine) == len(ref) == stored
        assert list(mine.build_stats) == [len(km), stored, 0]
        mine.upload(0)
        ref.upload(0)
        a, b = mine.lookup(q), ref.lookup(q)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[0][:len(ek)], np.where(ec >= 2, ec, 0))
        assert (a[1] > 0).any() == (j is not None)
        mine.close()
        ref.close()


# ------------------------------------------------------------------ 6. correction
@pytest.fixture(scope="module")
def deep_tables(deep):
    p = T.default_params(k=21)
    mine = build_both(deep, p)
    ref = T.Table.from_arrays(deep.km, deep.ct, p, device=0)
    return p, mine, ref


def test_correction_identical_on_both_tables(synth, deep_tables):
    p, mine, ref = deep_tables
    bases, offs = synth.reads(0, 300)
    mine.upload(0)
    ref.upload(0)
    outs = []
    for t in (mine, ref):
        ctx = T.Context(t, p, 0)
        recs, oo, st = ctx.correct(bases, offs)
        outs.append((recs.tobytes(), oo.tolist(), st.tolist()))
        ctx.close()
    assert outs[0] == outs[1]
    assert outs[0][2].count(T.READ_CORRECTED) > 100


# ------------------------------------------------------------------ 7. the CLI
def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_cli_both_strands_counts_out_and_back(synth, deep, tmp_path):
    b, o = deep.bases, deep.offs
    with open(tmp_path / "mixed.fq", "wb") as f:
        qual = b"I" * 150
        f.write(b"".join(b"@s%d\n" % i + bytes(b[int(o[i]):int(o[i + 1])]) + b"\n+\n" + qual[:int(o[i + 1] - o[i])] + b"\n"
                         for i in range(len(o) - 1)))
    synth.write_fasta(str(tmp_path / "reads.fa"), 0, 60)
    a = run(["reads.fa", "-k", "21", "--SRReads", "mixed.fq", "--both-strands", "--SRCountsOut", "c.txt", "-o", "a"], tmp_path)
    assert a.returncode == 0, a.stderr.decode()
    r = run(["reads.fa", "-k", "21", "-SR", "c.txt", "--both-strands", "-o", "b"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    fa = (tmp_path / "a.fa").read_bytes()
    assert fa == (tmp_path / "b.fa").read_bytes() and fa.count(b">") == 60
    lines = (tmp_path / "c.txt").read_bytes().splitlines()
    keep = deep.c >= 2
    R.write_dump(str(tmp_path / "want.txt"), deep.y[keep], deep.c[keep], 21)
    assert len(lines) == len(set(lines)) and set(lines) == set((tmp_path / "want.txt").read_bytes().splitlines())
    for ln in lines[:2000]:                                       # canonical as text too
        s = ln.split()[0].decode()
        assert s <= F.revcomp_text(s)
    for out in (a, r):
        assert b"Kmers are taken on both strands" in out.stdout and b"directional" not in out.stdout
    assert b"queryMode=memory\nBoth strands? 1\n" in (tmp_path / "a.config.txt").read_bytes()
    assert b"queryMode=memory\nBoth strands? 1\n" in (tmp_path / "b.config.txt").read_bytes()
    plain = run(["reads.fa", "-k", "21", "-SR", "c.txt", "-o", "plain"], tmp_path)
    assert plain.returncode == 0, plain.stderr.decode()
    assert b"Both strands" not in (tmp_path / "plain.config.txt").read_bytes()
    assert b"Kmers are assumed directional" in plain.stdout and b"both strands" not in plain.stdout


# ------------------------------------------------------------------ 8. poison
def test_poisoned_memory_changes_nothing(mixed):
    m = mixed
    p = T.default_params(k=21)
    ref = T.Table.from_arrays(m.km, m.ct, p, device=0)
    want = table_answers(ref, m)
    before = T.guard_report()
    with T.poisoned(0xA5, 4096):
        mine = build_both(m, p)
        stats = list(mine.build_stats)
        got = table_answers(mine, m)
        folded = T.Table.from_arrays(m.dk, m.dc, p, device=0, both_strands=True)
        got2 = table_answers(folded, m)
        mine.close()
        folded.close()
    after = T.guard_report()
    assert stats == [len(m.y), len(m.km), 0]
    assert same_answers(got, want) and same_answers(got2, want)
    assert after["checked"] > before["checked"] and after["violations"] == before["violations"]
