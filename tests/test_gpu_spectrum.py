"""The k-mer spectrum on the GPU (k_count_histo, k_table_histo, talc_counter_histo, talc_table_histo, talc_counter_set_min_count,
`talc --SRHisto / --AutoMinCount`) against the numpy contract (tests/spectrum_ref.py, docs/kmer_spectrum.md).  Every
comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import fold_ref as F
import kmer_ref as R
import spectrum_ref as S
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
HIGHS = [2, 3, 100, 0, 16382]          # 0: the default, 10000


def real(high):
    return high or 10000


def sorted_pairs(kmers, counts):
    o = np.argsort(kmers, kind="stable")
    return kmers[o], counts[o]


def check(counter, counts, highs=HIGHS):
    """histo() of the counter at every high against the reference of `counts`"""
    distinct = counter.stats()[1]
    for high in highs:
        hist, stats = counter.histo(high)
        want, wstats = S.histo(counts, real(high))
        assert hist.dtype == np.uint64 and len(hist) == real(high) + 2
        assert np.array_equal(hist, want), (high, np.nonzero(hist != want)[0][:10])
        assert stats == wstats, high
        assert int(hist.sum()) == stats[0] == distinct == len(counts)


# ------------------------------------------------------------------ planted counts
def planted():
    """(kmers, counts): every count 1 .. 40 with multiplicities from 1 to several hundred (both sides of the register / LDS
    split whatever it is), 5 000 k-mers of count 100 (whole waves on one LDS bin), and the counts high, high + 1, 2 high of
    every high of HIGHS, and 2^32 - 1."""
    rng = np.random.default_rng(40)
    counts = []
    for c in range(1, 41):
        counts += [c] * (1 + (c * 89) % 397 if c % 5 else c // 5)        # 1 (count 5) .. 393
    counts += [100] * 5000
    for high in HIGHS:
        counts += [real(high), real(high) + 1, 2 * real(high)]
    counts.append(0xFFFFFFFF)
    counts = np.array(counts, dtype=np.uint32)
    mult = np.bincount(counts[counts <= 40], minlength=41)[1:]
    assert mult.min() == 1 and mult.max() > 300 and 5000 < len(counts) < 0.7 * 65536
    kmers = np.unique(rng.integers(0, 1 << 42, size=2 * len(counts), dtype=np.uint64))[:len(counts)]
    assert len(kmers) == len(counts)
    order = rng.permutation(len(counts))
    return rng.permutation(kmers), counts[order]


def planted_counter():
    kmers, counts = planted()
    c = T.KmerCounter(T.default_params(k=21), 0)         # 2^16 slots, and it stays there
    half = len(kmers) // 2
    c.add_counts(kmers[:half], counts[:half])
    c.add_counts(kmers[half:], counts[half:])
    return c, kmers, counts


def test_planted_counts_at_every_high():
    c, kmers, counts = planted_counter()
    check(c, counts)
    check(c, counts, [100])                              # any number of times
    k1, c1 = sorted_pairs(*c.fetch(1))                   # and nothing was disturbed
    wk, wc = sorted_pairs(kmers, counts)
    assert np.array_equal(k1, wk) and np.array_equal(c1, wc)
    assert c.histo_timing() > 0
    c.close()


def test_empty_counter_is_all_zero():
    c = T.KmerCounter(T.default_params(k=21), 0)
    for high in HIGHS:
        hist, stats = c.histo(high)
        assert len(hist) == real(high) + 2 and not hist.any() and stats == (0, 0, 0, 0)
    c.close()


@pytest.mark.parametrize("k", [18, 21, 31])
def test_hand_records(k):
    bases, offs = R.records_to_arrays(R.hand_records())
    _, want_c = R.count(bases, offs, k)
    c = T.KmerCounter(T.default_params(k=k), 0)
    c.add(bases, offs)
    check(c, want_c, [2, 7, 8, 9, 0])
    c.close()


@pytest.mark.parametrize("byte", [0xA5, 0x00])
def test_poisoned_memory_changes_no_bin(byte):
    before = T.guard_report()
    with T.poisoned(byte):
        c, _, counts = planted_counter()
        check(c, counts)
        c.close()
    after = T.guard_report()
    assert after["violations"] == before["violations"] and after["checked"] > before["checked"]


# ------------------------------------------------------------------ counted reads
@pytest.fixture(scope="module")
def synth77():
    return Synth(target_kmers=150_000, k=21, seed=77)


def slices(bases, offsets, cuts):
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(offsets[a]), int(offsets[b])
        out.append((bases[lo:hi], offsets[a:b + 1] - offsets[a]))
    return out


def test_batches_and_growth_give_the_same_spectrum(synth77):
    bases, offs = synth77.short_reads(200_000, 30_000, length=150, sub_rate=0.01, n_rate=0.002)
    want_k, want_c = R.count(bases, offs, 21)
    want = S.histo(want_c, 10000)
    p = T.default_params(k=21)
    n = len(offs) - 1
    cuts = [0, 1, 2, 1000, 1001, 9000, 22000, n]
    for chunks, hint in (([(bases, offs)], 0), (slices(bases, offs, cuts), 0), (slices(bases, offs, cuts), 1)):
        c = T.KmerCounter(p, 0, hint)
        seen = 0
        for i, (b, o) in enumerate(chunks):
            c.add(b, o)
            hist, stats = c.histo()                      # between adds as well: the spectrum of what is in so far
            assert int(hist.sum()) == stats[0] >= seen and (stats[2], stats[0]) == c.stats()[:2]
            seen = stats[0]
        hist, stats = c.histo()
        assert np.array_equal(hist, want[0]) and stats == want[1]
        assert stats[0] > 4 * 65536 * 0.7                # (so the run that started small really grew)
        k1, c1 = sorted_pairs(*c.fetch(1))               # not spent, nothing disturbed
        assert np.array_equal(k1, want_k) and np.array_equal(c1, want_c)
        assert c.stats() == (int(want_c.sum()), len(want_k), int((want_c >= 2).sum()))
        c.close()


def test_both_strands_spectrum_is_that_of_the_folded_counts(synth77):
    k = 18
    bases, offs = synth77.short_reads(0, 3000, length=150, sub_rate=0.005, n_rate=0.001)
    flipped, flip = F.flip_records(bases, offs, np.random.default_rng(3))
    assert 1000 < flip.sum() < 2000
    hb, ho = R.records_to_arrays(R.hand_records() + F.palindrome_records(k))
    p = T.default_params(k=k)
    c = T.KmerCounter(p, 0, both_strands=True)
    c.add(flipped, offs)
    c.add(hb, ho)
    y1, c1 = F.fold_records(flipped, offs, k)
    y2, c2 = F.fold_records(hb, ho, k)
    wy, wc = F.fold(np.concatenate([y1, y2]), np.concatenate([c1, c2]), k)
    assert F.is_palindrome(wy, k).any()
    check(c, wc, [2, 50, 0])
    # its table stores both strands of every kept k-mer (a palindrome once): both are counted
    table = c.build_table()
    _, ec = F.expand(wy, wc, k, min_count=2)
    hist, stats = table.histo(0, 50)
    want, wstats = S.histo(ec, 50)
    assert np.array_equal(hist, want) and stats == wstats and stats[0] == len(table)
    table.close()
    c.close()


def test_a_spent_counter_has_no_spectrum():
    c, _, _ = planted_counter()
    t = c.build_table()
    with pytest.raises(T.TalcError, match="error -6"):       # TALC_ERR_STATE
        c.histo()
    with pytest.raises(T.TalcError, match="error -6"):
        c.set_min_count(3)
    t.close()
    c.close()


# ------------------------------------------------------------------ MIN_COUNT from the spectrum, and the table's spectrum
@pytest.fixture(scope="module")
def synth5():
    return Synth(target_kmers=20_000, k=21, seed=5)


@pytest.fixture(scope="module")
def short5(synth5):
    bases, offs = synth5.short_reads(0, 20_000, length=150, sub_rate=0.01, n_rate=0.001)
    want_k, want_c = R.count(bases, offs, 21)
    hist, _ = S.histo(want_c, 10000)
    chosen, valley = S.threshold(hist, 10000)
    assert chosen == valley >= 3                          # (7 on the CPU: nothing below passes by the default of 2)
    return bases, offs, want_k, want_c, chosen


@pytest.fixture(scope="module")
def chosen_table(short5):
    """the counter's table after set_min_count(chosen), staged on GPU 0, and what led to it"""
    bases, offs, want_k, want_c, want_chosen = short5
    p = T.default_params(k=21)
    c = T.KmerCounter(p, 0)
    c.add(bases, offs)
    hist, stats = c.histo()
    chosen, valley = T.spectrum_threshold(hist)
    before = c.stats()
    c.set_min_count(chosen)
    after = c.stats()
    table = c.build_table()
    c.close()
    return dict(p=p, hist=hist, stats=stats, chosen=chosen, valley=valley, before=before, after=after, table=table, counter_params=c.params)


def test_set_min_count_takes_the_value_the_spectrum_suggests(short5, chosen_table):
    _, _, want_k, want_c, want_chosen = short5
    g = chosen_table
    want_hist, want_stats = S.histo(want_c, 10000)
    assert np.array_equal(g["hist"], want_hist) and g["stats"] == want_stats
    assert (g["chosen"], g["valley"]) == (want_chosen, want_chosen) and g["chosen"] >= 3
    chosen, table = g["chosen"], g["table"]
    assert g["before"] == (int(want_c.sum()), len(want_k), int((want_c >= 2).sum()))
    assert g["after"] == (int(want_c.sum()), len(want_k), int((want_c >= chosen).sum()))
    assert len(table) == int((want_c >= chosen).sum()) and list(table.build_stats) == [len(want_k), len(table), 0]
    # the counter got its own copy of the parameters, the table carries it
    assert g["p"].min_count == 2 and g["counter_params"].min_count == chosen and table.params.min_count == chosen


def test_table_spectrum_staged_and_uploaded_and_correction_on_it(synth5, short5, chosen_table):
    _, _, want_k, want_c, _ = short5
    chosen, table = chosen_table["chosen"], chosen_table["table"]
    kept = want_c[want_c >= chosen]
    staged = {h: table.histo(0, h) for h in (2, 100, 0)}            # before upload(0): the image is staged
    table.upload(0)
    for high in (2, 100, 0):                                        # after: the in-degree bits sit in the RIGHT keys
        want, wstats = S.histo(kept, real(high))
        for hist, stats in (staged[high], table.histo(0, high)):
            assert np.array_equal(hist, want) and stats == wstats and stats[0] == len(table)
    below, at = want_k[want_c == chosen - 1], want_k[want_c == chosen]
    assert len(below) and len(at)
    assert not table.lookup(below)[0].any() and (table.lookup(at)[0] == chosen).all()
    # 200 long reads: the same records and statuses as on a table built from the reference counts with that MIN_COUNT
    pc = T.default_params(k=21, min_count=chosen)
    ref = T.Table.from_arrays(want_k, want_c, pc, device=0)
    ref.upload(0)
    bases, offs = synth5.reads(0, 200)
    outs = []
    for t, params in ((table, table.params), (ref, pc)):
        ctx = T.Context(t, params, 0)
        recs, oo, st = ctx.correct(bases, offs)
        outs.append((recs.tobytes(), oo.tolist(), st.tolist()))
        ctx.close()
    assert outs[0] == outs[1]
    assert outs[0][2].count(T.READ_CORRECTED) > 50
    ref.close()


def test_a_table_without_a_device_image_has_no_spectrum(short5):
    _, _, want_k, want_c, chosen = short5
    host = T.Table.from_arrays(want_k, want_c, T.default_params(k=21, min_count=chosen))
    with pytest.raises(T.TalcError, match="error -6"):
        host.histo(0)
    host.upload(0)                                                  # a host-built table, once it is on the device
    hist, stats = host.histo(0, 100)
    want, wstats = S.histo(want_c[want_c >= chosen], 100)
    assert np.array_equal(hist, want) and stats == wstats
    host.close()


# ------------------------------------------------------------------ the CLI
def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def outputs(prefix):
    """the run's files (None for one it did not write: <o>.log only exists once a read was logged)"""
    out = {}
    for ext in (".fa", ".log", ".stats_basics.txt"):
        out[ext] = open(prefix + ext, "rb").read() if os.path.exists(prefix + ext) else None
    assert out[".fa"]
    return out


@pytest.fixture(scope="module")
def clidata(synth5, short5, tmp_path_factory):
    bases, offs, _, _, _ = short5
    d = tmp_path_factory.mktemp("spectrum")
    synth5.write_fasta(str(d / "reads.fa"), 0, 60)
    with open(d / "sr.fa", "wb") as f:
        for i in range(len(offs) - 1):
            f.write(b">s%d\n" % i + bytes(bases[int(offs[i]):int(offs[i + 1])]) + b"\n")
    plain = run([str(d / "reads.fa"), "-k", "21", "--SRReads", str(d / "sr.fa"), "-o", "plain"], d)
    assert plain.returncode == 0, plain.stderr.decode()
    return d, plain


def test_cli_srhisto_writes_the_spectrum_and_changes_nothing_else(clidata, short5):
    d, plain = clidata
    _, _, _, want_c, _ = short5
    a = run([str(d / "reads.fa"), "-k", "21", "--SRReads", str(d / "sr.fa"), "--SRHisto", "-o", "a"], d)
    assert a.returncode == 0, a.stderr.decode()
    hist, stats = S.histo(want_c, 10000)
    assert (d / "a.histo.txt").read_bytes() == S.histo_text(hist)
    line = b"[TALC]: k-mer spectrum: %d distinct, %d unique, %d total, max %d\n" % stats
    assert a.stdout.count(line) == 1
    rest = [ln.replace(b"a.fa", b"plain.fa") if ln.startswith(b"Specified output") else ln for ln in a.stdout.replace(line, b"").splitlines()]
    assert rest == plain.stdout.splitlines()
    assert outputs(str(d / "a")) == outputs(str(d / "plain"))
    assert not (d / "plain.histo.txt").exists()
    # a smaller high: the last line gathers what lies above it
    b = run([str(d / "reads.fa"), "-k", "21", "--SRReads", str(d / "sr.fa"), "--SRHisto", "--SRHistoHigh", "5", "-o", "h5"], d)
    assert b.returncode == 0, b.stderr.decode()
    assert (d / "h5.histo.txt").read_bytes() == S.histo_text(S.histo(want_c, 5)[0])
    assert (d / "h5.histo.txt").read_bytes().splitlines()[-1].startswith(b"6 ")


def test_cli_auto_min_count_equals_the_run_with_that_min_count(clidata, short5):
    d, plain = clidata
    _, _, want_k, want_c, chosen = short5
    b = run([str(d / "reads.fa"), "-k", "21", "--SRReads", str(d / "sr.fa"), "--AutoMinCount", "--SRCountsOut", "b.dump", "-o", "b"], d)
    m = run([str(d / "reads.fa"), "-k", "21", "--SRReads", str(d / "sr.fa"), "--MIN_COUNT", str(chosen), "-o", "m"], d)
    assert b.returncode == 0 and m.returncode == 0, (b.stderr.decode(), m.stderr.decode())
    assert b"[TALC]: MIN_COUNT from the k-mer spectrum: %d (first minimum at %d)\n" % (chosen, chosen) in b.stdout
    assert outputs(str(d / "b")) == outputs(str(d / "m"))
    assert (d / "b.fa").read_bytes() != (d / "plain.fa").read_bytes()          # (the choice matters on this data)
    assert b"MIN_SR_COUNT=2" in (d / "b.config.txt").read_bytes().splitlines()    # the config keeps the given value
    assert not (d / "b.histo.txt").exists()
    keep = want_c >= chosen
    R.write_dump(str(d / "want.dump"), want_k[keep], want_c[keep], 21)
    got = (d / "b.dump").read_bytes().splitlines()
    assert len(got) == len(set(got)) == int(keep.sum()) and set(got) == set((d / "want.dump").read_bytes().splitlines())


def test_cli_auto_min_count_without_a_valley_keeps_the_given_value(clidata):
    d, _ = clidata
    rng = np.random.default_rng(9)
    (d / "once.fa").write_text(">x\n" + "".join(rng.choice(list("ACGT"), size=300)) + "\n")
    r = run([str(d / "reads.fa"), "-k", "21", "--SRReads", "once.fa", "--AutoMinCount", "--SRHisto", "--MIN_COUNT", "4", "-o", "once"], d)
    assert b"[TALC]: MIN_COUNT from the k-mer spectrum: 4 (no minimum up to 32; the given value stands)\n" in r.stdout, (r.stdout, r.stderr)
    assert r.returncode == 1 and b"The de Bruijn Graph is empty" in r.stdout          # every k-mer was seen once
    assert (d / "once.histo.txt").read_bytes() == b"1 280\n"
