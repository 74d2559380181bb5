"""What follows the search of a correction: the records' offsets, the segment offsets and the totals made on the device
(k_emit_sums, k_emit_offsets), k_pack writing the records in aligned words, the retry path, and the page-locked host arrays
and kept device buffers that one context's batches hand to each other.  Every expected record, status and map comes from the
oracle (tests/oracle_lib.py, tests/corr_map_ref.py), read by read: the oracle corrects a read whatever batch it is in, so a
pool of texts goes through it once per module and the batches are put together from the pool."""
import random

import numpy as np
import pytest

import corr_map_ref as M
import oracle_lib as O
import parity_util as PU
import solidity_ref as S
import strand_ref as R
from memcheck_util import PATTERNS, guards_checked
from talc_amd import lib as T

K = 21
EMIT_READS = 1024                       # reads per block of the offset kernels (kEmitReads, talc_kernels_search.h)
SCAN_SIZES = [0, 1, EMIT_READS - 1, EMIT_READS, EMIT_READS + 1, 2 * EMIT_READS + 1, 4095, 4096, 4097, 8193]
POISON = PATTERNS[1:]                   # (0x00 is the hook's control: what fresh memory reads as anyway)
_pool = {}


def random_text(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def oracle_both(pair, texts):
    """[(records, statuses)] of the oracle with reverse = 0 and 1."""
    bases, offs = PU.pack_reads(texts)
    runs = []
    for reverse in (0, 1):
        p, q = PU.both_params(k=K, reverse=reverse)
        ot = O.OracleTable(q, O.OracleTable.FLAT)
        ot.insert_packed(pair.keys, pair.counts)
        ot.decolour()
        out, oo, st = ot.correct_batch(bases, offs, nthreads=16)
        runs.append((PU.seqs_of(out, oo), np.asarray(st).tolist()))
        ot.close()
    return runs


def pool():
    """A 60 k-k-mer table on GPU 0 and the texts the batches are made of, with the oracle's answers.  `gen`: 64 generator
    reads, every second one reverse complemented.  `filler[L]`: one text of every length used, a piece of a generator read
    below K + 1 bases, random text (no k-mer of the table: the oracle's status says so) from there on."""
    if not _pool:
        pair = PU.Pair(target_kmers=60_000, k=K, seed=62)
        pair.upload(0)
        rng = random.Random(9)
        g = PU.seqs_of(*pair.reads(0, 64))
        gen = [PU.revcomp(s) if i % 2 else s for i, s in enumerate(g)]
        lengths = list(range(0, 73)) + list(range(4090, 4103))
        filler = {n: (g[n % 64][:n] if n <= K else random_text(rng, n)) for n in lengths}
        texts = gen + [filler[n] for n in lengths]
        runs = oracle_both(pair, texts)
        rows = R.rows(texts, K, pair.p.min_count, S.host_lookup(pair.ttab))
        for n in lengths:                                        # the fillers are passed through, by the oracle's word
            i = len(gen) + lengths.index(n)
            for recs, st in runs:
                assert st[i] == (T.READ_SKIPPED_SHORT if n <= K else T.READ_NO_SOLID_KMER) and len(recs[i]) == n, (n, st[i])
        exp = {i: M.expected(pair.otab, texts[i]) for i in range(len(texts)) if i % 2 == 0 or i >= len(gen)}   # (the map: plain contexts only)
        _pool.update(pair=pair, texts=texts, n_gen=len(gen), lengths=lengths, runs=runs, rows=rows, exp=exp)
    return _pool


def want_of(s, way, idx):
    """(records, statuses) the oracle gives the pool texts `idx` under `way`: plain, reverse = 1, or every read in the
    orientation strand_ref chooses."""
    pick = {"plain": lambda i: 0, "reverse": lambda i: 1, "auto": lambda i: int(s["rows"]["reverse"][i])}[way]
    return [s["runs"][pick(i)][0][i] for i in idx], [s["runs"][pick(i)][1][i] for i in idx]


def context(s, way):
    p, _ = PU.both_params(k=K, reverse=1 if way == "reverse" else 0)
    ctx = T.Context(s["pair"].ttab, p, 0)
    if way == "auto":
        ctx.auto_strand(True)
    return ctx


def corrected(ctx, s, idx, with_map=False):
    """(records, offsets, statuses[, segments, segment offsets]) of the pool texts `idx` as one batch."""
    ctx.record_map(with_map)
    b = ctx.batch(*PU.pack_reads([s["texts"][i] for i in idx]))
    try:
        assert b.correct() == 0
        out, oo, st = b.fetch_corrected()
        got = (PU.seqs_of(out, oo), oo.astype(np.int64).tolist(), np.asarray(st).tolist())
        return got + tuple(b.fetch_map()) if with_map else got
    finally:
        b.close()
        ctx.record_map(False)


def offsets_of(recs):
    return [0] + np.cumsum([len(x) for x in recs]).astype(np.int64).tolist()


# ---------------------------------------------------------------- every alignment of a record
def alignment_order(s, way):
    """The pool texts in an order in which the records of sixteen corrected reads start at every residue modulo 8, twice:
    before the j-th of them the fillers are drawn at random until one brings the offset to j mod 8 (the oracle's record
    lengths alone decide); the fillers left over follow, shuffled."""
    rng = random.Random(3)
    recs, st = want_of(s, way, range(len(s["texts"])))
    gen = [i for i in range(s["n_gen"]) if st[i] == T.READ_CORRECTED and recs[i] != s["texts"][i]]
    if way == "auto":                                            # both orientations among the sixteen
        turned = [i for i in gen if s["rows"]["reverse"][i]]
        gen = [x for pair in zip(turned, [i for i in gen if not s["rows"]["reverse"][i]]) for x in pair]
    gen = gen[:16]
    assert len(gen) == 16, (way, len(gen))
    fillers = list(range(s["n_gen"], len(s["texts"])))
    rng.shuffle(fillers)
    order, at = [], 0
    for j, gi in enumerate(gen):
        while at % 8 != j % 8:
            f = next(f for f in fillers if (at + len(recs[f])) % 8 == j % 8 or len(fillers) < 8)
            fillers.remove(f)
            order.append(f)
            at += len(recs[f])
        order.append(gi)
        at += len(recs[gi])
    rng.shuffle(fillers)
    return order + fillers, gen


def check_alignment(s, way, ctx):
    order, gen = alignment_order(s, way)
    assert len(order) <= 600 and sorted(len(s["texts"][i]) for i in order if i >= s["n_gen"]) == s["lengths"]
    recs, st = want_of(s, way, order)
    offs = offsets_of(recs)
    residues = sorted(offs[order.index(g)] % 8 for g in gen)
    assert residues == sorted(list(range(8)) * 2), residues      # by the oracle's records alone
    assert all(st[order.index(g)] == T.READ_CORRECTED for g in gen)
    got = corrected(ctx, s, order)
    assert got[2] == st and got[1] == offs
    bad = [i for i in range(len(order)) if got[0][i] != recs[i]]
    assert not bad, (way, bad[:5], [len(recs[i]) for i in bad[:5]], [offs[i] % 8 for i in bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["plain", "reverse", "auto"])
def test_records_at_every_alignment_equal_the_oracle(way):
    s = pool()
    ctx = context(s, way)
    try:
        check_alignment(s, way, ctx)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("byte", POISON, ids=lambda b: "0x%02X" % b)
@pytest.mark.parametrize("way", ["plain", "reverse", "auto"])
def test_records_at_every_alignment_on_a_poisoned_context(way, byte):
    s = pool()
    with guards_checked():
        with T.poisoned(byte):
            ctx = context(s, way)
            try:
                check_alignment(s, way, ctx)
            finally:
                ctx.close()


# ---------------------------------------------------------------- short corrected reads of consecutive lengths, reads with N
_short = {}


def short_set(way):
    """160 pieces of 200 .. 359 bases of generator reads that the oracle corrects under `way` (reverse: of their reverse
    complements, which is what -rev expects), and six such reads with 520 bases of random text with N bases before or behind
    them; the oracle's answers."""
    if way not in _short:
        s = pool()
        rev = way == "reverse"
        src = [t for i, t in enumerate(s["texts"][:s["n_gen"]]) if i % 2 == int(rev) and s["runs"][int(rev)][1][i] == T.READ_CORRECTED]
        assert len(src) >= 16
        texts = [src[j % 16][(7 * j) % 50:(7 * j) % 50 + 200 + j] for j in range(160)]
        rng = random.Random(11)
        for j in range(6):                                       # (an end longer than MAX_BORDER_LEN stays as it is, N bases included)
            junk = "".join("N" if i % 7 == j else c for i, c in enumerate(random_text(rng, 520 + j)))
            texts.append(junk + src[j] if j % 2 else src[j] + junk)
        p, q = PU.both_params(k=K, reverse=int(rev))
        ot = O.OracleTable(q, O.OracleTable.FLAT)
        ot.insert_packed(s["pair"].keys, s["pair"].counts)
        ot.decolour()
        out, oo, st = ot.correct_batch(*PU.pack_reads(texts), nthreads=16)
        ot.close()
        _short[way] = (texts, PU.seqs_of(out, oo), np.asarray(st).tolist())
    return _short[way]


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["plain", "reverse"])
def test_short_corrected_reads_and_reads_with_n_equal_the_oracle(way):
    s = pool()
    texts, recs, st = short_set(way)
    offs = offsets_of(recs)
    # by the oracle alone: corrected records start at every residue modulo 4 with every length modulo 4 (a record's first
    # bytes and the shift of its source words), and corrected records hold N bases
    pairs = {(offs[i] % 4, len(recs[i]) % 4) for i in range(160) if st[i] == T.READ_CORRECTED}
    assert len(pairs) == 16, sorted(pairs)
    with_n = [i for i in range(160, len(texts)) if st[i] == T.READ_CORRECTED and "N" in recs[i]]
    assert len(with_n) >= 3, [(st[i], recs[i].count("N")) for i in range(160, len(texts))]
    ctx = context(s, way)
    try:
        b = ctx.batch(*PU.pack_reads(texts))
        try:
            assert b.correct() == 0
            out, oo, got_st = b.fetch_corrected()
        finally:
            b.close()
    finally:
        ctx.close()
    assert np.asarray(got_st).tolist() == st and oo.astype(np.int64).tolist() == offs
    got = PU.seqs_of(out, oo)
    bad = [i for i in range(len(texts)) if got[i] != recs[i]]
    assert not bad, (way, bad[:5])


# ---------------------------------------------------------------- the offset kernels at their block edges
def scan_batch(s, n):
    """n pool texts: fillers of 0 .. 40 bases, every 50th read a corrected one (forward generator reads, in turn)."""
    fwd = [i for i in range(0, s["n_gen"], 2) if s["runs"][0][1][i] == T.READ_CORRECTED]
    fill = {L: s["n_gen"] + s["lengths"].index(L) for L in range(41)}
    return [fwd[(r // 50) % len(fwd)] if r % 50 == 49 else fill[(r * 7) % 41] for r in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_offsets_and_totals_at_the_scan_block_edges(n):
    s = pool()
    idx = scan_batch(s, n)
    recs, st = want_of(s, "plain", idx)
    offs = offsets_of(recs)
    ctx = context(s, "plain")
    try:
        got = corrected(ctx, s, idx)
        assert got[1] == offs and got[2] == st and got[0] == recs
        assert ctx.timing().n_retried == 0 and ctx.timing().n_failed == 0
        got = corrected(ctx, s, idx, with_map=True)
        assert got[1] == offs and got[2] == st and got[0] == recs
        segs, so = got[3], got[4].astype(np.int64).tolist()
        exp = [s["exp"][i] for i in idx]
        assert so == [0] + np.cumsum([len(e["segs"]) for e in exp]).astype(np.int64).tolist()
        n_corrected = 0
        for r, e in enumerate(exp):
            if e["status"] == T.READ_CORRECTED:
                n_corrected += 1
                assert np.array_equal(segs[so[r]:so[r + 1]], M.as_array(e["segs"])), (n, r)
        assert n_corrected == n // 50
        if n:                                                    # every other read: one RAW segment over the whole record
            first = segs[np.asarray(so[:-1])]
            plain = np.array([e["status"] != T.READ_CORRECTED for e in exp])
            assert (first["kind"][plain] == T.SEG_RAW).all() and (first["out_len"][plain] == np.diff(offs)[plain]).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------- the retry path
_retry = {}


def retry_inputs():
    if not _retry:
        pair = PU.Pair(target_kmers=60_000, k=K, seed=77, synth_kw=dict(paralog_frac=0.6, paralog_div=0.04))
        pair.ttab.upload(0)
        bases, offs = pair.reads(0, 200)
        out, oo, st = pair.otab.correct_batch(bases, offs, nthreads=16)
        _retry.update(pair=pair, bases=bases, offs=offs, recs=PU.seqs_of(out, oo), oo=np.asarray(oo).astype(np.int64).tolist(),
                      st=np.asarray(st).tolist())
    return _retry


def check_retry(s, monkeypatch):
    pair = s["pair"]
    plain = T.Context(pair.ttab, pair.p, 0)
    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "1")
    tiny = T.Context(pair.ttab, pair.p, 0)                       # (a context reads the switches when it is created)
    monkeypatch.delenv("TALC_TEST_TINY_CAPS")
    try:
        out, oo, st = plain.correct(s["bases"], s["offs"])
        assert plain.timing().n_retried == 0
        assert PU.seqs_of(out, oo) == s["recs"] and oo.astype(np.int64).tolist() == s["oo"] and np.asarray(st).tolist() == s["st"]
        b = tiny.batch(s["bases"], s["offs"])
        try:
            for rep in range(2):                                 # (the same batch corrected a second time)
                assert b.correct() == 0
                t = tiny.timing()
                assert t.n_retried > 0 and t.n_failed == 0, (rep, t.n_retried, t.n_failed)
                out, oo, st = b.fetch_corrected()
                assert PU.seqs_of(out, oo) == s["recs"] and oo.astype(np.int64).tolist() == s["oo"] and np.asarray(st).tolist() == s["st"], rep
        finally:
            b.close()
    finally:
        tiny.close()
        plain.close()


@pytest.mark.gpu
def test_a_batch_that_retries_equals_a_plain_context_and_the_oracle(monkeypatch):
    check_retry(retry_inputs(), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("byte", POISON, ids=lambda b: "0x%02X" % b)
def test_a_batch_that_retries_on_poisoned_contexts(byte, monkeypatch):
    s = retry_inputs()
    with guards_checked():
        with T.poisoned(byte):
            check_retry(s, monkeypatch)


# ---------------------------------------------------------------- one context, batches that take each other's arrays
@pytest.mark.gpu
def test_batches_of_one_context_in_turn_reuse_its_arrays(monkeypatch, capfd):
    pair = retry_inputs()["pair"]
    bases, offs = pair.reads(200, 500)
    reads = PU.seqs_of(bases, offs)
    out, oo, st = pair.otab.correct_batch(bases, offs, nthreads=16)
    recs, st = PU.seqs_of(out, oo), np.asarray(st).tolist()
    assert st.count(T.READ_CORRECTED) >= 300
    monkeypatch.setenv("TALC_TIMING", "1")                       # (read when the context is created: one line per correction)
    ctx = T.Context(pair.ttab, pair.p, 0)
    monkeypatch.delenv("TALC_TIMING")
    try:
        for a, e in ((0, 300), (300, 320), (0, 500), (0, 300)):
            got_out, got_oo, got_st = ctx.correct(*PU.pack_reads(reads[a:e]))      # (created, corrected, fetched, destroyed)
            assert PU.seqs_of(got_out, got_oo) == recs[a:e] and np.asarray(got_st).tolist() == st[a:e], (a, e)
            assert got_oo.astype(np.int64).tolist() == offsets_of(recs[a:e]), (a, e)
        # on a machine with a GPU the arrays the copies land in are page-locked, not the pageable fall-back
        lines = [x for x in capfd.readouterr().err.splitlines() if "host arrays page-locked" in x]
        assert len(lines) == 4 and all(x.endswith("states 1, offsets 1, landing area 1") for x in lines), lines
    finally:
        ctx.close()
