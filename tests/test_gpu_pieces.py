"""Trimmed and split output on the device (docs/trim_split.md; k_piece_count, k_piece_pack) against the numpy contract
(tests/pieces_ref.py) fed with the same batch's map and records — which tests/test_gpu_corr_map.py pins to the oracle —
and, for one set, with the map rebuilt from the oracle's trace.  All comparisons are integers and bytes."""
import contextlib
import os
import random
import subprocess

import numpy as np
import pytest

import corr_map_ref as M
import parity_util as PU
import pieces_ref as P
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
MODES = (P.TRIM, P.SPLIT)


def ctx_of(s):
    if s.pair.ctx is None:
        s.pair.upload(0)
    return s.pair.ctx


@contextlib.contextmanager
def corrected(ctx, bases, offs, on=True):
    """A fresh batch, corrected with the map on (or off)."""
    ctx.record_map(on)
    b = ctx.batch(bases, offs)
    try:
        b.rc = b.correct()
        yield b
    finally:
        b.close()
        ctx.record_map(False)


def maps_of(b):
    """What pieces_ref.pieces takes, from the batch itself: segments, their offsets, records, their offsets, masked records."""
    segs, so = b.fetch_map()
    out, oo, st = b.fetch_corrected()
    msk, _, _ = b.fetch_corrected(soft_mask=True)
    return segs, so, out, oo, msk


def same(got, want, what):
    names = ("bytes", "piece_offsets", "pieces", "read_piece_offsets")
    for g, w, n in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), \
            (what, n, g.shape, w.shape, np.nonzero(g != w)[0][:6].tolist() if g.shape == w.shape else None)


def check(b, args, mode, min_len=0, soft=False, what=""):
    got = b.pieces(mode, min_len, soft)
    want = P.pieces(*args[:4], mode, min_len, args[4] if soft else None)
    same(got, want, (what, mode, min_len, soft))
    L = T.lib()
    assert int(L.talc_batch_num_pieces(b._h)) == len(want[2]) and int(L.talc_batch_pieces_bytes(b._h)) == len(want[0])
    return want


def dropping_min_len(args, mode):
    """A min_len from the reference's own piece lengths (the median + 1), and how many pieces it keeps of how many."""
    lens = np.sort(P.pieces(*args[:4], mode)[2]["out_len"])
    ml = int(lens[len(lens) // 2]) + 1
    return ml, int((lens >= ml).sum()), len(lens)


def check_all(b, args, what):
    """Both modes at min_len 0 and at one that drops some pieces and keeps some; trim from the masked records; split with
    soft_mask set, which it ignores."""
    for mode in MODES:
        check(b, args, mode, 0, False, what)
        ml, kept, total = dropping_min_len(args, mode)
        assert 0 < kept < total, (what, mode, ml, kept, total)
        w = check(b, args, mode, ml, False, what)
        assert len(w[2]) == kept
    w = check(b, args, P.TRIM, 0, True, what)
    assert any(c.islower() for c in bytes(w[0]).decode()) == any(len(t) > 1 for t in P.piece_texts(P.pieces(*args[:4], P.SPLIT)))
    check(b, args, P.SPLIT, 0, True, what)


@pytest.mark.parametrize("name", list(M.SETS))
def test_pieces_equal_the_reference(name):
    s = M.map_set(name)
    K = int(s.pair.p.k)
    with corrected(ctx_of(s), *s.packed()) as b:
        args = maps_of(b)
        check_all(b, args, name)
        got = b.pieces(P.SPLIT)
        per_read = np.diff(got[3].astype(np.int64))
        assert int(got[2]["out_len"].min()) >= K and (per_read >= 2).any() and (per_read == 0).any()
        if name == "default":   # ... and against the map rebuilt from the oracle's trace and the oracle's records
            check_all(b, P.from_expected(s.exp), "oracle-derived")


def reads_with_regions(s, targets):
    """Prefixes of the set's comb reads that the oracle corrects with exactly R regions, one per target (2 R + 1 segments):
    R grows by one every K + g bases, so a bisection over the prefix length finds each."""
    out = {}
    for seq in s.reads:
        for R in targets:
            if R in out:
                continue
            lo, hi = 18 * R, min(len(seq), 34 * R)
            while lo < hi:
                mid = (lo + hi) // 2
                e = M.expected(s.pair.otab, seq[:mid])
                if e["R"] >= R:
                    hi = mid
                else:
                    lo = mid + 1
            for ln in range(lo, min(len(seq), lo + 4)):
                e = M.expected(s.pair.otab, seq[:ln])
                if e["status"] == 0 and e["R"] == R:
                    out[R] = seq[:ln]
                    break
        if len(out) == len(targets):
            break
    assert sorted(out) == sorted(targets), sorted(out)
    return [out[R] for R in targets]


@pytest.mark.parametrize("graph", M.COMB_SETS)
def test_pieces_of_reads_with_more_than_64_segments(graph):
    """The comb reads of the map tests (201 - 245 segments) and reads of 63, 65, 127 and 129 segments: where a pass of 64
    segments ends."""
    s = M.comb_set(graph)
    reads = s.reads + reads_with_regions(s, (31, 32, 63, 64))
    with corrected(ctx_of(s), *PU.pack_reads(reads)) as b:
        args = maps_of(b)
        nseg = np.diff(args[1].astype(np.int64)).tolist()
        assert nseg[-4:] == [63, 65, 127, 129] and min(nseg[:-4]) >= 201
        for mode in MODES:
            check(b, args, mode, 0, False, graph)
            lens = P.pieces(*args[:4], mode)[2]["out_len"]
            check(b, args, mode, int(np.median(lens)) + 1, False, graph)
        check(b, args, P.TRIM, 0, True, graph)
        print(graph, "split pieces per read:", np.diff(b.pieces(P.SPLIT)[3].astype(np.int64)).tolist())


def edge_reads(s0):
    r = PU.seqs_of(*s0.pair.reads(5000, 8))
    return ["", r[0][:21], r[0][:22], r[1].lower(), r[2][:400] + "N" + r[2][400:],
            r[3][:300] + "N" * 10 + r[3][300:900] + "RYKM" + r[3][900:], "ACGT" * 300, "A" * 500,
            "".join(random.Random(1).choice("ACGT") for _ in range(1500)), r[4], r[5][:60], r[6] + r[7]]


def test_pieces_of_passed_through_reads_and_of_a_batch_without_a_piece():
    s0 = M.map_set("default")
    ctx = ctx_of(s0)
    reads = edge_reads(s0)
    with corrected(ctx, *PU.pack_reads(reads)) as b:
        args = maps_of(b)
        st = b.fetch_corrected()[2]
        assert st[0] == T.READ_SKIPPED_SHORT and (st == T.READ_NO_SOLID_KMER).any() and (st == T.READ_CORRECTED).any()
        for mode in MODES:
            for ml in (0, 100):
                w = check(b, args, mode, ml, mode == P.TRIM, "edge inputs")
                per_read = np.diff(w[3].astype(np.int64))
                assert all(per_read[i] == 0 for i in range(len(reads)) if st[i] != T.READ_CORRECTED)
        assert len(w[2]) > 0
    nothing = ["", reads[1], "A" * 500, reads[8], "N" * 100]
    with corrected(ctx, *PU.pack_reads(nothing)) as b:
        assert (b.fetch_corrected()[2] != T.READ_CORRECTED).all()
        for mode in MODES:
            data, po, pc, rpo = b.pieces(mode, 0, True)
            assert len(data) == 0 and len(pc) == 0 and po.tolist() == [0] and rpo.tolist() == [0] * (len(nothing) + 1)
            same((data, po, pc, rpo), P.pieces(*maps_of(b)[:4], mode), "no piece")
    with corrected(ctx, *PU.pack_reads([""])) as b:
        assert b.pieces(P.SPLIT)[3].tolist() == [0, 0]


def test_pieces_of_reads_that_failed(monkeypatch):
    """TALC_TEST_TINY_CAPS with TALC_TEST_FAIL_RETRY_ALLOC: reads end as TALC_READ_ERROR, one RAW segment each: no piece."""
    s = M.map_set("default")
    ctx_of(s)
    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "1")
    monkeypatch.setenv("TALC_TEST_FAIL_RETRY_ALLOC", "1")
    ctx2 = T.Context(s.pair.ttab, s.pair.p, 0)
    try:
        with corrected(ctx2, *s.packed()) as b:
            assert b.rc == T.WARN_READ_ERRORS
            args = maps_of(b)
            st = b.fetch_corrected()[2]
            assert (st == T.READ_ERROR).any() and (st == T.READ_CORRECTED).any()
            for mode in MODES:
                w = check(b, args, mode, 0, True, "failed reads")
                per_read = np.diff(w[3].astype(np.int64))
                assert (per_read[st == T.READ_ERROR] == 0).all() and per_read.sum() > 0
    finally:
        ctx2.close()


def test_piece_calls_report_state_and_capacity():
    s = M.map_set("default")
    ctx = ctx_of(s)
    bases, offs = PU.pack_reads(s.reads[:20])
    L = T.lib()
    n_reads = 20
    rpo = np.zeros(n_reads + 1, dtype=np.uint64)

    def fetch(b, out=None, cap=0, po=None, pc=None, pcap=0):
        return L.talc_batch_fetch_pieces(ctx._h, b._h, None if out is None else out.ctypes.data, cap, None if po is None else po.ctypes.data,
                                         None if pc is None else pc.ctypes.data, pcap, rpo.ctypes.data)

    ctx.record_map(True)
    b = ctx.batch(bases, offs)
    try:
        assert L.talc_batch_pieces(ctx._h, b._h, P.SPLIT, 0, 0) == ERR_STATE          # not corrected yet
        assert fetch(b) == ERR_STATE and L.talc_batch_num_pieces(b._h) == 0 and L.talc_batch_pieces_bytes(b._h) == 0
        ctx.record_map(False)
        b.correct()
        assert L.talc_batch_pieces(ctx._h, b._h, P.SPLIT, 0, 0) == ERR_STATE          # corrected without the map
        ctx.record_map(True)
        b.correct()
        assert fetch(b) == ERR_STATE                                                   # talc_batch_pieces has not run
        for mode in (0, 3, -1):
            assert L.talc_batch_pieces(ctx._h, b._h, mode, 0, 0) == ERR_INVALID
        assert fetch(b) == ERR_STATE
        assert L.talc_batch_pieces(ctx._h, b._h, P.SPLIT, 0, 0) == 0
        n, nb = int(L.talc_batch_num_pieces(b._h)), int(L.talc_batch_pieces_bytes(b._h))
        want = P.pieces(*maps_of(b)[:4], P.SPLIT)
        assert n == len(want[2]) > n_reads and nb == len(want[0])
        assert fetch(b) == 0 and np.array_equal(rpo, want[3])                          # offsets only
        po = np.zeros(n + 1, dtype=np.uint64)
        assert fetch(b, po=po) == 0 and np.array_equal(po, want[1])
        out, pc = np.zeros(nb, dtype=np.uint8), np.zeros(n, dtype=T.PIECE_DTYPE)
        assert fetch(b, out, nb - 1, po, pc, n) == ERR_CAPACITY and str(nb).encode() in L.talc_last_error()
        assert fetch(b, out, nb, po, pc, n - 1) == ERR_CAPACITY and str(n).encode() in L.talc_last_error()
        assert fetch(b, out, nb, None, None, 0) == 0 and np.array_equal(out, want[0])
        assert fetch(b, None, 0, None, pc, n) == 0 and np.array_equal(pc, want[2])
        b.correct()                                                                    # a correction forgets the pieces
        assert L.talc_batch_num_pieces(b._h) == 0 and L.talc_batch_pieces_bytes(b._h) == 0 and fetch(b) == ERR_STATE
    finally:
        b.close()
        ctx.record_map(False)


def everything_else(ctx, b):
    segs, so = b.fetch_map()
    out, oo, st = b.fetch_corrected()
    msk, moo, mst = b.fetch_corrected(soft_mask=True)
    raw, cor = b.solidity()
    return dict(segs=segs, so=so, out=out, oo=oo, st=st, msk=msk, moo=moo, mst=mst, raw=raw, cor=cor)


def test_pieces_change_nothing_else_and_a_second_call_replaces_the_first():
    """A run with and a run without talc_batch_pieces: records, statuses, map, masked records, solidity rows and work
    counters are equal; on one batch, every fetch after the calls returns what it returned before them."""
    s = M.map_set("reverse")
    ctx = ctx_of(s)
    bases, offs = PU.pack_reads(s.reads[:120])
    with corrected(ctx, bases, offs) as b:
        t = ctx.timing()
        plain = dict(everything_else(ctx, b), rc=b.rc, work=(t.n_trail_steps, t.n_dp_cells))
    with corrected(ctx, bases, offs) as b:
        args = maps_of(b)
        first = check(b, args, P.SPLIT, 0, False, "first")
        second = check(b, args, P.TRIM, 30, True, "second")          # replaces the first
        assert len(second[2]) < len(first[2])
        data, po, pc, rpo = b.pieces(P.TRIM, 30, True)
        assert (np.diff(rpo.astype(np.int64)) <= 1).all()
        check(b, args, P.SPLIT, 50, True, "third")                   # and back
        t = ctx.timing()
        after = dict(everything_else(ctx, b), rc=b.rc, work=(t.n_trail_steps, t.n_dp_cells))
        check(b, args, P.TRIM, 0, False, "after the solidity report")
        assert all(a >= 0 for a in ctx.pieces_timing())
    assert plain["work"] == after["work"] and plain["work"][0] > 0 and plain["rc"] == after["rc"]
    for k in ("segs", "so", "out", "oo", "st", "msk", "moo", "mst", "raw", "cor"):
        assert np.array_equal(plain[k], after[k]), k
    assert np.array_equal(args[2], after["out"]) and np.array_equal(args[4], after["msk"]) and np.array_equal(args[0], after["segs"])


def cli(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_cli_trim_and_split_files(tmp_path, rev):
    """Several --batch-reads batches: <o>.trim.fa and <o>.split.fa against files written from the reference over the
    oracle-derived maps; <o>.fa against a run without the options."""
    S = Synth(target_kmers=150_000, k=21, seed=77)
    S.write_dump(str(tmp_path / "sr.dump"))
    S.write_fasta(str(tmp_path / "reads.fa"), 0, 60)
    lines = (tmp_path / "reads.fa").read_text().splitlines()
    names, reads = [x[1:] for x in lines[0::2]], lines[1::2]
    if rev:   # (k-mers are directional: -rev corrects the reads of the opposite strand)
        reads = [M.revcomp(r) for r in reads]
        (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, reads)))
    pair = PU.Pair(target_kmers=150_000, k=21, seed=77, reverse=int(rev))
    ref = P.from_expected([M.expected(pair.otab, r) for r in reads])
    ML = 60
    want = {mode: P.pieces(*ref[:4], mode, ML) for mode in MODES}
    assert 0 < len(want[P.SPLIT][2]) < len(P.pieces(*ref[:4], P.SPLIT)[2])             # ML drops some pieces, keeps some
    args = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7"] + (["-rev"] if rev else [])
    a = cli(args + ["--trim", "--split", "--min-piece-len", str(ML), "-o", "cut"], tmp_path)
    p = cli(args + ["-o", "plain"], tmp_path)
    assert a.returncode == 0 and p.returncode == 0, (a.stderr.decode(), p.stderr.decode())
    assert (tmp_path / "cut.trim.fa").read_text().splitlines() == P.fasta_lines(names, want[P.TRIM], False)
    assert (tmp_path / "cut.split.fa").read_text().splitlines() == P.fasta_lines(names, want[P.SPLIT], True)
    for ext in (".fa", ".log", ".stats_basics.txt"):
        fa, fp = tmp_path / ("cut" + ext), tmp_path / ("plain" + ext)
        assert fa.exists() == fp.exists() and (not fa.exists() or fa.read_bytes() == fp.read_bytes()), ext
    assert (tmp_path / "cut.config.txt").read_bytes().replace(b"cut", b"plain") == (tmp_path / "plain.config.txt").read_bytes()
    assert not (tmp_path / "plain.trim.fa").exists() and not (tmp_path / "plain.split.fa").exists() and not (tmp_path / "cut.map.tsv").exists()
    line = "[TALC]: trimmed: %d reads, %d bases; split: %d pieces, %d bases" % (len(want[P.TRIM][2]), len(want[P.TRIM][0]),
                                                                               len(want[P.SPLIT][2]), len(want[P.SPLIT][0]))
    out_a, out_p = a.stdout.decode().splitlines(), p.stdout.decode().splitlines()
    assert line in out_a and [l for l in out_a if l != line] == [l.replace("plain.fa", "cut.fa") for l in out_p]
    # with the other reports: the trimmed reads carry the mask, the map and the solidity files are those of a run without
    m = cli(args + ["--trim", "--soft-mask", "--corr-map", "--solidity", "-o", "all"], tmp_path)
    q = cli(args + ["--soft-mask", "--corr-map", "--solidity", "-o", "rest"], tmp_path)
    assert m.returncode == 0 and q.returncode == 0, (m.stderr.decode(), q.stderr.decode())
    soft = P.pieces(*ref[:4], P.TRIM, 0, ref[4])
    assert (tmp_path / "all.trim.fa").read_text().splitlines() == P.fasta_lines(names, soft, False)
    assert any(c.islower() for c in bytes(soft[0]).decode())
    for ext in (".fa", ".map.tsv", ".solidity.tsv", ".log"):
        fa, fq = tmp_path / ("all" + ext), tmp_path / ("rest" + ext)
        assert fa.exists() == fq.exists() and (not fa.exists() or fa.read_bytes() == fq.read_bytes()), ext
    assert "[TALC]: trimmed: %d reads, %d bases" % (len(soft[2]), len(soft[0])) in m.stdout.decode().splitlines()
    assert not (tmp_path / "all.split.fa").exists()
