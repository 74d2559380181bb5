"""Trimmed and split output without a GPU (docs/trim_split.md): the numpy contract (tests/pieces_ref.py) against a plain
per-byte loop on hand-made segment lists, its invariants, what it makes of the oracle-derived maps of the set the GPU
tests use, the exported symbols and their argument checks, and the command line's no-table path."""
import os
import subprocess

import numpy as np
import pytest

import corr_map_ref as M
import pieces_ref as P
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

TALC = os.path.join(B.OUT, "talc")
S, C, R = M.SOLID, M.CORRECTED, M.RAW
PIECE_SYMBOLS = ["talc_batch_pieces", "talc_batch_num_pieces", "talc_batch_pieces_bytes", "talc_batch_fetch_pieces", "talc_ctx_get_pieces_timing"]


def read_of(spec, rng, flip=False):
    """One read from [(kind, raw_len, out_len)]: its segment tuples, its record and its masked record (texts)."""
    segs, rs, os_ = [], 0, 0
    for kind, rl, ol in spec:
        assert kind == C or rl == ol
        segs.append((kind, rs, rl, os_, ol))
        rs, os_ = rs + rl, os_ + ol
    rec = "".join(rng.choice(list("ACGT"), size=os_)) if os_ else ""
    if flip:   # what -rev does to a corrected read's segments
        segs = [(k, rs - a - l, l, os_ - o - m, m) for k, a, l, o, m in reversed(segs)]
    msk = list(rec)
    for k, a, l, o, m in segs:
        if k == R:
            msk[o:o + m] = rec[o:o + m].lower()
    return segs, rec, "".join(msk)


def brute(segs, rec, msk, mode, min_len, soft):
    """The pieces of one read, byte by byte: [(out_start, text)]."""
    weak = [None] * len(rec)
    for k, a, l, o, m in segs:
        for i in range(o, o + m):
            assert weak[i] is None
            weak[i] = k == R
    assert None not in weak
    src = msk if (soft and mode == P.TRIM) else rec
    runs = []
    if mode == P.TRIM:
        t = [i for i, w in enumerate(weak) if not w]
        if t:
            runs = [(t[0], t[-1] + 1)]
    else:
        i = 0
        while i < len(rec):
            if weak[i]:
                i += 1
                continue
            j = i
            while j < len(rec) and not weak[j]:
                j += 1
            runs.append((i, j))
            i = j
    return [(a, src[a:b]) for a, b in runs if b - a >= min_len]


def batch_of(reads):
    segs = M.as_array([s for sg, _, _ in reads for s in sg])
    so = np.cumsum([0] + [len(sg) for sg, _, _ in reads]).astype(np.uint64)
    ro = np.cumsum([0] + [len(rec) for _, rec, _ in reads]).astype(np.uint64)
    rec = np.frombuffer("".join(rec for _, rec, _ in reads).encode(), dtype=np.uint8)
    msk = np.frombuffer("".join(m for _, _, m in reads).encode(), dtype=np.uint8)
    return segs, so, rec, ro, msk


def check_batch(reads, min_lens=(0,)):
    """pieces_ref on the batch equals the per-byte loop on every read, in both modes, plain and masked."""
    segs, so, rec, ro, msk = batch_of(reads)
    for mode in (P.TRIM, P.SPLIT):
        for ml in min_lens:
            for soft in (False, True):
                res = P.pieces(segs, so, rec, ro, mode, ml, msk if soft else None)
                data, po, pc, rpo = res
                want = [brute(sg, r, m, mode, ml, soft) for sg, r, m in reads]
                assert P.piece_texts(res) == [[t for _, t in w] for w in want], (mode, ml, soft)
                assert [(int(p["read"]), int(p["out_start"]), int(p["out_len"])) for p in pc] == \
                    [(i, a, len(t)) for i, w in enumerate(want) for a, t in w]
                assert len(rpo) == len(reads) + 1 and int(rpo[-1]) == len(pc) and int(po[-1]) == len(data)
                assert (np.diff(po.astype(np.int64)) == pc["out_len"]).all()


def test_reference_against_the_byte_loop_on_hand_made_reads():
    rng = np.random.default_rng(3)
    specs = {
        "raw head and tail": [(R, 30, 30), (S, 50, 50), (C, 20, 22), (S, 40, 40), (R, 10, 10)],
        "corrected head and tail": [(C, 30, 28), (S, 50, 50), (R, 20, 20), (S, 40, 40), (C, 10, 12)],
        "zero-length raw between two solids": [(R, 0, 0), (S, 50, 50), (R, 0, 0), (S, 40, 40), (R, 0, 0)],
        "zero-length corrected between": [(R, 5, 5), (S, 50, 50), (C, 25, 0), (S, 40, 40), (R, 5, 5)],
        "corrected head with out_len 0 and raw_len > 0": [(C, 12, 0), (S, 50, 50), (R, 7, 7), (S, 30, 30), (R, 0, 0)],
        "two raw stretches": [(C, 9, 9), (S, 30, 30), (R, 11, 11), (S, 31, 31), (C, 5, 6), (S, 32, 32), (R, 13, 13), (S, 33, 33), (R, 0, 0)],
        "one raw segment": [(R, 300, 300)],
        "empty read": [(R, 0, 0)],
        "weak between empties": [(R, 0, 0), (S, 21, 21), (C, 30, 0), (R, 4, 4), (C, 3, 0), (S, 22, 22), (C, 0, 0)],
    }
    reads = [read_of(sp, rng) for sp in specs.values()]
    reads += [read_of(sp, rng, flip=True) for sp in specs.values()]
    check_batch(reads, (0, 1, 21, 22, 23, 50, 51, 1000))
    # what the cases are there for
    one = lambda name, mode, ml=0: P.piece_texts(P.pieces(*batch_of([read_of(specs[name], np.random.default_rng(1))])[:4], mode, ml))[0]
    assert len(one("zero-length raw between two solids", P.SPLIT)) == 1 and len(one("zero-length raw between two solids", P.SPLIT)[0]) == 90
    assert len(one("zero-length corrected between", P.SPLIT)) == 1
    assert [len(t) for t in one("corrected head with out_len 0 and raw_len > 0", P.SPLIT)] == [50, 30]
    assert [len(t) for t in one("two raw stretches", P.SPLIT)] == [39, 69, 33] and len(one("two raw stretches", P.TRIM)[0]) == 39 + 11 + 69 + 13 + 33
    assert one("one raw segment", P.SPLIT) == [] and one("one raw segment", P.TRIM) == [] and one("empty read", P.SPLIT) == []
    assert [len(t) for t in one("raw head and tail", P.SPLIT, 50)] == [112]
    assert [len(t) for t in one("two raw stretches", P.SPLIT, 39)] == [39, 69]       # min_len equal to a piece's length: kept
    assert [len(t) for t in one("two raw stretches", P.SPLIT, 40)] == [69]           # one more: dropped
    assert [len(t) for t in one("weak between empties", P.SPLIT)] == [21, 22]


def pass_boundary_reads(rng):
    """Reads of 63, 65, 127 and 129 segments (R = 31, 32, 63, 64 regions) whose pieces start, end and straddle at segment
    63 / 64 and 127 / 128: where a walk of 64 segments per pass hands over."""
    reads = []
    for nseg in (63, 65, 127, 129):
        def spec(kinds, empty=()):
            out = []
            for j in range(nseg):
                k = kinds.get(j, S if j % 2 else C)
                ln = 0 if j in empty else int(rng.integers(1, 40))
                out.append((k, ln, ln))
            return out
        for b in (62, 63, 64, 65, 126, 127, 128):
            if b >= nseg:
                continue
            reads.append(read_of(spec({b: R}), rng))                                    # a piece ends at b - 1, one starts at b + 1
            reads.append(read_of(spec({b - 1: R, b + 1: R} if b + 1 < nseg else {b - 1: R}), rng))   # a piece that is segment b alone
            reads.append(read_of(spec({b - 2: R}, empty=(b - 1, b)), rng))              # looks through empties across the boundary
            reads.append(read_of(spec({b: R}, empty=(b,)), rng))                        # an empty RAW splits nothing
            reads.append(read_of(spec({b - 1: R}, empty=(b,) if b + 1 < nseg else ()), rng, flip=True))
        reads.append(read_of(spec({}), rng))                                            # one piece over every pass
        reads.append(read_of(spec({j: R for j in range(0, nseg, 2)}), rng))             # every second segment weak
        reads.append(read_of(spec({0: R, nseg - 1: R}, empty=tuple(range(60, min(nseg - 1, 70)))), rng))
        if nseg > 64:
            reads.append(read_of(spec({10: R}, empty=tuple(range(64, nseg))), rng))     # an open piece and a last pass without a byte
            reads.append(read_of(spec({70 if nseg > 71 else 64: R}, empty=tuple(range(0, 64))), rng))   # a first pass without a byte
        for _ in range(6):
            kinds = {int(j): R for j in rng.choice(nseg, size=int(rng.integers(1, 12)), replace=False)}
            reads.append(read_of(spec(kinds, empty=tuple(int(j) for j in rng.choice(nseg, size=8, replace=False))), rng))
    return reads


def test_reference_against_the_byte_loop_where_a_64_segment_pass_ends():
    reads = pass_boundary_reads(np.random.default_rng(11))
    assert {len(sg) for sg, _, _ in reads} == {63, 65, 127, 129}
    check_batch(reads, (0, 30, 200))


def check_invariants(segs, so, rec, ro, msk):
    split = P.pieces(segs, so, rec, ro, P.SPLIT)
    trim = P.pieces(segs, so, rec, ro, P.TRIM)
    soft = P.pieces(segs, so, rec, ro, P.TRIM, 0, msk)
    st, tt, mt = P.piece_texts(split), P.piece_texts(trim), P.piece_texts(soft)
    inner = 0
    for r in range(len(so) - 1):
        m = bytes(msk[int(ro[r]):int(ro[r + 1])]).decode()
        u = bytes(rec[int(ro[r]):int(ro[r + 1])]).decode()
        assert "".join(st[r]) == "".join(c for c in m if not c.islower())        # the record with its weak bytes removed
        up = [i for i, c in enumerate(m) if not c.islower()]
        assert tt[r] == ([u[up[0]:up[-1] + 1]] if up else [])
        assert mt[r] == ([m[up[0]:up[-1] + 1]] if up else [])
        if up and not any(c.islower() for c in m[up[0]:up[-1] + 1]):
            assert st[r] == tt[r]                                                 # no inner weak stretch: both modes agree
        elif up:
            inner += 1
            assert len(st[r]) >= 2
    return split, trim, inner


def test_invariants_on_hand_made_reads():
    rng = np.random.default_rng(11)
    assert check_invariants(*batch_of(pass_boundary_reads(rng)))[2] > 0


@pytest.fixture(scope="module")
def default_set():
    return M.map_set("default")


def test_pieces_of_the_oracle_derived_maps(default_set):
    """The 200-read default set of the map tests: every piece is at least K bases, so min_len <= K drops nothing; the set
    has a read with two or more split pieces, a read without a piece, and a trimmed piece with a weak stretch inside."""
    s = default_set
    K = int(s.pair.p.k)
    args = P.from_expected(s.exp)
    split, trim, inner = check_invariants(*args)
    lens = split[2]["out_len"]
    per_read = np.diff(split[3].astype(np.int64))
    print("default set: %d split pieces, shortest %d, reads with >= 2 pieces %d, without a piece %d, trimmed with a weak stretch inside %d"
          % (len(lens), int(lens.min()), int((per_read >= 2).sum()), int((per_read == 0).sum()), inner))
    assert len(lens) and int(lens.min()) >= K and int(trim[2]["out_len"].min()) >= K
    for mode, ref in ((P.SPLIT, split), (P.TRIM, trim)):
        again = P.pieces(*args[:4], mode, K)
        assert all(np.array_equal(a, b) for a, b in zip(again, ref))
    assert (per_read >= 2).any() and (per_read == 0).any() and inner > 0
    assert (np.diff(trim[3].astype(np.int64)) == (per_read > 0)).all()


def test_piece_symbols_are_exported_and_listed():
    L = T.lib()
    for name in PIECE_SYMBOLS:
        assert hasattr(L, name), name
        assert name in T.ABI_SYMBOLS
    assert T.PIECE_DTYPE.itemsize == 12 and T.PIECE_DTYPE == P.PIECE_DTYPE
    assert (T.PIECES_TRIM, T.PIECES_SPLIT) == (P.TRIM, P.SPLIT) == (1, 2)


def test_piece_calls_check_their_arguments():
    L = T.lib()
    assert L.talc_batch_pieces(None, None, P.SPLIT, 0, 0) == -1                    # TALC_ERR_INVALID
    assert L.talc_batch_num_pieces(None) == 0 and L.talc_batch_pieces_bytes(None) == 0
    assert L.talc_batch_fetch_pieces(None, None, None, 0, None, None, 0, None) == -1
    assert L.talc_ctx_get_pieces_timing(None, None, None) == -1
    assert L.talc_last_error()


def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_cli_lists_the_piece_options(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0 and all(o in r.stdout for o in (b"--trim", b"--split", b"--min-piece-len"))
    bad = run(["reads.fa", "-k", "21", "-SR", "x", "--min-piece-len", "-1"], tmp_path)
    assert bad.returncode == 1


def test_cli_pass_through_writes_two_empty_files(tmp_path):
    """Without a table (-qm jellyfish2 with neither -jf2 nor a .jf: no GPU needed) no read has a trusted base: both files
    exist and are empty, every other file is the plain run's, and stdout gains the one summary line."""
    syn = Synth(target_kmers=150_000, k=21, seed=77)
    syn.write_dump(str(tmp_path / "sr.dump"))
    syn.write_fasta(str(tmp_path / "reads.fa"), 0, 20)
    base = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "-qm", "jellyfish2", "--batch-reads", "7"]
    plain = run(base + ["-o", "p"], tmp_path)
    r = run(base + ["--trim", "--split", "--min-piece-len", "30", "-o", "m"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, (plain.stderr, r.stderr)
    assert (tmp_path / "m.trim.fa").read_bytes() == b"" and (tmp_path / "m.split.fa").read_bytes() == b""
    assert not (tmp_path / "p.trim.fa").exists() and not (tmp_path / "p.split.fa").exists()
    for ext in (".fa", ".log", ".stats_basics.txt"):
        assert (tmp_path / ("p" + ext)).read_bytes() == (tmp_path / ("m" + ext)).read_bytes(), ext
    assert (tmp_path / "p.config.txt").read_bytes().replace(b"OUTPUT=p", b"OUTPUT=m").replace(b"sample: p", b"sample: m") \
        .replace(b"p.stats", b"m.stats") == (tmp_path / "m.config.txt").read_bytes()
    assert not (tmp_path / "m.map.tsv").exists()
    a, b = plain.stdout.decode().splitlines(), r.stdout.decode().splitlines()
    line = "[TALC]: trimmed: 0 reads, 0 bases; split: 0 pieces, 0 bases"
    assert line in b and [l for l in b if l != line] == [l.replace("p.fa", "m.fa") for l in a]
    t = run(base + ["--trim", "-o", "t"], tmp_path)
    assert "[TALC]: trimmed: 0 reads, 0 bases" in t.stdout.decode().splitlines() and not (tmp_path / "t.split.fa").exists()
