"""The chimera scan's contract (docs/chimeras.md) without a GPU: the two statements of tests/chimera_ref.py against each
other and on hand cases; the piece rule of the library (talc_chimera_plan.h) and the kernel's lanes run one after another on
the CPU (pure_chimera_scan: the chunk, halo and tile arithmetic) against them; the binding table; the command line's parse
errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chimera_ref as CR
import ends_ref as R
from talc_amd import build as B
from talc_amd import lib as T

TALC = os.path.join(B.OUT, "talc")
SSP, VNP = CR.SSP, CR.VNP
P24 = "GATCCGTAGCTTGACCATGCAGTC"
RANDOM12 = "ACGTTGCAAGTC"
SETTINGS = [([SSP, VNP], 10), ([SSP, VNP], 20), ([RANDOM12], 30), ([P24], 30)]
A64 = "ACGTACGTTTGCAAGGCTTAACCGTATGCATGCAAGTCCGATTGCAAGTCGGATCCATGGTAC"       # (the longest adapter: test_the_longest_adapter_on_random_reads)

_pure = None


def pure():
    global _pure
    if _pure is None:
        L = C.CDLL(os.path.join(B.OUT, "libtalc_pure.so"))
        L.pure_chimera_scan.restype = C.c_int64
        L.pure_chimera_scan.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
        L.pure_split_pieces.restype = C.c_int64
        L.pure_split_pieces.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.pure_chimera_geometry.restype = None
        L.pure_chimera_geometry.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        _pure = L
    return _pure


def lanes_scan(reads, adapters, pct):
    """k_read_chimera's lanes one after another on the CPU."""
    bases, off = R.batch(reads)
    if len(bases) == 0:
        bases = np.zeros(1, np.uint8)
    n = pure().pure_chimera_scan(",".join(adapters).encode(), pct, bases.ctypes.data, off.ctypes.data, len(reads), None, 0)
    assert n >= 0
    out = np.zeros(max(n, 1), CR.HIT_DTYPE)
    assert pure().pure_chimera_scan(",".join(adapters).encode(), pct, bases.ctypes.data, off.ctypes.data, len(reads), out.ctypes.data, n) == n
    return out[:n]


def lib_pieces(lens, hits, min_piece):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    hits = np.ascontiguousarray(hits)
    cap = len(hits) + len(lens) + 1
    out = np.zeros(cap, CR.PIECE_DTYPE)
    rpo = np.zeros(len(lens) + 1, np.uint64)
    dropped = np.zeros(2, np.uint64)
    n = pure().pure_split_pieces(hits.ctypes.data if len(hits) else None, len(hits), off.ctypes.data, len(lens), min_piece, out.ctypes.data, cap, rpo.ctypes.data,
                                 dropped.ctypes.data)
    assert 0 <= n <= cap
    return out[:n], rpo, int(dropped[0]), int(dropped[1])


def all_ways(reads, adapters, pct, plain=True):
    """The hits by numpy, held against the lanes and (plain) the loops; the pieces three ways under two bounds."""
    want, off = CR.hits(reads, adapters, pct)
    got = lanes_scan(reads, adapters, pct)
    assert len(got) == len(want) and (got == want).all(), (len(got), len(want))
    if plain:
        loops = CR.hits_plain(reads, adapters, pct)
        assert len(loops) == len(want) and (loops == want).all()
    assert (off == np.searchsorted(want["read"], np.arange(len(reads) + 1))).all()
    lens = [len(r) for r in reads]
    for min_piece in (0, 100):
        a = CR.pieces(lens, want, min_piece)
        b = lib_pieces(lens, want, min_piece)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        if plain:
            for x, y in zip(a, CR.pieces_plain(lens, want, min_piece)):
                assert np.array_equal(x, y)
    return want


# ---------------------------------------------------------------- the two statements against each other
@pytest.mark.parametrize("setting", range(4))
def test_numpy_the_loops_and_the_lanes_agree_on_random_reads(setting):
    adapters, pct = SETTINGS[setting]
    rng = np.random.default_rng(40 + setting)
    reads = []
    for i in range(300):
        n = int(rng.integers(0, 3001))
        s = R.random_seq(rng, n)
        if i % 4 == 0 and n > 80:                                    # a copy of some pattern, within or over the bound
            a = adapters[int(rng.integers(len(adapters)))]
            a = R.revcomp(a).decode() if rng.integers(2) else a
            at = int(rng.integers(0, n))
            s = s[:at] + R.mutate(rng, a, int(rng.integers(0, 5)), "SIDN") + s[at:]
        reads.append(s.lower() if i % 7 == 0 else s)
    want = all_ways(reads, adapters, pct, plain=True)                # numpy, the loops and the lanes on all 300 reads; the pieces three ways
    if setting == 2:                                                 # about 4 hits per kb: overlapping hits of both strands, dropped pieces
        total = sum(len(r) for r in reads)
        assert len(want) > 2 * total // 1000 and (want["strand"] == 0).sum() > 200 and (want["strand"] == 1).sum() > 200
        nxt = want[1:][want["read"][1:] == want["read"][:-1]]
        prv = want[:-1][want["read"][1:] == want["read"][:-1]]
        assert (nxt["start"] < prv["end"]).sum() > 20
        _, off, dropped, _ = CR.pieces([len(r) for r in reads], want, 100)
        assert dropped > 300 and (np.diff(off.astype(np.int64)) == 0).any()
    else:
        assert len(want) >= 20


def test_the_longest_adapter_on_random_reads():
    """64 letters at 30 per cent (k_a 19, the longest warm-up) beside a 24-letter one: numpy against the lanes on 300 reads, the
    loops (a cell at a time, 128 rows per column here) on 30 of them."""
    rng = np.random.default_rng(44)
    adapters = [P24, A64]
    reads = []
    for i in range(300):
        n = int(rng.integers(0, 3001))
        s = R.random_seq(rng, n)
        if i % 3 == 0 and n > 80:
            a = adapters[i % 2]
            a = R.revcomp(a).decode() if rng.integers(2) else a
            at = int(rng.integers(0, n))
            s = s[:at] + R.mutate(rng, a, int(rng.integers(0, 22)), "SIDN") + s[at:]
        reads.append(s)
    want = all_ways(reads, adapters, 30, plain=False)
    assert (want["adapter"] == 2).sum() >= 30 and int(want["err"][want["adapter"] == 2].max()) >= 10
    all_ways(reads[:30], adapters, 30, plain=True)


# ---------------------------------------------------------------- hand cases
def test_the_three_cases_of_the_issue():
    rng = np.random.default_rng(3)
    planted = R.random_seq(rng, 500) + R.mutate(rng, SSP, 3, "SID") + R.random_seq(rng, 500)
    tandem = R.random_seq(rng, 100) + SSP * 5 + R.random_seq(rng, 100)
    joint = "A" * 40 + R.revcomp(VNP).decode() + SSP
    want = all_ways([planted, tandem, joint], [SSP, VNP], 20)
    one = want[want["read"] == 0]
    assert len(one) == 1 and abs(int(one[0]["start"]) - 500) <= 3 and 500 + 23 <= one[0]["end"] <= 500 + 29 and 1 <= one[0]["err"] <= 3
    five = want[want["read"] == 1]
    assert len(five) == 5 and five["start"].tolist() == [100 + 26 * i for i in range(5)] and (five["end"] - five["start"] == 26).all()
    two = want[want["read"] == 2]
    assert [(int(h["start"]), int(h["end"]), int(h["adapter"]), int(h["strand"])) for h in two] == [(40, 62, 2, 1), (62, 88, 1, 0)]
    pieces, off, dropped, bases = CR.pieces([len(planted), len(tandem), len(joint)], want, 30)
    assert [(int(p["read"]), int(p["start"]), int(p["len"]), int(p["ordinal"])) for p in pieces if p["read"] == 2] == [(2, 0, 40, 1)]
    assert pieces[pieces["read"] == 1]["ordinal"].tolist() == [1, 2] and dropped == 0


def test_a_tie_goes_to_the_larger_end_and_the_window_is_half_the_pattern():
    rng = np.random.default_rng(5)
    last = P24[-1]
    other = next(ch for ch in "ACGT" if ch != last and ch != P24[-2])
    tie = "G" * 30 + P24[:-1] + other + last + "G" * 40              # cost 1 at 53 (deletion), 54 (substitution), 55 (insertion)
    D = R.sellers_plain(P24.encode(), tie.encode())
    assert [e for e, d in enumerate(D) if d == 1] == [53, 54, 55]
    want = all_ways([tie], [P24], 20)
    assert len(want) == 1 and want[0]["end"] == 55 and want[0]["err"] == 1 and want[0]["start"] == 30
    w = 12                                                           # ceil(24 / 2): two ends w apart are one hit, w + 1 apart two
    for gap, ends in ((w, [86]), (w + 1, [74, 87])):
        # an adapter of period `gap`: one more period behind a copy is a second exact copy that ends `gap` columns on
        unit = "ACCGTAGGTCATG"[:gap]
        a = (unit * 3)[:24]
        read = "T" * 50 + (unit * 4)[:24 + gap] + "T" * 50
        D = R.sellers_plain(a.encode(), read.encode())
        assert [e for e, d in enumerate(D) if d == 0] == [74, 74 + gap]
        want = all_ways([read], [a], 20)
        assert want[want["strand"] == 0]["end"].tolist() == ends and (want["err"][want["strand"] == 0] == 0).all()


def test_ends_of_the_read_short_reads_n_and_lower_case():
    rng = np.random.default_rng(7)
    reads = ["", "A", P24[:23], P24, P24 + R.random_seq(rng, 50), R.random_seq(rng, 50) + P24, P24.lower(), P24[:12] + "N" + P24[12:],
             P24[:12] + "N" + P24[13:], "N" * 60, (R.random_seq(rng, 20) + P24 + R.random_seq(rng, 20)).lower(), R.revcomp(P24).decode()]
    want = all_ways(reads, [P24], 20)
    by = lambda r: want[want["read"] == r]
    assert len(by(0)) == 0 and len(by(1)) == 0 and len(by(9)) == 0
    assert [(int(h["start"]), int(h["end"]), int(h["err"])) for h in by(2)] == [(0, 23, 1)]        # L = m - 1
    assert [(int(h["start"]), int(h["end"]), int(h["err"])) for h in by(3)] == [(0, 24, 0)]        # a read that is one primer
    assert by(4)[0]["start"] == 0 and by(5)[-1]["end"] == 74 and by(6)[0]["err"] == 0
    assert by(7)[0]["err"] == 1 and by(8)[0]["err"] == 1 and by(10)[0]["start"] == 20
    assert by(11)["strand"].tolist() == [1]
    pieces, off, _, _ = CR.pieces([len(r) for r in reads], want, 0)
    assert pieces[0]["len"] == 0 and pieces[0]["ordinal"] == 0                                     # L = 0: one piece, uncut
    assert int(off[4] - off[3]) == 0                                                               # the primer alone: no piece left
    assert [(int(p["start"]), int(p["len"]), int(p["ordinal"])) for p in pieces[int(off[4]):int(off[5])]] == [(24, 50, 1)]


def test_the_piece_rule_on_overlapping_and_nested_hits():
    hit = lambda r, s, e: (r, s, e, 1, 0, 0, 0)
    hits = np.array([hit(0, 10, 20), hit(0, 15, 40), hit(0, 100, 130), hit(0, 105, 120), hit(0, 130, 140), hit(2, 0, 30), hit(2, 170, 200), hit(3, 0, 50)], CR.HIT_DTYPE)
    hits = hits[np.lexsort((hits["strand"], hits["adapter"], hits["end"], hits["read"]))]
    lens = [300, 80, 200, 50]
    for min_piece, want in ((0, [(0, 0, 10, 1), (0, 40, 60, 2), (0, 140, 160, 3), (1, 0, 80, 0), (2, 30, 140, 1)]),
                            (61, [(0, 140, 160, 1), (1, 0, 80, 0), (2, 30, 140, 1)]), (200, [(1, 0, 80, 0)])):
        for rule in (CR.pieces, CR.pieces_plain, lib_pieces):
            pieces, off, dropped, bases = rule(lens, hits, min_piece)
            assert [tuple(int(x) for x in p) for p in pieces] == want, (rule.__name__, min_piece)
            assert dropped == 4 - sum(1 for p in want if p[3]) and len(off) == 5 and int(off[4]) == len(want)
            assert bases == 10 + 60 + 160 + 140 - sum(p[2] for p in want if p[3])


# ---------------------------------------------------------------- the lanes at their borders
def test_the_geometry_is_stated_once():
    out = np.zeros(3, np.uint32)
    for npat in (2, 4, 6, 8):
        for L in (0, 1, 35, 36, 37, 1151, 1152, 1153, 1800, 4031, 4032, 4033, 8063, 8064, 8065, 20_000, 140_000):
            pure().pure_chimera_geometry(L, npat, out.ctypes.data)
            assert tuple(out.tolist()) == T.chimera_geometry(L, npat)
            lanes, chunk, tile = out.tolist()
            assert lanes == 64 // npat and T.CHIMERA_CHUNK_MIN <= chunk <= T.CHIMERA_CHUNK_MAX and chunk % 8 == 4 and tile == lanes * chunk
            assert chunk * lanes >= min(L, T.CHIMERA_CHUNK_MAX * lanes)                            # a read up to one full tile is one tile


@pytest.mark.parametrize("adapters", [[P24], [P24, SSP, VNP, P24[::-1]]])
def test_the_lanes_around_every_chunk_and_tile_border_of_a_20_kb_read(adapters):
    rng = np.random.default_rng(len(adapters))
    length = 20_000
    lanes, chunk, tile = T.chimera_geometry(length, 2 * len(adapters))
    assert chunk == T.CHIMERA_CHUNK_MAX and length > 2 * tile and length % tile and length % chunk
    borders = list(range(chunk, length, chunk))
    copy = list(R.mutate(rng, P24, 2, "S"))
    reads = []
    for d in range(-42, 43):                                         # w + m + k_a = 40 columns of warm-up before a chunk, w behind it
        s = list(R.random_seq(rng, length))
        for b in borders:
            e = b + d
            if e <= length:
                s[e - 24:e] = copy if d % 2 else list(P24)
        s = "".join(s)
        reads.append(R.revcomp(s).decode() if d % 3 == 1 else s)       # (d = 0 and d = 24 as they lie: ends and starts on the borders)
    want = all_ways(reads, adapters, 20, plain=False)
    assert (np.bincount(want["read"], minlength=len(reads)) >= len(borders) - 1).all()
    assert np.isin(want["end"], borders).sum() >= len(borders) and np.isin(want["start"], borders).sum() >= len(borders)
    assert np.isin(want["end"], [b for b in borders if b % tile == 0]).any()


# ---------------------------------------------------------------- the binding table, the command line
def test_the_binding_table_and_the_records():
    L = T.lib()
    for name in ("talc_ctx_set_chimera", "talc_batch_chimera", "talc_batch_num_chimera_hits", "talc_batch_fetch_chimera", "talc_batch_create_split",
                 "talc_batch_num_split_pieces", "talc_batch_fetch_split", "talc_ctx_get_chimera_timing"):
        assert hasattr(L, name) and name in T.ABI_SYMBOLS
    assert T.CHIMERA_DTYPE == CR.HIT_DTYPE and T.CHIMERA_DTYPE.itemsize == 16
    assert [T.CHIMERA_DTYPE.fields[f][1] for f in T.CHIMERA_DTYPE.names] == [0, 4, 8, 12, 13, 14, 15]
    assert T.SPLIT_PIECE_DTYPE == CR.PIECE_DTYPE and T.SPLIT_PIECE_DTYPE.itemsize == 16
    assert L.talc_ctx_set_chimera(None, 1, 10, 0) == -1 and L.talc_ctx_get_chimera_timing(None, None, None) == -1
    assert L.talc_batch_chimera(None, None) == -1 and L.talc_batch_fetch_chimera(None, None, None, 0, None) == -1
    assert L.talc_batch_fetch_split(None, None, None, None) == -1 and L.talc_batch_num_chimera_hits(None) == 0 and L.talc_batch_num_split_pieces(None) == 0
    assert L.talc_abi_version() == 1


BASE = ["reads.fa", "-k", "21", "-SR", "sr.dump", "-o", "o"]


@pytest.mark.parametrize("extra,word", [
    (["--LRChimeras"], "--LRChimeras needs --LRAdapter"),
    (["--LRSplit"], "--LRSplit needs --LRAdapter"),
    (["--LRSplit", "--LRPolyA", "12"], "--LRSplit needs --LRAdapter"),
    (["--LRChimeraErr", "10"], "--LRChimeraErr needs"),
    (["--LRAdapter", P24, "--LRChimeraErr", "10"], "--LRChimeraErr needs"),
    (["--LRAdapter", P24, "--LRMinPiece", "50"], "--LRMinPiece needs"),
    (["--LRAdapter", P24, "--LRChimeras", "--LRChimeraErr", "31"], "LRChimeraErr: 0..30"),
    (["--LRAdapter", P24, "--LRChimeras", "--LRChimeraErr", "2.5"], "LRChimeraErr"),
    (["--LRAdapter", P24, "--LRSplit", "--LRMinPiece", "-1"], "LRMinPiece"),
    (["--LRAdapter", P24, "--LRSplit", "--LRMinPiece"], "requires an argument"),
    (["--LRAdapter", P24, "--LRChimeras", "--LRClip"], "--LRChimeras with --LRClip needs --LRSplit"),
    (["--LRAdapter", P24, "--LRPolyA", "12", "--LRClip", "--LRChimeras", "--LRChimeraErr", "15"], "--LRChimeras with --LRClip needs --LRSplit"),
])
def test_cli_parse_errors_exit_1_and_write_nothing(tmp_path, extra, word):
    r = subprocess.run([TALC] + BASE + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and word in r.stderr.decode(), (r.returncode, r.stderr.decode())
    assert os.listdir(tmp_path) == []


def test_cli_help_names_the_options():
    r = subprocess.run([TALC, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0
    for opt in ("--LRChimeras", "--LRSplit", "--LRChimeraErr", "--LRMinPiece"):
        assert opt.encode() in r.stdout


@pytest.mark.parametrize("extra", [["--LRChimeras"], ["--LRSplit"], ["--LRSplit", "--LRClip", "--LRMinPiece", "50"]])
def test_cli_refuses_the_options_in_a_run_without_a_table(tmp_path, extra):
    (tmp_path / "reads.fa").write_text(">r\n" + "ACGT" * 30 + "\n")
    (tmp_path / "sr.dump").write_text("ACGTACGTACGTACGTACGTA 5\n")
    r = subprocess.run([TALC, "reads.fa", "-k", "21", "-SR", "sr.dump", "-qm", "jellyfish2", "-o", "o", "--LRAdapter", SSP] + extra, cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and b"no table" in r.stderr
    assert not (tmp_path / "o.fa").exists() and not (tmp_path / "o.chimera.tsv").exists()
