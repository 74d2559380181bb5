"""The edit scripts without a GPU (docs/correction_edits.md): the numpy contract (tests/edits_ref.py) against a plain
double-loop DP with an explicit traceback, its invariants, merging across segments, what it makes of the oracle-derived
maps of the sets the GPU tests use, the exported symbols and their argument checks, and the command line's no-table path."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import corr_map_ref as M
import edits_ref as E
from edits_util import batch_of, u8
import pieces_ref as P
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

TALC = os.path.join(B.OUT, "talc")
S, C, R = M.SOLID, M.CORRECTED, M.RAW
EDIT_SYMBOLS = ["talc_batch_edits", "talc_batch_num_edit_ops", "talc_batch_fetch_edits", "talc_ctx_get_edits_timing", "talc_test_edit_script"]


def brute(a, b):
    """(text, distance): the canonical script of two texts by the double loop and the rule as the contract words it."""
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    i, j, ops = n, m, []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == D[i][j]:
            ops.append("=" if a[i - 1] == b[j - 1] else "X")
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1][j] + 1 == D[i][j]:
            ops.append("D")
            i -= 1
        else:
            ops.append("I")
            j -= 1
    ops.reverse()
    return "".join("%d%s" % (len(list(g)), c) for c, g in itertools.groupby(ops)) or "*", D[n][m]


def text_of(a, b, max_cells=0):
    return E.cigar_text(E.pair_ops(a, b, max_cells))


def cost(ops):
    return sum(int(o) >> 4 for o in ops if int(o) & 15 != E.OP_EQ)


def check_pair(a, b):
    want, dist = brute(a, b)
    ops = E.pair_ops(a, b)
    assert E.cigar_text(ops) == want, (a, b)
    assert cost(ops) == dist
    codes = [int(o) & 15 for o in ops]
    assert all(x != y for x, y in zip(codes, codes[1:])) and all(int(o) >> 4 for o in ops)
    # applying the script to a gives b where it says '=', a base that differs where it says X
    used, src = E.apply(ops, u8(a))
    assert used == len(a) and len(src) == len(b)
    for j, (c, i) in enumerate(src):
        assert c == E.OP_I or (a[i] == b[j]) == (c == E.OP_EQ)


def test_reference_against_the_double_loop_on_all_short_pairs():
    words = [""] + ["".join(w) for n in range(1, 5) for w in itertools.product("AC", repeat=n)]
    for a in words:
        for b in words:
            check_pair(a, b)


def test_reference_on_hand_made_pairs():
    assert text_of("AA", "A") == "1D1="
    assert text_of("A", "AA") == "1I1="
    assert text_of("AAAAAAA", "AAA") == "4D3=" and text_of("AAA", "AAAAAAA") == "4I3="
    assert text_of("ACGT" * 5, "TGCA" * 5) == brute("ACGT" * 5, "TGCA" * 5)[0]
    assert text_of("AAAA", "CCCC") == "4X"
    assert text_of("ANA", "ANA") == "3=" and text_of("ANA", "AAA") == "1=1X1="
    assert text_of("", "ACG") == "3I" and text_of("ACG", "") == "3D" and text_of("", "") == "*"
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = "".join(rng.choice(list("ACGTN"), size=int(rng.integers(0, 40))))
        b = "".join(rng.choice(list("ACGTN"), size=int(rng.integers(0, 40))))
        check_pair(a, b)
    a, b = "ACGTTGCA" * 4, "ACGTAGCA" * 4 + "C"                      # 32 x 33 = 1056 cells
    assert text_of(a, b, 1056) == brute(a, b)[0]                     # exactly at the cap: aligned
    assert text_of(a, b, 1055) == "32D33I"                           # over it by one cell: not aligned


def test_parts_merge_across_segments():
    solid = "ACGTACGTAC"
    reads = [
        # '=' of a SOLID into the leading '=' of a CORRECTED part, and its trailing '=' into the next SOLID
        (solid + "GGTCC" + solid, [(S, 10, solid), (C, 5, "GGACC"), (S, 10, solid)]),
        # an empty part between two mergeable parts: I, nothing, I
        (solid + solid, [(S, 10, solid), (C, 0, "TT"), (C, 0, ""), (C, 0, "G"), (R, 10, solid)]),
        # D then (empty SOLID) then D; an unaligned part keeps its two runs but merges at both ends
        ("AAAA" + "CCCC" + "ACGTACGT", [(C, 4, ""), (S, 0, ""), (C, 4, ""), (C, 8, "TTTTTTTTT")]),
        ("", []),
        ("ACGTN", [(R, 5, "ACGTN")]),
    ]
    args = batch_of(reads)
    ops, oo, rows = E.edits(*args, max_cells=71)
    texts = [E.cigar_text(ops[int(oo[r]):int(oo[r + 1])]) for r in range(len(reads))]
    assert texts == ["12=1X12=", "10=3I10=", "16D9I", "*", "5="]
    assert rows["n_unaligned"].tolist() == [0, 0, 1, 0, 0] and rows["n_ops"].tolist() == [3, 3, 2, 0, 1]
    ops2, oo2, rows2 = E.edits(*args, max_cells=72)                  # 8 x 9 cells: now aligned
    assert rows2["n_unaligned"].sum() == 0 and E.cigar_text(ops2[int(oo2[2]):int(oo2[3])]).startswith("8D")
    check_rows(args, (ops, oo, rows))
    check_rows(args, (ops2, oo2, rows2))


def check_rows(args, result, as_seen=()):
    """The two length identities, the op count, no two equal neighbours, and the script applied to the read (for the
    reads listed in as_seen — passed through under -rev — to the read as the correction sees it)."""
    reads, segs, so, rec, ro = args
    ops, oo, rows = result
    for r in range(len(reads)):
        mine = ops[int(oo[r]):int(oo[r + 1])]
        w = rows[r]
        raw, out = E.dna5_bytes(M.revcomp(M.dna5(reads[r])) if r in as_seen else reads[r]), rec[int(ro[r]):int(ro[r + 1])]
        assert int(w["n_match"]) + int(w["n_mismatch"]) + int(w["n_del"]) == len(raw)
        assert int(w["n_match"]) + int(w["n_mismatch"]) + int(w["n_ins"]) == len(out)
        assert int(w["n_ops"]) == len(mine)
        codes = (mine & 15).tolist()
        assert all(x != y for x, y in zip(codes, codes[1:])) and ((mine >> 4) > 0).all()
        by = {c: int((mine[(mine & 15) == c] >> 4).sum()) for c in E.LETTER}
        assert (by[E.OP_EQ], by[E.OP_X], by[E.OP_I], by[E.OP_D]) == (int(w["n_match"]), int(w["n_mismatch"]), int(w["n_ins"]), int(w["n_del"]))
        used, src = E.apply(mine, raw)
        assert used == len(raw) and len(src) == len(out)
        idx = np.asarray([i for c, i in src if c == E.OP_EQ], dtype=np.int64)
        at = np.asarray([j for j, (c, i) in enumerate(src) if c == E.OP_EQ], dtype=np.int64)
        assert np.array_equal(raw[idx], out[at])
        idx = np.asarray([i for c, i in src if c == E.OP_X], dtype=np.int64)
        at = np.asarray([j for j, (c, i) in enumerate(src) if c == E.OP_X], dtype=np.int64)
        assert (raw[idx] != out[at]).all()


def set_args(name):
    s = M.map_set(name)
    segs, so, rec, ro, _ = P.from_expected(s.exp)
    return s, (s.reads, segs, so, rec, ro)


def corrected_pairs(args):
    reads, segs, so, rec, ro = args
    c = segs[segs["kind"] == C]
    return c["raw_len"].astype(np.int64), c["out_len"].astype(np.int64)


@pytest.fixture(scope="module")
def default_result():
    s, args = set_args("default")
    return s, args, E.edits(*args)


def test_edits_of_the_oracle_derived_maps(default_result):
    """The 200-read default set of the map tests.  SOLID and RAW stretches of a corrected read are equal byte for byte in
    the read and in its record, which is why nothing is compared there."""
    s, args, result = default_result
    reads, segs, so, rec, ro = args
    for r, e in enumerate(s.exp):
        if e["status"] != 0:
            continue
        raw, out = E.dna5_bytes(reads[r]), rec[int(ro[r]):int(ro[r + 1])]
        for g in segs[int(so[r]):int(so[r + 1])]:
            if g["kind"] != C:
                assert g["raw_len"] == g["out_len"]
                assert np.array_equal(raw[int(g["raw_start"]):int(g["raw_start"]) + int(g["raw_len"])], out[int(g["out_start"]):int(g["out_start"]) + int(g["out_len"])])
    n, m = corrected_pairs(args)
    big = int(np.argmax(n * m))
    assert len(n) == 2987 and int(((n == 0) | (m == 0)).sum()) == 150 and (int(n[big]), int(m[big])) == (601, 607)
    ops, oo, rows = result
    check_rows(args, result)
    corrected = np.asarray([e["status"] == 0 for e in s.exp])
    sums = tuple(int(rows[f][corrected].sum()) for f in ("n_match", "n_mismatch", "n_ins", "n_del"))
    print("default set: = X I D over the corrected reads", sums, "over all reads", tuple(int(rows[f].sum()) for f in ("n_match", "n_mismatch", "n_ins", "n_del")),
          "most ops in a read", int(rows["n_ops"].max()))
    assert sums[1:] == (15659, 11193, 9964) and sum(sums[1:]) == 36816
    assert int(rows["n_ops"].max()) <= 631 and int(rows["n_unaligned"].sum()) == 0
    assert tuple(int(rows[f].sum()) for f in ("n_match", "n_mismatch", "n_ins", "n_del")) == (326587, 15659, 11193, 9964)   # over all reads
    # a cap that leaves some segments unaligned and aligns others
    capped = E.edits(*args, max_cells=4096)
    check_rows(args, capped)
    assert 0 < int(capped[2]["n_unaligned"].sum()) == int(((n * m > 4096) & (n > 0) & (m > 0)).sum()) < len(n) - 150


def test_the_reverse_set_costs_the_same(default_result):
    s, args = set_args("reverse")
    result = E.edits(*args)
    passed = [r for r, e in enumerate(s.exp) if e["status"] != 0]
    assert passed
    check_rows(args, result, passed)
    rows = result[2]
    assert int(rows["n_mismatch"].sum() + rows["n_ins"].sum() + rows["n_del"].sum()) == 36816
    n, m = corrected_pairs(args)
    assert len(n) == 2987 and int(((n == 0) | (m == 0)).sum()) == 150


def test_reference_text_helpers():
    ops = np.asarray([812 << 4 | 7, 1 << 4 | 8, 40 << 4 | 7, 2 << 4 | 2, 3 << 4 | 1], dtype=np.uint32)
    assert E.cigar_text(ops) == "812=1X40=2D3I" == T.cigar_text(ops) and E.cigar_text(ops[:0]) == "*" == T.cigar_text(ops[:0])


def test_edit_symbols_are_exported_and_listed():
    L = T.lib()
    for name in EDIT_SYMBOLS:
        assert hasattr(L, name), name
        assert name in T.ABI_SYMBOLS
    assert T.EDIT_ROW_DTYPE.itemsize == 24 and T.EDIT_ROW_DTYPE == E.EDIT_ROW_DTYPE
    assert (T.EDIT_I, T.EDIT_D, T.EDIT_EQ, T.EDIT_X) == (E.OP_I, E.OP_D, E.OP_EQ, E.OP_X) == (1, 2, 7, 8)
    assert L.talc_abi_version() == 1


def test_edit_calls_check_their_arguments():
    L = T.lib()
    assert L.talc_batch_edits(None, None, 0) == -1                                 # TALC_ERR_INVALID
    assert L.talc_batch_num_edit_ops(None) == 0
    assert L.talc_batch_fetch_edits(None, None, None, 0, None, None) == -1
    assert L.talc_ctx_get_edits_timing(None, None, None) == -1
    assert L.talc_test_edit_script(None, b"A", 1, b"A", 1, 0, None, 0, None, None) == -1
    assert L.talc_last_error()


def run(args, cwd):
    return subprocess.run([TALC] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_cli_lists_the_edit_options(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0 and all(o in r.stdout for o in (b"--corr-edits", b"--max-edit-cells"))
    bad = run(["reads.fa", "-k", "21", "-SR", "x", "--max-edit-cells", "0"], tmp_path)
    assert bad.returncode == 1


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_cli_pass_through_writes_every_read_as_matches(tmp_path, rev):
    """Without a table (-qm jellyfish2 with neither -jf2 nor a .jf: no GPU needed) every read is L '='; under -rev the
    record is the read as the correction sees it (as_seen '-').  Every other file is the plain run's."""
    syn = Synth(target_kmers=150_000, k=21, seed=77)
    syn.write_dump(str(tmp_path / "sr.dump"))
    syn.write_fasta(str(tmp_path / "reads.fa"), 0, 20)
    with open(tmp_path / "reads.fa", "a") as f:
        f.write(">empty\n\n>short\nACGTN\n")
    lines = (tmp_path / "reads.fa").read_text().split("\n")
    names, reads = [x[1:] for x in lines[0:44:2]], lines[1:44:2]
    assert names[-2:] == ["empty", "short"] and reads[-2:] == ["", "ACGTN"]
    base = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump"), "-qm", "jellyfish2", "--batch-reads", "7"] + (["-rev"] if rev else [])
    plain = run(base + ["-o", "p"], tmp_path)
    r = run(base + ["--corr-edits", "--max-edit-cells", "100", "-o", "m"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, (plain.stderr, r.stderr)
    K = 21
    status = [2 if len(s) > K else 1 for s in reads]
    ro = np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64)
    segs = M.as_array([(R, 0, len(s), 0, len(s)) for s in reads])
    so = np.arange(len(reads) + 1, dtype=np.uint64)
    rec = u8("".join(M.revcomp(M.dna5(s)) if rev else M.dna5(s) for s in reads))
    # (the script of a passed-through read compares nothing: under -rev it is that of the read as the correction sees it)
    seen = [M.revcomp(M.dna5(s)) if rev else s for s in reads]
    want = E.tsv_lines(names, reads, status, ro, E.edits(seen, segs, so, rec, ro), [rev] * len(reads))
    got = (tmp_path / "m.edits.tsv").read_text().split("\n")
    assert got[0].split("\t") == ["read_name", "status", "raw_length", "corr_length", "n_match", "n_mismatch", "n_ins", "n_del", "n_unaligned", "as_seen", "cigar"]
    assert got[1:-1] == want and got[-1] == ""
    assert got[-3].endswith("\t*") and got[-2].endswith("\t5=")
    assert not (tmp_path / "p.edits.tsv").exists() and not (tmp_path / "m.map.tsv").exists()
    for ext in (".fa", ".log", ".stats_basics.txt"):
        assert (tmp_path / ("p" + ext)).read_bytes() == (tmp_path / ("m" + ext)).read_bytes(), ext
    assert (tmp_path / "p.config.txt").read_bytes().replace(b"OUTPUT=p", b"OUTPUT=m").replace(b"sample: p", b"sample: m") \
        .replace(b"p.stats", b"m.stats") == (tmp_path / "m.config.txt").read_bytes()
    a, b = plain.stdout.decode().splitlines(), r.stdout.decode().splitlines()
    line = "[TALC]: edits: 0 matches, 0 mismatches, 0 insertions, 0 deletions in 0 corrected reads (0 segments not aligned)"
    assert line in b and b.index(line) == len(b) - 2 and [l for l in b if l != line] == [l.replace("p.fa", "m.fa") for l in a]
