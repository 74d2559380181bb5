"""The text-dump reference (tests/dump_ref.py) checked by hand, the files of tests/dump_cases.py checked for what each case
claims (so that no GPU case passes vacuously), and the host parser (parseDumpFile, through talc_test_parse_text with where
= 0, and through Table.from_files for the lines only the tokeniser takes) on all of them.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import dump_cases as DC
import dump_ref as D
import oracle_lib as O
import parity_util as PU
from talc_amd import lib as T

TILE, SLICE = D.TILE, D.SLICE
K18 = "ACGTACGTACGTACGTAC"


def pack(text):
    v = 0
    for ch in text.upper():
        v = (v << 2) | "ACGT".index(ch)
    return v


# ---------------------------------------------------------------- parse and first_wins by hand
def test_parse_takes_canonical_lines():
    data = (K18 + " 7\n" + K18.lower() + "\t000000007\n" + "T" * 18 + " 999999999\n" + "A" * 18 + " 0\n").encode()
    km, ct, flagged = D.parse(data, 18)
    assert not flagged
    assert km.tolist() == [pack(K18), pack(K18), (1 << 36) - 1, 0] and ct.tolist() == [7, 7, 999999999, 0]
    assert km.dtype == np.uint64 and ct.dtype == np.uint32
    assert D.line_starts(data) == [0, 21, 50, 79]
    k31 = "ACGTTGCAACGTTGCAACGTTGCAACGTTGC"
    km, ct, flagged = D.parse(("T" * 31 + " 12\n" + k31 + " 3\n").encode(), 31)
    assert not flagged and km.tolist() == [(1 << 62) - 1, pack(k31)] and ct.tolist() == [12, 3]     # (bit 61 is used)


@pytest.mark.parametrize("kind", DC.KINDS + DC.END_KINDS)
def test_parse_flags_each_kind_of_line_that_is_not_canonical(kind):
    good = (K18 + " 5\n").encode()
    other = ("TTGCA" + K18[5:] + " 6\n").encode()
    if kind == "no-final-newline":
        data = good + other[:-1]
    elif kind == "cut-inside-last-kmer":
        data = good + other[:10]
    else:
        data = good + DC.bad_line(kind, other, 18) + good
    km, ct, flagged = D.parse(data, 18)
    assert flagged, kind
    want = 1 if kind in DC.END_KINDS else 2
    assert km.tolist() == [pack(K18)] * want and ct.tolist() == [5] * want       # the canonical lines around it are still read
    assert not D.parse(good + other + good, 18)[2]


def test_parse_flags_more_than_four_starts_in_a_slice_only():
    line = (K18 + " 5\n").encode()
    assert not D.parse(line * 4, 18)[2]                         # starts at 0, 21, 42, 63: four in slice 0
    assert D.starts_per_slice(D.line_starts(line * 4), 84).tolist() == [4, 0]
    assert D.parse(b"\n" * 5, 18)[2] and D.parse(line + b"\n" * 64 + line, 18)[2]
    assert D.parse(b"", 18)[2] is False and len(D.parse(b"", 18)[0]) == 0


def test_first_wins_by_hand():
    km = np.array([5, 9, 5, 7, 9, 5, 7], dtype=np.uint64)
    ct = np.array([1, 4, 3, 1, 8, 6, 0], dtype=np.uint32)
    keys, counts = D.first_wins(km, ct, 2)
    assert keys.tolist() == [5, 9] and counts.tolist() == [3, 4]       # 5's first line is below 2; 7 never reaches it
    keys, counts = D.first_wins(km, ct, 1)
    assert keys.tolist() == [5, 7, 9] and counts.tolist() == [1, 1, 4]
    keys, counts = D.first_wins(km, ct, 1000)
    assert len(keys) == 0 and len(counts) == 0


# ---------------------------------------------------------------- the layouts hold what the GPU cases claim
def check_layout(lay, k):
    """A layout is what it says: the line starts are where the bytes put them, every line is canonical, and the byte-by-byte
    parse reads the k-mers and counts it was written from."""
    assert D.line_starts(lay.data) == lay.starts.tolist()
    km, ct, flagged = D.parse(lay.data, k)
    assert not flagged and (km == lay.kmers).all() and (ct == lay.counts).all()
    assert all(k + 3 <= len(line) <= k + 11 for line in lay.lines)
    return km, ct


def test_layout_places_every_named_byte():
    rng = np.random.default_rng(3)
    for k in (18, 25, 31):
        place = [(1000 + 500 * i, what) for i, what in enumerate(D.WHATS)]
        lay = D.layout(k, None, rng, place=place, end=6001)
        check_layout(lay, k)
        assert len(lay.data) == 6001
        for off, what in place:
            names, line = D.what_is_at(lay, k, off)
            assert what in names, (k, off, what, names)
            byte = lay.data[off]
            assert {"start": byte in b"ACGTacgt", "first_letter": byte in b"ACGTacgt", "last_letter": byte in b"ACGTacgt" and lay.data[off + 1] in b" \t",
                    "blank": byte in b" \t", "first_digit": lay.data[off - 1] in b" \t", "last_digit": lay.data[off + 1] == 10,
                    "newline": byte == 10}[what]
    counts = set(D.layout(21, 4000, rng, min_count=5).counts.tolist())
    assert {0, 1, 4, 5, 999999999} <= counts
    lay = D.layout(21, 400, rng)
    assert any(line.split()[1].startswith(b"0") and len(line.split()[1]) > 1 for line in lay.lines)      # leading zeros
    assert any(b"\t" in line for line in lay.lines) and any(line[:21].islower() for line in lay.lines)
    with pytest.raises(ValueError):
        D.layout(21, None, rng, place=[(20, "start")], end=500)           # no whole line fits before it


def test_case_a_fills_a_slice_with_four_starts():
    lay = DC.case_a()
    check_layout(lay, 18)
    per = D.starts_per_slice(lay.starts, len(lay.data))
    assert per.max() == 4 and int((per == 4).sum()) >= 1 and len(lay.data) > 3 * TILE and len(lay.data) % TILE
    assert set((lay.starts % SLICE).tolist()) == set(range(SLICE))      # every phase of a line against a slice
    assert {len(line) for line in lay.lines} == {21}


@pytest.mark.parametrize("k", range(18, 32))
def test_case_b_holds_both_homopolymers_and_both_blanks(k):
    lay = DC.case_b(k)
    km, ct = check_layout(lay, k)
    assert len(lay.data) == 40960 and km[0] == (1 << (2 * k)) - 1 and km[1] == 0
    assert any(b"\t" in line for line in lay.lines) and any(b" " in line for line in lay.lines)
    assert any(line[:k].islower() for line in lay.lines) and any(line[:k].isupper() for line in lay.lines)
    kept = [int((ct >= m).sum()) for m in (1, 2, 1000)]
    assert kept[0] > kept[1] > kept[2] > 0                       # the three MIN_COUNTs keep different lines


@pytest.mark.parametrize("k", DC.BORDER_KS)
def test_case_c_puts_each_byte_of_a_line_on_each_side_of_the_borders(k):
    first, last = set(), set()
    for j in DC.sweep_js(k):
        lay = DC.case_c(k, j)
        for border in (DC.SLICE_BORDER, TILE, 2 * TILE):
            i = int(np.flatnonzero(lay.starts == border - j)[0])
            assert len(lay.lines[i]) == k + 11
            if j <= k + 10:
                first.add((border, j))                           # byte j of the line is the first byte after the border
            if j >= 1:
                last.add((border, j - 1))                        # byte j - 1 is the last byte before it
            assert lay.data[border - j:border - j + k + 11] == lay.lines[i]
    every = {(b, j) for b in (DC.SLICE_BORDER, TILE, 2 * TILE) for j in range(k + 11)}
    assert first == every and last == every
    lay = DC.case_c_plus_one(k)
    assert {DC.SLICE_BORDER + 1, TILE + 1, 2 * TILE + 1} <= set(lay.starts.tolist())
    assert TILE - 1 in DC.case_c(k, 1).starts and TILE in DC.case_c(k, 0).starts


@pytest.mark.parametrize("k", DC.BORDER_KS)
def test_case_d_ends_where_it_says(k):
    d = DC.case_d(k)
    for lay in d.values():
        check_layout(lay, k)
    assert len(d["one-line"].data) == k + 3 < SLICE and len(d["one-line"].starts) == 1
    assert len(d["multiple-of-64"].data) % SLICE == 0 and len(d["multiple-of-64"].data) % TILE
    assert len(d["multiple-of-tile"].data) == 2 * TILE and d["multiple-of-tile"].data[-1] == 10
    lay = d["tile-plus-one"]
    per_tile = D.starts_per_tile(lay.starts, len(lay.data))
    assert len(lay.data) == 2 * TILE + 1 and len(per_tile) == 3 and per_tile[2] == 0 and lay.data[2 * TILE] == 10
    assert len(d["last-line-shortest"].lines[-1]) == k + 3 and len(d["last-line-longest"].lines[-1]) == k + 11


def test_case_e_and_f_are_what_they_say():
    lay = DC.case_e()
    check_layout(lay, 21)
    assert len(lay.data) == 200_000 and any(c % 64 for c in DC.UPLOAD_CHUNKS) and len(lay.data) in DC.UPLOAD_CHUNKS
    base = DC.case_f_base()
    check_layout(base, DC.F_K)
    for kind, pos in DC.f_combinations():
        data, at = DC.case_f(base, kind, pos)
        assert D.parse(data, DC.F_K)[2], (kind, pos)
        if pos == "first-line":
            assert at == 0
        elif pos == "first-line-of-a-tile":
            assert at == 2 * TILE
        elif pos == "across-a-tile-border":
            assert at < TILE and (at + len(DC.bad_line(kind, base.lines[0])) > TILE or kind == "empty-line")
        elif pos == "mid-file":
            assert TILE // 4 < at < TILE // 2 + 100
        else:
            assert at == base.starts[-1]
    lay = DC.lower_and_tab()
    check_layout(lay, DC.F_K)
    assert all(line[:21].islower() and line[21:22] == b"\t" for line in lay.lines)


# ---------------------------------------------------------------- the host parser through the hook
def host_equals_reference(path, data, k, min_count=2):
    km, ct, flagged = D.parse(data, k)
    assert not flagged
    r = T.parse_text_hook(path, k, min_count, where=0)
    assert r["n_lines"] == r["nread"] == len(km) and r["nbad"] == 0 and r["kept"] == int((ct >= min_count).sum())
    assert (r["kmers"] == km).all() and (r["counts"] == ct).all()


def test_host_parser_on_every_canonical_file(tmp_path):
    p = str(tmp_path / "f.txt")
    host_equals_reference(DC.write(p, DC.case_a().data), DC.case_a().data, 18)
    for k in range(18, 32):
        host_equals_reference(DC.write(p, DC.case_b(k).data), DC.case_b(k).data, k, (1, 2, 1000)[k % 3])
    for k in DC.BORDER_KS:
        for lay in [DC.case_c(k, j) for j in DC.sweep_js(k)] + [DC.case_c_plus_one(k)] + list(DC.case_d(k).values()):
            host_equals_reference(DC.write(p, lay.data), lay.data, k)
    for lay in (DC.case_e(), DC.lower_and_tab(), DC.case_f_base()):
        host_equals_reference(DC.write(p, lay.data), lay.data, 21)


def test_hook_reports_sizes_and_refuses_what_it_cannot_do(tmp_path):
    lay = DC.case_d(21)["multiple-of-64"]
    p = DC.write(tmp_path / "f.txt", lay.data)
    L = T.lib()
    n, kept, flags = C.c_uint64(), C.c_uint64(), C.c_uint64()
    args = (p.encode(), 21, 2, 0, 0, 0, 0)
    assert L.talc_test_parse_text(*args, None, None, 0, C.byref(n), C.byref(kept), C.byref(flags)) == 0
    assert n.value == len(lay.starts) and kept.value == int((lay.counts >= 2).sum()) and flags.value == 0
    km = np.zeros(n.value, dtype=np.uint64)
    ct = np.zeros(n.value, dtype=np.uint32)
    n.value = 0
    assert L.talc_test_parse_text(*args, km.ctypes.data, ct.ctypes.data, len(km) - 1, C.byref(n), None, None) == -5      # TALC_ERR_CAPACITY
    assert n.value == len(km) and b"too small" in L.talc_last_error()
    assert L.talc_test_parse_text(*args, km.ctypes.data, None, len(km), None, None, None) == 0 and (km == lay.kmers).all()
    assert L.talc_test_parse_text(p.encode(), 21, 2, 2, 0, 0, 0, None, None, 0, None, None, None) == -1                 # no such `where`
    assert L.talc_test_parse_text(p.encode(), 17, 2, 0, 0, 0, 0, None, None, 0, None, None, None) == -1
    assert L.talc_test_parse_text(str(tmp_path / "none").encode(), 21, 2, 0, 0, 0, 0, None, None, 0, None, None, None) == -2


def test_host_parser_where_its_threads_cut_the_file(tmp_path):
    """parseDumpFile cuts a file of 1 MiB or more at size / T * t and moves each cut to the next line start.  Three files
    of one size: at every cut one has a line start, one a newline, one the inside of a line."""
    L = T.lib()
    threads = min(int(L.omp_get_max_threads()), 128)            # the OpenMP runtime the library itself runs on
    size = (1 << 20) + 12345
    cuts = [size // threads * t for t in range(1, threads)]
    whats = ("start", "newline", "last_letter")
    seen = set()
    for r in range(3):
        place = [(c, whats[(i + r) % 3]) for i, c in enumerate(cuts)]
        lay = D.layout(21, None, DC.rng_for(8, r), place=place, end=size, case="upper")
        assert len(lay.data) == size
        for (c, what), i in zip(place, range(len(place))):
            assert what in D.what_is_at(lay, 21, c)[0]
            seen.add((c, what))
        host_equals_reference(DC.write(tmp_path / "f.txt", lay.data), lay.data, 21)
    assert seen == {(c, w) for c in cuts for w in whats}


# ---------------------------------------------------------------- lines only the tokeniser takes: the oracle decides
def test_host_table_of_files_with_other_lines_equals_the_oracle(tmp_path):
    base = DC.case_f_base()
    p, q = PU.both_params(k=DC.F_K)
    probe = np.unique(np.concatenate([base.kmers, DC.rng_for(9).integers(0, 1 << 42, 2000, dtype=np.uint64)]))
    path = str(tmp_path / "f.txt")
    for kind, pos in DC.f_combinations():
        data, _ = DC.case_f(base, kind, pos)
        DC.write(path, data)
        ot = O.OracleTable(q, O.OracleTable.MAP)
        want = ot.build_from_files(path, None)
        tt = T.Table.from_files(path, None, p)
        assert tt.build_stats.tolist() == want.tolist(), (kind, pos)
        oc, oj = ot.lookup_packed(probe)
        tc, tj = tt.lookup_host(probe)
        assert (oc == tc).all() and (oj == tj).all(), (kind, pos)
        if kind not in ("k-minus-1-letters", "k-plus-1-letters", "an-N"):     # (the oracle's map also holds those keys: nothing can look them up)
            assert len(ot) == len(tt), (kind, pos)


# ---------------------------------------------------------------- the large file of the production constants
@pytest.fixture(scope="module")
def prod():
    return D.production_layout()


def test_production_file_is_what_its_arrays_say(prod):
    data, starts, size = prod["data"], prod["starts"], prod["size"]
    assert size > D.PROD_CHUNK and size - D.PROD_CHUNK < (2 << 20) and len(data) == size
    assert (np.concatenate([[0], np.flatnonzero(data == 10)[:-1] + 1]) == starts).all() and data[-1] == 10
    b = prod["border_line"]
    for lo, hi in ((0, 3000), (b - 1500, b + 1500), (len(starts) - 3000, len(starts))):       # byte by byte where it matters
        end = int(starts[hi]) if hi < len(starts) else size
        km, ct, flagged = D.parse(data[int(starts[lo]):end].tobytes(), D.PROD_K)
        assert not flagged and (km == prod["kmers"][lo:hi]).all() and (ct == prod["counts"][lo:hi]).all()
    assert D.starts_per_slice(starts, size).max() <= 4
    counts, i = prod["counts"], np.arange(len(starts))
    low = (i % 7 == 0) & ((i < prod["zone"][0]) | (i >= prod["zone"][1]))
    assert (counts[low] == 1).all() and (counts[~low] == i[~low] + 2).all() and low.sum() > 100_000


def test_production_file_has_duplicates_on_both_sides_of_the_chunk_border(prod):
    kmers, counts, b = prod["kmers"], prod["counts"], prod["border_line"]
    assert prod["starts"][b - 1] < D.PROD_CHUNK <= prod["starts"][b]
    keys, wins = D.first_wins(kmers, counts, D.PROD_MIN_COUNT)
    assert 55_000 < len(keys) <= 60_000 and len(kmers) / len(keys) > 15
    before, after = np.unique(kmers[:b]), np.unique(kmers[b:])
    assert len(np.intersect1d(before, after)) > 20_000                    # k-mers with lines in both upload chunks
    # the winner is read from the answer: a count names its line
    win_line = wins.astype(np.int64) - 2
    assert (kmers[win_line] == keys).all()
    # k-mers won after the border although they have earlier lines (all below MIN_COUNT), and the other way round
    late_winners = keys[win_line >= b]
    assert len(late_winners) > 500 and np.isin(late_winners, before).all()
    assert len(np.intersect1d(keys[win_line < b], after)) > 20_000
    z0, z1 = prod["zone"]
    zone = np.arange(z0, z1)
    assert np.isin(zone, win_line).all()                                  # every kept line of the border's tiles is a winner
    assert prod["starts"][z0] // TILE < D.PROD_CHUNK // TILE - 1 and prod["starts"][z1] // TILE > D.PROD_CHUNK // TILE + 1


def test_a_wrong_tile_base_changes_the_table_of_the_production_file(prod):
    """What the seam is there to catch, shown on the reference side: number the lines as the two kernels do, with the first
    line number of one tile one too large, and the first-wins table differs from the true one; so case G's file notices
    a tile (or a chunk) that lands off by one line."""
    starts, size, kmers, counts = prod["starts"], prod["size"], prod["kmers"], prod["counts"]
    ok_k, ok_c = D.numbered_by_tiles(starts, size, kmers, counts)
    assert (ok_k == kmers).all() and (ok_c == counts).all()
    keys, wins = D.first_wins(kmers, counts, D.PROD_MIN_COUNT)
    border_tile = D.PROD_CHUNK // TILE
    for tile in (border_tile - 2, border_tile - 1, border_tile, border_tile + 1):
        for later_tile_wins in (True, False):
            bk, bc = D.numbered_by_tiles(starts, size, kmers, counts, wrong_tile=tile, later_tile_wins=later_tile_wins)
            k2, w2 = D.first_wins(bk, bc, D.PROD_MIN_COUNT)
            assert not (len(k2) == len(keys) and (k2 == keys).all() and (w2 == wins).all()), (tile, later_tile_wins)
