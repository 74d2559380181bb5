"""The text dump parsed on the device (talc_kernels_build.h: k_parse_count, k_parse_lines, and the upload in front of them)
against the byte-by-byte contract of tests/dump_ref.py, through the hook talc_test_parse_text: every line's k-mer and count
in file order, the number of kept lines and the flag, on files built so that line starts, blanks, digits and newlines fall
on slice, tile and chunk borders (tests/dump_cases.py; test_dump_reference.py asserts that each file is what its case says).
All comparisons are exact."""
import re

import numpy as np
import pytest

import dump_cases as DC
import dump_ref as D
import parity_util as PU
from talc_amd import lib as T

pytestmark = pytest.mark.gpu
TILE = D.TILE


def device_equals_reference(path, data, k, min_counts=(2,), **upload):
    km, ct, flagged = D.parse(data, k)
    assert not flagged
    for m in min_counts:
        r = T.parse_text_hook(path, k, m, where=1, device=0, **upload)
        assert r["flags"] == 0 and r["n_lines"] == len(km) and r["kept"] == int((ct >= m).sum()), (k, m, upload)
        bad = np.flatnonzero((r["kmers"] != km) | (r["counts"] != ct))
        assert len(bad) == 0, (k, m, upload, "first differing line", int(bad[0]))


def test_a_fullest_slice(tmp_path):
    """K = 18, one-digit counts: 21-byte lines in every phase against a slice, four line starts in one slice."""
    lay = DC.case_a()
    device_equals_reference(DC.write(tmp_path / "a.txt", lay.data), lay.data, 18)


@pytest.mark.parametrize("k", range(18, 32))
def test_b_every_k(tmp_path, k):
    """Random line lengths over 2.5 tiles, both cases of letter, blank or tab, T...T and A...A, MIN_COUNT 1, 2 and 1000."""
    lay = DC.case_b(k)
    device_equals_reference(DC.write(tmp_path / "b.txt", lay.data), lay.data, k, min_counts=(1, 2, 1000))


@pytest.mark.parametrize("k", DC.BORDER_KS)
def test_c_each_byte_of_a_line_on_a_slice_border_and_on_the_tile_borders(tmp_path, k):
    """A line of K + 11 bytes starting j bytes before a slice border inside a tile, before 16384 and before 32768, for
    every j: each of its bytes is once the last byte before the border and once the first after it; and line starts one
    byte after the borders."""
    path = str(tmp_path / "c.txt")
    for lay in [DC.case_c(k, j) for j in DC.sweep_js(k)] + [DC.case_c_plus_one(k)]:
        device_equals_reference(DC.write(path, lay.data), lay.data, k)


@pytest.mark.parametrize("k", DC.BORDER_KS)
def test_d_file_ends(tmp_path, k):
    """One line shorter than a slice; sizes of 64 n, 16384 n and 16384 n + 1 (a last tile that holds the final newline
    only); a last line of the shortest and of the longest kind."""
    for name, lay in DC.case_d(k).items():
        device_equals_reference(DC.write(tmp_path / (name + ".txt"), lay.data), lay.data, k)


def test_e_upload_in_chunks_by_several_readers(tmp_path):
    """One 200 KB file in chunks of 4096, 5000 (device offsets that are no multiple of 64), 65536, the file's size and
    one byte less, by 1, 3 and 8 reader threads."""
    lay = DC.case_e()
    path = DC.write(tmp_path / "e.txt", lay.data)
    for chunk in DC.UPLOAD_CHUNKS:
        for readers in DC.UPLOAD_READERS:
            device_equals_reference(path, lay.data, 21, chunk_bytes=chunk, reader_threads=readers)


def test_f_lines_the_device_refuses(tmp_path):
    """Every kind of line that is not canonical, as the first line, the last, the first of a tile, across a tile border
    and mid-file: the flag is raised (the arrays of such a file mean nothing and are not compared)."""
    base = DC.case_f_base()
    path = str(tmp_path / "f.txt")
    for kind, pos in DC.f_combinations():
        data, _ = DC.case_f(base, kind, pos)
        r = T.parse_text_hook(DC.write(path, data), DC.F_K, 2, where=1, device=0, arrays=False)
        assert r["flags"] != 0, (kind, pos)
    device_equals_reference(DC.write(path, base.data), base.data, DC.F_K)      # the same file without the line: taken


def test_f_lower_case_and_tab_are_canonical(tmp_path):
    lay = DC.lower_and_tab()
    device_equals_reference(DC.write(tmp_path / "l.txt", lay.data), lay.data, DC.F_K)


def test_g_production_constants(tmp_path, capfd, monkeypatch):
    """A dump of a little over 32 MiB through Table.from_files as the product calls it: 32 MiB chunks, two reader threads.
    Every line's count names its line, so the table's answers say which line won: they equal first_wins of the arrays the
    file was written from (numpy only), for k-mers with lines on both sides of the 32 MiB border in particular."""
    prod = D.production_layout()
    kmers, counts, starts, b = prod["kmers"], prod["counts"], prod["starts"], prod["border_line"]
    assert prod["size"] > D.PROD_CHUNK and starts[b - 1] < D.PROD_CHUNK <= starts[b]
    keys, wins = D.first_wins(kmers, counts, D.PROD_MIN_COUNT)
    win_line = wins.astype(np.int64) - 2
    before = np.unique(kmers[:b])
    assert len(np.intersect1d(before, np.unique(kmers[b:]))) > 20_000              # duplicates on both sides of the border,
    assert int(np.isin(keys[win_line >= b], before).sum()) > 500                    # won after it (earlier lines below MIN_COUNT)
    assert int(np.isin(kmers[b:], keys[win_line < b]).sum()) > 20_000               # and won before it
    path = str(tmp_path / "g.txt")
    prod["data"].tofile(path)
    p, _ = PU.both_params(k=D.PROD_K, min_count=D.PROD_MIN_COUNT)
    monkeypatch.setenv("TALC_TIMING", "1")
    capfd.readouterr()
    t = T.Table.from_files(path, None, p, device=0)
    err = capfd.readouterr().err
    assert "dump parsed on the device" in err
    assert int(re.search(r"\((\d+) reader threads\)", err).group(1)) >= 2
    assert len(t) == len(keys)
    assert int(t.build_stats[0]) == len(kmers) and int(t.build_stats[1]) == int((counts >= D.PROD_MIN_COUNT).sum())
    absent = np.random.default_rng(12).integers(0, 1 << 42, 50_000, dtype=np.uint64)
    absent = absent[~np.isin(absent, keys)]
    got, _ = t.lookup_host(np.concatenate([keys, absent]))
    wrong = np.flatnonzero(got[:len(keys)] != wins)
    assert len(wrong) == 0, ("first k-mer with another winner: line", int(win_line[wrong[0]]), "answer", int(got[wrong[0]]))
    assert (got[len(keys):] == 0).all()
