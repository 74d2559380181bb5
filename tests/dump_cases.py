"""The files of the text-dump parser's tests (tests/dump_ref.py builds them): test_gpu_dump_parse.py runs them through the
device parser, test_dump_reference.py through the host parser and asserts of each what its case claims.  A case is built once per process
and shared: nothing changes a layout."""
import functools

import numpy as np

import dump_ref as D

TILE, SLICE = D.TILE, D.SLICE
BORDER_KS = (18, 21, 31)
SLICE_BORDER = 64 * 100          # a slice border inside tile 0


def rng_for(*key):
    return np.random.default_rng([91, *key])


@functools.lru_cache(maxsize=None)
def case_a():
    """A: K = 18, one-digit counts: 21-byte lines over 3 tiles and a partial one; gcd(21, 64) = 1, so a line takes every
    phase against a slice, four starts in one slice (0, 21, 42, 63) among them."""
    return D.layout(18, 2500, rng_for(1), digits=1)


@functools.lru_cache(maxsize=None)
def case_b(k):
    """B: 2.5 tiles of lines of random length, both cases of letter, blank or tab; the first two k-mers are T...T and A...A."""
    return D.layout(k, None, rng_for(2, k), end=TILE * 5 // 2, kmers=[(1 << (2 * k)) - 1, 0])


def sweep_js(k):
    return list(range(0, k + 12))      # a line of K + 11 bytes: j = K + 11 puts its newline last in the tile


@functools.lru_cache(maxsize=None)
def case_c(k, j):
    """C: lines of maximum length that start at the slice border - j, at 16384 - j and at 32768 - j."""
    return D.layout(k, None, rng_for(3, k, j), place=[(SLICE_BORDER - j, "start", 9), (TILE - j, "start", 9), (2 * TILE - j, "start", 9)],
                    end=2 * TILE + 2048)


@functools.lru_cache(maxsize=None)
def case_c_plus_one(k):
    """C: line starts one byte after the borders (one before and exactly on them are j = 1 and j = 0 of the sweep)."""
    return D.layout(k, None, rng_for(3, k, 99), place=[(SLICE_BORDER + 1, "start", 9), (TILE + 1, "start", 9), (2 * TILE + 1, "start", 9)],
                    end=2 * TILE + 2048)


@functools.lru_cache(maxsize=None)
def case_d(k):
    """D: the ends of a file, name -> layout."""
    r = lambda i: rng_for(4, k, i)
    return {
        "one-line": D.layout(k, 1, r(0), digits=1),
        "multiple-of-64": D.layout(k, None, r(1), end=SLICE * 313),
        "multiple-of-tile": D.layout(k, None, r(2), end=2 * TILE),
        "tile-plus-one": D.layout(k, None, r(3), end=2 * TILE + 1),
        "last-line-shortest": D.layout(k, None, r(4), place=[(30000 - (k + 3), "start", 1)], end=30000),
        "last-line-longest": D.layout(k, None, r(5), place=[(30011 - (k + 11), "start", 9)], end=30011),
    }


@functools.lru_cache(maxsize=None)
def case_e():
    """E: 200 KB for the upload's chunks."""
    return D.layout(21, None, rng_for(5), end=200_000)


UPLOAD_CHUNKS = (4096, 5000, 65536, 200_000, 199_999)
UPLOAD_READERS = (1, 3, 8)

# ---------------------------------------------------------------- F: lines the device parser must refuse
F_K = 21
KINDS = ("two-blanks", "leading-blank", "trailing-blank", "crlf", "k-minus-1-letters", "k-plus-1-letters", "an-N", "plus-sign",
         "minus-sign", "kmer-only", "kmer-blank-only", "ten-digits", "empty-line", "64-empty-lines")
END_KINDS = ("no-final-newline", "cut-inside-last-kmer")
POSITIONS = ("first-line", "last-line", "first-line-of-a-tile", "across-a-tile-border", "mid-file")


@functools.lru_cache(maxsize=None)
def case_f_base():
    return D.layout(F_K, None, rng_for(6), place=[(TILE - 10, "start"), (2 * TILE, "start")], end=50_000, case="upper", blank=" ")


def bad_line(kind, line, k=F_K):
    km = line[:k]
    return {
        "two-blanks": km + b"  7\n", "leading-blank": b" " + km + b" 7\n", "trailing-blank": km + b" 7 \n", "crlf": km + b" 7\r\n",
        "k-minus-1-letters": km[:-1] + b" 7\n", "k-plus-1-letters": km + b"A 7\n", "an-N": km[:k // 2] + b"N" + km[k // 2 + 1:] + b" 7\n",
        "plus-sign": km + b" +7\n", "minus-sign": km + b" -7\n", "kmer-only": km + b"\n", "kmer-blank-only": km + b" \n",
        "ten-digits": km + b" 1234567890\n", "empty-line": b"\n", "64-empty-lines": b"\n" * 64,
    }[kind]


def position_line(base, position):
    """Index of the line of case F's base file that `position` names."""
    starts = base.starts
    return {"first-line": 0, "last-line": len(starts) - 1, "first-line-of-a-tile": int(np.flatnonzero(starts == 2 * TILE)[0]),
            "across-a-tile-border": int(np.flatnonzero(starts == TILE - 10)[0]), "mid-file": int(np.searchsorted(starts, 8000))}[position]


def case_f(base, kind, position=None):
    """The base file with one line replaced by its `kind`; the kinds of END_KINDS take no position.  (bytes, byte offset of
    the bad line)"""
    if kind == "no-final-newline":
        return base.data[:-1], int(base.starts[-1])
    if kind == "cut-inside-last-kmer":
        return base.data[:int(base.starts[-1]) + 10], int(base.starts[-1])
    i = position_line(base, position)
    lines = list(base.lines)
    lines[i] = bad_line(kind, lines[i])
    return b"".join(lines), int(base.starts[i])


def f_combinations():
    return [(kind, pos) for kind in KINDS for pos in POSITIONS] + [(kind, None) for kind in END_KINDS]


@functools.lru_cache(maxsize=None)
def lower_and_tab():
    """F, the other way round: all-lower-case k-mers and a tab as the blank are canonical."""
    return D.layout(F_K, None, rng_for(7), end=40_000, case="lower", blank="\t")


def write(path, data):
    with open(path, "wb") as f:
        f.write(bytes(data))
    return str(path)
