"""The solidity report's contract (docs/solidity.md) in plain numpy: the six integers of talc_solidity for one sequence,
from the table's counts alone — a {packed k-mer: count} dict or Table.lookup_host.  Never from a device result."""
import numpy as np

FIELDS = ("n_kmers", "n_solid", "n_in", "n_regions", "solid_bases", "longest_weak")
DTYPE = np.dtype([(f, "<u4") for f in FIELDS])
COMP = str.maketrans("ACGTN", "TGCAN")
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def dna5(seq):
    """SeqAn's Dna5 conversion: upper case, everything but ACGT becomes N."""
    return "".join(c if c in "ACGT" else "N" for c in seq.upper())


def revcomp(s):
    return s.translate(COMP)[::-1]


def pack(kmer):
    """A k-mer of ACGT as the table packs it: 2 bits per base, first base most significant."""
    v = 0
    for ch in kmer:
        v = (v << 2) | "ACGT".index(ch)
    return v


def kmers_of(seq, k):
    """(packed k-mers uint64[n], has_N bool[n]) of the n = max(0, L - k + 1) positions of seq."""
    codes = _CODE[np.frombuffer(seq.encode(), dtype=np.uint8)] if seq else np.zeros(0, np.uint8)
    n = max(0, len(seq) - k + 1)
    km = np.zeros(n, dtype=np.uint64)
    bad = np.zeros(n, dtype=bool)
    for j in range(k if n else 0):
        c = codes[j:j + n]
        km = (km << np.uint64(2)) | (c & 3).astype(np.uint64)
        bad |= c > 3
    return km, bad


def dict_lookup(table):
    """A lookup over a {packed k-mer: count} dict."""
    return lambda kms: np.array([table.get(int(x), 0) for x in kms.tolist()], dtype=np.uint32)


def host_lookup(ttab):
    """A lookup over the host image of a product table (Table.lookup_host: no device involved)."""
    return lambda kms: ttab.lookup_host(kms)[0] if len(kms) else np.zeros(0, np.uint32)


def counts(seq, k, lookup):
    """c[i]: the table count of seq[i, i + k), 0 when the k-mer is absent or holds an N."""
    km, bad = kmers_of(seq, k)
    c = np.zeros(len(km), dtype=np.uint32)
    if (~bad).any():
        c[~bad] = lookup(km[~bad])
    return c


def row_of_counts(c, L, k, minc):
    """The six integers from c[0 .. n) for a sequence of L bases."""
    n = len(c)
    assert n == max(0, L - k + 1)
    solid = np.asarray(c) >= minc
    d = np.diff(np.concatenate([[0], solid.astype(np.int8), [0]]))
    starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]          # runs [start, end)
    cover = np.zeros(L + 1, dtype=np.int64)
    np.add.at(cover, starts, 1)
    np.add.at(cover, ends + k - 1, -1)                                      # the run's k-mers cover bases [start, end - 1 + k)
    wd = np.diff(np.concatenate([[0], (~solid).astype(np.int8), [0]]))
    wl = np.nonzero(wd == -1)[0] - np.nonzero(wd == 1)[0]
    return (n, int(solid.sum()), int((np.asarray(c) > minc).sum()), len(starts), int((np.cumsum(cover)[:L] > 0).sum()),
            int(wl.max()) if len(wl) else 0)


def row(seq, k, minc, lookup):
    return row_of_counts(counts(seq, k, lookup), len(seq), k, minc)


def rows(seqs, k, minc, lookup):
    """One DTYPE record per sequence."""
    out = np.zeros(len(seqs), dtype=DTYPE)
    for i, s in enumerate(seqs):
        out[i] = row(s, k, minc, lookup)
    return out


def brute_row(seq, k, minc, table):
    """The same six integers by loops over positions and bases, from a {packed k-mer: count} dict."""
    L = len(seq)
    n = max(0, L - k + 1)
    c = []
    for i in range(n):
        w = seq[i:i + k]
        c.append(0 if any(ch not in "ACGT" for ch in w) else table.get(pack(w), 0))
    covered = [False] * L
    n_solid = n_in = n_regions = longest = run = 0
    for i in range(n):
        if c[i] >= minc:
            n_solid += 1
            n_regions += 1 if (i == 0 or c[i - 1] < minc) else 0
            run = 0
            for j in range(i, i + k):
                covered[j] = True
        else:
            run += 1
            longest = max(longest, run)
        n_in += 1 if c[i] > minc else 0
    return (n, n_solid, n_in, n_regions, sum(covered), longest)
