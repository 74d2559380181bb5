"""The k-mer spectrum contract in numpy (docs/kmer_spectrum.md): the reference the GPU histogram, the threshold rule and
the CLI's <o>.histo.txt are tested against.

With bins = high + 2: hist[c], 1 <= c <= high, is the number of k-mers with count c; hist[high + 1] gathers every larger
count; hist[0] the entries with count 0.  stats = (distinct, unique, total, max_count)."""
import numpy as np


def histo(counts, high):
    """(hist u64[high + 2], (distinct, unique, total, max_count)) of an array of counts."""
    counts = np.asarray(counts, dtype=np.uint64)
    hist = np.bincount(np.minimum(counts, np.uint64(high + 1)).astype(np.int64), minlength=high + 2).astype(np.uint64)
    stats = (len(counts), int((counts == 1).sum()), int(counts.sum(dtype=np.uint64)), int(counts.max()) if len(counts) else 0)
    return hist, stats


def threshold(hist, high, limit=0, fallback=2):
    """(chosen, valley): valley = the smallest c in [1, min(limit, high - 1)] with hist[c + 1] > 0 and hist[c] <= hist[c + 1],
    0 when there is none; limit 0 means 32.  chosen = max(2, valley) with a valley, else fallback."""
    L = min(limit or 32, high - 1)
    for c in range(1, L + 1):
        if int(hist[c + 1]) > 0 and int(hist[c]) <= int(hist[c + 1]):
            return max(2, c), c
    return fallback, 0


def histo_text(hist):
    """`jellyfish histo` text with its defaults: 'c n' for every c in 1 .. high + 1 with n > 0, ascending."""
    return b"".join(b"%d %d\n" % (c, int(hist[c])) for c in range(1, len(hist)) if int(hist[c]) > 0)
