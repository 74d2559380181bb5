"""Barcode demultiplexing (docs/demux.md) stated twice: in plain Python, one read and one cell at a time over
ends_ref.sellers_plain (end_plain, row_plain), and in numpy, Sellers row by row over all columns of an end window and all
barcodes at once (rows).  Neither knows anything of the device's bit vectors, of its chunks or of how it deals patterns to
lanes; tests/test_demux_reference.py holds the two against each other, the GPU tests hold the device against rows()."""
import numpy as np

import ends_ref as R

DTYPE = np.dtype([("barcode", "u1"), ("status", "u1"), ("head_best", "u1"), ("head_err", "u1"), ("head_margin", "u1"),
                  ("tail_best", "u1"), ("tail_err", "u1"), ("tail_margin", "u1"), ("head_end", "<u4"), ("tail_end", "<u4")])
assert DTYPE.itemsize == 16
NONE, BOTH, HEAD_ONLY, TAIL_ONLY, CONFLICT = range(5)
DEFAULT_WINDOW = 256


def check_params(barcodes, max_error_pct, min_margin, window):
    assert 1 <= len(barcodes) <= 96 and len({len(b) for b in barcodes}) == 1 and 12 <= len(barcodes[0]) <= 64
    assert all(set(R.as_bytes(b).upper()) <= set(b"ACGT") for b in barcodes)
    k = max_error_pct * len(barcodes[0]) // 100
    assert 0 <= max_error_pct <= 30 and 32 <= window <= 4096 and 0 <= min_margin <= k + 1
    return k


def read_call(h, t, both_ends):
    """(barcode, status) from the two ends' calls (0: none)."""
    if h and h == t:
        return h, BOTH
    if h and t:
        return 0, CONFLICT
    if h:
        return (0 if both_ends else h), HEAD_ONLY
    if t:
        return (0 if both_ends else t), TAIL_ONLY
    return 0, NONE


# ------------------------------------------------------------------ plain loops
def end_plain(S, barcodes, max_error_pct, min_margin, window=DEFAULT_WINDOW):
    """E(S): (best, err, margin, end, call)."""
    S = R.as_bytes(S).upper()
    T = S[:min(len(S), window)]
    m = len(barcodes[0])
    k = max_error_pct * m // 100
    Ds, c = [], []
    for b in barcodes:
        D = R.sellers_plain(R.as_bytes(b).upper(), T)
        d = min(D[1:]) if T else m
        Ds.append((D, d))
        c.append(min(d, k + 1))
    best = min(range(len(barcodes)), key=lambda b: (c[b], b))
    if c[best] > k:
        return 0, 0, 0, 0, 0
    D, d = Ds[best]
    end = max(e for e in range(1, len(T) + 1) if D[e] == d)
    second = min([c[b] for b in range(len(barcodes)) if b != best], default=k + 1)
    margin = second - c[best]
    return best + 1, c[best], margin, end, (best + 1 if margin >= min_margin else 0)


def row_plain(S, barcodes, max_error_pct, min_margin, window=DEFAULT_WINDOW, both_ends=False):
    h = end_plain(S, barcodes, max_error_pct, min_margin, window)
    t = end_plain(R.revcomp(S), barcodes, max_error_pct, min_margin, window)
    barcode, status = read_call(h[4], t[4], both_ends)
    return (barcode, status, h[0], h[1], h[2], t[0], t[1], t[2], h[3], t[3])


def rows_plain(reads, barcodes, max_error_pct, min_margin, window=DEFAULT_WINDOW, both_ends=False):
    check_params(barcodes, max_error_pct, min_margin, window)
    return np.array([row_plain(r, barcodes, max_error_pct, min_margin, window, both_ends) for r in reads], dtype=DTYPE)


# ------------------------------------------------------------------ numpy, Sellers row by row
def _patterns(barcodes):
    return np.stack([R._CODE[np.frombuffer(R.as_bytes(b), np.uint8)].astype(np.int64) for b in barcodes])


def sellers_rows(pats, texts):
    """D[t, b, e], e = 0 .. n, of every pattern of pats (B x m codes) over each of the texts (E x n codes; 4: matches nothing):
    row i of the table from row i - 1 for all columns at once; the run of steps along a row is a running minimum."""
    B, m = pats.shape
    E, n = texts.shape
    idx = np.arange(n + 1, dtype=np.int16)                            # (no value exceeds m + n <= 64 + 4096)
    prev = np.zeros((E, B, n + 1), np.int16)                          # row 0: a match may start anywhere
    texts = texts.astype(np.int64)
    for i in range(1, m + 1):
        cost = (pats[None, :, i - 1, None] != texts[:, None, :]).astype(np.int16)
        new = np.empty_like(prev)
        new[:, :, 0] = i
        new[:, :, 1:] = np.minimum(prev[:, :, :-1] + cost, prev[:, :, 1:] + 1)
        prev = np.minimum.accumulate(new - idx, axis=2) + idx
    return prev


def _end_numpy(D, n, pats, k, min_margin):
    """The end rule on D[b, e], e = 1 .. n, of one end window."""
    B, m = pats.shape
    d = D.min(axis=1) if n else np.full(B, m, np.int64)
    c = np.minimum(d, k + 1)
    best = int(np.argmin(c))                                          # (the first of equal minima)
    if c[best] > k:
        return 0, 0, 0, 0, 0
    end = n - int(np.argmax(D[best][::-1] == d[best]))
    others = np.delete(c, best)
    margin = int(others.min() if len(others) else k + 1) - int(c[best])
    return best + 1, int(c[best]), margin, end, (best + 1 if margin >= min_margin else 0)


def rows(reads, barcodes, max_error_pct, min_margin, window=DEFAULT_WINDOW, both_ends=False):
    """One DTYPE row per read of `reads` (bytes or str)."""
    k = check_params(barcodes, max_error_pct, min_margin, window)
    pats = _patterns(barcodes)
    out = np.zeros(len(reads), DTYPE)
    for r, rd in enumerate(reads):
        c = R._CODE[np.frombuffer(R.as_bytes(rd), np.uint8)]
        n = min(len(c), window)
        tc = c[len(c) - n:][::-1]
        D = sellers_rows(pats, np.stack([c[:n], np.where(tc < 4, 3 - tc, tc)]))[:, :, 1:] if n else (None, None)
        h = _end_numpy(D[0], n, pats, k, min_margin)
        t = _end_numpy(D[1], n, pats, k, min_margin)
        barcode, status = read_call(h[4], t[4], both_ends)
        out[r] = (barcode, status, h[0], h[1], h[2], t[0], t[1], t[2], h[3], t[3])
    return out


# ------------------------------------------------------------------ barcode sets, dressed reads
def edit_distances(cand, others):
    """The global unit-cost edit distance of `cand` to each of `others` (equal lengths), row by row."""
    a = np.frombuffer(R.as_bytes(cand), np.uint8)
    O = np.stack([np.frombuffer(R.as_bytes(o), np.uint8) for o in others])
    n = O.shape[1]
    idx = np.arange(n + 1)
    prev = np.tile(idx, (len(others), 1))
    for i in range(1, len(a) + 1):
        new = np.empty_like(prev)
        new[:, 0] = i
        new[:, 1:] = np.minimum(prev[:, :-1] + (O != a[i - 1]), prev[:, 1:] + 1)
        prev = np.minimum.accumulate(new - idx, axis=1) + idx
    return prev[:, n]


def barcode_set(count, m=24, seed=0, min_dist=9):
    """`count` random m-mers from a fixed seed, each redrawn until its edit distance to every earlier one is >= min_dist."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        cand = R.random_seq(rng, m)
        if not out or int(edit_distances(cand, out).min()) >= min_dist:
            out.append(cand)
    return out


def min_pairwise_distance(barcodes):
    return min(int(edit_distances(barcodes[i], barcodes[:i]).min()) for i in range(1, len(barcodes)))


def dress(rng, body, barcode, primers, max_edits=0):
    """barcode, junk of 0 to 10 bases, primer, poly-T, the body, and the mirror image at the tail; `max_edits` edits at most
    in each copy of the barcode."""
    ssp, vnp = primers
    copy = lambda: R.mutate(rng, barcode, int(rng.integers(0, max_edits + 1)), "SID") if max_edits else barcode
    head = copy() + R.random_seq(rng, int(rng.integers(0, 11))) + vnp + "T" * int(rng.integers(15, 40))
    tail = "A" * int(rng.integers(15, 40)) + R.revcomp(ssp).decode() + R.random_seq(rng, int(rng.integers(0, 11))) + R.revcomp(copy()).decode()
    return head + body + tail
