"""The UMI read-out (docs/umi.md) stated twice: in plain Python, the full Sellers matrix one cell at a time and the
traceback as the contract words it (end_plain, row_plain), and in numpy, the matrix row by row over both end windows of a
read at once (rows).  Neither knows anything of the device's bit vectors, of its chunks or of its restarted columns;
tests/test_umi_reference.py holds the two against each other, the GPU tests hold the device against rows()."""
import numpy as np

import ends_ref as R

DTYPE = np.dtype([("end", "u1"), ("err", "u1"), ("other_err", "u1"), ("umi_len", "u1"), ("start", "<u4"), ("stop", "<u4"),
                  ("kept_start", "<u4"), ("kept_len", "<u4"), ("umi", "S32"), ("pad_", "<u4")])
assert DTYPE.itemsize == 56
DEFAULT_WINDOW = 256
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
BARE = "TTTVVVVTTVVVVTTVVVVTTVVVVTTT"
ANCHORED = "GCTGATATTGCTTTVVVVTTVVVVTTVVVVTTVVVVTTTGGG"


def sets_of(pattern):
    return [IUPAC[ch] for ch in (pattern.decode() if isinstance(pattern, bytes) else pattern).upper()]


def degenerate(pattern):
    """The 0-based positions of the pattern whose set has more than one base."""
    return [i for i, s in enumerate(sets_of(pattern)) if len(s) > 1]


def check_params(pattern, max_error_pct, window):
    sets = sets_of(pattern)
    assert 12 <= len(sets) <= 64 and 1 <= len(degenerate(pattern)) <= 32
    assert 0 <= max_error_pct <= 30 and 32 <= window <= 4096
    return max_error_pct * len(sets) // 100


def kept(L, end, stop, head=0, tail=0):
    """(kept_start, kept_len) of a read of L bytes: the end clean-up claims head and tail, the UMI `stop` at its end."""
    h = max(head, stop if end == 1 else 0)
    t = max(tail, stop if end == 2 else 0)
    return h, L - h - min(t, L - h)


# ------------------------------------------------------------------ plain loops
def end_plain(S, pattern, max_error_pct, window=DEFAULT_WINDOW):
    """U(S): None when the end is not accepted, else (err, start, stop, umi)."""
    S = R.as_bytes(S).upper()
    T = S[:min(len(S), window)]
    sets = sets_of(pattern)
    m, n = len(sets), len(T)
    k = max_error_pct * m // 100
    cost = lambda i, j: 0 if chr(T[j - 1]) in sets[i - 1] else 1
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        D[i][0] = i
        for j in range(1, n + 1):
            D[i][j] = min(D[i - 1][j - 1] + cost(i, j), D[i - 1][j] + 1, D[i][j - 1] + 1)
    d = min(D[m][1:]) if n else m
    if d > k:
        return None
    stop = max(j for j in range(1, n + 1) if D[m][j] == d)
    under = {}
    i, j = m, stop
    while i > 0:
        if j > 0 and D[i - 1][j - 1] + cost(i, j) == D[i][j]:
            under[i - 1] = chr(T[j - 1]) if chr(T[j - 1]) in "ACGT" else "N"
            i, j = i - 1, j - 1
        elif D[i - 1][j] + 1 == D[i][j]:
            under[i - 1] = "-"
            i -= 1
        else:
            j -= 1
    return d, j, stop, "".join(under[p] for p in degenerate(pattern))


def steps_plain(S, pattern, window=DEFAULT_WINDOW):
    """The canonical traceback of U(S) from the smallest D of the last row, whatever it is, as a list of
    (i, j, diagonal holds, up holds, left holds, the step taken: "D", "U" or "L"): what the hand cases aim at."""
    S = R.as_bytes(S).upper()
    T = S[:min(len(S), window)]
    sets = sets_of(pattern)
    m, n = len(sets), len(T)
    cost = lambda i, j: 0 if chr(T[j - 1]) in sets[i - 1] else 1
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        D[i][0] = i
        for j in range(1, n + 1):
            D[i][j] = min(D[i - 1][j - 1] + cost(i, j), D[i - 1][j] + 1, D[i][j - 1] + 1)
    d = min(D[m][1:])
    i, j = m, max(j for j in range(1, n + 1) if D[m][j] == d)
    out = []
    while i > 0:
        dg = j > 0 and D[i - 1][j - 1] + cost(i, j) == D[i][j]
        up = D[i - 1][j] + 1 == D[i][j]
        lf = j > 0 and D[i][j - 1] + 1 == D[i][j]
        take = "D" if dg else "U" if up else "L"
        out.append((i, j, dg, up, lf, take))
        i, j = (i - 1, j - 1) if dg else (i - 1, j) if up else (i, j - 1)
    return out


def pick(h, t):
    """(end, err, other_err, start, stop, umi) of a read from its two ends (None: not accepted)."""
    if h is None and t is None:
        return 0, 0, 255, 0, 0, ""
    if h is not None and (t is None or h[0] <= t[0]):
        return (1, h[0], 255 if t is None else t[0]) + tuple(h[1:])
    return (2, t[0], 255 if h is None else h[0]) + tuple(t[1:])


def row_plain(S, pattern, max_error_pct, window=DEFAULT_WINDOW):
    p = pick(end_plain(S, pattern, max_error_pct, window), end_plain(R.revcomp(S), pattern, max_error_pct, window))
    ks, kl = kept(len(S), p[0], p[4])
    return (p[0], p[1], p[2], len(p[5]), p[3], p[4], ks, kl, p[5].encode(), 0)


def rows_plain(reads, pattern, max_error_pct, window=DEFAULT_WINDOW):
    check_params(pattern, max_error_pct, window)
    return np.array([row_plain(r, pattern, max_error_pct, window) for r in reads], dtype=DTYPE)


# ------------------------------------------------------------------ numpy, the matrix row by row
_MASK = np.zeros(256, np.int64)
for _ch, _set in IUPAC.items():
    _MASK[ord(_ch)] = _MASK[ord(_ch) + 32] = sum(1 << "ACGT".index(b) for b in _set)


def matrix(masks, texts):
    """D[t, i, j] of the pattern (m sets as masks over the codes) over each of the texts (E x n codes; 4: in no set): row i
    from row i - 1 for all columns at once; the run of steps along a row is a running minimum."""
    m = len(masks)
    E, n = texts.shape
    idx = np.arange(n + 1, dtype=np.int32)
    D = np.zeros((E, m + 1, n + 1), np.int32)
    hit = (masks[:, None, None] >> np.minimum(texts, 4)[None, :, :].astype(np.int64)) & 1      # m x E x n
    hit &= (texts < 4)[None, :, :]
    for i in range(1, m + 1):
        new = np.empty((E, n + 1), np.int32)
        new[:, 0] = i
        new[:, 1:] = np.minimum(D[:, i - 1, :-1] + (1 - hit[i - 1]).astype(np.int32), D[:, i - 1, 1:] + 1)
        D[:, i, :] = np.minimum.accumulate(new - idx, axis=1) + idx
    return D


def _end_numpy(D, codes, masks, degen, k):
    """The end rule and the traceback on the matrix D[i, j] of one end window."""
    m, n = D.shape[0] - 1, D.shape[1] - 1
    if not n:
        return None
    d = int(D[m, 1:].min())
    if d > k:
        return None
    stop = n - int(np.argmax(D[m, :0:-1] == d))
    under = {}
    i, j = m, stop
    while i > 0:
        c = int(codes[j - 1]) if j > 0 else 4
        cost = 0 if c < 4 and (int(masks[i - 1]) >> c) & 1 else 1
        if j > 0 and D[i - 1, j - 1] + cost == D[i, j]:
            under[i - 1] = "ACGTN"[c]
            i, j = i - 1, j - 1
        elif D[i - 1, j] + 1 == D[i, j]:
            under[i - 1] = "-"
            i -= 1
        else:
            j -= 1
    return d, j, stop, "".join(under[p] for p in degen)


def rows(reads, pattern, max_error_pct, window=DEFAULT_WINDOW, claims=None):
    """One DTYPE row per read of `reads` (bytes or str).  claims: per read (head, tail) of the end clean-up, which the kept
    interval combines with."""
    k = check_params(pattern, max_error_pct, window)
    masks = _MASK[np.frombuffer(R.as_bytes(pattern), np.uint8)]
    degen = degenerate(pattern)
    out = np.zeros(len(reads), DTYPE)
    for r, rd in enumerate(reads):
        c = R._CODE[np.frombuffer(R.as_bytes(rd), np.uint8)]
        n = min(len(c), window)
        h = t = None
        if n:
            tc = c[len(c) - n:][::-1]
            both = np.stack([c[:n], np.where(tc < 4, 3 - tc, tc)])
            D = matrix(masks, both)
            h = _end_numpy(D[0], both[0], masks, degen, k)
            t = _end_numpy(D[1], both[1], masks, degen, k)
        p = pick(h, t)
        head, tail = claims[r] if claims is not None else (0, 0)
        ks, kl = kept(len(c), p[0], p[4], int(head), int(tail))
        out[r] = (p[0], p[1], p[2], len(p[5]), p[3], p[4], ks, kl, p[5].encode(), 0)
    return out


def claims_of(end_rows):
    """(head, tail) per read from ends_ref.DTYPE rows."""
    return [(int(e["head_adapter_len"]) + int(e["head_poly_len"]), int(e["tail_adapter_len"]) + int(e["tail_poly_len"])) for e in end_rows]


def clip(reads, table):
    """The kept interval of every read, as bytes."""
    return [R.as_bytes(r)[int(t["kept_start"]):int(t["kept_start"]) + int(t["kept_len"])] for r, t in zip(reads, table)]


# ------------------------------------------------------------------ planting
def instance(rng, pattern):
    """One concrete copy of the pattern: a random base of every letter's set."""
    return "".join(s[int(rng.integers(len(s)))] for s in sets_of(pattern))


def plant(rng, body, pattern, where, max_edits=0):
    """A copy of the pattern (with up to max_edits edits) before `body` (where 1), its reverse complement behind it (2), both
    (3) or neither (0)."""
    copy = lambda: R.mutate(rng, instance(rng, pattern), int(rng.integers(0, max_edits + 1)), "SID") if max_edits else instance(rng, pattern)
    junk = lambda: R.random_seq(rng, int(rng.integers(0, 6)))
    head = junk() + copy() if where & 1 else ""
    tail = R.revcomp(copy()).decode() + junk() if where & 2 else ""
    return head + body + tail
