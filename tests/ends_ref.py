"""The long-read end clean-up (docs/read_ends.md) stated twice: in plain Python, one read and one cell at a time
(head_plain, row_plain), and in numpy over a whole batch (rows).  Neither knows anything of the device's bit vectors or of
its chunking; tests/test_ends_reference.py holds the two against each other, the GPU tests hold the device against rows()."""
import numpy as np

DTYPE = np.dtype([("head_adapter_len", "<u4"), ("head_poly_len", "<u4"), ("tail_adapter_len", "<u4"), ("tail_poly_len", "<u4"),
                  ("head_adapter", "u1"), ("head_adapter_err", "u1"), ("tail_adapter", "u1"), ("tail_adapter_err", "u1"),
                  ("kept_start", "<u4"), ("kept_len", "<u4"), ("orient", "<i4")])
assert DTYPE.itemsize == 32

DEFAULT_WINDOW = 512
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def as_bytes(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode("latin-1")


def revcomp(s):
    """Upper-cased, back to front, ACGT complemented; every other byte stays what it is (and still matches nothing)."""
    return as_bytes(s).upper().translate(_COMP)[::-1]


def check_params(adapters, max_error_pct, poly_min, window):
    assert 0 <= len(adapters) <= 4 and all(12 <= len(a) <= 64 and set(as_bytes(a).upper()) <= set(b"ACGT") for a in adapters)
    assert 0 <= max_error_pct <= 30 and 32 <= window <= 4096 and (poly_min == 0 or 8 <= poly_min <= window)


# ------------------------------------------------------------------ plain loops
def sellers_plain(pattern, text):
    """D[e], e = 0 .. len(text): the smallest edit distance between `pattern` and a substring of `text` that ends at e.
    Letters are compared as given; only ACGT letters of the text can match."""
    m = len(pattern)
    col = list(range(m + 1))
    out = [m]
    for ch in text:
        new = [0] * (m + 1)
        for i in range(1, m + 1):
            same = ch == pattern[i - 1] and ch in b"ACGT"
            new[i] = min(col[i - 1] + (0 if same else 1), col[i] + 1, new[i - 1] + 1)
        col = new
        out.append(col[m])
    return out


def head_plain(S, adapters=(), max_error_pct=20, poly_min=0, window=DEFAULT_WINDOW):
    """H(S): (adapter_len, adapter, adapter_err, poly_len)."""
    S = as_bytes(S).upper()
    L = len(S)
    alen = aidx = aerr = 0
    T = S[:min(L, window)]
    for index, a in enumerate(adapters):
        a = as_bytes(a).upper()
        k = max_error_pct * len(a) // 100
        D = sellers_plain(a, T)
        match = None
        for e in range(1, len(T) + 1):
            if D[e] <= k and (match is None or D[e] <= match[1]):
                match = (e, D[e])
        if match and match[0] > alen:
            alen, aidx, aerr = match[0], index + 1, match[1]
    U = S[alen:min(L, alen + window)]
    score = best = p = 0
    for j, ch in enumerate(U):
        score += 1 if ch == ord("T") else -2
        if score > best:
            best, p = score, j + 1
    poly = p if poly_min > 0 and p >= poly_min else 0
    return alen, aidx, aerr, poly


def kept(L, head, tail):
    """(kept_start, kept_len) of a read of L bytes whose ends claim `head` and `tail` bytes."""
    return head, L - head - min(tail, L - head)


def row_plain(S, adapters=(), max_error_pct=20, poly_min=0, window=DEFAULT_WINDOW):
    h = head_plain(S, adapters, max_error_pct, poly_min, window)
    t = head_plain(revcomp(S), adapters, max_error_pct, poly_min, window)
    ks, kl = kept(len(S), h[0] + h[3], t[0] + t[3])
    orient = 1 if t[3] and not h[3] else -1 if h[3] and not t[3] else 0
    return (h[0], h[3], t[0], t[3], h[1], h[2], t[1], t[2], ks, kl, orient)


def rows_plain(reads, **kw):
    return np.array([row_plain(r, **kw) for r in reads], dtype=DTYPE)


# ------------------------------------------------------------------ numpy, a batch at a time
_CODE = np.full(256, 4, np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _CODE[_ch + 32] = _i


def _end_matrix(reads, lens, start, width, tail):
    """codes[r, j] = the code of letter start[r] + j of read r's end text (the read, or its reverse complement), 5 beyond
    the read's end: a code no letter has."""
    n = len(reads)
    M = np.full((n, width), 5, np.uint8)
    for r, rd in enumerate(reads):
        a = int(start[r])
        w = min(width, int(lens[r]) - a)
        if w <= 0:
            continue
        c = _CODE[np.frombuffer(rd, np.uint8)]
        if tail:
            c = np.where(c < 4, 3 - c, c)[::-1]
        M[r, :w] = c[a:a + w]
    return M


def _head_batch(reads, lens, adapters, max_error_pct, poly_min, window, tail):
    n = len(reads)
    alen = np.zeros(n, np.int64)
    aidx = np.zeros(n, np.int64)
    aerr = np.zeros(n, np.int64)
    if adapters:
        width = int(min(window, lens.max(initial=0)))
        T = _end_matrix(reads, lens, np.zeros(n, np.int64), width, tail)
        for index, a in enumerate(adapters):
            pat = _CODE[np.frombuffer(as_bytes(a), np.uint8)].astype(np.int64)
            m = len(pat)
            k = max_error_pct * m // 100
            rows_i = np.arange(m + 1)
            col = np.tile(rows_i, (n, 1))                             # column 0: D[i] = i
            bestD = np.full(n, m + 1, np.int64)
            bestE = np.zeros(n, np.int64)
            for j in range(width):
                t = T[:, j].astype(np.int64)
                cost = (pat[None, :] != t[:, None]).astype(np.int64)  # a code of 4 or 5 equals no pattern code
                new = np.empty_like(col)
                new[:, 0] = 0
                new[:, 1:] = np.minimum(col[:, :-1] + cost, col[:, 1:] + 1)
                new = np.minimum.accumulate(new - rows_i, axis=1) + rows_i   # the run of insertions down the column
                col = new
                d = col[:, m]
                take = (d <= k) & (d <= bestD) & (j < lens)
                bestD[take] = d[take]
                bestE[take] = j + 1
            better = bestE > alen
            alen[better] = bestE[better]
            aidx[better] = index + 1
            aerr[better] = bestD[better]
    poly = np.zeros(n, np.int64)
    if poly_min > 0:
        width = int(min(window, (lens - alen).max(initial=0)))
        U = _end_matrix(reads, lens, alen, width, tail)
        step = np.where(U == 3, 1, -2).astype(np.int64)
        step[U == 5] = -(1 << 20)                                     # beyond the read: never a maximum
        score = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(step, axis=1)], axis=1)
        p = np.argmax(score, axis=1)                                  # (the first of equal maxima)
        poly = np.where(p >= poly_min, p, 0)
    return alen, aidx, aerr, poly


def rows(reads, adapters=(), max_error_pct=20, poly_min=0, window=DEFAULT_WINDOW):
    """One DTYPE row per read of `reads` (bytes or str)."""
    reads = [as_bytes(r) for r in reads]
    adapters = [as_bytes(a).upper() for a in adapters]
    check_params(adapters, max_error_pct, poly_min, window)
    out = np.zeros(len(reads), DTYPE)
    if not reads:
        return out
    lens = np.array([len(r) for r in reads], np.int64)
    h = _head_batch(reads, lens, adapters, max_error_pct, poly_min, window, False)
    t = _head_batch(reads, lens, adapters, max_error_pct, poly_min, window, True)
    head, tl = h[0] + h[3], t[0] + t[3]
    out["head_adapter_len"], out["head_adapter"], out["head_adapter_err"], out["head_poly_len"] = h
    out["tail_adapter_len"], out["tail_adapter"], out["tail_adapter_err"], out["tail_poly_len"] = t
    out["kept_start"] = head
    out["kept_len"] = lens - head - np.minimum(tl, lens - head)
    out["orient"] = np.where((t[3] > 0) & (h[3] == 0), 1, np.where((h[3] > 0) & (t[3] == 0), -1, 0))
    return out


def batch(reads):
    """(bases uint8, offsets uint64) of a list of reads, as Context.batch takes them."""
    reads = [as_bytes(r) for r in reads]
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), np.uint8).copy(), off


def clip(reads, table):
    """The kept interval of every read, as bytes."""
    return [as_bytes(r)[int(t["kept_start"]):int(t["kept_start"]) + int(t["kept_len"])] for r, t in zip(reads, table)]


# ------------------------------------------------------------------ planting
def mutate(rng, seq, n_edits, kinds="SID"):
    """`seq` (str) with n_edits edits of the given kinds at distinct places: S substitution, I insertion, D deletion,
    N a letter replaced by N.  Returns the edited text; its edit distance to seq is at most n_edits."""
    s = list(seq)
    places = sorted(rng.choice(len(s), size=n_edits, replace=False).tolist(), reverse=True)
    for at in places:
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind == "S":
            s[at] = "ACGT"[("ACGT".index(s[at]) + 1 + int(rng.integers(3))) % 4]
        elif kind == "N":
            s[at] = "N"
        elif kind == "I":
            s.insert(at, "ACGT"[int(rng.integers(4))])
        else:
            del s[at]
    return "".join(s)


def random_seq(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n).tolist())
