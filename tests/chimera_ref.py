"""The chimera scan and the piece rule (docs/chimeras.md) stated twice: in plain Python over ends_ref.sellers_plain, one cell
at a time (hits_plain), and in numpy, Sellers row by row over all columns of a read (hits).  Neither knows anything of the
device's bit vectors, chunks or tiles; tests/test_chimera_reference.py holds the two against each other and the lanes of
the kernel (run on the CPU) against them, the GPU tests hold the device against hits()."""
import numpy as np

import ends_ref as ER

HIT_DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("end", "<u4"), ("adapter", "u1"), ("strand", "u1"), ("err", "u1"), ("pad", "u1")])
PIECE_DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("len", "<u4"), ("ordinal", "<u4")])
assert HIT_DTYPE.itemsize == 16 and PIECE_DTYPE.itemsize == 16

SSP = "TTTCTGTTGGTGCTGATATTGCTGGG"       # the strand-switch primer of the README's example (26 letters)
VNP = "ACTTGCCTGTCGCTCTATCTTC"           # the VN primer (22 letters)


def patterns(adapters):
    """[(adapter number from 1, strand, pattern bytes)], in the order of the hits' tie-break."""
    out = []
    for i, a in enumerate(adapters):
        a = ER.as_bytes(a).upper()
        out.append((i + 1, 0, a))
        out.append((i + 1, 1, ER.revcomp(a)))
    return out


def check_params(adapters, max_error_pct):
    assert 1 <= len(adapters) <= 4 and all(12 <= len(a) <= 64 and set(ER.as_bytes(a).upper()) <= set(b"ACGT") for a in adapters)
    assert 0 <= max_error_pct <= 30


# ------------------------------------------------------------------ plain loops
def edit_distance_plain(a, b):
    """Global unit-cost edit distance; only ACGT letters match."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            same = a[i - 1] == b[j - 1] and a[i - 1] in b"ACGT"
            cur[j] = min(prev[j - 1] + (0 if same else 1), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def hit_ends_plain(D, k, w):
    """The hit ends of one pattern from its Sellers row D[0 .. L]."""
    L = len(D) - 1
    C = [min(d, k + 1) for d in D]
    out = []
    for e in range(1, L + 1):
        if C[e] > k:
            continue
        if any(C[e] >= C[x] for x in range(e + 1, min(L, e + w) + 1)):
            continue
        if any(C[e] > C[x] for x in range(max(1, e - w), e)):
            continue
        out.append(e)
    return out


def hits_plain_read(S, adapters, max_error_pct, read=0):
    S = ER.as_bytes(S).upper()
    out = []
    for number, strand, pat in patterns(adapters):
        m = len(pat)
        k = max_error_pct * m // 100
        D = ER.sellers_plain(pat, S)
        for e in hit_ends_plain(D, k, (m + 1) // 2):
            j = 0
            while edit_distance_plain(pat, S[e - j:e]) != D[e]:
                j += 1
                assert j <= min(e, m + k)
            out.append((read, e - j, e, number, strand, D[e], 0))
    out.sort(key=lambda h: (h[0], h[2], h[3], h[4]))
    return out


def hits_plain(reads, adapters, max_error_pct=10):
    check_params(adapters, max_error_pct)
    rows = []
    for r, S in enumerate(reads):
        rows += hits_plain_read(S, adapters, max_error_pct, r)
    return np.array(rows, dtype=HIT_DTYPE).reshape(-1)


def pieces_plain(lens, hit_table, min_piece=0):
    """(pieces PIECE_DTYPE, read_piece_offsets, dropped, dropped_bases): one byte of every read at a time."""
    rows, off, dropped, dropped_bases = [], [0], 0, 0
    for r, L in enumerate(lens):
        mine = hit_table[hit_table["read"] == r]
        if len(mine) == 0:
            rows.append((r, 0, L, 0))
            off.append(len(rows))
            continue
        covered = [False] * L
        for h in mine:
            for i in range(int(h["start"]), min(L, int(h["end"]))):
                covered[i] = True
        ordinal, i = 0, 0
        while i < L:
            if covered[i]:
                i += 1
                continue
            j = i
            while j < L and not covered[j]:
                j += 1
            if j - i < min_piece:
                dropped += 1
                dropped_bases += j - i
            else:
                ordinal += 1
                rows.append((r, i, j - i, ordinal))
            i = j
        off.append(len(rows))
    return np.array(rows, dtype=PIECE_DTYPE).reshape(-1), np.array(off, np.uint64), dropped, dropped_bases


# ------------------------------------------------------------------ numpy, a read at a time
def sellers_rows(pat_codes, text_codes, top_is_j=False):
    """The last row of the edit-distance table of the pattern against the text, over all columns 0 .. n at once: the top row
    is 0 (Sellers) or j (the anchored form of the hit start); the first column is i."""
    n = len(text_codes)
    cols = np.arange(n + 1, dtype=np.int64)
    row = cols.copy() if top_is_j else np.zeros(n + 1, np.int64)
    for i, p in enumerate(pat_codes.tolist(), start=1):
        cost = (text_codes != p).astype(np.int64)               # codes of 4 equal no pattern code
        new = np.empty(n + 1, np.int64)
        new[0] = i
        new[1:] = np.minimum(row[:-1] + cost, row[1:] + 1)
        row = np.minimum.accumulate(new - cols) + cols          # the run of horizontal steps along the row
    return row


def hit_ends(D, k, w):
    L = len(D) - 1
    if L == 0:
        return np.zeros(0, np.int64)
    C = np.minimum(D, k + 1)[1:]                                # C[e - 1] is column e
    big = k + 2
    ok = C <= k
    for d in range(1, min(w, L - 1) + 1):                      # columns outside 1 .. L forbid nothing
        nxt = np.full(L, big, np.int64)
        nxt[:L - d] = C[d:]
        prv = np.full(L, big, np.int64)
        prv[d:] = C[:L - d]
        ok &= (C < nxt) & (C <= prv)
    return np.nonzero(ok)[0] + 1


def hits_read(S, adapters, max_error_pct, read=0):
    S = ER.as_bytes(S)
    text = ER._CODE[np.frombuffer(S, np.uint8)].astype(np.int64)
    out = []
    for number, strand, pat in patterns(adapters):
        pc = ER._CODE[np.frombuffer(pat, np.uint8)].astype(np.int64)
        m = len(pc)
        k = max_error_pct * m // 100
        D = sellers_rows(pc, text)
        for e in hit_ends(D, k, (m + 1) // 2).tolist():
            far = min(e, m + k)
            back = sellers_rows(pc[::-1], text[e - far:e][::-1], top_is_j=True)     # back[j]: pattern against S[e - j, e)
            j = int(np.nonzero(back == D[e])[0][0])
            out.append((read, e - j, e, number, strand, int(D[e]), 0))
    out.sort(key=lambda h: (h[0], h[2], h[3], h[4]))
    return out


def hits(reads, adapters, max_error_pct=10):
    """The batch's hits in the contract's order, as a HIT_DTYPE array, and read_hit_offsets."""
    check_params(adapters, max_error_pct)
    rows = []
    off = [0]
    for r, S in enumerate(reads):
        rows += hits_read(S, adapters, max_error_pct, r)
        off.append(len(rows))
    return np.array(rows, dtype=HIT_DTYPE).reshape(-1), np.array(off, np.uint64)


def pieces(lens, hit_table, min_piece=0):
    """(pieces PIECE_DTYPE, read_piece_offsets, dropped, dropped_bases), by the intervals."""
    rows, off, dropped, dropped_bases = [], [0], 0, 0
    hit_table = hit_table[np.argsort(hit_table["read"], kind="stable")]
    first = np.searchsorted(hit_table["read"], np.arange(len(lens) + 1))
    for r, L in enumerate(lens):
        mine = hit_table[first[r]:first[r + 1]]
        if len(mine) == 0:
            rows.append((r, 0, L, 0))
            off.append(len(rows))
            continue
        at, ordinal = 0, 0
        gaps = []
        for s, e in sorted((min(int(h["start"]), L), min(int(h["end"]), L)) for h in mine):
            if s > at:
                gaps.append((at, s))
            at = max(at, e)
        if at < L:
            gaps.append((at, L))
        for a, b in gaps:
            if b - a < min_piece:
                dropped += 1
                dropped_bases += b - a
            else:
                ordinal += 1
                rows.append((r, a, b - a, ordinal))
        off.append(len(rows))
    return np.array(rows, dtype=PIECE_DTYPE).reshape(-1), np.array(off, np.uint64), dropped, dropped_bases


def cut(reads, piece_table):
    """The pieces as bytes."""
    return [ER.as_bytes(reads[int(p["read"])])[int(p["start"]):int(p["start"]) + int(p["len"])] for p in piece_table]


def piece_names(names, piece_table):
    return [names[int(p["read"])] + ("_c%d" % int(p["ordinal"]) if int(p["ordinal"]) else "") for p in piece_table]


def joint(rng, edits=(0, 2)):
    """What sits between the two transcripts of a chimeric read: A x 30 . revcomp(VNP) . SSP, each primer with some edits."""
    a = ER.mutate(rng, ER.revcomp(VNP).decode(), int(rng.integers(edits[0], edits[1] + 1)))
    b = ER.mutate(rng, SSP, int(rng.integers(edits[0], edits[1] + 1)))
    return "A" * 30 + a + b


def dress(rng, reads, every=10):
    """Every `every`-th read joined to the next through joint(); returns the new list of reads (bytes)."""
    out, i = [], 0
    reads = [ER.as_bytes(r) for r in reads]
    while i < len(reads):
        if i % every == 0 and i + 1 < len(reads):
            out.append(reads[i] + joint(rng).encode() + reads[i + 1])
            i += 2
        else:
            out.append(reads[i])
            i += 1
    return out
