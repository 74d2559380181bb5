"""The text-dump contract in plain Python, and the builder of the files the parser is tested on.

The contract is the comment above k_parse_count (talc_kernels_build.h): a canonical line is exactly K letters of ACGTacgt,
one blank or tab, one to nine decimal digits, a newline; line i of the file is entry i; a file with any other line (an
empty one, a last line without its newline, more than four line starts in one 64-byte slice) is flagged as a whole and
left to the host's tokeniser.  k-mers are 2 bits per base (A=0 C=1 G=2 T=3), first base most significant.  Nothing here
shares code with the library."""
import collections

import numpy as np

SLICE, TILE = 64, 16384
WHATS = ("start", "first_letter", "last_letter", "blank", "first_digit", "last_digit", "newline")
_VAL = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}


def line_starts(data):
    """Offsets at which a line starts: 0 and the byte after every newline, as long as the file has a byte there."""
    out = []
    for i in range(len(data)):
        if i == 0 or data[i - 1] == 10:
            out.append(i)
    return out


def parse(data, k):
    """(kmers u64[n], counts u32[n], flagged) of the canonical lines of `data`, byte by byte; flagged: some line is not
    canonical (the arrays then hold the canonical ones only)."""
    data = bytes(data)
    kmers, counts = [], []
    flagged = False
    per_slice = collections.Counter()
    n = len(data)
    p = 0
    while p < n:
        per_slice[p // SLICE] += 1
        q = p
        v = 0
        letters = 0
        while q < n and chr(data[q]) in _VAL:
            v = (v << 2) | _VAL[chr(data[q])]
            letters += 1
            q += 1
        ok = letters == k and q < n and data[q] in (32, 9)
        if ok:
            q += 1
            c = 0
            digits = 0
            while q < n and 48 <= data[q] <= 57:
                c = c * 10 + (data[q] - 48)
                digits += 1
                q += 1
            ok = 1 <= digits <= 9 and q < n and data[q] == 10
        if ok:
            kmers.append(v)
            counts.append(c)
        else:
            flagged = True
        while p < n and data[p] != 10:      # the next line starts after this one's newline
            p += 1
        p += 1
    if max(per_slice.values(), default=0) > 4:
        flagged = True
    return np.array(kmers, dtype=np.uint64), np.array(counts, dtype=np.uint32), flagged


def first_wins(kmers, counts, min_count):
    """The builder's rule: lines with count >= min_count are kept, the first kept line of a k-mer decides its count.
    Returns (distinct keys u64, sorted; their counts u32)."""
    kmers = np.asarray(kmers, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint32)
    keep = counts >= np.uint32(min_count)
    keys, first = np.unique(kmers[keep], return_index=True)     # (the index of the first occurrence)
    return keys, counts[keep][first]


def starts_per_slice(starts, size):
    """Line starts in each 64-byte slice of a file of `size` bytes."""
    return np.bincount(np.asarray(starts, dtype=np.int64) // SLICE, minlength=(size + SLICE - 1) // SLICE)


def starts_per_tile(starts, size):
    """Line starts in each 16 KiB tile."""
    return np.bincount(np.asarray(starts, dtype=np.int64) // TILE, minlength=(size + TILE - 1) // TILE)


def numbered_by_tiles(starts, size, kmers, counts, wrong_tile=None, later_tile_wins=True):
    """The arrays as the two-kernel numbering stores them: a tile's first line number is the sum of the counts of the tiles
    before it, a line's index is that plus its rank in the tile.  wrong_tile: that tile's first line number is one too
    large (the fault the per-line tests are there to catch): its lines land one index further, the slot it should have
    started at is never written (k-mer 0, count 0), and its last line and the next tile's first line want the same slot."""
    starts = np.asarray(starts, dtype=np.int64)
    per_tile = starts_per_tile(starts, size)
    base = np.concatenate([[0], np.cumsum(per_tile)[:-1]])
    tile = starts // TILE
    rank = np.arange(len(starts)) - base[tile]
    index = base[tile] + rank
    if wrong_tile is not None:
        index = index + (tile == wrong_tile)
    outk = np.zeros(len(starts), dtype=np.uint64)
    outc = np.zeros(len(starts), dtype=np.uint32)
    order = np.arange(len(starts)) if later_tile_wins else np.arange(len(starts))[::-1]
    order = order[index[order] < len(starts)]
    outk[index[order]] = np.asarray(kmers, dtype=np.uint64)[order]      # (numpy keeps the last of equal indices)
    outc[index[order]] = np.asarray(counts, dtype=np.uint32)[order]
    return outk, outc


def unpack(km, k):
    return "".join("ACGT"[(int(km) >> (2 * (k - 1 - i))) & 3] for i in range(k))


Layout = collections.namedtuple("Layout", "data starts kmers counts lines")


def _byte_of(what, k, nd):
    """Offset within a line of k letters and nd digits of the byte that `what` names."""
    return {"start": 0, "first_letter": 0, "last_letter": k - 1, "blank": k, "first_digit": k + 1, "last_digit": k + nd,
            "newline": k + 1 + nd}[what]


def _digit_counts(gap, k, rng, digits):
    """Digit counts of lines that fill `gap` bytes exactly."""
    lo, hi = (k + 2 + digits, k + 2 + digits) if digits else (k + 3, k + 11)
    if gap == 0:
        return []
    m_min, m_max = -(-gap // hi), gap // lo
    if m_min > m_max:
        raise ValueError("no whole lines of K = %d fill %d bytes" % (k, gap))
    m = int(min(max(round(gap / ((lo + hi) / 2)), m_min), m_max))
    extra = rng.integers(0, hi - lo + 1, m)
    diff = gap - m * lo - int(extra.sum())
    while diff:
        i = int(rng.integers(0, m))
        step = 1 if diff > 0 else -1
        if 0 <= extra[i] + step <= hi - lo:
            extra[i] += step
            diff -= step
    return [int(lo - k - 2 + e) for e in extra]


def layout(k, n_lines, rng, place=(), end=None, digits=None, min_count=2, case="mixed", blank="mixed", kmers=None):
    """Canonical lines whose digit counts (1-9: a line is K + 3 .. K + 11 bytes) are chosen so that every (offset, what[,
    nd]) of `place` holds: the byte `what` names (WHATS) of some line is at `offset`; nd fixes that line's digit count.
    end: the file's size (n_lines is then ignored); digits: every line has that many; kmers: the first lines' k-mers.
    Counts include 0, 1, min_count - 1, min_count, 999999999 and values with leading zeros.  Returns Layout(data bytes,
    starts (offset of every line start), kmers, counts, lines (the lines as a list of bytes))."""
    nds = []           # digit count of every line
    cur = 0
    for item in sorted(place, key=lambda it: it[0]):
        off, what = item[0], item[1]
        nd = item[2] if len(item) > 2 else (digits or int(rng.integers(1, 10)))
        start = off - _byte_of(what, k, nd)
        if start < cur:
            raise ValueError("placement %r overlaps the line before it" % (item,))
        nds += _digit_counts(start - cur, k, rng, digits) + [nd]
        cur = start + k + 2 + nd
    if end is not None:
        nds += _digit_counts(end - cur, k, rng, digits)
    else:
        if len(nds) > n_lines:
            raise ValueError("the placements need %d lines" % len(nds))
        nds += [digits or int(x) for x in rng.integers(1, 10, n_lines - len(nds))]
    special = [0, 1, max(min_count - 1, 0), min_count, 999999999, 7]
    lines, starts, kms, cts = [], [], [], []
    pos = 0
    for i, nd in enumerate(nds):
        km = int(kmers[i]) if kmers is not None and i < len(kmers) else int(rng.integers(0, 1 << (2 * k), dtype=np.uint64))
        text = unpack(km, k)
        style = case if case != "mixed" else ("upper", "lower", "each")[int(rng.integers(0, 3))]
        if style == "lower":
            text = text.lower()
        elif style == "each":
            text = "".join(ch.lower() if low else ch for ch, low in zip(text, rng.integers(0, 2, k)))
        fits = [s for s in special if s < 10 ** nd]
        c = int(fits[int(rng.integers(0, len(fits)))]) if rng.integers(0, 3) == 0 else int(rng.integers(0, 10 ** nd))
        sep = blank if blank != "mixed" else " \t"[int(rng.integers(0, 2))]
        line = (text + sep + str(c).zfill(nd) + "\n").encode()       # (zfill: the leading zeros)
        lines.append(line)
        starts.append(pos)
        kms.append(km)
        cts.append(c)
        pos += len(line)
    return Layout(b"".join(lines), np.array(starts, dtype=np.int64), np.array(kms, dtype=np.uint64),
                  np.array(cts, dtype=np.uint32), lines)


def what_is_at(lay, k, offset):
    """The name (WHATS, 'letter' / 'digit' for the inner ones) of the byte of `lay` at `offset`, and its line."""
    i = int(np.searchsorted(lay.starts, offset, side="right")) - 1
    j = offset - int(lay.starts[i])
    nd = len(lay.lines[i]) - k - 2
    names = [w for w in WHATS[1:] if _byte_of(w, k, nd) == j]
    if j == 0:
        names.insert(0, "start")
    return names or ["letter" if j < k else "digit"], i


# ---------------------------------------------------------------- the one large file: the production constants
PROD_K, PROD_CHUNK, PROD_MIN_COUNT = 21, 32 << 20, 2


def production_layout(seed=7, n_lines=1_120_000, distinct=60_000):
    """A file of a little over 32 MiB at K = 21 as numpy arrays: ~`distinct` k-mers, each on about n_lines / distinct lines
    spread over the whole file; line i carries the count i + 2, written with 7-9 digits (leading zeros), so that a table's
    answer names the line that won; outside the zone every seventh line carries 1 instead (below MIN_COUNT 2).  The zone
    is the lines of the tiles around the 32 MiB border: each is the first kept line of a k-mer of its own that has earlier
    lines below MIN_COUNT and later duplicates, so a line lost or misnumbered there changes the table.
    Returns dict(data u8[size], starts, kmers, counts, border_line, zone=(first, last + 1))."""
    rng = np.random.default_rng(seed)
    k = PROD_K
    nd = rng.integers(7, 10, n_lines)
    lens = k + 2 + nd
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    size = int(lens.sum())
    i = np.arange(n_lines, dtype=np.int64)
    border_line = int(np.searchsorted(starts, PROD_CHUNK))
    z0, z1 = border_line - 1100, border_line + 1100         # ~2 tiles of lines on either side
    zone = i[z0:z1]
    counts = np.where((i % 7 == 0) & ((i < z0) | (i >= z1)), 1, i + 2).astype(np.uint32)
    pool = np.unique(rng.integers(0, 1 << (2 * k), distinct + 1000, dtype=np.uint64))[:distinct]
    rng.shuffle(pool)
    own, common = pool[:len(zone)], pool[len(zone):]
    kmers = common[rng.integers(0, len(common), n_lines)]
    kmers[zone] = own
    early = i[(i < z0) & (i % 7 == 0)]
    late = i[i >= z1]
    for picks in (rng.choice(early, 2 * len(zone), replace=False), rng.choice(late, 3 * len(zone), replace=False)):
        kmers[picks] = np.tile(own, len(picks) // len(own))
    # the bytes, column by column
    data = np.empty(size, dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(k):
        data[starts + j] = letters[((kmers >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.int64)]
    data[starts + k] = 32
    c64 = counts.astype(np.int64)
    for d in range(9):                                       # digit d of a line, from the left
        has = nd > d
        data[starts[has] + k + 1 + d] = 48 + (c64[has] // 10 ** (nd[has] - 1 - d)) % 10
    data[starts + k + 1 + nd] = 10
    return dict(data=data, starts=starts, kmers=kmers, counts=counts, border_line=border_line, zone=(z0, z1), size=size)
