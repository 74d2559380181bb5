"""The short-read filter's contract in numpy (docs/sr_filter.md): the reference the GPU pass (k_sr_mask) is tested against.

Per record S of L bytes with optional qualities q: for a start p and an adapter A of m letters, o = min(m, L - p) and mm =
the number of i < o where S[p+i] and A[i] differ after upper-casing (a byte of S outside ACGTacgt always differs); p is
accepted when o >= min_overlap and 100 mm <= err_pct o.  clip = the smallest accepted p over all adapters, L without one.
Bytes [clip, L) and every byte j < clip with q[j] < 33 + min_qual become N; everything else stays.  stats = (records,
records with clip < L, sum of L - clip, bytes below the floor among [0, clip))."""
import numpy as np

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[_ch + 32] = _i

DEFAULT_OVERLAP = 5
N = ord("N")


def _adapters(adapters):
    if isinstance(adapters, (str, bytes)):
        adapters = [adapters]
    out = [a.encode() if isinstance(a, str) else bytes(a) for a in adapters]
    assert len(out) <= 4 and all(1 <= len(a) <= 64 and all(_CODE[c] < 4 for c in a) for a in out)
    return out


def mask(bases, quals, offsets, min_qual=0, adapters=(), min_overlap=0, err_pct=10):
    """(masked uint8[n bytes of the batch], clip u32[n records], stats 4-tuple); offsets may start anywhere in `bases`."""
    adapters = _adapters(adapters)
    min_overlap = int(min_overlap) or DEFAULT_OVERLAP
    bases = np.asarray(np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else bases, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    lo, hi = int(offsets[0]), int(offsets[-1])
    text = bases[lo:hi].copy()
    n = len(offsets) - 1
    start = offsets[:-1] - lo
    lens = np.diff(offsets)
    nb = hi - lo
    rec = np.repeat(np.arange(n), lens)
    end = (start + lens)[rec] if nb else np.zeros(0, np.int64)       # the end of every byte's record
    pos = np.arange(nb, dtype=np.int64)
    code = _CODE[text]
    clip_abs = (start + lens).copy()                                 # absolute: the record's end while nothing is accepted
    for a in adapters:
        m = len(a)
        ac = _CODE[np.frombuffer(a, dtype=np.uint8)]
        o = np.minimum(m, end - pos)
        mm = np.zeros(nb, dtype=np.int64)
        padded = np.concatenate([code, np.full(m, 4, np.uint8)])
        for i in range(m):
            inside = pos + i < end
            mm += inside & (padded[i:i + nb] != ac[i])
        acc = np.flatnonzero((o >= min_overlap) & (100 * mm <= err_pct * o))
        np.minimum.at(clip_abs, rec[acc], acc)
    clip = clip_abs - start
    out = text.copy()
    clipped = pos >= clip_abs[rec] if nb else np.zeros(0, bool)
    low = np.zeros(nb, dtype=bool)
    if quals is not None and min_qual:
        q = np.asarray(np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else quals, dtype=np.uint8)[lo:hi]
        low = ~clipped & (q.astype(np.int64) < 33 + int(min_qual))
    out[clipped | low] = N
    stats = (n, int((clip < lens).sum()), int((lens - clip).sum()), int(low.sum()))
    return out, clip.astype(np.uint32), stats


def naive_mask(records, quals, min_qual=0, adapters=(), min_overlap=0, err_pct=10):
    """The same, record by record in plain Python, as directly from the contract as possible.  records: list of bytes;
    quals: list of bytes or None.  Returns (list of masked bytes, list of clip, stats)."""
    adapters = _adapters(adapters)
    min_overlap = int(min_overlap) or DEFAULT_OVERLAP
    is_base = set(b"ACGTacgt")
    outs, clips = [], []
    n_clipped = n_clip_bytes = n_low = 0
    for r, S in enumerate(records):
        L = len(S)
        clip = L
        for A in adapters:
            for p in range(L):
                o = min(len(A), L - p)
                mm = 0
                for i in range(o):
                    s = S[p + i]
                    if s not in is_base or bytes([s]).upper() != bytes([A[i]]).upper():
                        mm += 1
                if o >= min_overlap and 100 * mm <= err_pct * o:
                    clip = min(clip, p)
                    break
        out = bytearray(S)
        for j in range(L):
            if j >= clip:
                out[j] = N
            elif quals is not None and min_qual and quals[r][j] < 33 + min_qual:
                out[j] = N
                n_low += 1
        outs.append(bytes(out))
        clips.append(clip)
        n_clipped += clip < L
        n_clip_bytes += L - clip
    return outs, clips, (len(records), n_clipped, n_clip_bytes, n_low)


# ---------------------------------------------------------------------------------------------------------------- cases
AD33 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"        # 33 letters


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=n))


def hand_cases():
    """[(name, records, quals or None, dict of filter arguments)]: every case of the contract that can go wrong on its own."""
    rng = np.random.default_rng(11)
    body = _rand(rng, 80)          # (random: an accidental match of >= 5 bases with <= 10 % errors is what the reference decides too)
    A = AD33
    one_off = A[:9][:4] + ("C" if A[4] != "C" else "G") + A[5:9]
    ten_1 = A[:10][:6] + ("C" if A[6] != "C" else "G") + A[7:10]
    ten_2 = ten_1[:2] + ("C" if A[2] != "C" else "G") + ten_1[3:]
    cases = []
    add = lambda name, recs, quals=None, **kw: cases.append((name, [r.encode() if isinstance(r, str) else r for r in recs], quals, kw))
    add("lengths 0, 1, min_overlap - 1, min_overlap", ["", "A", A[:4], A[:5]], adapters=[A])
    add("adapter at p = 0", [A + body[:30], A], adapters=[A])
    add("full adapter mid-read, bases behind it", [body[:40] + A + body[40:70]], adapters=[A])
    add("overhang of exactly min_overlap", [body[:60] + A[:5]], adapters=[A])
    add("overhang of min_overlap - 1", [body[:60] + A[:4]], adapters=[A])
    add("o = 9, one mismatch: rejected", [body[:50] + one_off], adapters=[A])
    add("o = 10, one mismatch: accepted", [body[:50] + ten_1], adapters=[A])
    add("o = 10, two mismatches: rejected", [body[:50] + ten_2], adapters=[A])
    add("two accepted starts: the leftmost", [body[:20] + A + body[20:30] + A + body[30:40]], adapters=[A])
    B = _rand(rng, 20)
    add("two adapters, the second matches earlier", [body[:15] + B + body[15:40] + A], adapters=[A, B])
    add("lower-case read, upper-case adapter", [body[:30].lower() + A.lower() + "acgt"], adapters=[A])
    add("upper-case read, lower-case adapter", [body[:30] + A], adapters=[A.lower()])
    add("an N inside the overlap is a mismatch", [body[:50] + A[:4] + "N" + A[5:9], body[:50] + A[:6] + "N" + A[7:20], body[:50] + A[:4] + "n" + A[5:]], adapters=[A])
    add("adapter of length 1", [body[:30], "ACGTTTGCA"], adapters=["T"], min_overlap=1)
    A64 = _rand(rng, 64)
    add("adapter of length 64", [body[:33] + A64 + body[:7], body[:70] + A64[:40], A64[:63]], adapters=[A64])
    long = _rand(rng, 700)
    add("a read longer than 64 x 4, adapter late", [long + A + body[:5], long + A[:6], long, long[:511] + A, long[:512] + A, long[:508] + A + long[:100]], adapters=[A])
    recs = [body[:40], body[10:50]]
    qa = [bytes([33 + 20]) * 10 + bytes([33 + 19]) * 10 + bytes([33 + 20, 33 + 19] * 10), bytes([33]) * 40]
    add("quality exactly 33 + Q kept, 33 + Q - 1 masked", recs, qa, min_qual=20)
    add("quals = None under a floor", recs, None, min_qual=20, adapters=[A])
    add("adapters without floor, qualities given", [body[:40] + A[:12]], [bytes([33 + 2]) * 52], adapters=[A])
    add("floor without adapters", [body[:40] + A[:12]], [bytes([33 + 2]) * 30 + bytes([33 + 30]) * 22], min_qual=10)
    add("floor and adapter: low qualities behind the clip are not counted", [body[:40] + A[:12]], [bytes([33 + 30]) * 35 + bytes([33 + 2]) * 17], min_qual=10, adapters=[A])
    add("zero error allowed", [body[:50] + ten_1, body[:50] + A[:10]], adapters=[A], err_pct=0)
    add("30 % errors", [body[:50] + ten_2 + "T"], adapters=[A], err_pct=30, min_overlap=10)
    add("IUPAC and CR in the read", [body[:20] + "R\r" + A + "YY"], adapters=[A])
    return cases


def to_arrays(records, quals=None):
    """(bases uint8, quals uint8 or None, offsets u64[n+1]) of lists of bytes."""
    offsets = np.zeros(len(records) + 1, dtype=np.uint64)
    if records:
        offsets[1:] = np.cumsum([len(r) for r in records])
    b = np.frombuffer(b"".join(records), dtype=np.uint8).copy()
    q = None if quals is None else np.frombuffer(b"".join(quals), dtype=np.uint8).copy()
    return b, q, offsets


def split(masked, offsets):
    offsets = np.asarray(offsets, dtype=np.int64) - int(offsets[0])
    return [bytes(masked[offsets[i]:offsets[i + 1]]) for i in range(len(offsets) - 1)]


def random_records(seed, n, max_len=120, adapters=(AD33,)):
    """n records over ACGTacgtNn with adapter pieces planted in most of them, and qualities."""
    rng = np.random.default_rng(seed)
    adapters = _adapters(adapters)
    recs, quals = [], []
    for _ in range(n):
        L = int(rng.integers(0, max_len))
        r = bytearray(_rand(rng, L, "ACGTACGTACGTacgtNn").encode())
        if adapters and rng.random() < 0.7 and L:
            a = bytearray(adapters[int(rng.integers(0, len(adapters)))])
            for _e in range(int(rng.integers(0, 3))):     # a few substitutions
                a[int(rng.integers(0, len(a)))] = ord(_rand(rng, 1, "ACGTn"))
            p = int(rng.integers(0, L))
            piece = a[:L - p]
            r[p:p + len(piece)] = piece
        recs.append(bytes(r))
        quals.append(bytes(rng.integers(33, 33 + 42, size=L, dtype=np.uint8)))
    return recs, quals
