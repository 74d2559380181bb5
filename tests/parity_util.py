"""Shared helpers for the parity tests: build the same table on both sides (oracle = checker,
libtalc_hip = product) from one synthetic spec and compare the two on seeded reads."""
import contextlib
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle_lib as O  # noqa: E402
from talc_amd import lib as T  # noqa: E402
from talc_amd.synth import Synth  # noqa: E402

PARAM_FIELDS = [f for f, _ in T.Params._fields_]


def both_params(**kw):
    """(product Params, oracle OrcParams) with identical field values."""
    p = T.default_params(**kw)
    q = O.params(**{f: getattr(p, f) for f in PARAM_FIELDS})
    return p, q


class Pair:
    """Oracle table + product table (uploaded) from one synthetic transcriptome."""

    def __init__(self, target_kmers=300_000, k=21, seed=1, junctions=False, oracle_backend=O.OracleTable.FLAT,
                 synth_kw=None, count_scale=1, device_built=False, **params_kw):
        self.synth = Synth(target_kmers=target_kmers, k=k, seed=seed, **(synth_kw or {}))
        self.p, self.q = both_params(k=k, use_junctions=int(junctions), **params_kw)
        keys, counts = self.synth.dump_arrays()
        if count_scale != 1:   # (every count times count_scale: the caller scales min_count with it)
            counts = (counts.astype(np.uint64) * count_scale).astype(np.uint32)
        self.keys, self.counts = keys, counts
        self.otab = O.OracleTable(self.q, oracle_backend)
        self.otab.insert_packed(keys, counts)
        self.ttab = T.Table.from_arrays(keys, counts, self.p, device=0 if device_built else None)
        if junctions:
            jk, jc = self.synth.junction_arrays()
            self.otab.colour_packed(jk, jc)
            self.ttab.colour(jk, jc)
        self.otab.decolour()
        self.ttab.decolour_repeats()
        self.ctx = None

    def upload(self, device=0):
        self.ttab.upload(device)
        self.ctx = T.Context(self.ttab, self.p, device)
        return self.ctx

    def reads(self, first, n):
        return self.synth.reads(first, n)


class CustomPair:
    """Oracle table + product table from explicit transcripts (forward-strand k-mers, `depth` per occurrence): for graph
    shapes the synthetic generator does not make (tandem repeats -> cycles)."""

    def __init__(self, transcripts, k=21, depth=20, **params_kw):
        self.p, self.q = both_params(k=k, **params_kw)
        code = {"A": 0, "C": 1, "G": 2, "T": 3}
        cnt = {}
        mask = (1 << (2 * k)) - 1
        for t in transcripts:
            v = 0
            for i, ch in enumerate(t):
                v = ((v << 2) | code[ch]) & mask
                if i >= k - 1:
                    cnt[v] = cnt.get(v, 0) + depth
        self.keys = np.fromiter(cnt.keys(), dtype=np.uint64, count=len(cnt))
        self.counts = np.fromiter(cnt.values(), dtype=np.uint32, count=len(cnt))
        self.otab = O.OracleTable(self.q, O.OracleTable.FLAT)
        self.otab.insert_packed(self.keys, self.counts)
        self.ttab = T.Table.from_arrays(self.keys, self.counts, self.p)
        self.otab.decolour()
        self.ttab.decolour_repeats()
        self.ctx = None

    def upload(self, device=0):
        self.ttab.upload(device)
        self.ctx = T.Context(self.ttab, self.p, device)
        return self.ctx


def seqs_of(buf, offs):
    b = bytes(buf)
    return [b[int(offs[i]):int(offs[i + 1])].decode() for i in range(len(offs) - 1)]


def compare_correction(pair, bases, offs, nthreads=8, verbose=True):
    """Run both sides; returns the list of read indices that differ (sequence or status)."""
    import time
    t0 = time.time()
    o_out, o_off, o_st = pair.otab.correct_batch(bases, offs, nthreads=nthreads)
    t1 = time.time()
    g_out, g_off, g_st = pair.ctx.correct(bases, offs)
    pair.last_times = (t1 - t0, time.time() - t1)   # (oracle seconds, HIP path seconds incl. transfers)
    so, sg = seqs_of(o_out, o_off), seqs_of(g_out, g_off)
    bad = [i for i in range(len(so)) if so[i] != sg[i] or int(o_st[i]) != int(g_st[i])]
    if verbose:
        print("reads %d  status(oracle) %s  mismatches %d" % (len(so), np.bincount(o_st, minlength=5).tolist(), len(bad)))
    return bad, (so, o_st), (sg, g_st)


def first_trace_diff(pair, bases, offs, idx):
    """Textual traces of read idx on both sides and the first differing line."""
    seq = bytes(bases[int(offs[idx]):int(offs[idx + 1])]).decode()
    to = pair.otab.trace(seq, steps=bool(os.environ.get("TALC_TRACE_STEPS"))).splitlines()
    b = pair.ctx.batch(np.frombuffer(seq.encode(), dtype=np.uint8), np.array([0, len(seq)], dtype=np.uint64))
    tg = b.trace(0).splitlines()
    b.close()
    return first_line_diff(to, tg)


def first_line_diff(to, tg):
    """The first line at which two traces (lists of lines: oracle, HIP path) differ, with the lines around it; None if
    none does."""
    n = min(len(to), len(tg))
    for i in range(n):
        if to[i] != tg[i]:
            return i, to[max(0, i - 3):i + 2], tg[max(0, i - 3):i + 2]
    if len(to) != len(tg):
        return n, to[n - 2:n + 2], tg[n - 2:n + 2]
    return None


# ---------------------------------------------------------------- references for what sits between coverage and search
COMP = str.maketrans("ACGTN", "TGCAN")
COV_TILE = 512        # TALC_COV_TILE (talc_common.h)
REG_CLEAN = 1 << 31   # kRegClean (talc_kernels_search.h)
HEAD_COV = 16         # kHeadCov


def revcomp(s):
    return s.translate(COMP)[::-1]


def pack_reads(reads):
    rb = "".join(reads).encode()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in reads])
    return (np.frombuffer(rb, dtype=np.uint8) if rb else np.zeros(0, np.uint8)), offs


def runs(mask):
    """Maximal runs of True as int[n, 2] (first, last position): findINRegions (Read.cpp:440-489) on `count >= MIN_COUNT`."""
    mask = np.asarray(mask, dtype=bool)
    if len(mask) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    return np.stack([np.nonzero(d == 1)[0], np.nonzero(d == -1)[0] - 1], 1).astype(np.int64)


def region_words_reference(hit, regions):
    """What k_structure must leave beside every region, from a dense hit vector (bool per k-mer position) alone: the index
    of the start's pair among the read's hits — the hits of tile t are packed from index t * COV_TILE, so that is the tile's
    base plus the hits of the tile below the start — with REG_CLEAN when start and end lie in one tile and every position
    from start to end is a hit."""
    hit = np.asarray(hit, dtype=bool)
    out = np.zeros(len(regions), dtype=np.uint32)
    for i, (s, e) in enumerate(np.asarray(regions, dtype=np.int64).tolist()):
        base = s - s % COV_TILE
        w = base + int(hit[base:s].sum())
        if s // COV_TILE == e // COV_TILE and e >= s and bool(hit[s:e + 1].all()):
            w |= REG_CLEAN
        out[i] = w
    return out


def head_counts_reference(counts):
    h = np.zeros(HEAD_COV, dtype=np.uint32)
    n = min(HEAD_COV, len(counts))
    h[:n] = counts[:n]
    return h


def in_span_reference(regions):
    r = np.asarray(regions, dtype=np.int64)
    return int((r[:, 1] - r[:, 0] + 1).sum()) & 0xFFFFFFFF if len(r) else 0


def comb(s, k, how, rng, g=(1, 2, 3, 5)):
    """One base every k + g positions (g drawn from `g`) replaced by N (how == "N") or substituted: an error-free read
    becomes a comb of solid stretches of g k-mers — hundreds of IN regions per read."""
    s = list(s)
    p = int(rng.integers(0, k))
    while p < len(s):
        s[p] = "N" if how == "N" else "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
        p += k + g[int(rng.integers(0, len(g)))]
    return "".join(s)


COMB_GRAPHS = {   # name -> (k, seed, extra generator settings)
    "unique-k21": (21, 921, {}),
    "branching-k21": (21, 921, dict(paralog_frac=0.8, paralog_div=0.04)),
    "unique-k31": (31, 931, {}),
}


def comb_synth_kw(name):
    k, seed, extra = COMB_GRAPHS[name]
    return k, seed, dict(mixed_lengths=1, sub_rate=0.0, ins_rate=0.0, del_rate=0.0, **extra)


def comb_reads(synth, k):
    """The two comb sets of a graph: the longest 24 of the generator's first 120 error-free reads, N set first, one
    generator shared over both sets."""
    bases, offs = synth.reads(0, 120)
    seqs = sorted(seqs_of(bases, offs), key=len)[-24:]
    rng = np.random.default_rng(5)
    return {how: [comb(s, k, how, rng) for s in seqs] for how in ("N", "sub")}


STRUCT_DEG_CAP = 512   # k_structure keeps the region-end degrees of that many regions in LDS


def structure_facts(otab, seq, minc):
    """From the oracle alone: what a read gives k_structure to do."""
    c, j, nin = otab.coverage(seq)
    raw = runs(c >= minc)
    reg, thr, ok = otab.structure(seq) if (len(seq) > otab.p.k and nin > 0) else (np.zeros((0, 2), np.uint32), 0.0, False)
    f = dict(cov=c, nin=nin, raw=raw, reg=reg.astype(np.int64), thr=thr, ok=ok)
    f["changed"] = not (len(raw) == len(reg) and (raw == reg).all())
    f["beyond_cap_changed"] = False
    if len(raw) > STRUCT_DEG_CAP:
        p0 = int(raw[STRUCT_DEG_CAP][0])
        want = set(map(tuple, raw[STRUCT_DEG_CAP:].tolist()))
        got = set(tuple(x) for x in f["reg"].tolist() if x[1] >= p0)
        f["beyond_cap_changed"] = want != got
    return f


WALK_LEVELS, WALK_TOP_NONE, WALK_SINGLE, WALK_BASE_SHIFT = 12, 0x1FFF, 1 << 13, 14


def walk_reference(succ, key, direction, k, minc):
    """The WalkEntry levels of the bucket `key` (a packed (K-1)-mer) as talc_common.h describes them, and why the walk
    ended ("count0", "clamp", "missing", "last").  succ(key, direction) = the bucket's four counts (A, C, G, T) or None when
    the table has no such bucket; direction 1 = RIGHT (the base is appended, the first base dropped), 0 = LEFT."""
    lv = [0] * WALK_LEVELS
    m1 = (1 << (2 * (k - 1))) - 1
    why = "last"
    for lev in range(WALK_LEVELS):
        c = succ(key, direction)
        if c is None:
            why = "missing"
            break
        top = max(c)
        am = list(c).index(top)                      # the first base wins a tie
        nx = max(c[b] for b in range(4) if b != am)
        fits = top < WALK_TOP_NONE
        single = fits and top >= minc and nx < minc
        lv[lev] = (top if fits else WALK_TOP_NONE) | (WALK_SINGLE if single else 0) | (am << WALK_BASE_SHIFT)
        if top == 0:
            why = "count0"
            break
        if not fits:
            why = "clamp"
            break
        key = (((key << 2) | am) & m1) if direction else ((am << (2 * (k - 2))) | (key >> 2))
    return lv, why


def bucket_dicts(keys, counts, k, minc):
    """{(K-1)-mer: [4 counts]} of the RIGHT and of the LEFT table from a dump (count >= minc, first duplicate wins)."""
    right, left = {}, {}
    seen = set()
    sh = 2 * (k - 1)
    m1 = (1 << sh) - 1
    for km, c in zip(np.asarray(keys).tolist(), np.asarray(counts).tolist()):
        if c < minc or km in seen:
            continue
        seen.add(km)
        right.setdefault(km >> 2, [0, 0, 0, 0])[km & 3] = c
        left.setdefault(km & m1, [0, 0, 0, 0])[km >> sh] = c
    return right, left


def assert_comb_reach(graph, how, facts):
    """What a comb set is there for, as conditions on the oracle's data (`facts`: structure_facts of its reads)."""
    nraw = [len(f["raw"]) for f in facts]
    beyond = sum(n > STRUCT_DEG_CAP for n in nraw)
    edited = sum(bool(f["beyond_cap_changed"]) for f in facts)
    kept_beyond = sum(len(f["reg"]) > STRUCT_DEG_CAP for f in facts)
    print("comb %s %s: raw regions %d..%d, reads beyond %d raw regions %d, of them edited beyond it %d, final regions beyond it in %d, without structure %d"
          % (graph, how, min(nraw), max(nraw), STRUCT_DEG_CAP, beyond, edited, kept_beyond, sum(not f["ok"] for f in facts)))
    if graph.endswith("k21"):
        assert beyond >= 10, (graph, how, beyond)               # the degree reads beyond the regions kept in LDS
        if how == "sub":
            assert edited >= 8, (graph, how, edited)            # ... and the per-position walks there
        else:
            assert kept_beyond >= 10, (graph, how, kept_beyond)
    else:   # K = 31: region counts between one and eight 64-region passes
        assert sum(64 < n <= STRUCT_DEG_CAP for n in nraw) >= 12, (graph, how, sorted(nraw))


# ---------------------------------------------------------------- the device image of a table, and where its keys live
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
KEY_MASK = np.uint64((1 << 61) - 1)
BUCKET = np.dtype([("key", "<u8"), ("cnt", "<u4", (4,)), ("jc", "<u2", (4,))])
assert BUCKET.itemsize == 32


def _hip():
    hip = C.CDLL("libamdhip64.so")     # the HIP runtime libtalc_hip.so itself runs on: plain device buffers from it
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


class DeviceImage:
    """The image of a table on GPU 0 in two caller-owned device buffers, and its copy on the host."""

    def __init__(self, ttab):
        self.hip = _hip()
        self.nb = ttab.image_bytes
        self.right_ptr, self.left_ptr = C.c_void_p(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.right_ptr), self.nb) == 0 and self.hip.hipMalloc(C.byref(self.left_ptr), self.nb) == 0
        ttab.export_device(0, self.right_ptr.value, self.left_ptr.value)
        self.right, self.left = np.empty(ttab.capacity, BUCKET), np.empty(ttab.capacity, BUCKET)
        assert self.hip.hipMemcpy(self.right.ctypes.data, self.right_ptr, self.nb, 2) == 0      # (2: device to host)
        assert self.hip.hipMemcpy(self.left.ctypes.data, self.left_ptr, self.nb, 2) == 0

    def store(self):
        """The host copy (edited by the caller) back into the two device buffers."""
        assert self.hip.hipMemcpy(self.right_ptr, self.right.ctypes.data, self.nb, 1) == 0     # (1: host to device)
        assert self.hip.hipMemcpy(self.left_ptr, self.left.ctypes.data, self.nb, 1) == 0

    def free(self):
        self.hip.hipFree(self.right_ptr)
        self.hip.hipFree(self.left_ptr)


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def table_home(keys, cap):
    """table_slot(table_hash(key), cap) of talc_common.h for an array of (K-1)-mer keys: int64 home slots."""
    k = _u64(keys)
    x = k ^ (k >> np.uint64(29))
    h = x * np.uint64(0x9E3779B97F4A7C15)                      # (uint64 arrays multiply modulo 2^64)
    return (((h >> np.uint64(32)) * np.uint64(cap & 0xFFFFFFFF)) >> np.uint64(32)).astype(np.int64)


def mix64(x):
    x = _u64(x).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def count_home(keys, mask):
    """count_home of talc_kernels_count.h (mix64(key) & mask) for an array of packed k-mers: int64 home slots."""
    return (mix64(keys) & np.uint64(mask)).astype(np.int64)


def image_homes(tab, what=""):
    """One bucket table of an exported image (BUCKET[cap]) against table_home: from the home of every stored key, walking
    over occupied slots with the wrap at the end of the table, the key's own slot is reached before an empty one.  That
    holds for a linear-probing table whatever order its keys went in, and for a wrong mirror of the hash it fails at once.
    Returns (slots of the occupied buckets, their keys without degree bits, their homes)."""
    cap = len(tab)
    occ = tab["key"] != EMPTY
    slots = np.nonzero(occ)[0].astype(np.int64)
    keys = tab["key"][occ] & KEY_MASK
    home = table_home(keys, cap)
    assert ((home >= 0) & (home < cap)).all()
    holes = np.concatenate([[0], np.cumsum(~occ)]).astype(np.int64)      # holes[i] = empty slots below i
    inside = holes[slots + 1] - holes[home]                              # empty slots in [home, slot] when home <= slot
    around = (holes[cap] - holes[home]) + holes[slots + 1]               # ... in [home, cap) and [0, slot] otherwise
    gaps = np.where(home <= slots, inside, around)
    assert (gaps == 0).all(), (what, int((gaps != 0).sum()), len(slots))
    return slots, keys, home


@contextlib.contextmanager
def table_slots_x10(x10):
    """TALC_TABLE_SLOTS_X10 for the table calls made inside (a table call reads the switches when it starts)."""
    old = os.environ.get("TALC_TABLE_SLOTS_X10")
    os.environ["TALC_TABLE_SLOTS_X10"] = str(x10)
    try:
        yield
    finally:
        if old is None:
            del os.environ["TALC_TABLE_SLOTS_X10"]
        else:
            os.environ["TALC_TABLE_SLOTS_X10"] = old


def kmer_text(key, n):
    return "".join("ACGT"[(int(key) >> (2 * (n - 1 - i))) & 3] for i in range(n))


def revcomp_packed(kms, k):
    kms = _u64(kms).copy()
    r = np.zeros_like(kms)
    for _ in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - (kms & np.uint64(3)))
        kms >>= np.uint64(2)
    return r


def zone_kmers(k, cap, W, n, rng, avoid=()):
    """Random k-mers by rejection: n whose RIGHT key (km >> 2) and n whose LEFT key (km & m1) has its home in the last W
    slots of a table of `cap` buckets; none of `avoid`, all distinct, and every one of the W slots is the home of at
    least two of each n (the first 2 W of them go round the slots), so the zone is full whatever order they go in."""
    assert n >= 2 * W
    m1 = np.uint64((1 << (2 * (k - 1))) - 1)
    per = {1: [[] for _ in range(W)], 0: [[] for _ in range(W)]}      # candidates by home slot
    seen = set(int(x) for x in avoid)

    def enough(slots):
        return min(len(s) for s in slots) >= 2 and sum(len(s) for s in slots) >= n

    while not (enough(per[0]) and enough(per[1])):
        km = rng.integers(0, 1 << (2 * k), 4_000_000, dtype=np.uint64)
        for d, key in ((1, km >> np.uint64(2)), (0, km & m1)):
            home = table_home(key, cap)
            sel = np.nonzero(home >= cap - W)[0]
            for x, h in zip(km[sel].tolist(), home[sel].tolist()):
                if x not in seen:
                    seen.add(x)
                    per[d][h - (cap - W)].append(x)
    out = []
    for d in (1, 0):
        first = [s[i] for i in (0, 1) for s in per[d]]
        rest = [x for s in per[d] for x in s[2:]]
        out.append(np.array((first + rest)[:n], dtype=np.uint64))
    return out[0], out[1]


class EndLoaded:
    """What end_loaded_table returns: the dump (keys, counts) and the junction lines (jk, jc) both sides were built
    from, the oracle table and the product table, and the k-mers of the zone (the last W slots of either table)."""

    def upload(self, device=0):
        self.ttab.upload(device)
        self.ctx = T.Context(self.ttab, self.p, device)
        return self.ctx

    def reads(self, first, n):
        return self.synth.reads(first, n)

    def build_product(self, device=None):
        """Another product table from the same dump, colours applied (for runs under other switches)."""
        with table_slots_x10(self.x10):
            t = T.Table.from_arrays(self.keys, self.counts, self.p, device=device)
        assert t.capacity == self.capacity
        if len(self.jk):
            t.colour(self.jk, self.jc)
        t.decolour_repeats()
        return t


def end_loaded_dump(base_keys, base_counts, fill_r, fill_l, minc, rng):
    """The dump of an end-loaded table, fillers first (a host builder inserts in dump order: what comes later with its
    home in the zone goes over the end): every filler once with a count below MIN_COUNT, then with the count it keeps,
    then the base dump, then every filler again with another count (the first KEPT line wins)."""
    fill = np.concatenate([fill_r, fill_l]).astype(np.uint64)
    kept = rng.integers(minc, 60, len(fill)).astype(np.uint32)
    keys = np.concatenate([fill, fill, np.asarray(base_keys, np.uint64), fill[::-1]])
    counts = np.concatenate([np.full(len(fill), minc - 1, np.uint32), kept, np.asarray(base_counts, np.uint32),
                             (kept[::-1] + 9).astype(np.uint32)])
    return keys, counts


def end_loaded_junctions(fill, k, thr, rng):
    """Junction lines over the fillers and their reverse complements: several lines reach one k-mer (the last in
    (line, strand) order wins), colours at, above and below colouredCountThr, a negative one; and the four homopolymers."""
    fill = np.asarray(fill, np.uint64)
    rc = revcomp_packed(fill, k)
    n = len(fill)
    jk = np.concatenate([fill, rc, fill[: n // 2], rc[n // 3:], fill[::3]])
    jc = np.concatenate([rng.integers(1, 200, n), rng.integers(200, 400, n), rng.integers(400, 600, n // 2),
                         rng.integers(600, 800, n - n // 3), rng.integers(800, 900, len(fill[::3]))]).astype(np.int64)
    special = np.array([thr, thr + 1, thr - 1, -5, thr, -1], dtype=np.int64)
    sk = np.concatenate([fill[:3], rc[3:6]])                                   # (late lines: these decide)
    hom = np.array([int(d * k, 4) for d in "0123"], dtype=np.uint64)
    return np.concatenate([jk, sk, hom]), np.concatenate([jc, special, np.full(4, 77, np.int64)])


def end_loaded_table(synth, k, x10, W, F, rng, device=None, colour=True, admit=None, **params_kw):
    """A table whose probe chains must cross the end: the generator's dump plus F filler k-mers, half with their RIGHT
    key's home in the last W slots of the table and half with their LEFT key's.  The capacity depends on the number of kept
    lines alone, so it is learnt from a build with placeholder fillers, the real ones are drawn by rejection against it,
    and the rebuilt table must have the same capacity.  Also draws absent k-mers of the zone, F / 2 per direction.  The
    dump both sides are built from is the generator's without the few lines whose key is at home in slot 0 (below).
    admit(base_keys, base_counts, capacity), if given, is asked once the capacity is known and before anything else is
    drawn or built; None is returned if it says no."""
    E = EndLoaded()
    E.synth, E.k, E.x10, E.W = synth, k, x10, W
    E.p, E.q = both_params(k=k, use_junctions=int(colour), **params_kw)
    minc = E.p.min_count
    base_keys, base_counts = synth.dump_arrays(release=False)
    # homopolymers, stored: de-colouring finds them.  Not poly-A: its keys are 0, whose home is slot 0 at every capacity,
    # and slot 0 is wanted for a key that comes over the end (below); its junction line stays, for a k-mer not stored.
    hom = np.array([int(d * k, 4) for d in "123"], dtype=np.uint64)
    base_keys = np.concatenate([base_keys, hom])
    base_counts = np.concatenate([base_counts, np.full(3, 50, np.uint32)])
    h = F // 2
    place = rng.integers(0, 1 << (2 * k), F, dtype=np.uint64)
    m1 = np.uint64((1 << (2 * (k - 1))) - 1)
    for _ in range(10):
        with table_slots_x10(x10):
            t0 = T.Table.from_arrays(*end_loaded_dump(base_keys, base_counts, place[:h], place[h:], minc, rng), E.p)
        E.capacity = t0.capacity
        t0.close()
        # slot 0 must go to a key that comes over the end, so no key of the base dump may have its home there: the lines
        # that do (a key is at home in slot 0 when the top 32 bits of its hash are below 2^32 / capacity, whatever the
        # capacity nearby: one or two lines of 60 000) are left out of the dump, on both sides
        at0 = (table_home(base_keys >> np.uint64(2), E.capacity) == 0) | (table_home(base_keys & m1, E.capacity) == 0)
        if not at0.any():
            break
        base_keys, base_counts = base_keys[~at0], base_counts[~at0]
    else:
        raise AssertionError("the capacity does not settle")
    if admit is not None and not admit(base_keys, base_counts, E.capacity):
        return None
    stored = base_keys[base_counts >= minc]
    zr, zl = zone_kmers(k, E.capacity, W, 2 * h, rng, avoid=stored.tolist())
    E.fill_r, E.fill_l, E.absent_r, E.absent_l = zr[:h], zl[:h].copy(), zr[h:], zl[h:]
    # every second LEFT filler (from the 2 W-th on) is a RIGHT filler's predecessor instead: b + (the first K - 1 bases of the
    # RIGHT filler), so its LEFT key is that filler's RIGHT key — the same value, so the same home, in the zone of the LEFT
    # table too — and a read can hold both at consecutive positions (E.chain: such pairs).  At most W RIGHT keys of the
    # zone are stored at or above their home, so with more than W pairs some pair's RIGHT bucket is a wrapped one.
    E.chain = []
    taken = set(stored.tolist()) | set(zr.tolist()) | set(zl.tolist())
    for i in range(2 * W, h, 2):
        g = (int(rng.integers(0, 4)) << (2 * (k - 1))) | (int(E.fill_r[i]) >> 2)
        if g not in taken:
            taken.add(g)
            E.fill_l[i] = g
            E.chain.append((g, int(E.fill_r[i])))
    E.fill = np.concatenate([E.fill_r, E.fill_l])
    E.keys, E.counts = end_loaded_dump(base_keys, base_counts, E.fill_r, E.fill_l, minc, rng)
    E.jk, E.jc = end_loaded_junctions(E.fill, k, E.p.coloured_count_thr, rng) if colour else (np.zeros(0, np.uint64), np.zeros(0, np.int64))
    E.otab = O.OracleTable(E.q, O.OracleTable.FLAT)
    E.otab.insert_packed(E.keys, E.counts)
    if colour:
        E.otab.colour_packed(E.jk, E.jc)
    E.otab.decolour()
    E.ttab = E.build_product(device)
    E.ctx = None
    return E


def refill_end_cluster(tab, first):
    """One bucket table of an image with the run of occupied slots that crosses the end of the table filled again, the
    buckets whose key is in `first` before the others: each bucket (key, counts, colours) goes to the first free slot from
    its key's home on, with the wrap.  A linear-probing table's occupied slots do not depend on the order its keys went
    in, only which key sits where does; so the result is the same table as the device builder would have left had the
    CASes of `first` landed first.  Returns the new table; the occupied slots are asserted unchanged."""
    cap = len(tab)
    occ = tab["key"] != EMPTY
    assert not occ.all()
    s, e = cap, 0
    while occ[s - 1]:
        s -= 1
    while occ[e]:
        e += 1
    slots = np.array(list(range(s, cap)) + list(range(e)), dtype=np.int64)
    if s == cap or e == 0:
        return tab.copy()
    buckets = tab[slots].copy()
    home = table_home(buckets["key"] & KEY_MASK, cap).tolist()
    keys = (buckets["key"] & KEY_MASK).tolist()
    out = tab.copy()
    out[slots] = tab[np.nonzero(~occ)[0][0]]                       # (an empty bucket)
    for i in sorted(range(len(slots)), key=lambda i: (keys[i] not in first, i)):
        j = home[i]
        assert s <= j or j < e, (keys[i], j, s, e)                 # a key's home lies in the run that holds it
        while out["key"][j] != EMPTY:
            j = j + 1 if j + 1 < cap else 0
        out[j] = buckets[i]
    assert ((out["key"] != EMPTY) == occ).all()
    return out


def zone_reach(tab, W, genuine=None, what=""):
    """The reach conditions of an end-loaded bucket table, from its exported image and the homes alone: the last W slots
    and slot 0 are occupied, more keys than W have their home in the last W slots, and the keys stored below their home
    (after the wrap) are counted — all of them, and those of `genuine` (a set of keys) among them."""
    cap = len(tab)
    slots, keys, home = image_homes(tab, what)
    occ = tab["key"] != EMPTY
    assert occ[cap - W:].all() and occ[0], (what, occ[cap - W:].tolist(), bool(occ[0]))
    in_zone = int((home >= cap - W).sum())
    assert in_zone > W, (what, in_zone)
    below = home > slots
    assert home[slots == 0][0] >= cap - W, (what, int(home[slots == 0][0]))       # slot 0 holds a key that came over the end
    gen = sum(1 for x in keys[below].tolist() if x in genuine) if genuine is not None else 0
    return dict(in_zone=in_zone, below=int(below.sum()), genuine_below=gen, last_wrapped_slot=int(slots[below].max()) if below.any() else -1)


# ---------------------------------------------------------------- the checkers of the derived device tables
# (tests/test_gpu_derived_tables.py on the generator's tables, tests/test_gpu_table_edges.py on end-loaded ones).  `small`:
# a pair uploaded to GPU 0 with .name, .before / .after (its DeviceImage before and after the upload) and .right / .left
# (bucket_dicts of its dump).
def check_indegree_bits_of_every_right_bucket(small):
    before, after = small.before, small.after
    occ = after.right["key"] != EMPTY
    assert ((before.right["key"] != EMPTY) == occ).all() and int(occ.sum()) == len(small.right)
    assert (before.right["key"][occ] >> np.uint64(61) == 0).all()                       # nothing there before the upload
    assert ((after.right["key"][occ] & KEY_MASK) == before.right["key"][occ]).all()     # the key itself is untouched
    assert (after.right["cnt"] == before.right["cnt"]).all() and (after.right["jc"] == before.right["jc"]).all()
    assert after.left.tobytes() == before.left.tobytes()
    keys = (after.right["key"][occ] & KEY_MASK).tolist()
    got = (after.right["key"][occ] >> np.uint64(61)).astype(np.int64)
    minc = small.p.min_count
    want = np.array([sum(1 for c in small.left.get(p, ()) if c >= minc) for p in keys], dtype=np.int64)
    assert (got == want).all(), (np.nonzero(got != want)[0][:5], got[got != want][:5], want[got != want][:5])
    assert set(keys) == set(small.right)
    hist = np.bincount(want, minlength=5)
    print(small.name, "in-degrees 0..4:", hist.tolist())
    assert hist[0] > 0 and hist[1] > 0.5 * len(keys)
    if small.name.startswith("branching"):
        assert hist[2:].sum() >= 100


def cov_degrees(ctx, bases, offs):
    b = ctx.batch(bases, offs)
    b.coverage()
    c, j, ko, nin = b.fetch_coverage()
    d = b.fetch_coverage_degrees()
    b.close()
    return c, j, d


def check_image_exported_after_an_upload_imports_to_the_same_table(small):
    t2 = T.Table.import_device(small.p, small.ttab.capacity, len(small.ttab), small.after.right_ptr.value, small.after.left_ptr.value, 0)
    staged = DeviceImage(t2)
    assert staged.right.tobytes() == small.after.right.tobytes() and staged.left.tobytes() == small.after.left.tobytes()
    staged.free()
    t2.upload(0)
    again = DeviceImage(t2)
    assert again.right.tobytes() == small.after.right.tobytes() and again.left.tobytes() == small.after.left.tobytes()
    again.free()
    for d in (0, 1):
        assert t2.fetch_walk(d).tobytes() == small.ttab.fetch_walk(d).tobytes()
    ctx2 = T.Context(t2, small.p, 0)
    bases, offs = small.reads(0, 80)
    a, b = cov_degrees(small.ctx, bases, offs), cov_degrees(ctx2, bases, offs)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and int((a[2] != 0).sum()) > 1000
    ctx2.close()
    t2.close()


def check_every_walk_record_equals_the_plain_walk(small):
    k, minc = small.p.k, small.p.min_count
    t0 = time.time()
    why_all = {}
    for d, image, tab in ((1, small.after.right, small.right), (0, small.after.left, small.left)):
        w = small.ttab.fetch_walk(d)
        occ = image["key"] != EMPTY
        assert ((w["key"] == EMPTY) == ~occ).all() and (w["lvl"][~occ] == 0).all()
        assert (w["key"][occ] == (image["key"][occ] & KEY_MASK)).all()
        succ = lambda key, direction, tab=tab: tab.get(key)
        keys = w["key"][occ].tolist()
        got = w["lvl"][occ].astype(np.int64)
        want = np.zeros_like(got)
        for i, key in enumerate(keys):
            want[i], why = walk_reference(succ, key, d, k, minc)
            why_all[why] = why_all.get(why, 0) + 1
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (d, len(bad), keys[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
        single = (want & WALK_SINGLE) != 0
        assert single.sum() > (0 if small.name.startswith("x700") else 0.5 * want.shape[0]) and (~single[:, 0]).sum() > 0
    print(small.name, "walks ended by", why_all, "%.1f s" % (time.time() - t0))
    assert why_all.get("missing", 0) > 0 and why_all.get("last", 0) > 0 and why_all.get("count0", 0) == 0
    assert (why_all.get("clamp", 0) > 100) == small.name.startswith("x700")


def flank(tab, key, direction, k, n, rng):
    """n bases that continue the (K-1)-mer `key` in the graph (the first stored successor each time), random ones where
    the graph ends."""
    m1 = (1 << (2 * (k - 1))) - 1
    out = []
    for _ in range(n):
        c = tab.get(key)
        b = next((i for i in range(4) if c[i]), None) if c else None
        if b is None:
            b = int(rng.integers(0, 4))
        out.append("ACGT"[b])
        key = (((key << 2) | b) & m1) if direction else ((b << (2 * (k - 2))) | (key >> 2))
    return "".join(out) if direction else "".join(reversed(out))


def check_presence_filter_has_no_false_negative(small):
    k, minc = small.p.k, small.p.min_count
    stored = small.keys[small.counts >= minc]
    oc, _ = small.otab.lookup_packed(stored)
    assert (oc >= minc).all() and len(stored) > 40_000
    texts = [kmer_text(int(x), k) for x in stored.tolist()]
    bases, offs = pack_reads(texts)
    c, j, d = cov_degrees(small.ctx, bases, offs)
    assert len(c) == len(stored) and (c == oc).all(), int((c != oc).sum())
    assert (d != 0).all()
    rng = np.random.default_rng(8)
    m1 = (1 << (2 * (k - 1))) - 1
    long_reads = [flank(small.left, int(x) >> 2, 0, k, k - 1, rng) + t + flank(small.right, int(x) & m1, 1, k, k - 1, rng)
                  for x, t in zip(stored.tolist(), texts)]
    bases, offs = pack_reads(long_reads)
    c, j, d = cov_degrees(small.ctx, bases, offs)
    c = c.reshape(len(stored), 2 * k - 1)
    assert (c[:, k - 1] == oc).all(), int((c[:, k - 1] != oc).sum())
    nhit = 0
    for i in range(0, len(long_reads), 7):            # and every position of every seventh read against the oracle's coverage
        want, _, _ = small.otab.coverage(long_reads[i])
        assert (c[i] == want).all(), i
        nhit += int((want > 0).sum())
    print(small.name, "flanked reads: %.1f of %d positions are hits" % (nhit / len(range(0, len(long_reads), 7)), 2 * k - 1))


# ---------------------------------------------------------------- what is asked of an end-loaded table (host and device)
def zone_queries(E):
    """Every k-mer worth a point lookup on an end-loaded table: every dump line, the absent k-mers of the zone (their
    probe runs over the end to the first empty slot), every filler with its last base changed and with its first base
    changed (the key is there, the count slot is 0), the junction lines and their reverse complements."""
    k = E.k
    top = np.uint64(2 * (k - 1))
    last = np.concatenate([E.fill ^ np.uint64(x) for x in (1, 2, 3)])
    first = np.concatenate([E.fill ^ (np.uint64(x) << top) for x in (1, 2, 3)])
    parts = dict(dump=E.keys, absent=np.concatenate([E.absent_r, E.absent_l]), last=last, first=first,
                 junction=np.concatenate([E.jk, revcomp_packed(E.jk, k)]) if len(E.jk) else np.zeros(0, np.uint64))
    return parts


def check_zone_lookups(E, lookups):
    """Point lookups of zone_queries against the oracle table; `lookups`: (label, function(kmers) -> (counts, colours)).
    What the queries are there for is asserted on the oracle's answers."""
    parts = zone_queries(E)
    minc = E.p.min_count
    stored = set(E.keys[E.counts >= minc].tolist())
    for name, q in parts.items():
        if not len(q):
            continue
        oc, oj = E.otab.lookup_packed(q)
        if name == "absent":
            assert (oc == 0).all() and len(q) >= E.W
        elif name in ("last", "first"):
            free = np.array([x not in stored for x in q.tolist()])
            assert (oc[free] == 0).all() and free.sum() > 2 * len(E.fill)
        elif name == "dump":
            assert (oc[E.counts >= minc] >= minc).all()
            fl = np.isin(q, E.fill)                                   # the fillers' lines: below MIN_COUNT, kept, a later duplicate
            assert int(fl.sum()) == 3 * len(E.fill) and len(set(oc[fl].tolist())) > 5
        elif name == "junction":
            assert int((oj > 0).sum()) >= len(E.fill) // 2 and (oj < E.p.coloured_count_thr).all()
        for label, fn in lookups:
            c, j = fn(q)
            assert (c == oc).all() and (j == oj).all(), (label, name, int((c != oc).sum()), int((j != oj).sum()))
    return {n: len(q) for n, q in parts.items()}


def zone_successor_queries(E):
    """(direction, k-mers) whose successor query reads a bucket of the zone: direction 1 (RIGHT) probes RIGHT[km & m1],
    direction 0 probes LEFT[km >> 2]; from the fillers' keys (present) and the absent k-mers' keys (not there)."""
    k = E.k
    m1 = np.uint64((1 << (2 * (k - 1))) - 1)
    top = np.uint64(2 * (k - 1))
    rkeys = np.concatenate([E.fill_r, E.absent_r]) >> np.uint64(2)
    lkeys = np.concatenate([E.fill_l, E.absent_l]) & m1
    return ((1, np.concatenate([(np.uint64(b) << top) | rkeys for b in range(4)])),
            (0, np.concatenate([(lkeys << np.uint64(2)) | np.uint64(b) for b in range(4)])))


def junction_dump_files(E, tmp_path):
    """The dump and the junction lines of an end-loaded table as text files (`KMER count` per line)."""
    import kmer_ref
    dump, junc = str(tmp_path / "dump.txt"), str(tmp_path / "junctions.txt")
    kmer_ref.write_dump(dump, E.keys, E.counts, E.k)
    kmer_ref.write_dump(junc, E.jk, E.jc, E.k)
    return dump, junc


COUNT_EDGES = ("count-ffffffff", "no-lines", "one-prefix")


def count_edge_dump(name, k, rng):
    """(keys, counts) of the count edges: a count of exactly 0xFFFFFFFF (beside ordinary counts, a duplicate of it later
    and one before it below MIN_COUNT), a dump without a kept line, a dump whose kept k-mers share one (K-1)-prefix (one
    RIGHT bucket, four LEFT buckets)."""
    r = rng.integers(0, 1 << (2 * k), 40, dtype=np.uint64)
    if name == "count-ffffffff":
        keys = np.concatenate([r[:1], r, r[:3]])
        counts = np.concatenate([[1], np.full(40, 0xFFFFFFFF), [5, 6, 7]]).astype(np.uint32)
        counts[10:30] = rng.integers(0, 50, 20)
        return keys, counts
    if name == "no-lines":
        return r[:8], np.array([0, 1, 1, 0, 1, 1, 1, 0], dtype=np.uint32)
    prefix = r[0] >> np.uint64(2) << np.uint64(2)
    return np.array([prefix | np.uint64(b) for b in (0, 1, 2, 3, 2)], dtype=np.uint64), np.array([9, 0xFFFFFFFF, 3, 4, 8], dtype=np.uint32)


def check_count_edge(name, k, device):
    """A count edge through one builder (device None: the host's; lookups through the host image either way, which for a
    device-built table is the device's image copied back) against the oracle.  Returns the product table."""
    rng = np.random.default_rng(5)
    keys, counts = count_edge_dump(name, k, rng)
    p, q = both_params(k=k)
    ot = O.OracleTable(q, O.OracleTable.FLAT)
    ot.insert_packed(keys, counts)
    ot.decolour()
    om = O.OracleTable(q, O.OracleTable.MAP)
    om.insert_packed(keys, counts)
    tt = T.Table.from_arrays(keys, counts, p, device=device)
    tt.decolour_repeats()
    assert len(tt) == len(ot) == len(om), (name, len(tt), len(ot))
    assert (len(tt) > 30) if name == "count-ffffffff" else len(tt) == {"no-lines": 0, "one-prefix": 4}[name]
    m1 = np.uint64((1 << (2 * (k - 1))) - 1)
    qs = np.concatenate([keys, keys ^ np.uint64(1), keys ^ np.uint64(2), rng.integers(0, 1 << (2 * k), 500, dtype=np.uint64),
                         (keys & m1), keys >> np.uint64(2)])
    oc, oj = ot.lookup_packed(qs)
    mc, _ = om.lookup_packed(qs)
    assert (mc == oc).all()
    if name == "count-ffffffff":
        assert int((oc == 0xFFFFFFFF).sum()) >= 20
    c, j = tt.lookup_host(qs)
    assert (c == oc).all() and (j == oj).all(), (name, device, c[c != oc][:5], oc[c != oc][:5])
    return tt, ot, keys, qs, oc, oj
