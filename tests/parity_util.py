"""Shared helpers for the parity tests: build the same table on both sides (oracle = checker,
libtalc_hip = product) from one synthetic spec and compare the two on seeded reads."""
import os
import sys

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
