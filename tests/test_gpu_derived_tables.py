"""-m gpu: the device tables an upload derives from the bucket tables — the in-degree bits in the RIGHT keys
(k_build_indegree), the walk records (k_build_walk), the presence filter (k_build_filter) — and the count model's threshold
table (k_build_thresholds), each compared with a plain reference instead of through the records it leads to.

Small tables (about 60 k k-mers): unique sequence, a branching graph of stress set 103's kind, junction colours, and
counts x 700 (level counts pass the 13-bit field of a walk level); K = 18, 21, 31."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
KEY_MASK = np.uint64((1 << 61) - 1)
BUCKET = np.dtype([("key", "<u8"), ("cnt", "<u4", (4,)), ("jc", "<u2", (4,))])
assert BUCKET.itemsize == 32

TABLES = {
    "unique-k21": dict(target_kmers=60_000, k=21, seed=61),
    "branching-k18": dict(target_kmers=60_000, k=18, seed=62, synth_kw=dict(paralog_frac=0.8, paralog_div=0.04)),
    "junctions-k31": dict(target_kmers=60_000, k=31, seed=63, junctions=True),
    "x700-k21": dict(target_kmers=60_000, k=21, seed=64, count_scale=700, min_count=2 * 700),
}


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

    def free(self):
        self.hip.hipFree(self.right_ptr)
        self.hip.hipFree(self.left_ptr)


@pytest.fixture(scope="module", params=list(TABLES))
def small(request):
    """A device-built pair (its image can be exported before the upload), the image before and after the upload, and the
    bucket dictionaries of its dump."""
    pair = PU.Pair(device_built=True, **TABLES[request.param])
    pair.name = request.param
    before = DeviceImage(pair.ttab)
    pair.upload(0)
    pair.before, pair.after = before, DeviceImage(pair.ttab)
    k, minc = pair.p.k, pair.p.min_count
    pair.right, pair.left = PU.bucket_dicts(pair.keys, pair.counts, k, minc)
    yield pair
    pair.before.free()
    pair.after.free()


def _text(key, n):
    return "".join("ACGT"[(key >> (2 * (n - 1 - i))) & 3] for i in range(n))


def test_bucket_dictionaries_are_the_oracles_successor_counts(small):
    """The numpy / dictionary view of the dump that the references below read, against getNextCounts of the oracle."""
    k = small.p.k
    for d, tab in ((1, small.right), (0, small.left)):
        for key in list(tab)[::40]:
            kmer = ("A" + _text(key, k - 1)) if d else (_text(key, k - 1) + "A")      # any k-mer whose successors these are
            c, _ = small.otab.next_counts(kmer, d)
            assert c.tolist() == tab[key], (d, key)
    assert len(small.right) > 40_000


def test_indegree_bits_of_every_right_bucket(small):
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


def _cov_degrees(ctx, bases, offs):
    b = ctx.batch(bases, offs)
    b.coverage()
    c, j, ko, nin = b.fetch_coverage()
    d = b.fetch_coverage_degrees()
    b.close()
    return c, j, d


def test_image_exported_after_an_upload_imports_to_the_same_table(small):
    """An image that already carries in-degree bits (test_table_image_export_and_import sends such an image without
    looking): its own upload writes the same bits again, and the coverage kernel reads the same degrees from it."""
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
    a, b = _cov_degrees(small.ctx, bases, offs), _cov_degrees(ctx2, bases, offs)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and int((a[2] != 0).sum()) > 1000
    ctx2.close()
    t2.close()


def test_every_walk_record_equals_the_plain_walk(small):
    """Level j + 1 follows level j's largest count (the first base wins a tie); a count that does not fit 13 bits ends the
    walk, as does a bucket that does not exist (the remaining levels stay 0); an unused slot has an empty key and no
    levels.  A level with count 0 cannot occur: a bucket exists only because one of its four k-mers is stored."""
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
            want[i], why = PU.walk_reference(succ, key, d, k, minc)
            why_all[why] = why_all.get(why, 0) + 1
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (d, len(bad), keys[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
        single = (want & PU.WALK_SINGLE) != 0
        assert single.sum() > (0 if small.name.startswith("x700") else 0.5 * want.shape[0]) and (~single[:, 0]).sum() > 0
    print(small.name, "walks ended by", why_all, "%.1f s" % (time.time() - t0))
    assert why_all.get("missing", 0) > 0 and why_all.get("last", 0) > 0 and why_all.get("count0", 0) == 0
    assert (why_all.get("clamp", 0) > 100) == small.name.startswith("x700")


def _flank(tab, key, direction, k, n, rng):
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


def test_presence_filter_has_no_false_negative(small):
    """Through the kernel that reads it: every stored k-mer as a read of exactly K bases, and in the middle of a read of
    3 K - 2 bases (its minimizer window then holds foreign M-mers, and its neighbours in the tile are looked up too) —
    every count equals the oracle's."""
    k, minc = small.p.k, small.p.min_count
    stored = small.keys[small.counts >= minc]
    oc, _ = small.otab.lookup_packed(stored)
    assert (oc >= minc).all() and len(stored) > 40_000
    texts = [_text(int(x), k) for x in stored.tolist()]
    bases, offs = PU.pack_reads(texts)
    c, j, d = _cov_degrees(small.ctx, bases, offs)
    assert len(c) == len(stored) and (c == oc).all(), int((c != oc).sum())
    assert (d != 0).all()
    rng = np.random.default_rng(8)
    m1 = (1 << (2 * (k - 1))) - 1
    long_reads = [_flank(small.left, int(x) >> 2, 0, k, k - 1, rng) + t + _flank(small.right, int(x) & m1, 1, k, k - 1, rng)
                  for x, t in zip(stored.tolist(), texts)]
    bases, offs = PU.pack_reads(long_reads)
    c, j, d = _cov_degrees(small.ctx, bases, offs)
    c = c.reshape(len(stored), 2 * k - 1)
    assert (c[:, k - 1] == oc).all(), int((c[:, k - 1] != oc).sum())
    nhit = 0
    for i in range(0, len(long_reads), 7):            # and every position of every seventh read against the oracle's coverage
        want, _, _ = small.otab.coverage(long_reads[i])
        assert (c[i] == want).all(), i
        nhit += int((want > 0).sum())
    print(small.name, "flanked reads: %.1f of %d positions are hits" % (nhit / len(range(0, len(long_reads), 7)), 2 * k - 1))


@pytest.mark.parametrize("alpha,err", [(2.57, 0.025), (0.5, 0.025), (1.3, 0.025), (2.57, 1.5), (0.5, 1.5), (1.3, 1.5)])
def test_tagging_through_the_threshold_table(gpu_pair, alpha, err):
    """tagNextNodes as the search calls it — the count model read from the per-context threshold table for counts (and
    lambda_noise) below 4096, from the formula beyond — against the oracle's, for every count 0 .. 4200 and successor
    counts around both thresholds of that count."""
    L = O.lib()
    p, q = PU.both_params(k=gpu_pair.p.k, alpha=alpha, sr_error_rate=err)
    minc = p.min_count
    ctx = T.Context(gpu_pair.ttab, p, 0)
    qp = C.byref(q)

    def first_true(pred, hi):       # smallest n in [0, hi] with pred(n), hi if none (pred is monotone)
        lo = 0
        while lo < hi:
            mid = (lo + hi) // 2
            if pred(mid):
                hi = mid
            else:
                lo = mid + 1
        return lo

    t0 = time.time()
    recs = []
    for c in range(0, 4201):
        ln = int(c * err)
        t1 = first_true(lambda n: L.orc_is_expected_by_model(qp, n, c, 0), c + 8)
        t2 = first_true(lambda n: not L.orc_is_expected_by_model(qp, n, ln, 1), ln + 4 * int(ln ** 0.5) + 16)
        vals = sorted({0, 1, minc} | {max(0, t + x) for t in (t1, t2) for x in (-2, -1, 0, 1, 2)})
        for v in vals:
            recs.append((v, c, 0, 0, 0, 0, 0, 0, c))       # one successor beside the count itself
            recs.append((v, c, 0, 0, 3, 0, 0, 0, c))       # ... coloured
            recs.append((0, v, c, v, 0, 0, 0, 0, c))       # two alike: the sum of the unexpected ones decides
    recs = np.array(recs, dtype=np.uint32)
    t1_ = time.time()
    cn, jn = np.ascontiguousarray(recs[:, :4]), np.ascontiguousarray(recs[:, 4:8])
    tags, dist = np.zeros(4, np.int32), np.zeros(4, np.float64)
    cp, jp, tp, dp = cn.ctypes.data, jn.ctypes.data, tags.ctypes.data, dist.ctypes.data
    n_table = 0
    for cx in (0, 1):
        sel = np.arange(len(recs)) if cx == 0 else np.arange(2, len(recs), 3)      # (complex only matters to the sum rule)
        got = ctx.test_dp(3, recs[sel].tobytes(), b"", p0=cx, p1=1, p2=len(sel))
        assert len(got) == len(sel)
        for w, i in zip(got.tolist(), sel.tolist()):
            count = int(recs[i, 8])
            L.orc_tag_next_nodes(qp, cp + 16 * i, jp + 16 * i, count, cx, tp, dp)
            g = [((w >> (4 * b)) & 15) for b in range(4)]
            g = [-1 if x == 15 else x for x in g]
            assert g == tags.tolist(), (recs[i].tolist(), cx, g, tags.tolist())
            used = (w >> 16) & 1
            assert used == int(count < 4096 and int(count * err) < 4096), (count, used)
            n_table += used
    print("alpha %.2f err %.3f: %d records, thresholds %.1f s, compare %.1f s, %d through the table" % (alpha, err, len(recs), t1_ - t0, time.time() - t1_, n_table))
    assert n_table > 0 and n_table < len(recs) + len(recs) // 3
    ctx.close()
