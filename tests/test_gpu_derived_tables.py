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

TABLES = {
    "unique-k21": dict(target_kmers=60_000, k=21, seed=61),
    "branching-k18": dict(target_kmers=60_000, k=18, seed=62, synth_kw=dict(paralog_frac=0.8, paralog_div=0.04)),
    "junctions-k31": dict(target_kmers=60_000, k=31, seed=63, junctions=True),
    "x700-k21": dict(target_kmers=60_000, k=21, seed=64, count_scale=700, min_count=2 * 700),
}


@pytest.fixture(scope="module", params=list(TABLES))
def small(request):
    """A device-built pair (its image can be exported before the upload), the image before and after the upload, and the
    bucket dictionaries of its dump."""
    pair = PU.Pair(device_built=True, **TABLES[request.param])
    pair.name = request.param
    before = PU.DeviceImage(pair.ttab)
    pair.upload(0)
    pair.before, pair.after = before, PU.DeviceImage(pair.ttab)
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
    PU.check_indegree_bits_of_every_right_bucket(small)


def test_image_exported_after_an_upload_imports_to_the_same_table(small):
    """An image that already carries in-degree bits (test_table_image_export_and_import sends such an image without
    looking): its own upload writes the same bits again, and the coverage kernel reads the same degrees from it."""
    PU.check_image_exported_after_an_upload_imports_to_the_same_table(small)


def test_every_walk_record_equals_the_plain_walk(small):
    """Level j + 1 follows level j's largest count (the first base wins a tie); a count that does not fit 13 bits ends the
    walk, as does a bucket that does not exist (the remaining levels stay 0); an unused slot has an empty key and no
    levels.  A level with count 0 cannot occur: a bucket exists only because one of its four k-mers is stored."""
    PU.check_every_walk_record_equals_the_plain_walk(small)


def test_presence_filter_has_no_false_negative(small):
    """Through the kernel that reads it: every stored k-mer as a read of exactly K bases, and in the middle of a read of
    3 K - 2 bases (its minimizer window then holds foreign M-mers, and its neighbours in the tile are looked up too) —
    every count equals the oracle's."""
    PU.check_presence_filter_has_no_false_negative(small)


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
