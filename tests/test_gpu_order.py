"""The work queue of a batch (k_order_hist, k_order_scan, k_order_scatter through the hook talc_batch_order): a permutation of
the reads with buckets that never decrease along it, at the batch sizes around a wave, a block of 256 and the kernels' block
of 1024 reads, with every read in one bucket (the same read repeated: the worst case for the ranks taken in LDS), with every
read passed through, and over a branching graph, where the device weighs the inner gaps.  And the bucket function itself
(talc_pure.h: order_key_bucket, which the kernels and the hook share) against a restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import parity_util as PU
from talc_amd import build as B
from talc_amd import lib as T

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]   # (the kernels' block is 1024 reads: 1023 .. 1025 are its edges)
N_BUCKETS = 1024
_sets = {}


def order_set(name):
    """A 60 k-k-mer table on GPU 0 with 2049 generator reads: over unique sequence, or over the branching graph of stress
    set 103."""
    if name not in _sets:
        if name == "unique":
            pair = PU.Pair(target_kmers=60_000, k=21, seed=61)
        else:
            pair = PU.Pair(target_kmers=60_000, k=21, seed=103, synth_kw=dict(paralog_frac=0.8, paralog_div=0.04),
                           max_nb_competing_paths=8, check_interval=4)
        pair.upload(0)
        _sets[name] = (pair, PU.seqs_of(*pair.reads(0, max(SIZES))))
    return _sets[name]


def queue_of(pair, reads):
    """(order, bucket, gap scale, status after the structure kernel) of a batch, with the hook's invariants asserted."""
    b = pair.ctx.batch(*PU.pack_reads(reads))
    try:
        b.structure()
        order, bucket, scale = b.order()
        status = b.fetch_structure()["status"]
    finally:
        b.close()
    n = len(reads)
    assert len(order) == n and np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), "the queue is a permutation of the reads"
    assert (bucket < N_BUCKETS).all()
    along = bucket[order].astype(np.int64)
    assert (np.diff(along) >= 0).all(), "buckets never decrease along the queue"
    assert np.array_equal(bucket == N_BUCKETS - 1, status != T.READ_CORRECTED), "the last bucket holds the reads without a structure, and only them"
    return order, bucket, scale, status


def searched_read(pair, reads):
    """The longest of the first 64 reads that the structure kernel leaves to be searched."""
    if "searched" not in _sets:
        status = queue_of(pair, reads[:64])[3]
        _sets["searched"] = max((i for i in range(64) if status[i] == T.READ_CORRECTED), key=lambda i: len(reads[i]))
    return _sets["searched"]


def python_bucket(cost_est, cost_gap, gap_scale):
    extra = max(gap_scale, 256) - 256
    key = min(cost_est + ((cost_gap * extra) >> 8), 0xFFFFFFFF) | 1
    e = key.bit_length() - 1
    m = ((key >> (e - 5)) if e >= 5 else (key << (5 - e))) & 31
    return N_BUCKETS - 2 - min(N_BUCKETS - 2, e * 32 + m)


def test_the_bucket_function_equals_its_restatement():
    L = C.CDLL(os.path.join(B.OUT, "libtalc_pure.so"))
    L.talc_pure_order_bucket.restype = C.c_uint32
    L.talc_pure_order_bucket.argtypes = [C.c_uint32] * 3
    keys = [0, 1, 31, 32, 33, 63, 64, 1000, 2 ** 31, 2 ** 32 - 1]
    for est in keys:
        for gap, scale in ((0, 256), (est, 256), (est, 0), (est, 255), (est, 257), (est, 512), (est, 768), (2 ** 32 - 1, 768)):
            got, want = L.talc_pure_order_bucket(est, gap, scale), python_bucket(est, gap, scale)
            assert got == want, (est, gap, scale, got, want)
            assert 0 <= got <= N_BUCKETS - 2
    assert L.talc_pure_order_bucket(0, 0, 256) == N_BUCKETS - 2 and L.talc_pure_order_bucket(1, 0, 256) == N_BUCKETS - 2
    assert L.talc_pure_order_bucket(31, 0, 256) == N_BUCKETS - 2 - (4 * 32 + 30) and L.talc_pure_order_bucket(32, 0, 256) == N_BUCKETS - 2 - (5 * 32 + 1)
    # a sum beyond 32 bits is the largest key, and a scale of 256 (or below) leaves the estimate as it is
    assert L.talc_pure_order_bucket(2 ** 32 - 1, 2 ** 32 - 1, 768) == L.talc_pure_order_bucket(2 ** 32 - 1, 0, 256) == 0
    assert L.talc_pure_order_bucket(5000, 4000, 256) == L.talc_pure_order_bucket(5000, 4000, 100) == L.talc_pure_order_bucket(5000, 0, 768)
    assert L.talc_pure_order_bucket(5000, 4000, 768) == python_bucket(13000, 0, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_queue_is_a_permutation_in_bucket_order(n):
    pair, reads = order_set("unique")
    order, bucket, scale, status = queue_of(pair, reads[:n])
    assert 256 <= scale <= 768, scale                           # (k_order_scale's range; the batch's fork share decides)
    if n >= 63:
        assert len(set(bucket.tolist())) >= 5, "generator reads spread over several buckets"
    # the same read for the whole batch: one bucket, every rank of a block taken from one LDS word
    order, bucket, scale, status = queue_of(pair, [reads[searched_read(pair, reads)]] * n)
    assert status[0] == T.READ_CORRECTED and (bucket == bucket[0]).all() and bucket[0] < N_BUCKETS - 1


@pytest.mark.gpu
def test_reads_that_are_passed_through_share_the_last_bucket():
    pair, reads = order_set("unique")
    k = pair.p.k
    short = [reads[i % 50][: i % (k + 1)] for i in range(1500)]          # 0 .. K bases: every read shorter than K + 1
    st = np.asarray(pair.otab.correct_batch(*PU.pack_reads(short), nthreads=8)[2])
    assert (st == T.READ_SKIPPED_SHORT).all()                           # (the oracle's word for it)
    order, bucket, scale, status = queue_of(pair, short)
    assert (bucket == N_BUCKETS - 1).all()
    mixed = [short[i] if i % 3 else reads[i] for i in range(1500)]
    order, bucket, scale, status = queue_of(pair, mixed)
    n_last = int((bucket == N_BUCKETS - 1).sum())
    assert n_last >= 1000 and (bucket[order[-n_last:]] == N_BUCKETS - 1).all() and (bucket[order[:-n_last]] < N_BUCKETS - 1).all()
    assert set(np.nonzero(bucket < N_BUCKETS - 1)[0].tolist()) <= set(range(0, 1500, 3))


@pytest.mark.gpu
def test_a_branching_batch_is_ordered_by_the_weighed_key():
    pair, reads = order_set("branching")
    order, bucket, scale, status = queue_of(pair, reads[:1500])
    assert 256 < scale <= 768, scale                            # the device's gap scale: the graph branches
    assert len(set(bucket.tolist())) >= 5
