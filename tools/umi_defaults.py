#!/usr/bin/env python3
"""How the default max_error_pct of the UMI read-out was chosen (docs/umi.md): on 2000 uniform random reads of 2000 bytes
(numpy.random.default_rng(0)), the anchored pattern GCTGATATTGCTTTVVVVTTVVVVTTVVVVTTVVVVTTTGGG and a window of 256, how many
ends the numpy reference (tests/umi_ref.py) accepts at 5, 10, 15 and 20 per cent.  The default is the largest of them at
which no end of any read is accepted.  CPU only.  The record is profiles/r14/umi_defaults.txt.
    python tools/umi_defaults.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ends_ref as R  # noqa: E402
import umi_ref as U  # noqa: E402

rng = np.random.default_rng(0)
reads = [R.random_seq(rng, 2000) for _ in range(2000)]
masks = U._MASK[np.frombuffer(U.ANCHORED.encode(), np.uint8)]
m = len(U.ANCHORED)
d = np.zeros((len(reads), 2), np.int64)                     # d of every read and end: the setting only compares it with k
for r, rd in enumerate(reads):
    c = R._CODE[np.frombuffer(rd.encode(), np.uint8)]
    tc = c[-256:][::-1]
    d[r] = U.matrix(masks, np.stack([c[:256], np.where(tc < 4, 3 - tc, tc)]))[:, m, 1:].min(axis=1)
default = None
for pct in (5, 10, 15, 20):
    k = pct * m // 100
    ends = int((d <= k).sum())
    if ends == 0:
        default = pct
    print("pct %d (k %d): %d ends accepted, %d reads with an accepted end" % (pct, k, ends, int((d <= k).any(axis=1).sum())), flush=True)
print("smallest d over all ends: %d" % int(d.min()))
check = U.rows(reads[:200], U.ANCHORED, 20)
print("rows() on the first 200 reads at 20 per cent: %d with an end" % int((check["end"] != 0).sum()))
print("default: %s" % default)
