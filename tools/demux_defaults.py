#!/usr/bin/env python3
"""How the defaults of barcode demultiplexing were chosen (docs/demux.md): on 2000 uniform random reads of 2000 bytes
(numpy.random.default_rng(0)), 96 random 24-mers of pairwise edit distance >= 9 and a window of 256, how many ends accept a
barcode, how many call one and how many reads are called by either end, under the reference (tests/demux_ref.py), at 10, 15,
20 and 25 per cent and margins 0 to 3.  CPU only.  The record is profiles/r13/demux_defaults.txt.
    python tools/demux_defaults.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import demux_ref as DR  # noqa: E402
import ends_ref as R  # noqa: E402

rng = np.random.default_rng(0)
reads = [R.random_seq(rng, 2000) for _ in range(2000)]
barcodes = DR.barcode_set(96, 24, seed=11, min_dist=9)
pats = DR._patterns(barcodes)
d = np.zeros((len(reads), 2, len(barcodes)), np.int64)      # d_b of every read, end and barcode: the setting only clamps it
for r, rd in enumerate(reads):
    c = R._CODE[np.frombuffer(rd.encode(), np.uint8)]
    tc = c[-256:][::-1]
    d[r] = DR.sellers_rows(pats, np.stack([c[:256], np.where(tc < 4, 3 - tc, tc)]))[:, :, 1:].min(axis=2)
for pct in (10, 15, 20, 25):
    k = pct * 24 // 100
    for margin in range(0, min(3, k + 1) + 1):
        s = np.sort(np.minimum(d, k + 1), axis=2)
        accepted = s[:, :, 0] <= k
        calling = accepted & (s[:, :, 1] - s[:, :, 0] >= margin)
        print("pct %d (k %d) margin %d: %d ends accept, %d ends call, %d reads called by either end" % (
            pct, k, margin, int(accepted.sum()), int(calling.sum()), int(calling.any(axis=1).sum())), flush=True)
check = DR.rows(reads[:200], barcodes, 25, 2)
print("rows() on the first 200 reads at 25 per cent, margin 2: %d with a status other than 0" % int((check["status"] != 0).sum()))
