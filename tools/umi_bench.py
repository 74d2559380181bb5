#!/usr/bin/env python3
"""What the UMI read-out costs (docs/umi.md): BASELINE config 2 (100 k reads, 50 M-entry k = 21 dump) on one GPU, every read
dressed on the host: the head of the strand-switch primer, a copy of the anchored pattern
GCTGATATTGCTTTVVVVTTVVVVTTVVVVTTVVVVTTTGGG with 0 to 2 edits, the read, poly-A and the VN primer's reverse complement; every
second read reverse-complemented.  `--reps` fresh plain batches after a warm-up: the device time of k_read_umi (median,
minimum, maximum), the counts of the rows, and k_read_ends over the same reads in the same job as the yardstick.  Prints one
JSON line.
    python tools/umi_bench.py [--reps R] [--reads N] [--kmers N] [--k K] [--pct P] [--window W]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from talc_amd import lib as T  # noqa: E402
from talc_amd.synth import Synth  # noqa: E402

SSP_HEAD, VNP = "TTTCTGTTGGT", "ACTTGCCTGTCGCTCTATCTTC"
ANCHORED = "GCTGATATTGCTTTVVVVTTVVVVTTVVVVTTVVVVTTTGGG"

ap = argparse.ArgumentParser()
ap.add_argument("--kmers", type=int, default=50_000_000)
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--k", type=int, default=21)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--pct", type=int, default=T.UMI_DEFAULT_ERR)
ap.add_argument("--window", type=int, default=T.UMI_DEFAULT_WINDOW)
a = ap.parse_args()

rng = np.random.default_rng(0)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
revcomp = lambda s: s.translate(COMP)[::-1]


def instance():
    return bytes(b"ACG"[int(rng.integers(3))] if ch == "V" else ord(ch) for ch in ANCHORED)


def edited(seq, n):
    s = bytearray(seq)
    for at in sorted(rng.choice(len(s), size=n, replace=False).tolist(), reverse=True):
        kind = int(rng.integers(3))
        if kind == 0:
            s[at] = b"ACGT"[(b"ACGT".index(s[at]) + 1 + int(rng.integers(3))) % 4]
        elif kind == 1:
            s.insert(at, b"ACGT"[int(rng.integers(4))])
        else:
            del s[at]
    return bytes(s)


S = Synth(target_kmers=a.kmers, k=a.k, seed=0)
keys, counts = S.dump_arrays()
p = T.default_params(k=a.k)
tab = T.Table.from_arrays(keys, counts, p, device=0)
tab.decolour_repeats()
tab.upload(0)
bases, offs = S.reads(0, a.reads)
plain = bytes(bases)
parts = []
for r in range(a.reads):
    s = SSP_HEAD.encode() + edited(instance(), int(rng.integers(0, 3))) + plain[int(offs[r]):int(offs[r + 1])] + b"A" * int(rng.integers(15, 40)) + revcomp(VNP.encode())
    parts.append(revcomp(s) if r % 2 else s)
dressed = np.frombuffer(b"".join(parts), np.uint8)
lens = np.array([len(x) for x in parts], np.int64)
doffs = np.zeros(len(parts) + 1, np.uint64)
doffs[1:] = np.cumsum(lens)
ctx = T.Context(tab, p, 0)
ctx.set_umi(ANCHORED, a.pct, a.window)
ctx.set_ends(adapters=[SSP_HEAD + ANCHORED[:12], VNP], poly_min=12)
scans, ends = [], []
for rep in range(a.reps + 1):                      # (the first is the warm-up: code objects, the context's buffers)
    b = ctx.batch(dressed, doffs)
    rows = b.umi()
    scans.append(ctx.umi_timing())
    b.ends()
    ends.append(ctx.ends_timing()[0])
    b.close()
positions = int(np.minimum(lens, a.window).sum()) * 2
end_positions = int(np.minimum(lens, 512).sum()) * 2 * 2
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps, "pct": a.pct, "window": a.window,
       "raw_bases": int(doffs[-1]), "pattern_positions": positions, "scan_ms": [round(float(v), 4) for v in scans[1:]],
       "scan_ms_median": round(float(np.median(scans[1:])), 4), "scan_ms_min": round(float(min(scans[1:])), 4), "scan_ms_max": round(float(max(scans[1:])), 4),
       "pattern_positions_per_s": round(positions / (float(np.median(scans[1:])) * 1e-3), 0),
       "end_counts": np.bincount(rows["end"], minlength=3).tolist(), "both_ends_accepted": int((rows["other_err"] != 255).sum()),
       "err_counts": np.bincount(rows["err"][rows["end"] > 0], minlength=5).tolist(),
       "ends_scan_ms": [round(float(v), 4) for v in ends[1:]], "ends_scan_ms_median": round(float(np.median(ends[1:])), 4),
       "ends_position_adapters": end_positions, "ends_position_adapters_per_s": round(end_positions / (float(np.median(ends[1:])) * 1e-3), 0)}
print(json.dumps(res), flush=True)
ctx.close()
tab.close()
