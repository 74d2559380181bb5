#!/usr/bin/env python3
"""What barcode demultiplexing costs (docs/demux.md): BASELINE config 2 (100 k reads, 50 M-entry k = 21 dump) on one GPU, every
read dressed on the host: barcode (0 to 2 edits), junk of 0 to 10 bases, VN primer, poly-T in front, the mirror image with
the strand-switch primer behind.  For 24 and for 96 barcodes, `--reps` fresh plain batches after a warm-up: the device time of
k_read_demux and its pattern positions per second (2 x B x window positions per read), the classification counts, and
search_ms of the correction beside them.  The same job runs k_read_ends over the same reads as the yardstick.  Prints one
JSON line.
    python tools/demux_bench.py [--reps R] [--reads N] [--kmers N] [--k K] [--pct P] [--margin M] [--window W]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from talc_amd import lib as T  # noqa: E402
from talc_amd.synth import Synth  # noqa: E402

SSP, VNP = "TTTCTGTTGGTGCTGATATTGCTGGG", "ACTTGCCTGTCGCTCTATCTTC"

ap = argparse.ArgumentParser()
ap.add_argument("--kmers", type=int, default=50_000_000)
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--k", type=int, default=21)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--pct", type=int, default=T.DEMUX_DEFAULT_ERR)
ap.add_argument("--margin", type=int, default=T.DEMUX_DEFAULT_MARGIN)
ap.add_argument("--window", type=int, default=T.DEMUX_DEFAULT_WINDOW)
a = ap.parse_args()

rng = np.random.default_rng(0)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
revcomp = lambda s: s.translate(COMP)[::-1]
random_seq = lambda n: bytes(b"ACGT"[x] for x in rng.integers(0, 4, n).tolist())


def distance(x, y):
    prev = list(range(len(y) + 1))
    for i, cx in enumerate(x, 1):
        cur = [i]
        for j, cy in enumerate(y, 1):
            cur.append(min(prev[j - 1] + (cx != cy), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def barcode_set(count, m=24, min_dist=9):
    out = []
    while len(out) < count:
        cand = random_seq(m)
        if all(distance(cand, o) >= min_dist for o in out):
            out.append(cand)
    return out


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
barcodes = barcode_set(96)
KERNELS = ("encode_ms", "coverage_ms", "structure_ms", "search_ms", "retry_ms", "emit_ms")
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps, "pct": a.pct, "margin": a.margin,
       "window": a.window}
ctx = T.Context(tab, p, 0)
for B in (24, 96):
    parts = []
    for r in range(a.reads):
        bc = barcodes[int(rng.integers(B))]
        head = edited(bc, int(rng.integers(0, 3))) + random_seq(int(rng.integers(0, 11))) + VNP.encode() + b"T" * int(rng.integers(15, 40))
        tail = b"A" * int(rng.integers(15, 40)) + revcomp(SSP.encode()) + random_seq(int(rng.integers(0, 11))) + revcomp(edited(bc, int(rng.integers(0, 3))))
        parts.append(head + plain[int(offs[r]):int(offs[r + 1])] + tail)
    dressed = np.frombuffer(b"".join(parts), np.uint8)
    lens = np.array([len(x) for x in parts], np.int64)
    doffs = np.zeros(len(parts) + 1, np.uint64)
    doffs[1:] = np.cumsum(lens)
    positions = int(np.minimum(lens, a.window).sum()) * 2 * B
    ctx.set_demux([x.decode() for x in barcodes[:B]], a.pct, a.margin, a.window)
    ctx.set_ends(adapters=[SSP, VNP], poly_min=12)
    scans, ends, rows = [], [], []
    for rep in range(a.reps + 1):                  # (the first is the warm-up: code objects, the context's buffers)
        b = ctx.batch(dressed, doffs)
        calls = b.demux()
        scans.append(ctx.demux_timing())
        b.ends()
        ends.append(ctx.ends_timing()[0])
        b.correct()
        t = ctx.timing()
        rows.append([getattr(t, f) for f in KERNELS])
        b.close()
    ctx.set_ends()
    med = float(np.median(scans[1:]))
    end_positions = int(np.minimum(lens, 512).sum()) * 2 * 2
    res["B%d" % B] = {"raw_bases": int(doffs[-1]), "pattern_positions": positions, "scan_ms": [round(float(v), 4) for v in scans[1:]],
                      "scan_ms_median": round(med, 4), "pattern_positions_per_s": round(positions / (med * 1e-3), 0),
                      "status_counts": np.bincount(calls["status"], minlength=5).tolist(), "classified": int((calls["barcode"] > 0).sum()),
                      "ends_scan_ms": [round(float(v), 4) for v in ends[1:]], "ends_position_adapters": end_positions,
                      "ends_position_adapters_per_s": round(end_positions / (float(np.median(ends[1:])) * 1e-3), 0),
                      **{f + "_median": round(float(v), 4) for f, v in zip(KERNELS, np.median(np.array(rows[1:]), axis=0))}}
print(json.dumps(res), flush=True)
ctx.close()
tab.close()
