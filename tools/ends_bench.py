#!/usr/bin/env python3
"""What the long-read end clean-up costs and what it is worth (docs/read_ends.md): BASELINE config 2 (100 k reads, 50 M-entry
k = 21 dump) on one GPU, the reads dressed on the host: a fraction `--frac` of them (each class drawn on its own) gets a head
primer (the strand-switch primer with 0 to 4 edits behind 0 to 30 bases of junk), a poly-T head of 12 to 120 bases, a tail
primer (the reverse complement of the VN primer with 0 to 3 edits, junk behind it), a poly-A tail.  `--reps` fresh batches
after a warm-up are made plain and clipped; prints one JSON line with the device time of k_read_ends and k_gather
beside coverage_ms, vote_ms and search_ms of the same batch, the scan's window positions per second, and the reads corrected
and RAW bases with and without clipping.
    python tools/ends_bench.py [--reps R] [--reads N] [--kmers N] [--k K] [--frac F] [--window W]"""
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
ap.add_argument("--frac", type=float, default=0.5)
ap.add_argument("--window", type=int, default=512)
a = ap.parse_args()

rng = np.random.default_rng(0)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def letters(n):
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n).tolist())


def edited(seq, n):
    s = bytearray(seq.encode())
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
parts, lens, classes = [], [], np.zeros(4, np.int64)
for r in range(a.reads):
    hp, ht, tp, ta = (rng.random(4) < a.frac).tolist()
    classes += (hp, ht, tp, ta)
    head = (letters(int(rng.integers(0, 31))) + edited(SSP, int(rng.integers(0, 5))) if hp else b"") + (b"T" * int(rng.integers(12, 121)) if ht else b"")
    tail = (b"A" * int(rng.integers(12, 121)) if ta else b"") + (edited(VNP, int(rng.integers(0, 4))).translate(COMP)[::-1] + letters(int(rng.integers(0, 31))) if tp else b"")
    rd = head + plain[int(offs[r]):int(offs[r + 1])] + tail
    parts.append(rd)
    lens.append(len(rd))
dressed = np.frombuffer(b"".join(parts), np.uint8)
doffs = np.zeros(a.reads + 1, np.uint64)
doffs[1:] = np.cumsum(lens)
positions = 2 * int(np.minimum(np.array(lens), a.window).sum())

KERNELS = ("encode_ms", "coverage_ms", "structure_ms", "search_ms", "retry_ms", "emit_ms")
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps, "frac": a.frac, "window": a.window,
       "dressed": dict(zip(("head_primer", "head_poly", "tail_primer", "tail_poly"), classes.tolist())), "raw_bases": int(doffs[-1]),
       "scan_window_positions": positions}
ctx = T.Context(tab, p, 0)
ctx.record_map(True)
ctx.set_ends(adapters=[SSP, VNP], max_error_pct=20, poly_min=12, window=a.window)
for name, clip in (("unclipped", False), ("clipped", True)):
    rows, scans, gathers, votes = [], [], [], []
    for rep in range(a.reps + 1):              # (the first is the warm-up: code objects, the context's buffers)
        b = ctx.batch(dressed, doffs, clip=clip)
        ends = b.ends()
        scan, gather = ctx.ends_timing()
        b.correct()
        t = ctx.timing()
        st = b.fetch_corrected()[2]
        segs, _ = b.fetch_map()
        b.strand()
        votes.append(ctx.strand_timing())
        b.close()
        scans.append(scan)
        gathers.append(gather)
        rows.append([getattr(t, f) for f in KERNELS])
    med = np.median(np.array(rows[1:]), axis=0)
    res[name] = {"corrected": int((st == T.READ_CORRECTED).sum()), "no_solid_kmer": int((st == T.READ_NO_SOLID_KMER).sum()),
                 "no_structure": int((st == T.READ_NO_STRUCTURE).sum()), "batch_bases": int(t.n_bases),
                 "raw_segment_bases": int(segs["out_len"][segs["kind"] == T.SEG_RAW].astype(np.int64).sum()),
                 "scan_ms": [round(float(v), 4) for v in scans[1:]], "vote_ms": [round(float(v), 4) for v in votes[1:]],
                 **{f + "_median": round(float(v), 4) for f, v in zip(KERNELS, med)}}
    if clip:
        res[name]["gather_ms"] = [round(float(v), 4) for v in gathers[1:]]
        res["found"] = {f: int((ends[f] > 0).sum()) for f in ("head_adapter", "head_poly_len", "tail_adapter", "tail_poly_len")}
        res["bases_clipped"] = int(doffs[-1]) - int(ends["kept_len"].astype(np.int64).sum())
        res["oriented"] = {"plus": int((ends["orient"] > 0).sum()), "minus": int((ends["orient"] < 0).sum())}
allscans = res["unclipped"]["scan_ms"] + res["clipped"]["scan_ms"]
res["scan_ms_median"] = round(float(np.median(allscans)), 4)
res["scan_ms_spread"] = [min(allscans), max(allscans)]
res["gather_ms_median"] = round(float(np.median(res["clipped"]["gather_ms"])), 4)
res["scan_positions_per_s"] = round(positions / (res["scan_ms_median"] * 1e-3), 0)
res["coverage_ms"] = res["unclipped"]["coverage_ms_median"]
res["search_ms"] = res["unclipped"]["search_ms_median"]
res["vote_ms"] = round(float(np.median(res["unclipped"]["vote_ms"])), 4)
print(json.dumps(res), flush=True)
ctx.close()
tab.close()
