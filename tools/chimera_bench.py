#!/usr/bin/env python3
"""What the chimera scan costs and what a split is worth (docs/chimeras.md): BASELINE config 2 (100 k reads, 50 M-entry
k = 21 dump) on one GPU, the reads dressed on the host: every `--every`-th read is joined to the next through
A x 30 . revcomp(VN primer) . strand-switch primer, each primer with 0 to 2 edits.  `--reps` fresh batches after a warm-up
are made plain (the scan alone, then the correction) and split; prints one JSON line with the device time of k_read_chimera
and k_gather, the scan's bases x patterns per second, the hits and the pieces, and search_ms of the split batch
against the unsplit one.
    python tools/chimera_bench.py [--reps R] [--reads N] [--kmers N] [--k K] [--every E] [--pct P] [--min-piece M]"""
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
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--pct", type=int, default=10)
ap.add_argument("--min-piece", type=int, default=100)
a = ap.parse_args()

rng = np.random.default_rng(0)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


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
parts, joints, r = [], 0, 0
while r < a.reads:
    rd = plain[int(offs[r]):int(offs[r + 1])]
    if r % a.every == 0 and r + 1 < a.reads:
        rd += b"A" * 30 + edited(VNP, int(rng.integers(0, 3))).translate(COMP)[::-1] + edited(SSP, int(rng.integers(0, 3))) + plain[int(offs[r + 1]):int(offs[r + 2])]
        joints += 1
        r += 1
    parts.append(rd)
    r += 1
dressed = np.frombuffer(b"".join(parts), np.uint8)
doffs = np.zeros(len(parts) + 1, np.uint64)
doffs[1:] = np.cumsum([len(x) for x in parts])
n_patterns = 4

KERNELS = ("encode_ms", "coverage_ms", "structure_ms", "search_ms", "retry_ms", "emit_ms")
res = {"lib": os.path.basename(T.lib_path()), "reads": len(parts), "joints": joints, "kmers": a.kmers, "k": a.k, "reps": a.reps, "pct": a.pct,
       "min_piece": a.min_piece, "raw_bases": int(doffs[-1]), "patterns": n_patterns}
ctx = T.Context(tab, p, 0)
ctx.record_map(True)
ctx.set_ends(adapters=[SSP, VNP])
ctx.set_chimera(True, a.pct, a.min_piece)
for name, split in (("unsplit", False), ("split", True)):
    rows, scans, gathers = [], [], []
    for rep in range(a.reps + 1):              # (the first is the warm-up: code objects, the context's buffers)
        b = ctx.batch(dressed, doffs, split=split)
        hits, _ = b.chimera()
        scan, gather = ctx.chimera_timing()
        b.correct()
        t = ctx.timing()
        st = b.fetch_corrected()[2]
        segs, _ = b.fetch_map()
        if split:
            pieces, _ = b.split_pieces()
        b.close()
        scans.append(scan)
        gathers.append(gather)
        rows.append([getattr(t, f) for f in KERNELS])
    med = np.median(np.array(rows[1:]), axis=0)
    res[name] = {"batch_reads": int(len(st)), "corrected": int((st == T.READ_CORRECTED).sum()), "batch_bases": int(t.n_bases),
                 "raw_segment_bases": int(segs["out_len"][segs["kind"] == T.SEG_RAW].astype(np.int64).sum()),
                 "scan_ms": [round(float(v), 4) for v in scans[1:]], **{f + "_median": round(float(v), 4) for f, v in zip(KERNELS, med)}}
    if split:
        res[name]["gather_ms"] = [round(float(v), 4) for v in gathers[1:]]
        res["pieces"] = int(len(pieces))
        res["cut_reads"] = int(len(np.unique(pieces["read"][pieces["ordinal"] > 0])))
    res["hits"] = int(len(hits))
    res["reads_with_hits"] = int(len(np.unique(hits["read"])))
allscans = res["unsplit"]["scan_ms"] + res["split"]["scan_ms"]
res["scan_ms_median"] = round(float(np.median(allscans)), 4)
res["scan_ms_spread"] = [min(allscans), max(allscans)]
res["gather_ms_median"] = round(float(np.median(res["split"]["gather_ms"])), 4)
res["scan_base_patterns_per_s"] = round(int(doffs[-1]) * n_patterns / (res["scan_ms_median"] * 1e-3), 0)
res["search_ms"] = {"unsplit": res["unsplit"]["search_ms_median"], "split": res["split"]["search_ms_median"]}
print(json.dumps(res), flush=True)
ctx.close()
tab.close()
