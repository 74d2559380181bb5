#!/usr/bin/env python3
"""What auto strand costs and what it is worth: BASELINE config 2 (100 k reads, 50 M-entry k = 21 dump) on one GPU with every
second read reverse complemented on the host.  The batch is corrected by a plain context, by a -rev context and by an
auto-strand context (`--reps` fresh batches each, so that every repetition votes); prints one JSON line with the device time
of k_strand_vote beside coverage_ms and the step's other kernel times, the vote's positions per second, and the reads each
of the three corrects.
    python tools/strand_bench.py [--reps R] [--reads N] [--kmers N] [--k K]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from talc_amd import lib as T  # noqa: E402
from talc_amd.synth import Synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kmers", type=int, default=50_000_000)
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--k", type=int, default=21)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

S = Synth(target_kmers=a.kmers, k=a.k, seed=0)
keys, counts = S.dump_arrays()
p = T.default_params(k=a.k)
tab = T.Table.from_arrays(keys, counts, p, device=0)
tab.decolour_repeats()
tab.upload(0)
bases, offs = S.reads(0, a.reads)
bases = np.array(bases, dtype=np.uint8)
comp = np.arange(256, dtype=np.uint8)
for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
    comp[x] = y
for r in range(1, a.reads, 2):                 # every second read: its reverse complement
    lo, hi = int(offs[r]), int(offs[r + 1])
    bases[lo:hi] = comp[bases[lo:hi]][::-1]

KERNELS = ("encode_ms", "coverage_ms", "structure_ms", "search_ms", "retry_ms", "emit_ms")
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps,
       "table_device_bytes": tab.device_bytes, "raw_bases": int(offs[-1])}
for name, params, auto in (("off", p, False), ("rev", T.default_params(k=a.k, reverse=1), False), ("auto", p, True)):
    ctx = T.Context(tab, params, 0)
    ctx.auto_strand(True) if auto else None
    rows, votes = [], []
    for rep in range(a.reps + 1):              # (the first is the warm-up: code objects, the context's buffers)
        b = ctx.batch(bases, offs)
        b.correct()
        t = ctx.timing()
        st = b.fetch_corrected()[2]
        if auto:
            votes.append(ctx.strand_timing())
            strand = b.strand()
        b.close()
        rows.append([getattr(t, f) for f in KERNELS])
    med = np.median(np.array(rows[1:]), axis=0)
    res[name] = {"corrected": int((st == T.READ_CORRECTED).sum()), "no_solid_kmer": int((st == T.READ_NO_SOLID_KMER).sum()),
                 "no_structure": int((st == T.READ_NO_STRUCTURE).sum()), **{f + "_median": round(float(v), 4) for f, v in zip(KERNELS, med)}}
    if auto:
        vote = float(np.median(votes[1:]))
        positions = int(strand["n_kmers"].astype(np.int64).sum())
        res["vote_ms"] = [round(float(v), 4) for v in votes[1:]]
        res["vote_ms_median"] = round(vote, 4)
        res["vote_positions"] = positions
        res["vote_positions_per_s"] = round(positions / (vote * 1e-3), 0)
        res["voted_reverse"] = int(strand["reverse"].sum())
        res["vote_sums"] = {f: int(strand[f].astype(np.int64).sum()) for f in T.STRAND_FIELDS[1:5]}
    ctx.close()
res["coverage_ms"] = res["auto"]["coverage_ms_median"]
res["search_ms"] = res["auto"]["search_ms_median"]
print(json.dumps(res), flush=True)
tab.close()
