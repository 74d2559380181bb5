#!/usr/bin/env python3
"""What the solidity report costs: BASELINE config 2 (100 k reads, 50 M-entry k = 21 dump) on one GPU, one resident batch,
corrected and then reported `--reps` times in one process; prints the device time of k_solidity over the reads (raw rows)
and over the records (corrected rows) beside coverage_ms and the kernels of the whole talc_batch_correct of the same batch,
the probes per second and the algorithmic bytes per second (one 32-byte bucket per probed position), and the report's sums.
    python tools/solidity_bench.py [--reps R] [--reads N] [--kmers N] [--k K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from talc_amd import lib as T  # noqa: E402
from talc_amd.synth import Synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kmers", type=int, default=50_000_000)
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--k", type=int, default=21)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

S = Synth(target_kmers=a.kmers, k=a.k, seed=0)
keys, counts = S.dump_arrays()
p = T.default_params(k=a.k)
tab = T.Table.from_arrays(keys, counts, p, device=0)
tab.decolour_repeats()
tab.upload(0)
ctx = T.Context(tab, p, 0)
bases, offs = S.reads(0, a.reads)
b = ctx.batch(bases, offs)
b.correct()                                   # warm-up: both kernels' code objects, the batch's buffers
b.solidity()
rows = []
for rep in range(a.reps):
    b.correct()
    t = ctx.timing()
    t0 = time.perf_counter()
    raw, cor = b.solidity()
    wall = 1e3 * (time.perf_counter() - t0)
    raw_ms, cor_ms = ctx.solidity_timing()
    rows.append((raw_ms, cor_ms, t.coverage_ms, t.encode_ms + t.coverage_ms + t.structure_ms + t.search_ms + t.retry_ms + t.emit_ms, wall))
r = np.array(rows)
med = [float(np.median(r[:, i])) for i in range(5)]
probes = {"raw": int(raw["n_kmers"].sum()), "corrected": int(cor["n_kmers"].sum())}
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps,
       "table_device_bytes": tab.device_bytes, "raw_bases": int(offs[-1]), "record_bases": b.corrected_bytes, "probes": probes,
       "k_solidity_raw_ms": [round(float(x), 4) for x in r[:, 0]], "k_solidity_corrected_ms": [round(float(x), 4) for x in r[:, 1]],
       "k_solidity_raw_ms_median": round(med[0], 4), "k_solidity_corrected_ms_median": round(med[1], 4),
       "coverage_ms_median": round(med[2], 4), "correct_kernels_ms_median": round(med[3], 3), "solidity_call_wall_ms_median": round(med[4], 3)}
for i, key in enumerate(("raw", "corrected")):
    res[key + "_probes_per_s"] = round(probes[key] / (med[i] * 1e-3), 0)
    res[key + "_algorithmic_TB_per_s"] = round(32.0 * probes[key] / (med[i] * 1e-3) / 1e12, 4)
    rw = raw if key == "raw" else cor
    res[key + "_sums"] = {f: int(rw[f].astype(np.int64).sum()) for f in T.SOLIDITY_FIELDS if f != "longest_weak"}
    res[key + "_longest_weak_max"] = int(rw["longest_weak"].max())
print(json.dumps(res), flush=True)
b.close(); ctx.close(); tab.close()
