#!/usr/bin/env python3
"""What the per-base support costs: BASELINE config 2 (100 k reads, 50 M-entry k = 21 dump) on one GPU, one resident batch.
After a warm-up, `--reps` fresh batches are corrected and given qualities (RECORD source, Phred form); prints one JSON
line with the medians of the device time of k_base_support, of k_solidity over the same records (the same probes, nothing
written per position: the difference is the price of the sliding count and the store), of coverage_ms and search_ms of
the same batch's correction, the bases per second and the bytes written.
    python tools/support_bench.py [--reps R] [--reads N] [--kmers N] [--k K]"""
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
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

S = Synth(target_kmers=a.kmers, k=a.k, seed=0)
keys, counts = S.dump_arrays()
p = T.default_params(k=a.k)
tab = T.Table.from_arrays(keys, counts, p, device=0)
tab.decolour_repeats()
tab.upload(0)
ctx = T.Context(tab, p, 0)
bases, offs = S.reads(0, a.reads)


def one():
    """A fresh batch: corrected, its records' qualities and their cover, its solidity rows."""
    b = ctx.batch(bases, offs)
    try:
        b.correct()
        t = ctx.timing()
        t0 = time.perf_counter()
        q, oo = b.support("record", (2, 40))
        wall = 1e3 * (time.perf_counter() - t0)
        sup = ctx.support_timing()
        cov, _ = b.support("record")
        cover_ms = ctx.support_timing()
        b.support("raw", (2, 40))
        raw_ms = ctx.support_timing()
        raw, cor = b.solidity()
        sol_raw, sol_cor = ctx.solidity_timing()
        return dict(support_ms=sup, support_cover_ms=cover_ms, support_raw_ms=raw_ms, k_solidity_corrected_ms=sol_cor, k_solidity_raw_ms=sol_raw,
                    coverage_ms=t.coverage_ms, search_ms=t.search_ms, support_call_wall_ms=wall), q, cov, cor
    finally:
        b.close()


one()                                         # warm-up: the kernels' code objects, the context's buffer cache
rows = []
for rep in range(a.reps):
    row, q, cov, cor = one()
    rows.append(row)
med = {k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]}
n_bytes = int(len(q))
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps, "table_device_bytes": tab.device_bytes,
       "raw_bases": int(offs[-1]), "bytes_written": n_bytes}
res.update(med)
res["support_ms_all"] = [round(r["support_ms"], 4) for r in rows]
res["k_solidity_corrected_ms_all"] = [round(r["k_solidity_corrected_ms"], 4) for r in rows]
res["support_minus_k_solidity_ms"] = round(med["support_ms"] - med["k_solidity_corrected_ms"], 4)
res["support_over_k_solidity"] = round(med["support_ms"] / med["k_solidity_corrected_ms"], 3) if med["k_solidity_corrected_ms"] else None
res["support_share_of_search"] = round(med["support_ms"] / med["search_ms"], 5) if med["search_ms"] else None
res["bases_per_s"] = round(n_bytes / (med["support_ms"] * 1e-3), 0) if med["support_ms"] else None
# the two identities, over the whole batch, and the quality histogram's ends
res["cover_sum"] = int(cov.astype(np.int64).sum())
res["k_times_n_solid"] = int(a.k * cor["n_solid"].astype(np.int64).sum())
res["covered_bases"] = int((cov > 0).sum())
res["solid_bases"] = int(cor["solid_bases"].astype(np.int64).sum())
res["bases_at_qmax"] = int((q == 33 + 40).sum())
res["bases_at_qmin"] = int((q == 33 + 2).sum())
print(json.dumps(res), flush=True)
ctx.close(); tab.close()
