#!/usr/bin/env python3
"""What the edit scripts cost (docs/correction_edits.md): BASELINE config 2 (100 k reads, 50 M-entry k = 21 dump)
corrected once with the map on, then talc_batch_edits on the resident batch; prints the device time of the alignment
(align_ms: both runs of k_edit_align) and of k_edit_count + k_edit_pack (pack_ms) beside search_ms and emit_ms of the same
batch, the DP cells and cells per second, the segments aligned and not aligned, and the ops and bytes fetched against
fetch_corrected's, as one JSON line.
    python tools/edits_bench.py [--reps R] [--reads N] [--kmers N] [--k K] [--max-cells C]"""
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
ap.add_argument("--max-cells", type=int, default=0)
a = ap.parse_args()

S = Synth(target_kmers=a.kmers, k=a.k, seed=0)
keys, counts = S.dump_arrays()
p = T.default_params(k=a.k)
tab = T.Table.from_arrays(keys, counts, p, device=0)
tab.decolour_repeats()
tab.upload(0)
ctx = T.Context(tab, p, 0)
ctx.record_map(True)
bases, offs = S.reads(0, a.reads)
b = ctx.batch(bases, offs)
b.correct()                                   # warm-up
b.correct()
t = ctx.timing()
record_bytes = b.corrected_bytes
rec = np.empty(max(record_bytes, 1), dtype=np.uint8)
segs, so = b.fetch_map()
c = segs[segs["kind"] == T.SEG_CORRECTED]
cells = c["raw_len"].astype(np.int64) * c["out_len"]
cap = a.max_cells or (1 << 26)
dp = (cells > 0) & (cells <= cap)
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps, "max_cells": cap,
       "search_ms": round(t.search_ms, 4), "emit_ms": round(t.emit_ms, 4), "segments": int(len(segs)), "corrected_segments": int(len(c)),
       "segments_aligned": int(dp.sum()), "segments_unaligned": int((cells > cap).sum()), "dp_cells": int(cells[dp].sum()),
       "largest_pair": [int(x) for x in c[int(np.argmax(cells))][["raw_len", "out_len"]].tolist()] if len(c) else None, "record_bytes": record_bytes}
fetch_rec = []
for rep in range(a.reps + 1):
    t0 = time.perf_counter()
    b.fetch_corrected(rec)
    fetch_rec.append(1e3 * (time.perf_counter() - t0))
res["fetch_corrected_wall_ms_median"] = round(float(np.median(fetch_rec[1:])), 3)
L = T.lib()
align_ms, pack_ms, call_ms, fetch_ms = [], [], [], []
for rep in range(a.reps + 1):                 # (the first repetition allocates the buffers)
    t0 = time.perf_counter()
    if L.talc_batch_edits(ctx._h, b._h, a.max_cells) != 0:
        raise SystemExit(L.talc_last_error().decode())
    cm = 1e3 * (time.perf_counter() - t0)
    am, pm = ctx.edits_timing()
    n = int(L.talc_batch_num_edit_ops(b._h))
    ops = np.empty(max(n, 1), dtype=np.uint32)
    oo = np.empty(a.reads + 1, dtype=np.uint64)
    rows = np.zeros(a.reads, dtype=T.EDIT_ROW_DTYPE)
    t0 = time.perf_counter()
    if L.talc_batch_fetch_edits(ctx._h, b._h, ops.ctypes.data, n, oo.ctypes.data, rows.ctypes.data) != 0:
        raise SystemExit(L.talc_last_error().decode())
    fm = 1e3 * (time.perf_counter() - t0)
    if rep:
        align_ms.append(am); pack_ms.append(pm); call_ms.append(cm); fetch_ms.append(fm)
am = float(np.median(align_ms))
res.update({"align_ms": [round(x, 4) for x in align_ms], "pack_ms": [round(x, 4) for x in pack_ms], "align_ms_median": round(am, 4),
            "pack_ms_median": round(float(np.median(pack_ms)), 4), "edits_call_wall_ms_median": round(float(np.median(call_ms)), 3),
            "dp_cells_per_s": round(2 * res["dp_cells"] / (am * 1e-3), 1) if am > 0 else None,   # (every pair is aligned twice: count, write)
            "ops": n, "op_bytes": 4 * n, "op_bytes_share_of_records": round(4 * n / max(record_bytes, 1), 4),
            "fetch_edits_wall_ms_median": round(float(np.median(fetch_ms)), 3),
            "sums": {f: int(rows[f].sum()) for f in T.EDIT_ROW_FIELDS}})
print(json.dumps(res), flush=True)
b.close(); ctx.close(); tab.close()
