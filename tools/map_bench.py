#!/usr/bin/env python3
"""What the correction map costs: BASELINE config 2 (100 k reads, 50 M-entry k = 21 dump) corrected in one process with
the map off and on, alternating; prints the kernel times of both (search_ms, the whole step), the device time of
k_pack_map and k_mask_case, the map's size, and whether the records of the two are the same.
    python tools/map_bench.py [--reps R] [--reads N] [--kmers N] [--k K]"""
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
b.correct()                                   # warm-up
rows = {False: [], True: []}
pack_ms, mask_ms, fetch_ms = [], [], []
records = {}
for rep in range(a.reps):
    for on in (False, True):
        ctx.record_map(on)
        t0 = time.perf_counter()
        b.correct()
        wall = 1e3 * (time.perf_counter() - t0)
        t = ctx.timing()
        rows[on].append((t.search_ms, t.encode_ms + t.coverage_ms + t.structure_ms + t.search_ms + t.retry_ms + t.emit_ms, wall))
        if on:
            t0 = time.perf_counter()
            segs, so = b.fetch_map()
            fetch_ms.append(1e3 * (time.perf_counter() - t0))
            masked, _, _ = b.fetch_corrected(soft_mask=True)
            pk, mk = ctx.map_timing()
            pack_ms.append(pk)
            mask_ms.append(mk)
        if rep == 0:
            out, oo, st = b.fetch_corrected()
            records[on] = (out.copy(), oo.copy(), st.copy(), t.n_trail_steps, t.n_dp_cells)
same = all(np.array_equal(x, y) for x, y in zip(records[False][:3], records[True][:3])) and records[False][3:] == records[True][3:]
kinds = np.bincount(segs["kind"], minlength=3)
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps,
       "records_and_counters_equal": bool(same), "segments": int(len(segs)), "segments_S_C_R": kinds.tolist(),
       "map_bytes": int(segs.nbytes), "masked_is_upper_equal": bool(np.array_equal(masked & 0xDF, records[True][0] & 0xDF)),
       "raw_bases_lower_case": int((masked >= 97).sum()), "record_bases": int(len(masked))}
for on in (False, True):
    r = np.array(rows[on])
    key = "map_on" if on else "map_off"
    res[key] = {"search_ms": [round(float(x), 3) for x in r[:, 0]], "search_ms_median": round(float(np.median(r[:, 0])), 3),
                "kernels_ms_median": round(float(np.median(r[:, 1])), 3), "step_wall_ms_median": round(float(np.median(r[:, 2])), 3)}
res["k_pack_map_ms"] = [round(x, 4) for x in pack_ms]
res["k_mask_case_ms"] = [round(x, 4) for x in mask_ms]
res["fetch_map_wall_ms_median"] = round(float(np.median(fetch_ms)), 3)
print(json.dumps(res), flush=True)
b.close(); ctx.close(); tab.close()
