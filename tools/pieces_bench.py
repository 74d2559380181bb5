#!/usr/bin/env python3
"""What trimmed and split output costs (docs/trim_split.md): BASELINE config 2 (100 k reads, 50 M-entry k = 21 dump)
corrected once with the map on, then talc_batch_pieces in both modes on the resident batch; prints the device time of
k_piece_count and k_piece_pack beside emit_ms (k_pack) and k_pack_map of the same batch, the bytes kept as a share of the
record bytes, and the wall time of fetching the pieces against fetching the records, as one JSON line.
    python tools/pieces_bench.py [--reps R] [--reads N] [--kmers N] [--k K] [--min-len L]"""
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
ap.add_argument("--min-len", type=int, default=0)
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
pack_map_ms = ctx.map_timing()[0]
L = T.lib()
record_bytes = b.corrected_bytes
rec = np.empty(max(record_bytes, 1), dtype=np.uint8)
res = {"lib": os.path.basename(T.lib_path()), "reads": a.reads, "kmers": a.kmers, "k": a.k, "reps": a.reps, "min_len": a.min_len,
       "emit_ms": round(t.emit_ms, 4), "k_pack_map_ms": round(pack_map_ms, 4), "segments": b.n_segments, "record_bytes": record_bytes}
fetch_rec = []
for rep in range(a.reps + 1):
    t0 = time.perf_counter()
    b.fetch_corrected(rec)
    fetch_rec.append(1e3 * (time.perf_counter() - t0))
res["fetch_corrected_wall_ms"] = [round(x, 3) for x in fetch_rec[1:]]
res["fetch_corrected_wall_ms_median"] = round(float(np.median(fetch_rec[1:])), 3)
for mode, name in ((T.PIECES_TRIM, "trim"), (T.PIECES_SPLIT, "split")):
    count_ms, pack_ms, fetch_ms = [], [], []
    for rep in range(a.reps + 1):             # (the first repetition allocates the buffers)
        if L.talc_batch_pieces(ctx._h, b._h, mode, a.min_len, 0) != 0:
            raise SystemExit(L.talc_last_error().decode())
        cm, pm = ctx.pieces_timing()
        n, nb = int(L.talc_batch_num_pieces(b._h)), int(L.talc_batch_pieces_bytes(b._h))
        out = np.empty(max(nb, 1), dtype=np.uint8)
        po = np.empty(n + 1, dtype=np.uint64)
        pc = np.empty(max(n, 1), dtype=T.PIECE_DTYPE)
        rpo = np.empty(a.reads + 1, dtype=np.uint64)
        t0 = time.perf_counter()
        if L.talc_batch_fetch_pieces(ctx._h, b._h, out.ctypes.data, nb, po.ctypes.data, pc.ctypes.data, n, rpo.ctypes.data) != 0:
            raise SystemExit(L.talc_last_error().decode())
        fm = 1e3 * (time.perf_counter() - t0)
        if rep:
            count_ms.append(cm); pack_ms.append(pm); fetch_ms.append(fm)
    res[name] = {"pieces": n, "bytes": nb, "kept_share": round(nb / max(record_bytes, 1), 4),
                 "reads_with_a_piece": int((np.diff(rpo.astype(np.int64)) > 0).sum()),
                 "k_piece_count_ms": [round(x, 4) for x in count_ms], "k_piece_pack_ms": [round(x, 4) for x in pack_ms],
                 "k_piece_count_ms_median": round(float(np.median(count_ms)), 4), "k_piece_pack_ms_median": round(float(np.median(pack_ms)), 4),
                 "fetch_pieces_wall_ms": [round(x, 3) for x in fetch_ms], "fetch_pieces_wall_ms_median": round(float(np.median(fetch_ms)), 3),
                 "shortest_piece": int(pc["out_len"][:n].min()) if n else 0}
print(json.dumps(res), flush=True)
b.close(); ctx.close(); tab.close()
