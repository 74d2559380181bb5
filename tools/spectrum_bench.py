"""Cost of the k-mer spectrum pass (k_count_histo, docs/kmer_spectrum.md) beside the count-only compaction pass over the
same hash (k_count_compact without output arrays: what talc_counter_fetch(c, 1, NULL, NULL, 0, &n) runs, and what
talc_counter_stats runs for its third number); prints one JSON line.

The short reads are tests/test_gpu_kmer_count.py's: Synth(150_000, k=21, seed=77), 200 000 x 150 b, 0.5 % substitutions.
Both passes stream capacity x 16 bytes once.  Reported, over --runs runs after --warmup:
  histo_kernel_ms    device events around k_count_histo (talc_counter_get_histo_timing)
  histo_call_ms      host clock around talc_counter_histo: zeroing, the kernel, the copy of the bins, the synchronise
  count_call_ms      host clock around the count-only talc_counter_fetch: zeroing, k_count_compact, 8 bytes back, the synchronise
and capacity x 16 / time for each.  There is no event around k_count_compact: its device time is the figure of a separate
`rocprofv3 --kernel-trace --stats -- python tools/spectrum_bench.py ...` run, which lists both kernels by name.

The capacity.  The counter sizes its hash for the windows of a batch, an upper bound of the k-mers the batch can add, not
for the distinct k-mers it ends up with (counter_make_room and the rule itself, counter_capacity_for, in
talc_capi_counter.inc): before a batch of W windows, with D distinct k-mers known, it doubles its capacity until
D + W <= 0.7 capacity.  So the capacity depends on how the reads
were handed over.  The tool hands them over in batches of --batch reads, reads the exact D back after every batch
(stats(): the library then knows it too) and replays that rule; "capacity_slots" is the result.  --slots-log2 N sizes the
hash to 2^N slots from the start (the same k-mers in a larger hash: the streaming cost at the size of a real data set); it
still grows when a batch's bound asks for it.

  python tools/spectrum_bench.py [--reads 200000] [--batch 20000] [--high 0] [--slots-log2 0] [--runs 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--target-kmers", type=int, default=150_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.005)
    ap.add_argument("--n-rate", type=float, default=0.001)
    ap.add_argument("--batch", type=int, default=20_000, help="reads per add")
    ap.add_argument("--high", type=int, default=0)
    ap.add_argument("--slots-log2", type=int, default=0, help="size the hash to 2^N slots from the start (0: as the reads need)")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    from talc_amd import lib as T
    from talc_amd.synth import Synth
    L = T.lib()
    S = Synth(target_kmers=a.target_kmers, k=a.k, seed=a.seed)
    bases, offs = S.short_reads(0, a.reads, length=a.length, sub_rate=a.sub_rate, n_rate=a.n_rate)
    hint = int(0.7 * (1 << a.slots_log2)) if a.slots_log2 else 0
    c = T.KmerCounter(T.default_params(k=a.k), 0, hint)
    capacity = 1 << 16
    while hint > 0.7 * capacity:                         # counter_capacity_for, from talc_counter_create
        capacity *= 2
    distinct = 0
    for first in range(0, a.reads, a.batch):
        o = offs[first:min(first + a.batch, a.reads) + 1]
        lens = np.diff(o.astype(np.int64))
        bound = distinct + int(np.maximum(lens - a.k + 1, 0).sum())   # counter_make_room: D + the batch's windows
        while bound > 0.7 * capacity:                    # counter_capacity_for, from counter_grow
            capacity *= 2
        c.add(bases[int(o[0]):int(o[-1])], o - o[0])
        windows, distinct, kept = c.stats()              # (synchronises: D is exact, in the library too)

    n = C.c_uint64()
    kernel_ms, histo_ms, count_ms = [], [], []
    hist = stats = None
    for run in range(a.warmup + a.runs):                 # (alternating: drift of the machine lands on both alike)
        t0 = time.perf_counter()
        hist, stats = c.histo(a.high)
        t1 = time.perf_counter()
        T._chk(L.talc_counter_fetch(c._h, 1, None, None, 0, C.byref(n)))
        t2 = time.perf_counter()
        if run >= a.warmup:
            kernel_ms.append(c.histo_timing())
            histo_ms.append((t1 - t0) * 1e3)
            count_ms.append((t2 - t1) * 1e3)
    assert n.value == distinct == stats[0] == int(hist.sum())
    c.close()

    nbytes = capacity * 16

    def leg(ms):
        med = statistics.median(ms)
        return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "gb_per_s_at_median": round(nbytes / med / 1e6, 1)}

    print(json.dumps({"metric": "kmer_spectrum", "reads": a.reads, "windows": windows, "distinct": distinct, "batch_reads": a.batch, "capacity_slots": capacity,
                      "bytes_streamed": nbytes, "high": a.high or 10000, "runs": a.runs, "spectrum_head": [int(x) for x in hist[1:9]],
                      "stats": list(stats), "chosen_valley": list(T.spectrum_threshold(hist)),
                      "histo_kernel": leg(kernel_ms), "histo_call": leg(histo_ms), "count_only_call": leg(count_ms)}), flush=True)


if __name__ == "__main__":
    main()
