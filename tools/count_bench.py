"""Throughput of the GPU k-mer counter (talc_counter_*, docs/kmer_counting.md); prints one JSON line.

Two legs:
  memory  synthetic short reads (Synth.short_reads) of config 2's transcriptome handed to KmerCounter in batches: windows
          counted per second over the whole counting (adds + the final wait) and over the count kernels alone (device
          events, from the library's TALC_TIMING report), the atomics that implies, distinct and kept k-mers;
  file    the whole program on config 2's long reads: `talc --SRReads sr.fq` against `talc -SR <dump of the same counts>`
          (the dump is a separate run's --SRCountsOut), wall time of each and the corrected records compared.
  stage   the counting stage of `talc --SRReads` (the "[talc] short reads:" line of TALC_TIMING=1) on one FASTQ file whose
          reads carry adapters and low qualities (--adapter-frac, --min-qual): filter on against filter off, and, with
          --other-talc PATH, filter off against another build's program on the same file; medians of --runs runs each.
With --adapter-frac F, F of the reads are cut to a random insert length and continued with ADAPTER up to their length; with
--min-qual Q the reads get qualities, low at 1 % of the positions, and the counter a floor of Q (docs/sr_filter.md).  The
memory leg then runs the filter and reports the mask kernels' summed device time beside the count kernels'.
Kernel times of a separate `rocprofv3 --kernel-trace --stats -- python tools/count_bench.py --leg memory ...` run are the
figures to quote for the kernels themselves.

  python tools/count_bench.py [--reads 40000000] [--file-reads 4000000] [--long-reads 20000] [--leg all|memory|file]
                              [--both-strands] [--adapter-frac F] [--min-qual Q] [--other-talc PATH] [--runs 5]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"   # 33 letters


def dirty(bases, n, length, adapter_frac, seed):
    """The reads with adapters (a fixed-seed numpy pass: adapter_frac of them cut to a random insert length, ADAPTER behind
    it, truncated at the read length) and a quality per base, low at 1 % of the positions."""
    import numpy as np
    rng = np.random.default_rng(seed)
    rows = np.asarray(bases, dtype=np.uint8).reshape(n, length).copy()
    cut = rng.random(n) < adapter_frac
    insert = rng.integers(20, length, size=n)
    tail = np.frombuffer((ADAPTER * (length // len(ADAPTER) + 1)).encode(), dtype=np.uint8)
    col = np.arange(length)
    behind = cut[:, None] & (col[None, :] >= insert[:, None])
    rows[behind] = tail[(col[None, :] - insert[:, None]) % len(tail)][behind]
    quals = np.where(rng.random((n, length)) < 0.01, 33 + 5, 33 + 37).astype(np.uint8)
    return rows.reshape(-1), quals.reshape(-1)


def filtered(a):
    return a.adapter_frac > 0 or a.min_qual > 0


def memory_leg(a):
    from talc_amd import lib as T
    from talc_amd.synth import Synth
    S = Synth(target_kmers=a.target_kmers, k=a.k, seed=a.seed)
    p = T.default_params(k=a.k)
    c = T.KmerCounter(p, 0, both_strands=a.both_strands)
    if filtered(a):
        c.set_filter(a.min_qual, [ADAPTER] if a.adapter_frac > 0 else [])
    add_s, nbytes = 0.0, 0
    for first in range(0, a.reads, a.batch):
        n = min(a.batch, a.reads - first)
        b, o = S.short_reads(first, n, length=a.length, sub_rate=a.sub_rate)
        q = None
        if filtered(a):
            b, q = dirty(b, n, a.length, a.adapter_frac, a.seed + first)
            if not a.min_qual:
                q = None
        t0 = time.perf_counter()
        c.add(b, o, q)
        add_s += time.perf_counter() - t0
        nbytes += len(b)
    t0 = time.perf_counter()
    windows, distinct, kept = c.stats()
    wait_s = time.perf_counter() - t0
    fstats = c.filter_stats()
    t0 = time.perf_counter()
    t = c.build_table()
    build_s = time.perf_counter() - t0
    c.close()
    out = {"both_strands": a.both_strands, "reads": a.reads, "bytes": nbytes, "windows": windows, "distinct": distinct, "kept": kept, "table_size": len(t),
           "add_s": round(add_s, 4), "final_wait_s": round(wait_s, 4), "table_build_s": round(build_s, 4),
           "windows_per_s_whole": windows / max(add_s + wait_s, 1e-9)}
    if filtered(a):
        out.update(adapter_frac=a.adapter_frac, min_qual=a.min_qual, filter_stats=fstats)
    t.close()
    print("MEMORY_LEG " + json.dumps(out), flush=True)


def run_memory_child(a):
    env = dict(os.environ, TALC_TIMING="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "memory-child", "--reads", str(a.reads), "--batch", str(a.batch),
           "--target-kmers", str(a.target_kmers), "--k", str(a.k), "--length", str(a.length), "--sub-rate", str(a.sub_rate),
           "--seed", str(a.seed), "--adapter-frac", str(a.adapter_frac), "--min-qual", str(a.min_qual)] + (["--both-strands"] if a.both_strands else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=1800)
    if r.returncode != 0:
        raise SystemExit("memory leg failed (%d): %s" % (r.returncode, r.stderr.decode()[-2000:]))
    res = json.loads(r.stdout.decode().split("MEMORY_LEG ", 1)[1].splitlines()[0])
    m = re.search(r"count kernels ([0-9.]+) ms \(([0-9.]+) ms per batch\), (\d+) grows ([0-9.]+) s, "
                  r"last batch wait [0-9.]+ s, compaction ([0-9.]+) s", r.stderr.decode())
    if m:
        kms = float(m.group(1))
        res.update(kernel_ms=kms, kernel_ms_per_batch=float(m.group(2)), grows=int(m.group(3)), grow_s=float(m.group(4)),
                   compaction_s=float(m.group(5)),
                   windows_per_s_kernel=res["windows"] / (kms / 1e3) if kms > 0 else None,
                   # one add per window at most (runs of one k-mer in a lane share one) plus one CAS per distinct k-mer
                   atomics_per_s_kernel_upper=(res["windows"] + res["distinct"]) / (kms / 1e3) if kms > 0 else None)
    m = re.search(r"mask kernels ([0-9.]+) ms \(([0-9.]+) ms per batch\)", r.stderr.decode())
    if m:
        res.update(mask_kernel_ms=float(m.group(1)), mask_kernel_ms_per_batch=float(m.group(2)))
    return res


def write_dirty_fastq(S, path, a):
    """a.file_reads reads as FASTQ records of one fixed width (numpy builds them a batch at a time)."""
    import numpy as np
    L = a.length
    with open(path, "wb") as f:
        for first in range(0, a.file_reads, 500_000):
            n = min(500_000, a.file_reads - first)
            b, _ = S.short_reads(first, n, length=L, sub_rate=a.sub_rate)
            b, q = dirty(b, n, L, a.adapter_frac, a.seed + first)
            ids = np.frombuffer(b"".join(b"@r%010d\n" % i for i in range(first, first + n)), dtype=np.uint8).reshape(n, 13)
            rec = np.empty((n, 13 + L + 3 + L + 1), dtype=np.uint8)
            rec[:, :13] = ids
            rec[:, 13:13 + L] = b.reshape(n, L)
            rec[:, 13 + L:16 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, 16 + L:16 + 2 * L] = q.reshape(n, L)
            rec[:, 16 + 2 * L] = 10
            f.write(rec.tobytes())


def stage_leg(a, d):
    """The counting stage's seconds (TALC_TIMING=1) over a.runs runs: this build with the filter off and on, and another
    build's program (--other-talc) with the filter off, all on one file."""
    import statistics
    from talc_amd import build as B
    from talc_amd.synth import Synth
    S = Synth(target_kmers=a.target_kmers, k=a.k, seed=a.seed)
    fq, fa = os.path.join(d, "dirty.fq"), os.path.join(d, "reads.fa")
    write_dirty_fastq(S, fq, a)
    S.write_fasta(fa, 0, a.long_reads)
    env = dict(os.environ, TALC_TIMING="1")
    on = (["--SRAdapter", ADAPTER] if a.adapter_frac > 0 else []) + (["--SRMinQual", str(a.min_qual)] if a.min_qual else [])
    legs = [("this_off", os.path.join(B.OUT, "talc"), []), ("this_on", os.path.join(B.OUT, "talc"), on)]
    if a.other_talc:
        legs.insert(1, ("other_off", a.other_talc, []))
    times = {name: [] for name, _, _ in legs}
    notes = {}
    for run in range(a.runs):          # (interleaved: drift of the machine lands on every leg alike)
        for name, exe, extra in legs:
            r = subprocess.run([exe, fa, "-k", str(a.k), "--SRReads", fq] + extra + ["-o", os.path.join(d, name)], stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, env=env, timeout=1800)
            if r.returncode != 0:
                raise SystemExit("talc %s failed (%d): %s" % (name, r.returncode, r.stderr.decode()[-2000:]))
            err = r.stderr.decode()
            times[name].append(float(re.search(r"counting stage ([0-9.]+) s", err).group(1)))
            notes[name] = [m.group(0) for m in (re.search(r"\[talc\] short reads: .*", err), re.search(r"\[talc-lib\] k-mer counter: .*", err),
                                                re.search(r"\[TALC\]: short-read filter: .*", r.stdout.decode())) if m]
    res = {"file_reads": a.file_reads, "fastq_bytes": os.path.getsize(fq), "runs": a.runs, "adapter_frac": a.adapter_frac, "min_qual": a.min_qual}
    for name, ts in times.items():
        res[name] = {"counting_stage_s": ts, "median": statistics.median(ts), "min": min(ts), "max": max(ts), "last_run": notes[name]}
    return res


def file_leg(a, d):
    from talc_amd import build as B
    from talc_amd.synth import Synth
    talc = os.path.join(B.OUT, "talc")
    S = Synth(target_kmers=a.target_kmers, k=a.k, seed=a.seed)
    fq, fa = os.path.join(d, "sr.fq"), os.path.join(d, "reads.fa")
    S.write_short_fastq(fq, 0, a.file_reads, length=a.length, sub_rate=a.sub_rate)
    S.write_fasta(fa, 0, a.long_reads)
    env = dict(os.environ, TALC_TIMING="1")
    res = {"file_reads": a.file_reads, "fastq_bytes": os.path.getsize(fq), "long_reads": a.long_reads}

    def timed(args, name):
        t0 = time.perf_counter()
        r = subprocess.run([talc, fa, "-k", str(a.k)] + args + ["-o", os.path.join(d, name)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, timeout=1800)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit("talc %s failed (%d): %s" % (name, r.returncode, r.stderr.decode()[-2000:]))
        return wall, r.stderr.decode()

    res["srreads_wall_s"], err = timed(["--SRReads", fq], "counted")
    m = re.search(r"\[talc\] short reads: .*", err)
    res["srreads_timing"] = m.group(0) if m else None
    m = re.search(r"\[talc-lib\] k-mer counter: .*", err)
    res["counter_timing"] = m.group(0) if m else None
    res["srcountsout_wall_s"], _ = timed(["--SRReads", fq, "--SRCountsOut", os.path.join(d, "sr.dump")], "written")
    res["dump_bytes"] = os.path.getsize(os.path.join(d, "sr.dump"))
    res["dump_wall_s"], err = timed(["-SR", os.path.join(d, "sr.dump")], "dumped")
    m = re.search(r"\[talc\] scan=.*", err)
    res["dump_split"] = m.group(0) if m else None
    with open(os.path.join(d, "counted.fa"), "rb") as f1, open(os.path.join(d, "dumped.fa"), "rb") as f2:
        res["same_corrected_records"] = f1.read() == f2.read()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", default="all", choices=["all", "memory", "file", "stage", "memory-child"])
    ap.add_argument("--target-kmers", type=int, default=50_000_000)   # config 2's transcriptome
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reads", type=int, default=40_000_000)
    ap.add_argument("--batch", type=int, default=2_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.005)
    ap.add_argument("--file-reads", type=int, default=4_000_000)
    ap.add_argument("--long-reads", type=int, default=20_000)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--both-strands", action="store_true",
                    help="the memory leg with the canonical kernel and the expanding compaction (docs/both_strands.md)")
    ap.add_argument("--adapter-frac", type=float, default=0.0, help="share of the reads that end in the adapter (docs/sr_filter.md)")
    ap.add_argument("--min-qual", type=int, default=0, help="quality floor; the reads then carry qualities, low at 1 %% of the positions")
    ap.add_argument("--other-talc", default=None, help="the stage leg: another build's talc program to run beside this one, filter off")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.leg == "memory-child":
        memory_leg(a)
        return
    out = {"metric": "kmer_count", "k": a.k, "target_kmers": a.target_kmers}
    if a.leg in ("all", "memory"):
        out["memory"] = run_memory_child(a)
    if a.leg in ("all", "file"):
        with tempfile.TemporaryDirectory(dir=a.workdir) as d:
            out["file"] = file_leg(a, d)
    if a.leg == "stage":
        with tempfile.TemporaryDirectory(dir=a.workdir) as d:
            out["stage"] = stage_leg(a, d)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
