"""Throughput of the GPU k-mer counter (talc_counter_*, docs/kmer_counting.md); prints one JSON line.

Two legs:
  memory  synthetic short reads (Synth.short_reads) of config 2's transcriptome handed to KmerCounter in batches: windows
          counted per second over the whole counting (adds + the final wait) and over the count kernels alone (device
          events, from the library's TALC_TIMING report), the atomics that implies, distinct and kept k-mers;
  file    the whole program on config 2's long reads: `talc --SRReads sr.fq` against `talc -SR <dump of the same counts>`
          (the dump is a separate run's --SRCountsOut), wall time of each and the corrected records compared.
Kernel times of a separate `rocprofv3 --kernel-trace --stats -- python tools/count_bench.py --leg memory ...` run are the
figures to quote for the kernels themselves.

  python tools/count_bench.py [--reads 40000000] [--file-reads 4000000] [--long-reads 20000] [--leg all|memory|file]
                              [--both-strands]
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


def memory_leg(a):
    from talc_amd import lib as T
    from talc_amd.synth import Synth
    S = Synth(target_kmers=a.target_kmers, k=a.k, seed=a.seed)
    p = T.default_params(k=a.k)
    c = T.KmerCounter(p, 0, both_strands=a.both_strands)
    add_s, nbytes = 0.0, 0
    for first in range(0, a.reads, a.batch):
        n = min(a.batch, a.reads - first)
        b, o = S.short_reads(first, n, length=a.length, sub_rate=a.sub_rate)
        t0 = time.perf_counter()
        c.add(b, o)
        add_s += time.perf_counter() - t0
        nbytes += len(b)
    t0 = time.perf_counter()
    windows, distinct, kept = c.stats()
    wait_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    t = c.build_table()
    build_s = time.perf_counter() - t0
    c.close()
    out = {"both_strands": a.both_strands, "reads": a.reads, "bytes": nbytes, "windows": windows, "distinct": distinct, "kept": kept, "table_size": len(t),
           "add_s": round(add_s, 4), "final_wait_s": round(wait_s, 4), "table_build_s": round(build_s, 4),
           "windows_per_s_whole": windows / max(add_s + wait_s, 1e-9)}
    t.close()
    print("MEMORY_LEG " + json.dumps(out), flush=True)


def run_memory_child(a):
    env = dict(os.environ, TALC_TIMING="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "memory-child", "--reads", str(a.reads), "--batch", str(a.batch),
           "--target-kmers", str(a.target_kmers), "--k", str(a.k), "--length", str(a.length), "--sub-rate", str(a.sub_rate),
           "--seed", str(a.seed)] + (["--both-strands"] if a.both_strands else [])
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
    ap.add_argument("--leg", default="all", choices=["all", "memory", "file", "memory-child"])
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
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
