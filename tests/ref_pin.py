"""Shared helpers of the reference pin (docs/reference_pin.md): the reference's own binaries built into oracle/_ref/
(`talc_zero`, `talc_gxx`), the oracle's driver (`oracle/_build/talc_ref`), the inputs both read, and how a parameter set
becomes the reference's command line.  tests/test_reference_pin.py, tests/test_gpu_reference_pin.py and
tests/golden/make_ref_golden.py use it; the GPU test uses only the parts that need neither binary nor reference tree."""
import os
import random
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from talc_amd import build as B  # noqa: E402

REF_SRC = os.path.join(B.REFERENCE_SRC, "src")
TALC_ZERO = os.path.join(B.REF_OUT, "talc_zero")
TALC_GXX = os.path.join(B.REF_OUT, "talc_gxx")
TALC_REF = os.path.join(ROOT, "oracle", "_build", "talc_ref")
REF_GOLDEN = os.path.join(ROOT, "tests", "golden", "ref")

D = "ACGT"
COMP = str.maketrans("ACGTN", "TGCAN")

# what the reference's command line can set (main.cpp:105-195), by the name the parameter has in this project
OPTION_OF = {
    "min_count": "--MIN_COUNT", "max_nb_competing_paths": "--MAX_NB_BRANCHES", "window_size": "--WINDOW_SIZE",
    "alpha": "--ALPHA_FOR_PRED", "sr_error_rate": "--SR_ERROR_RATE", "min_inner_score": "--MIN_INNER_SCORE",
    "min_border_score": "--MIN_BORDER_SCORE",
}


def dna5(s):
    return "".join(ch if ch in "ACGT" else "N" for ch in s.upper())


def revcomp(s):
    return dna5(s).translate(COMP)[::-1]


def unpack(km, k):
    return "".join(D[(int(km) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def write_dump(path, keys, counts, k):
    """The text dump both drivers read (Jellyfish.cpp:249-269): `kmer count` per line, in array order."""
    with open(path, "w") as f:
        f.write("".join("%s %d\n" % (unpack(keys[i], k), int(counts[i])) for i in range(len(keys))))


def write_fasta(path, ids, reads):
    with open(path, "w") as f:
        for i, s in zip(ids, reads):
            f.write(">%s\n%s\n" % (i, s) if s else ">%s\n" % i)


def pack(reads):
    rb = "".join(reads).encode()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in reads])
    return (np.frombuffer(rb, dtype=np.uint8) if rb else np.zeros(0, np.uint8)), offs


def reference_args(k, params, junctions=False):
    """The reference's argument list for a parameter set, with the file names every run of the pin uses (relative to
    the directory it runs in, so that <o>.config.txt does not depend on where that is)."""
    args = ["reads.fa", "-k", str(k), "-SR", "sr.dump"]
    if junctions:
        args += ["-j", "junc.dump"]
    for name, v in params.items():
        if name == "reverse":
            if v:
                args.append("-rev")
        elif name in ("k", "use_junctions"):
            continue
        else:
            args += [OPTION_OF[name], repr(v) if isinstance(v, float) else str(v)]   # KeyError: the reference cannot set it
    return args


def run(exe, args, cwd, prefix, threads=1, timeout=300):
    """One run of a driver; stdout is dropped (DEBUG_READ / DEBUG_TEST print every coverage vector)."""
    r = subprocess.run([exe] + list(args) + ["-o", prefix, "-t", str(threads)], cwd=cwd, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, timeout=timeout)
    return r.returncode


def outputs(cwd, prefix):
    out = {}
    for ext in (".fa", ".log", ".config.txt", ".stats_basics.txt"):
        p = os.path.join(str(cwd), prefix + ext)
        out[ext] = open(p, "rb").read() if os.path.exists(p) else None
    return out


def fa_records(text):
    """[(id, sequence)] of a FASTA text."""
    recs = []
    for line in text.splitlines():
        if line.startswith(">"):
            recs.append([line[1:], []])
        elif recs:
            recs[-1][1].append(line)
    return [(i, "".join(s)) for i, s in recs]


NO_SOLID = "No solid kmer could be found."
NO_STRUCTURE = "Unable to define convenient structure."


def statuses(ids, reads, k, log_text):
    """The per-read status (tests/oracle_lib.py STATUS_NAMES) that the reference's log implies: a read of at most K
    bases is skipped (main.cpp:262), a read named in the log has that line's outcome, every other read is corrected."""
    said = {}
    for line in (log_text or "").splitlines():
        name, _, msg = line[len("[Read: "):].partition(" ]: ")
        said[name] = {NO_SOLID: 2, NO_STRUCTURE: 3}[msg]
    return [1 if len(s) <= k else said.get(i, 0) for i, s in zip(ids, reads)]


# ---------------------------------------------------------------- tandem repeats (cycles in the graph)
def noisy(rnd, seq, rate):
    out = []
    for ch in seq:
        x = rnd.random()
        if x < rate * 0.4:
            out.append(rnd.choice("ACGT"))          # substitution
        elif x < rate * 0.7:
            continue                                # deletion
        elif x < rate:
            out.append(ch)
            out.append(rnd.choice("ACGT"))          # insertion
        else:
            out.append(ch)
    return "".join(out)


def tandem_case(seed=1234, k=21, n_transcripts=60, reads_per=4, depth=20):
    """The generator of test_correction_across_tandem_repeats_and_cycles (tests/test_gpu_parity.py): transcripts with
    tandem repeats of a unit longer than K (2-6 copies, some diverged), every k-mer occurrence counted `depth` times,
    and reads with 8-14 % errors across them.  Returns (keys u64, counts u32, reads)."""
    rnd = random.Random(seed)
    transcripts = []
    for t in range(n_transcripts):
        parts = ["".join(rnd.choice("ACGT") for _ in range(rnd.randint(150, 400)))]
        for _ in range(rnd.randint(1, 3)):
            unit = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(k + 2, 3 * k)))
            for c in range(rnd.randint(2, 6)):
                u = unit
                if rnd.random() < 0.3:   # a copy with one substitution
                    i = rnd.randrange(len(u))
                    u = u[:i] + rnd.choice("ACGT".replace(u[i], "")) + u[i + 1:]
                parts.append(u)
            parts.append("".join(rnd.choice("ACGT") for _ in range(rnd.randint(100, 350))))
        transcripts.append("".join(parts))
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    cnt = {}
    mask = (1 << (2 * k)) - 1
    for t in transcripts:
        v = 0
        for i, ch in enumerate(t):
            v = ((v << 2) | code[ch]) & mask
            if i >= k - 1:
                cnt[v] = cnt.get(v, 0) + depth
    keys = np.fromiter(cnt.keys(), dtype=np.uint64, count=len(cnt))
    counts = np.fromiter(cnt.values(), dtype=np.uint32, count=len(cnt))
    reads = []
    for t in transcripts:
        for _ in range(reads_per):
            a = rnd.randint(0, 60)
            b = len(t) - rnd.randint(0, 60)
            reads.append(noisy(rnd, t[a:b], rnd.choice([0.08, 0.11, 0.14])))
    return keys, counts, reads
