"""The GPU k-mer counter (talc_counter_*, KmerCounter, `talc --SRReads`) against the numpy reference of the counting
contract (tests/kmer_ref.py) and against the dump route it replaces (docs/kmer_counting.md)."""
import os
import subprocess
import threading

import numpy as np
import pytest

import kmer_ref as R
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALC = os.path.join(B.OUT, "talc")
TALC_REF = os.path.join(ROOT, "oracle", "_build", "talc_ref")
N_SHORT = 200_000


def sorted_pairs(kmers, counts):
    o = np.argsort(kmers, kind="stable")
    return kmers[o], counts[o]


def counted(params, chunks, expected_distinct=0):
    c = T.KmerCounter(params, 0, expected_distinct)
    for b, o in chunks:
        c.add(b, o)
    st = c.stats()
    k1, c1 = sorted_pairs(*c.fetch(1))
    return c, st, k1, c1


def slices(bases, offsets, cuts):
    """the records split into batches at the given record numbers (offsets rebased to each batch's bytes)"""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(offsets[a]), int(offsets[b])
        out.append((bases[lo:hi], offsets[a:b + 1] - offsets[a]))
    return out


@pytest.fixture(scope="module")
def synth():
    return Synth(target_kmers=150_000, k=21, seed=77)


@pytest.fixture(scope="module")
def short(synth):
    bases, offs = synth.short_reads(0, N_SHORT, length=150, sub_rate=0.005, n_rate=0.001)
    kmers, counts = R.count(bases, offs, 21)
    return bases, offs, kmers, counts


@pytest.mark.parametrize("k", [18, 21, 25, 31])
def test_fetch_equals_reference_on_hand_cases(k):
    recs = R.hand_records()
    bases, offs = R.records_to_arrays(recs)
    want_k, want_c = R.count(bases, offs, k)
    c, st, got_k, got_c = counted(T.default_params(k=k), [(bases, offs)])
    assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c)
    assert st == (int(want_c.sum()), len(want_k), int((want_c >= 2).sum()))
    k2, c2 = sorted_pairs(*c.fetch(2))
    assert np.array_equal(k2, want_k[want_c >= 2]) and np.array_equal(c2, want_c[want_c >= 2])
    c.close()


def test_batches_and_growth_give_the_same_counts(synth):
    bases, offs = synth.short_reads(N_SHORT, 30_000, length=150, sub_rate=0.01, n_rate=0.002)
    p = T.default_params(k=21)
    n = len(offs) - 1
    one = counted(p, [(bases, offs)])
    cuts = [0, 1, 2, 1000, 1001, 9000, 22000, n]
    seven = counted(p, slices(bases, offs, cuts))
    grown = counted(p, slices(bases, offs, cuts), expected_distinct=1)    # starts at 64 K slots: grows several times
    want_k, want_c = R.count(bases, offs, 21)
    assert one[1][1] > 4 * 65536 * 0.7     # (so the last run really grew)
    for c, st, k1, c1 in (one, seven, grown):
        assert st == one[1]
        assert np.array_equal(k1, want_k) and np.array_equal(c1, want_c)
        c.close()


def test_synthetic_short_reads_equal_reference(short):
    bases, offs, want_k, want_c = short
    c, st, k1, c1 = counted(T.default_params(k=21), slices(bases, offs, [0, 70_000, N_SHORT]))
    assert np.array_equal(k1, want_k) and np.array_equal(c1, want_c)
    k2, c2 = sorted_pairs(*c.fetch(2))
    keep = want_c >= 2
    assert np.array_equal(k2, want_k[keep]) and np.array_equal(c2, want_c[keep])
    assert st == (int(want_c.sum()), len(want_k), int(keep.sum()))
    c.close()


@pytest.fixture(scope="module")
def tables(short, synth, tmp_path_factory):
    bases, offs, want_k, want_c = short
    d = tmp_path_factory.mktemp("kc")
    R.write_dump(str(d / "ref.dump"), want_k, want_c, 21)
    synth.write_junctions(str(d / "junc.dump"))
    p = T.default_params(k=21)
    c = T.KmerCounter(p, 0)
    c.add(bases, offs)
    mine = c.build_table()
    c.close()
    ref = T.Table.from_arrays(want_k, want_c, p, device=0)
    return d, p, mine, ref


def test_table_from_counter_equals_table_from_reference_counts(short, tables):
    bases, offs, want_k, want_c = short
    d, p, mine, ref = tables
    assert len(mine) == len(ref) == int((want_c >= 2).sum())
    assert list(mine.build_stats) == [len(want_k), len(ref), 0]
    mine.upload(0)
    ref.upload(0)
    rng = np.random.default_rng(3)
    absent = rng.integers(0, 1 << 42, size=100_000, dtype=np.uint64)
    q = np.concatenate([want_k, absent])
    a, b = mine.lookup(q), ref.lookup(q)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    sample = rng.choice(want_k, size=20_000)
    for direction in (0, 1):
        a, b = mine.next_counts(sample, direction), ref.next_counts(sample, direction)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_table_from_counter_with_junctions_equals_dump_route(short, tables):
    bases, offs, want_k, want_c = short
    d, p, _, _ = tables
    c = T.KmerCounter(p, 0)
    c.add(bases, offs)
    mine = c.build_table(junctions=str(d / "junc.dump"))
    c.close()
    ref = T.Table.from_files(str(d / "ref.dump"), str(d / "junc.dump"), p, device=0)
    assert len(mine) == len(ref)
    assert mine.build_stats[1] == ref.build_stats[1] and mine.build_stats[2] == ref.build_stats[2]
    mine.upload(0)
    ref.upload(0)
    jk, _ = Synth(target_kmers=150_000, k=21, seed=77).junction_arrays()
    q = np.concatenate([want_k, jk])
    a, b = mine.lookup(q), ref.lookup(q)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[1] > 0).any()


def test_correction_identical_with_counter_table(synth, tables):
    d, p, mine, ref = tables
    mine.upload(0)
    ref.upload(0)
    bases, offs = synth.reads(0, 300)
    outs = []
    for t in (mine, ref):
        ctx = T.Context(t, p, 0)
        recs, oo, st = ctx.correct(bases, offs)
        outs.append((recs.tobytes(), oo.tolist(), st.tolist()))
        ctx.close()
    assert outs[0] == outs[1]
    assert outs[0][2].count(T.READ_CORRECTED) > 100


# ------------------------------------------------------------------ the CLI
def run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def files(prefix):
    out = {}
    for ext in (".fa", ".log", ".config.txt", ".stats_basics.txt"):
        p = prefix + ext
        out[ext] = open(p, "rb").read() if os.path.exists(p) else None
    return out


@pytest.fixture(scope="module")
def clidata(synth, tables):
    d, p, _, _ = tables
    synth.write_fasta(str(d / "reads.fa"), 0, 60)
    synth.write_short_fastq(str(d / "a.fq"), 0, 100_000, length=150, sub_rate=0.005, n_rate=0.001)
    b, o = synth.short_reads(100_000, N_SHORT - 100_000, length=150, sub_rate=0.005, n_rate=0.001)
    with open(d / "b.fa", "wb") as f:   # FASTA wrapped at 60 columns
        for i in range(len(o) - 1):
            s = bytes(b[int(o[i]):int(o[i + 1])])
            f.write(b">s%d\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n")
    return d


@pytest.mark.parametrize("junctions", [False, True], ids=["plain", "junctions"])
def test_cli_srreads_files_identical_to_reference_driver_on_the_dump(clidata, tmp_path, junctions):
    d = clidata
    extra = ["-j", str(d / "junc.dump")] if junctions else []
    a = run(TALC, [str(d / "reads.fa"), "-k", "21", "--SRReads", str(d / "a.fq"), "--SRReads", str(d / "b.fa"), "-o", "gpu"] + extra, tmp_path)
    b = run(TALC_REF, [str(d / "reads.fa"), "-k", "21", "-SR", str(d / "ref.dump"), "-o", "ref", "-t", "8"] + extra, tmp_path)
    assert a.returncode == 0, a.stderr.decode()
    assert b.returncode == 0, b.stderr.decode()
    fa, fb = files(str(tmp_path / "gpu")), files(str(tmp_path / "ref"))
    assert fa[".fa"] == fb[".fa"] and fa[".log"] == fb[".log"]
    assert fa[".config.txt"].replace(b"gpu", b"ref") == fb[".config.txt"]
    assert fa[".stats_basics.txt"] == fb[".stats_basics.txt"]
    assert b"k-mers retrieved from database" in a.stdout and fa[".fa"].count(b">") == 60


def test_cli_counts_out_and_fifo(clidata, short, tmp_path):
    d = clidata
    _, _, want_k, want_c = short
    a = run(TALC, [str(d / "reads.fa"), "-k", "21", "--SRReads", str(d / "a.fq"), "--SRReads", str(d / "b.fa"),
                   "--SRCountsOut", "counts.dump", "-o", "gpu"], tmp_path)
    assert a.returncode == 0, a.stderr.decode()
    R.write_dump(str(tmp_path / "want.dump"), want_k[want_c >= 2], want_c[want_c >= 2], 21)
    got = (tmp_path / "counts.dump").read_bytes().splitlines()
    assert len(got) == len(set(got)) and set(got) == set((tmp_path / "want.dump").read_bytes().splitlines())
    b = run(TALC, [str(d / "reads.fa"), "-k", "21", "-SR", "counts.dump", "-o", "again"], tmp_path)
    assert b.returncode == 0, b.stderr.decode()
    assert files(str(tmp_path / "again"))[".fa"] == files(str(tmp_path / "gpu"))[".fa"]
    # a pipe: the same records through a FIFO give the same corrected reads
    fifo = str(tmp_path / "sr.pipe")
    os.mkfifo(fifo)
    both = (d / "a.fq").read_bytes(), (d / "b.fa").read_bytes()
    fifo2 = str(tmp_path / "sr2.pipe")
    os.mkfifo(fifo2)

    def feed(path, data):
        with open(path, "wb") as f:
            f.write(data)
    th = [threading.Thread(target=feed, args=(fifo, both[0]), daemon=True), threading.Thread(target=feed, args=(fifo2, both[1]), daemon=True)]
    for t in th:
        t.start()
    c = run(TALC, [str(d / "reads.fa"), "-k", "21", "--SRReads", fifo, "--SRReads", fifo2, "-o", "pipe"], tmp_path)
    for t in th:
        t.join(timeout=60)
    assert c.returncode == 0, c.stderr.decode()
    assert files(str(tmp_path / "pipe"))[".fa"] == files(str(tmp_path / "gpu"))[".fa"]


def test_cli_srreads_below_min_count_is_the_empty_graph(clidata, tmp_path):
    rng = np.random.default_rng(9)
    (tmp_path / "once.fa").write_text(">x\n" + "".join(rng.choice(list("ACGT"), size=300)) + "\n")
    r = run(TALC, [str(clidata / "reads.fa"), "-k", "21", "--SRReads", "once.fa"], tmp_path)
    assert r.returncode == 1 and b"The de Bruijn Graph is empty" in r.stdout, (r.stdout, r.stderr)


def test_cli_malformed_fastq_short_reads_is_an_error(clidata, tmp_path):
    (tmp_path / "bad.fq").write_text("@a\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\nACGT\n+\nIIII\n")
    r = run(TALC, [str(clidata / "reads.fa"), "-k", "21", "--SRReads", "bad.fq"], tmp_path)
    assert r.returncode == 2 and b"bad.fq" in r.stderr and b"record 2" in r.stderr, r.stderr
