#!/usr/bin/env python3
"""Records the reference-made fixtures tests/golden/ref/*.json.gz: what the reference's OWN program text writes,
compiled unmodified into oracle/_ref/talc_zero (oracle/Makefile target `ref`, docs/reference_pin.md).  The oracle is
not consulted.  tests/test_gpu_reference_pin.py holds the HIP path to these files; tests/test_reference_pin.py
re-records them and compares, and holds the oracle to them.

Each fixture is data only: the input recipe (generator parameters and the sha256 of the dump and junction arrays they
must reproduce), the reads as text with their ids, the reference's argument list, and the four files it wrote
(<o>.fa, <o>.log, <o>.stats_basics.txt, <o>.config.txt) as text.  The cases mirror make_golden.py's g1-g5 and g7-g10
(same seeds, same reads; g6 is K = 31, which the reference's command line refuses; g10 runs with MAX_NB_BRANCHES 5,
the smallest value it accepts, and window_size 7), and add a set of many near-identical paralogs with
MAX_NB_BRANCHES 10, a tandem-repeat set, and a second edge set (g13) that reaches the third outcome.

"Unable to define convenient structure." cannot happen under default parameters: it needs analyzeINRegions to merge
a region into the next one and then drop every region as LOWCOUNT (Read.cpp:586-601, 257), so every IN k-mer of the read
must lie within the noise interval of floor(SR_ERROR_RATE * robust mean) — at most 2.32 for ALPHA 2.57 — while
reCoverage wants one count above MIN_COUNT = 2 (Read.cpp:190).  g8 mirrors the oracle's edge fixture under defaults and
shows two outcomes; g13 is the same table and reads under --ALPHA_FOR_PRED 8 (the option has no upper bound) with eight
hand k-mers of count 3 and one hand read over them added, built so that exactly that merge-and-drop happens.

The recorder refuses a fixture set that could be reproduced without correcting anything (check_set).

usage: python tests/golden/make_ref_golden.py [outdir]     (default: tests/golden/ref)
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_pin as RP  # noqa: E402
from talc_amd.synth import Synth  # noqa: E402

CASES = {
    "g1_default_k21": dict(k=21, kmers=20_000, seed=101, reads=16),
    "g2_junctions_k21": dict(k=21, kmers=60_000, seed=102, reads=24, junctions=True),
    "g3_reverse_k21": dict(k=21, kmers=60_000, seed=103, reads=24, params=dict(reverse=1)),
    "g4_k18": dict(k=18, kmers=60_000, seed=104, reads=20),
    "g5_k30": dict(k=30, kmers=60_000, seed=105, reads=20),
    "g7_params": dict(k=21, kmers=60_000, seed=107, reads=20,
                      params=dict(min_count=3, window_size=6, max_nb_competing_paths=5, alpha=1.96,
                                  sr_error_rate=0.05, min_inner_score=0.5, min_border_score=0.6)),
    "g8_edge_inputs": dict(k=21, kmers=60_000, seed=108, reads=12, edge=True),
    "g9_paralogs_k21": dict(k=21, kmers=80_000, seed=109, reads=24, synth=dict(paralog_frac=0.5, paralog_div=0.03)),
    "g10_paralogs_junctions_maxb5": dict(k=21, kmers=80_000, seed=110, reads=20, junctions=True,
                                         synth=dict(paralog_frac=0.6, paralog_div=0.015),
                                         params=dict(max_nb_competing_paths=5, window_size=7)),
    "g11_paralogs_maxb10": dict(k=21, kmers=80_000, seed=301, reads=24, synth=dict(paralog_frac=0.9, paralog_div=0.015),
                                params=dict(max_nb_competing_paths=10)),
    "g12_tandem_repeats": dict(k=21, tandem=dict(seed=1234, n_transcripts=60, reads_per=4), reads=24),
    "g13_edge_no_structure": dict(k=21, kmers=60_000, seed=108, reads=12, edge=True, no_structure=True, params=dict(alpha=8.0)),
}


def no_structure_read(k, seed=108, a=5):
    """(hand k-mers, hand read): k-mers 0..a of a random sequence are one IN region whose last k-mer has a successor in
    the table that the read does not follow, and the k-mer at a+K-2 alone is the next: they lie closer than K, the second
    is shorter than the overlap, so the first is merged into it (Read.cpp:590-594) and the list keeps both."""
    import random
    rnd = random.Random(seed)
    p = a + k - 2
    x = "".join(rnd.choice("ACGT") for _ in range(p + k + 10))
    succ = x[a + 1:a + k] + [b for b in "ACGT" if b != x[a + k]][0]
    return [x[i:i + k] for i in range(a + 1)] + [succ, x[p:p + k]], x


def pack_kmer(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def case_inputs(c):
    """(synth recipe, keys, counts, junction arrays or None, reads as text) — the same reads make_golden.py takes."""
    k = c["k"]
    if "tandem" in c:
        keys, counts, reads = RP.tandem_case(k=k, **c["tandem"])
        step = len(reads) // c["reads"]
        return dict(tandem=dict(c["tandem"], k=k)), keys, counts, None, reads[::step][:c["reads"]]
    recipe = dict({"target_kmers": c["kmers"], "k": k, "seed": c["seed"]}, **c.get("synth", {}))
    S = Synth(**recipe)
    keys, counts = S.dump_arrays()
    junc = S.junction_arrays() if c.get("junctions") else None
    bases, offs = S.reads(0, c["reads"])
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]).decode() for i in range(c["reads"])]
    if c.get("params", {}).get("reverse"):
        # the table is forward-strand only (k-mers are directional, main.cpp:89): reads from the opposite strand, so
        # that -rev brings them back onto the table's strand
        reads = [RP.revcomp(x) for x in reads]
    if c.get("edge"):
        r = reads
        reads = [
            "",                                   # empty read
            r[0][:k],                             # exactly K bases: skipped (main.cpp:262)
            r[0][:k + 1],                         # K+1: two k-mers
            r[1].lower(),                         # lower case accepted by Dna5
            r[2][:400] + "N" + r[2][400:],        # one N
            r[3][:300] + "NNNNNNNNNN" + r[3][300:900] + "RYKM" + r[3][900:],   # IUPAC -> N
            "ACGT" * 300,                         # low-complexity, probably no solid k-mer
            "A" * 500,                            # homopolymer
        ] + r[4:8]
    if c.get("no_structure"):
        import numpy as np
        extra, x = no_structure_read(k)
        reads = reads + [x]
        keys = np.concatenate([keys, np.array([pack_kmer(e) for e in extra], dtype=np.uint64)])
        counts = np.concatenate([counts, np.full(len(extra), 3, dtype=np.uint32)])
        return dict(synth=recipe, extra_kmers=[[e, 3] for e in extra]), keys, counts, junc, reads
    return dict(synth=recipe), keys, counts, junc, reads


def fixture_inputs(fx):
    """(keys, counts, junction keys, junction counts, bases, offsets) of a recorded fixture, from its recipe alone;
    the generators must still make the arrays the reference was given."""
    import numpy as np
    if "tandem" in fx:
        keys, counts, _ = RP.tandem_case(**fx["tandem"])
        jk = jc = None
    else:
        S = Synth(**fx["synth"])
        keys, counts = S.dump_arrays()
        jk, jc = S.junction_arrays() if fx["params"]["use_junctions"] else (None, None)
        if "extra_kmers" in fx:
            keys = np.concatenate([keys, np.array([pack_kmer(e) for e, _ in fx["extra_kmers"]], dtype=np.uint64)])
            counts = np.concatenate([counts, np.array([n for _, n in fx["extra_kmers"]], dtype=np.uint32)])
    assert hashlib.sha256(keys.tobytes() + counts.tobytes()).hexdigest() == fx["dump_sha256"], "generator drifted"
    if jk is not None:
        assert hashlib.sha256(jk.tobytes() + jc.tobytes()).hexdigest() == fx["junction_sha256"], "generator drifted"
    bases, offs = RP.pack(fx["reads"])
    return keys, counts, jk, jc, bases, offs


def record(name, c, exe=None):
    k = c["k"]
    recipe, keys, counts, junc, reads = case_inputs(c)
    ids = ["%s_r%d" % (name.split("_")[0], i) for i in range(len(reads))]
    args = RP.reference_args(k, c.get("params", {}), junctions=junc is not None)
    with tempfile.TemporaryDirectory() as d:
        RP.write_dump(os.path.join(d, "sr.dump"), keys, counts, k)
        if junc is not None:
            RP.write_dump(os.path.join(d, "junc.dump"), junc[0], junc[1], k)
        RP.write_fasta(os.path.join(d, "reads.fa"), ids, reads)
        rc = RP.run(exe or RP.TALC_ZERO, args, d, "out", timeout=300)
        assert rc == 0, (name, rc)
        out = RP.outputs(d, "out")
    fx = dict(recipe, name=name, k=k, params=dict(c.get("params", {}), k=k, use_junctions=int(junc is not None)),
              dump_sha256=hashlib.sha256(keys.tobytes() + counts.tobytes()).hexdigest(),
              junction_sha256=hashlib.sha256(junc[0].tobytes() + junc[1].tobytes()).hexdigest() if junc is not None else None,
              ids=ids, reads=reads, args=args, edge=bool(c.get("edge")),
              fa=out[".fa"].decode(), log=(out[".log"] or b"").decode(), stats=out[".stats_basics.txt"].decode(),
              config=out[".config.txt"].decode())
    return fx


def changed(fx):
    """Indices of the reads longer than K that came out different from their input (as Dna5 text)."""
    recs = RP.fa_records(fx["fa"])
    return [i for i, s in enumerate(fx["reads"]) if len(s) > fx["k"] and recs[i][1] != RP.dna5(s)]


def part_corrected_with_n(fx):
    """Reads with a corrected stretch, an uncorrected stretch and an N: the record differs from the input, and an N of
    the input is still in it — no k-mer over an N is in the table and a path holds only ACGT, so the stretch around a
    surviving N is a weak one that was left as it was."""
    recs = RP.fa_records(fx["fa"])
    return [i for i in changed(fx) if "N" in recs[i][1]]


def check_set(fixtures):
    """The conditions on the set as the reference recorded it; an identity 'correction' must not be able to pass."""
    for fx in fixtures:
        recs = RP.fa_records(fx["fa"])
        assert [i for i, _ in recs] == fx["ids"], fx["name"]
        longer = [i for i, s in enumerate(fx["reads"]) if len(s) > fx["k"]]
        if not fx["edge"]:
            assert 4 * len(changed(fx)) >= 3 * len(longer), (fx["name"], len(changed(fx)), len(longer))
        else:
            st = RP.statuses(fx["ids"], fx["reads"], fx["k"], fx["log"])
            assert changed(fx) and 2 in st and (3 in st or "extra_kmers" not in fx), (fx["name"], st)
    assert any(fx["edge"] and "extra_kmers" in fx for fx in fixtures)      # an edge case with all three outcomes
    assert any(part_corrected_with_n(fx) for fx in fixtures)


def write(fx, outdir):
    os.makedirs(outdir, exist_ok=True)
    with gzip.GzipFile(os.path.join(outdir, fx["name"] + ".json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(fx, sort_keys=True).encode())


def record_all(outdir, exe=None):
    fixtures = [record(n, c, exe) for n, c in CASES.items()]
    check_set(fixtures)
    for fx in fixtures:
        write(fx, outdir)
    return fixtures


if __name__ == "__main__":
    for fx in record_all(sys.argv[1] if len(sys.argv) > 1 else RP.REF_GOLDEN):
        longer = [s for s in fx["reads"] if len(s) > fx["k"]]
        print(fx["name"], "reads", len(fx["reads"]), "changed %d of %d" % (len(changed(fx)), len(longer)),
              "log lines", len(fx["log"].splitlines()), "with N", part_corrected_with_n(fx))
