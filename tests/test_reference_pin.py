"""The CPU oracle held to the reference's own program text (docs/reference_pin.md).

oracle/_ref/talc_zero and oracle/_ref/talc_gxx are the reference's nine translation units, compiled unmodified against
oracle/seqan_compat (oracle/Makefile, target `ref`); oracle/_build/talc_ref is the oracle's restatement of the same
driver.  Everything here runs them as programs, with -t 1 and stdout dropped, and compares the files they write.

A test skips only where neither the binaries nor the reference sources exist; where the sources exist the binaries are
built, and a missing binary fails."""
import glob
import gzip
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
import ref_pin as RP
from stress_cases import CASES
from talc_amd import build as B
from talc_amd.synth import Synth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ref_golden as MRG  # noqa: E402


@pytest.fixture(scope="module")
def bins():
    have_src = os.path.isdir(RP.REF_SRC)
    if have_src:
        B.build_reference()
    if not have_src and not (os.path.exists(RP.TALC_ZERO) and os.path.exists(RP.TALC_GXX)):
        pytest.skip("neither the reference binaries nor the reference sources are here")
    assert os.path.exists(RP.TALC_ZERO) and os.path.exists(RP.TALC_GXX) and os.path.exists(RP.TALC_REF)
    return {"zero": RP.TALC_ZERO, "gxx": RP.TALC_GXX, "oracle": RP.TALC_REF}


def run3(bins, args, cwd, timeout=300):
    """The three drivers on the same arguments, side by side: {name: (exit code, files)} with prefixes zero/gxx/oracle."""
    with ThreadPoolExecutor(3) as ex:
        rc = dict(zip(bins, ex.map(lambda n: RP.run(bins[n], args, cwd, n, timeout=timeout), bins)))
    return {n: (rc[n], RP.outputs(cwd, n)) for n in bins}


def same_files(got, want, name, exts=(".fa", ".log", ".config.txt", ".stats_basics.txt"), sort_log=False):
    (rc_g, fg), (rc_w, fw) = got, want
    assert rc_g == rc_w, name
    for ext in exts:
        a, b = fg[ext], fw[ext]
        if ext == ".config.txt" and a is not None and b is not None:
            a = a.replace(name.encode(), b"oracle")
        if ext == ".log" and sort_log:
            a, b = sorted((a or b"").splitlines()), sorted((b or b"").splitlines())
        assert a == b, (name, ext)


# ---------------------------------------------------------------- driver against driver
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The inputs of tests/test_cli.py: 150 k k-mers, 60 reads, as FASTA, as FASTQ with sequence and qualities over
    several lines, and as FASTA wrapped at 60 columns with CRLF line ends and blank lines."""
    d = tmp_path_factory.mktemp("pindata")
    S = Synth(target_kmers=150_000, k=21, seed=77)
    S.write_dump(str(d / "sr.dump"))
    S.write_junctions(str(d / "junc.dump"))
    S.write_fasta(str(d / "reads.fa"), 0, 60)
    recs = RP.fa_records((d / "reads.fa").read_text())
    with open(d / "reads.fq", "w") as g:
        for i, s in recs:
            g.write("@%s\n" % i + "".join(s[p:p + 80] + "\n" for p in range(0, len(s), 80)) + "+\n"
                    + "".join("I" * len(s[p:p + 80]) + "\n" for p in range(0, len(s), 80)))
    with open(d / "wrapped.fa", "w", newline="") as g:
        g.write("\r\n")
        for i, s in recs:
            g.write(">%s\r\n" % i + "".join(s[p:p + 60] + "\r\n" for p in range(0, len(s), 60)) + "\r\n")
    (d / "bad.txt").write_text("hello\nworld\n")
    (d / "empty.dump").write_text("ACGTACGTACGTACGTACGTA 1\n")     # below MIN_COUNT
    return d


DRIVER_CASES = {
    "default": ("reads.fa", "sr.dump", [], 0),
    "junctions": ("reads.fa", "sr.dump", ["-j", "junc.dump"], 0),
    "reverse-fastq": ("reads.fq", "sr.dump", ["-rev"], 0),
    "params": ("reads.fa", "sr.dump", ["--MIN_COUNT", "3", "--MAX_NB_BRANCHES", "5"], 0),
    "wrapped-crlf-fasta": ("wrapped.fa", "sr.dump", [], 0),
    "unreadable-input": ("missing.fa", "sr.dump", ["--MIN_INNER_SCORE", "0.55", "--WINDOW_SIZE", "11", "-j", "junc.dump"], 0),
    "unrecognised-input": ("bad.txt", "sr.dump", [], 0),
    "jellyfish2": ("reads.fa", "sr.dump", ["-qm", "jellyfish2"], 0),
    "empty-graph": ("reads.fa", "empty.dump", [], 1),
}


@pytest.mark.parametrize("name", list(DRIVER_CASES))
def test_driver_files_and_exit_codes_equal_the_oracle_drivers(bins, data, tmp_path, name):
    reads, dump, extra, want_rc = DRIVER_CASES[name]
    for f in os.listdir(data):
        os.symlink(data / f, tmp_path / f)
    r = run3(bins, [reads, "-k", "21", "-SR", dump] + extra, tmp_path)
    assert r["oracle"][0] == want_rc
    for n in ("zero", "gxx"):
        same_files(r[n], r["oracle"], n)
    if want_rc == 0 and "input" not in name:
        assert r["zero"][1][".fa"].count(b">") == 60
    if name in ("default", "junctions", "params", "wrapped-crlf-fasta"):     # a run that corrects, not a pass-through
        recs = RP.fa_records(r["zero"][1][".fa"].decode())
        raw = RP.fa_records((data / "reads.fa").read_text())
        assert sum(a[1] != b[1] for a, b in zip(recs, raw)) >= 45
    if name == "jellyfish2":
        assert r["zero"][1][".log"].count(RP.NO_SOLID.encode()) == 60


def test_wrapped_and_plain_input_give_the_same_records(bins, data, tmp_path):
    for f in os.listdir(data):
        os.symlink(data / f, tmp_path / f)
    assert RP.run(bins["zero"], ["reads.fa", "-k", "21", "-SR", "sr.dump"], tmp_path, "plain") == 0
    assert RP.run(bins["zero"], ["wrapped.fa", "-k", "21", "-SR", "sr.dump"], tmp_path, "wrapped") == 0
    assert RP.run(bins["zero"], ["reads.fq", "-k", "21", "-SR", "sr.dump"], tmp_path, "fastq") == 0
    a, b, c = (RP.outputs(tmp_path, n) for n in ("plain", "wrapped", "fastq"))
    assert a[".fa"] == b[".fa"] == c[".fa"] and a[".log"] == b[".log"] == c[".log"]


# the list of tests/test_cli.py test_cli_parse_errors_and_version, less what the reference's option table does not
# cover (-k 31 is the oracle driver's documented extension)
PARSE_CASES = [
    ([], 1), (["reads.fa", "-SR", "x"], 1), (["reads.fa", "-k", "21"], 1), (["reads.fa", "-k", "17", "-SR", "x"], 1),
    (["reads.fa", "-k", "21", "-SR", "x", "--MIN_COUNT", "1"], 1), (["reads.fa", "-k", "21", "-SR", "x", "-qm", "kmc"], 1),
    (["reads.fa", "-k", "21", "-SR", "x", "--bogus"], 1), (["--version"], 0), (["--help"], 0),
    (["reads.fa", "-k", "21", "-SR", "x", "--SR_ERROR_RATE", "0.2"], 1), (["reads.fa", "-k", "21", "-SR", "x", "--MAX_NB_BRANCHES", "4"], 1),
    (["reads.fa", "-k", "21", "-SR", "x", "--WINDOW_SIZE", "5"], 1), (["reads.fa", "-k", "21", "-SR"], 1),
]


def test_parse_errors_and_version_exit_as_the_oracle_driver(bins, tmp_path):
    import subprocess
    for args, want in PARSE_CASES:
        rcs = {n: subprocess.run([exe] + args, cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=60).returncode
               for n, exe in bins.items()}
        assert rcs == {"zero": want, "gxx": want, "oracle": want}, (args, rcs)
    assert not os.listdir(tmp_path)        # nothing is written before the command line is accepted (main.cpp:199-204)


# ---------------------------------------------------------------- stress sets through the reference's command line
# The sets of tests/stress_cases.py whose parameters the reference's command line can express, and the tandem-repeat
# generator; read counts are what keeps one set under about a minute of CPU (docs/reference_pin.md has the timings).
STRESS = {"101": 100, "102": 100, "201": 150, "202": 150, "204": 150, "205": 150, "301": 100, "304": 100, "tandem": 240}
BRANCHING = ("101", "102", "301", "304", "tandem")
_stress = {}


def stress_run(bins, name, root):
    """Inputs written with Synth, the three drivers' files, and per read how often the oracle entered scoreBridges
    (computed once per set and shared)."""
    if name in _stress:
        return _stress[name]
    d = root.mktemp("stress" + name)
    n = STRESS[name]
    if name == "tandem":
        k, params, junctions = 21, {}, False
        keys, counts, reads = RP.tandem_case()
        reads = reads[:n]
        RP.write_dump(str(d / "sr.dump"), keys, counts, k)
    else:
        kw, pkw = CASES[int(name)]
        k, junctions = kw["k"], bool(kw.get("junctions"))
        params = {a: v for a, v in pkw.items()}
        S = Synth(target_kmers=kw["target_kmers"], k=k, seed=kw["seed"], **kw.get("synth_kw", {}))
        S.write_dump(str(d / "sr.dump"))
        if junctions:
            S.write_junctions(str(d / "junc.dump"))
        reads = PU.seqs_of(*S.reads(0, n))
        if params.get("reverse"):      # reads from the opposite strand, so that -rev puts them onto the table's
            reads = [RP.revcomp(s) for s in reads]
    ids = ["s%s_%d" % (name, i) for i in range(len(reads))]
    RP.write_fasta(str(d / "reads.fa"), ids, reads)
    r = run3(bins, RP.reference_args(k, params, junctions), d, timeout=600)
    # per read: does the oracle enter scoreBridges (Explorer.cpp:689-706, the one place the two flavours may differ)?
    q = O.params(k=k, use_junctions=int(junctions), **params)
    tab = O.OracleTable(q, O.OracleTable.FLAT)
    tab.build_from_files(str(d / "sr.dump"), str(d / "junc.dump") if junctions else None)
    tab.decolour()
    calls = []
    for s in reads:
        before = O.ub_counters()["scoreBridgesCalls"]
        tab.correct_batch(*RP.pack([s]), nthreads=1)
        calls.append(O.ub_counters()["scoreBridgesCalls"] - before)
    tab.close()
    _stress[name] = dict(r=r, ids=ids, reads=reads, k=k, calls=calls)
    return _stress[name]


@pytest.mark.parametrize("name", list(STRESS))
def test_stress_set_records_and_log_equal_the_oracle_drivers(bins, tmp_path_factory, name):
    s = stress_run(bins, name, tmp_path_factory)
    r = s["r"]
    assert r["zero"][0] == 0 and r["oracle"][0] == 0
    same_files(r["zero"], r["oracle"], "zero", exts=(".fa", ".log"), sort_log=True)
    recs = RP.fa_records(r["zero"][1][".fa"].decode())
    assert [i for i, _ in recs] == s["ids"]
    assert sum(rec[1] != RP.dna5(raw) for rec, raw in zip(recs, s["reads"])) >= 0.75 * len(recs)      # it did correct


@pytest.mark.parametrize("name", list(STRESS))
def test_undefined_loop_index_gxx_flavour_equals_the_zeroed_one(bins, tmp_path_factory, name):
    """Explorer.cpp:705 reads an uninitialised loop index.  talc_zero gives it the value the oracle documents (0);
    talc_gxx is what the reference's own build line makes of it.  Both must write the same files."""
    s = stress_run(bins, name, tmp_path_factory)
    same_files(s["r"]["gxx"], s["r"]["zero"], "gxx", exts=(".fa", ".log"), sort_log=True)


def test_both_flavours_are_exercised_in_score_bridges(bins, tmp_path_factory):
    entering = sum(sum(c > 0 for c in stress_run(bins, name, tmp_path_factory)["calls"]) for name in BRANCHING)
    assert entering >= 20, entering


# ---------------------------------------------------------------- the reference-recorded fixtures
REF_FIXTURES = sorted(glob.glob(os.path.join(RP.REF_GOLDEN, "*.json.gz")))


def load(path):
    with gzip.open(path, "rb") as f:
        return json.loads(f.read().decode())


def test_reference_fixtures_are_current(bins, tmp_path):
    """The recorder run again gives the committed files, byte for byte, and nothing else."""
    MRG.record_all(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == [os.path.basename(p) for p in REF_FIXTURES] and len(REF_FIXTURES) == len(MRG.CASES)
    for p in REF_FIXTURES:
        assert open(p, "rb").read() == open(tmp_path / os.path.basename(p), "rb").read(), p


def test_reference_fixture_set_meets_its_conditions():
    MRG.check_set([load(p) for p in REF_FIXTURES])


@pytest.mark.parametrize("path", REF_FIXTURES, ids=[os.path.basename(p)[:-8] for p in REF_FIXTURES])
def test_oracle_reproduces_reference_fixture(path):
    """The oracle run live gives the reference's records and statuses; where the oracle-made fixture of the same name
    has the same parameters (all mirrored cases but g10, which the reference runs with MAX_NB_BRANCHES 5), its
    `expected` holds the same records."""
    fx = load(path)
    keys, counts, jk, jc, bases, offs = MRG.fixture_inputs(fx)
    tab = O.OracleTable(O.params(**fx["params"]), O.OracleTable.FLAT)
    tab.insert_packed(keys, counts)
    if jk is not None:
        tab.colour_packed(jk, jc)
    tab.decolour()
    out, oo, st = tab.correct_batch(bases, offs, nthreads=4)
    tab.close()
    want = [s for _, s in RP.fa_records(fx["fa"])]
    assert PU.seqs_of(out, oo) == want
    assert [int(x) for x in st] == RP.statuses(fx["ids"], fx["reads"], fx["k"], fx["log"])
    twin = os.path.join(HERE, "golden", fx["name"] + ".json.gz")
    if os.path.exists(twin):
        ofx = load(twin)
        assert ofx["reads"] == fx["reads"] and ofx["params"] == fx["params"]
        assert ofx["expected"] == want
    else:
        assert fx["name"].split("_")[0] in ("g10", "g11", "g12", "g13")
