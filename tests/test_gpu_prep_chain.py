"""The long-read preparation options together on the device (docs/read_preparation.md): end clean-up, chimera split,
barcode demultiplexing and UMI read-out set on one context, every batch kind, against the composed contract in numpy
(tests/prep_ref.py: never from a device result) and against plain batches of the texts cut on the host.  Integers and bytes,
tolerance 0.  tests/test_prep_reference.py asserts, from the reference alone, that the input reaches what it is there for."""
import os
import subprocess

import numpy as np
import pytest

import chimera_ref as CR
import demux_ref as DR
import ends_ref as R
import parity_util as PU
import prep_ref as P
import test_gpu_chimera as GC
import test_gpu_solidity as G
from memcheck_util import guards_checked
from talc_amd import build as B
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

TALC = os.path.join(B.OUT, "talc")
ALL_ON = (True, True, True, True)
MODES = ("plain", "auto")
REPORTS = ("demux", "hits", "hit_off", "pieces", "piece_off", "ends", "umi")

_in = {}


def fresh(c, mode, subset=(False, False, False, False)):
    """A context of its own over the shared table, in the strand mode, with the settings of `subset` (ends, chimera, demux,
    UMI) switched on and no call ever made for the others."""
    ctx = T.Context(c.ttab, c.p, 0)
    if mode == "auto":
        ctx.auto_strand()
    ends_on, chimera_on, demux_on, umi_on = subset
    if ends_on:
        ctx.set_ends(**P.ENDS_KW)
    if chimera_on:
        ctx.set_chimera(*P.CHIMERA)
    if demux_on:
        ctx.set_demux(*P.DEMUX)
    if umi_on:
        ctx.set_umi(*P.UMI)
    return ctx


def inputs():
    """200 generator reads dressed as prep_ref.reads_of does (185 reads), and the first 40 of them with the four edge reads
    (44); per strand mode a context that never had any of the four settings, and what plain batches of host-cut texts give on
    it (computed once per list of texts, shared, left unchanged)."""
    if not _in:
        c = G.gen_set("default")
        reads = P.reads_of(c.reads[:200], np.random.default_rng(8))
        _in.update(c=c, reads=reads, small=reads[:40] + reads[-4:], never={mode: fresh(c, mode) for mode in MODES}, base={})
    return _in


def base_of(mode, texts):
    s = inputs()
    key = (mode, tuple(texts))
    if key not in s["base"]:
        s["base"][key] = GC.everything_of(s["never"][mode], *PU.pack_reads(texts))
    return s["base"][key]


def wanted(reads, subset, clip, split):
    ends_on, chimera_on, demux_on, umi_on = subset
    return P.chain(reads, P.ENDS_KW if ends_on else None, P.CHIMERA if chimera_on else None, P.DEMUX if demux_on else None,
                   P.UMI if umi_on else None, clip=clip, split=split)


def asked(call):
    """What a report call returns, or None when the library refuses it with TALC_ERR_STATE."""
    try:
        return call()
    except T.TalcError as e:
        assert str(e).startswith("libtalc_hip error -6:"), str(e)
        return None


def reports_of(ctx, reads, clip, split):
    """Every report of a fresh batch of that kind (None: refused), and the scan times read after demux() and umi()."""
    b = ctx.batch(*R.batch(reads), clip=clip, split=split)
    try:
        r = dict(n=b.n_reads)
        r["demux"] = asked(b.demux)
        r["demux_ms"] = ctx.demux_timing()
        r["umi"] = asked(b.umi)
        r["umi_ms"] = ctx.umi_timing()
        r["ends"] = asked(b.ends)
        r["hits"], r["hit_off"] = asked(b.chimera) or (None, None)
        r["pieces"], r["piece_off"] = asked(b.split_pieces) or (None, None)
        return r
    finally:
        b.close()


def run_kinds(ctx, reads, subset):
    """{kind: (reports, every output)} of the kinds the context allows; the others are asserted to raise what they raise."""
    ends_on, chimera_on, _, umi_on = subset
    got = {}
    for name, clip, split in P.KINDS:
        if P.legal(ends_on, chimera_on, umi_on, clip, split):
            got[name] = (reports_of(ctx, reads, clip, split), GC.everything_of(ctx, *R.batch(reads), clip=clip, split=split))
        else:
            word = "the chimera scan is off" if split else "the end clean-up is off"
            with pytest.raises(T.TalcError, match=word):
                ctx.batch(*R.batch(reads), clip=clip, split=split)
    return got


def check_kinds(got, reads, subset, mode, prefix=""):
    ends_on, chimera_on, demux_on, umi_on = subset
    assert sorted(got) == sorted(name for name, clip, split in P.KINDS if P.legal(ends_on, chimera_on, umi_on, clip, split))
    for name, clip, split in P.KINDS:
        if name not in got:
            continue
        what = "%s%s %s %s" % (prefix, mode, subset, name)
        want = wanted(reads, subset, clip, split)
        rep, outs = got[name]
        assert rep["n"] == len(want["texts"]), what
        for key in REPORTS:
            assert (rep[key] is None) == (want[key] is None), (what, key)
            if want[key] is not None:
                assert rep[key].dtype == want[key].dtype and len(rep[key]) == len(want[key]), (what, key)
                bad = np.flatnonzero(rep[key] != want[key])
                assert len(bad) == 0, (what, key, len(bad), int(bad[0]), rep[key][bad[0]].tolist(), want[key][bad[0]].tolist())
        if clip or split:                                                # the rows came with the batch: nothing ran again
            assert not demux_on or rep["demux_ms"] == 0.0, what
            assert not umi_on or rep["umi_ms"] == 0.0, what
        GC.same_batches(outs, base_of(mode, want["texts"]), what)
        if split:
            assert (outs["pieces"] == want["pieces"]).all() and (outs["hits"] == want["hits"]).all(), what


def ends_alone(c, reads, subset, kinds):
    """{kind: the end rows} of a context that has only the ends on: of the reads, plain and clipped, and of the pieces cut on
    the host (it cannot split)."""
    only = fresh(c, "plain", (True, False, False, False))
    try:
        rows = {}
        for name, clip, split in P.KINDS:
            if name not in kinds:
                continue
            came = wanted(reads, subset, clip, split)["came"] if split else reads
            b = only.batch(*R.batch(came), clip=clip)
            try:
                rows[name] = b.ends()
            finally:
                b.close()
        return rows
    finally:
        only.close()


# ---------------------------------------------------------------- a. everything on, every batch kind, plain and auto strand
@pytest.mark.parametrize("mode", MODES)
def test_everything_on_every_batch_kind(mode):
    s = inputs()
    reads = s["reads"]
    assert len(reads) == 185
    ctx = fresh(s["c"], mode, ALL_ON)
    try:
        got = run_kinds(ctx, reads, ALL_ON)
    finally:
        ctx.close()
    check_kinds(got, reads, ALL_ON, mode)
    for name, clip, split in P.KINDS:                                    # the correction does real work on every baseline
        base = base_of(mode, wanted(reads, ALL_ON, clip, split)["texts"])
        assert base["work"][1] > 0, name
    alone = ends_alone(s["c"], reads, ALL_ON, got)
    for name, _, _ in P.KINDS:
        assert (got[name][0]["ends"] == alone[name]).all(), name         # the end rows keep what k_read_ends wrote


# ---------------------------------------------------------------- b. every legal subset of the settings
@pytest.mark.parametrize("subset", P.subsets(), ids=lambda t: "".join(n for n, on in zip(("E", "C", "D", "U"), t) if on) or "none")
def test_every_legal_subset_of_the_settings(subset):
    s = inputs()
    reads = s["small"]
    assert len(reads) == 44 and reads[-4:-2] == ["", "ACGT"] and len(P.subsets()) == 12
    ctx = fresh(s["c"], "plain", subset)
    try:
        got = run_kinds(ctx, reads, subset)
    finally:
        ctx.close()
    check_kinds(got, reads, subset, "plain")
    assert base_of("plain", reads)["work"][1] > 0
    if subset[0]:
        alone = ends_alone(s["c"], reads, subset, got)
        for name in got:
            assert (got[name][0]["ends"] == alone[name]).all(), name


# ---------------------------------------------------------------- c. on poisoned memory between red zones
@pytest.mark.parametrize("byte", [0xA5, 0xFF])
def test_everything_on_on_poisoned_memory_between_red_zones(byte):
    s = inputs()
    reads = s["reads"]
    for name, clip, split in P.KINDS:                                    # (the baselines, made before the poison is on)
        base_of("plain", wanted(reads, ALL_ON, clip, split)["texts"])
    with guards_checked():
        with T.poisoned(byte):
            ctx = fresh(s["c"], "plain", ALL_ON)
            try:
                got = run_kinds(ctx, reads, ALL_ON)
            finally:
                ctx.close()
    check_kinds(got, reads, ALL_ON, "plain", "poisoned %#x, " % byte)


# ---------------------------------------------------------------- d. the command line
REPORT_OPTIONS = ["--corr-map", "--soft-mask", "--trim", "--split", "--min-piece-len", "50", "--corr-edits", "--fastq", "--solidity", "--read-stats"]
REPORT_FILES = {".fa", ".map.tsv", ".solidity.tsv", ".trim.fa", ".split.fa", ".edits.tsv", ".fq", ".trim.fq", ".split.fq", ".stats_basics.txt"}
LR_FILES = {".ends.tsv", ".chimera.tsv", ".chimera_pieces.tsv", ".demux.tsv", ".demux_counts.tsv", ".umi.tsv"}


def test_cli_every_lr_option_with_every_report_option(tmp_path):
    c = G.gen_set("default")
    reads = P.reads_of(c.reads[:60], np.random.default_rng(34))
    names = ["read%d/x" % i for i in range(len(reads))]
    bc_names = ["bc%02d" % (i + 1) for i in range(96)]
    ref = P.chain(reads, P.ENDS_KW, P.CHIMERA, P.DEMUX, P.UMI, clip=True, split=True)
    pieces, came, texts = ref["pieces"], ref["came"], ref["texts"]
    _, _, dropped, dropped_bases = CR.pieces([len(x) for x in reads], ref["hits"], P.CHIMERA[2])
    piece_names = CR.piece_names(names, pieces)
    seen = np.bincount(ref["demux"]["status"], minlength=5)
    assert len(reads) == 59 and len(pieces) > len(reads) + 3 and seen[DR.BOTH] >= 30 and seen[DR.CONFLICT] >= 3 and seen[DR.NONE] >= 5, (len(reads), len(pieces), seen)
    assert (ref["umi"]["end"] == 1).sum() >= 10 and (ref["umi"]["end"] == 2).sum() >= 10 and (ref["umi"]["kept_len"] == 0).sum() >= 1
    assert len(set(piece_names)) == len(piece_names) and any("_c2" in x for x in piece_names)
    c.syn.write_dump(str(tmp_path / "sr.dump"))
    fasta = lambda nms, seqs: "".join(">%s\n%s\n" % (nm, x) for nm, x in zip(nms, seqs))
    (tmp_path / "dressed.fa").write_text(fasta(names, reads))
    (tmp_path / "host.fa").write_text(fasta(piece_names, texts))
    (tmp_path / "bc.fa").write_text(fasta(bc_names, P.BC24))
    common = ["-k", "21", "-SR", str(tmp_path / "sr.dump"), "--batch-reads", "7", "-o", "o"] + REPORT_OPTIONS
    lr = ["--LRBarcodes", str(tmp_path / "bc.fa"), "--LRDemuxOut", "--LRAdapter", P.SSP23, "--LRAdapter", P.VNP, "--LRPolyA", "12", "--LRSplit", "--LRClip",
          "--LRUmi", P.UMI[0]]
    two = dict(os.environ, TALC_FAKE_GPUS="2")
    runs = {}
    for d, args, env in (("full", ["dressed.fa"] + lr, None), ("full2", ["dressed.fa"] + lr + ["--gpus", "2"], two), ("full_auto", ["dressed.fa"] + lr + ["--auto-strand"], None),
                         ("host", ["host.fa"], None), ("host_auto", ["host.fa", "--auto-strand"], None)):
        (tmp_path / d).mkdir()
        runs[d] = subprocess.run([TALC, str(tmp_path / args[0])] + args[1:] + common, cwd=tmp_path / d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert runs[d].returncode == 0, (d, runs[d].stderr.decode())
    files = lambda d: {f[1:] for f in os.listdir(tmp_path / d) if f.startswith("o.")}
    read = lambda d, ext: (tmp_path / d / ("o" + ext)).read_bytes() if (tmp_path / d / ("o" + ext)).exists() else None
    per_barcode = {".%s.fa" % nm for nm in bc_names + ["unclassified"]}
    # every output is that of the clipped pieces: the run on the texts cut beforehand on the host, under the pieces' names
    for full, host in (("full", "host"), ("full2", "host"), ("full_auto", "host_auto")):
        extra = {".strand.tsv"} if host == "host_auto" else set()
        assert REPORT_FILES | extra | {".config.txt"} <= files(host) <= REPORT_FILES | extra | {".config.txt", ".log"}, (host, sorted(files(host)))
        assert files(full) == files(host) | LR_FILES | per_barcode, (full, sorted(files(full) ^ files(host)))
        for ext in sorted(files(host) - {".config.txt"}):
            assert read(full, ext) == read(host, ext), (full, ext)
        cfg = read(full, ".config.txt").decode().splitlines()
        assert [x for x in cfg if x.startswith("LR")] == ["LRAdapter=" + P.SSP23, "LRAdapter=" + P.VNP, "LRPolyA=12", "LRClip=1", "LRSplit=1", "LRUmi=" + P.UMI[0],
                                                          "LRBarcodes=" + str(tmp_path / "bc.fa"), "LRDemuxOut=1"]
        assert not [x for x in read(host, ".config.txt").decode().splitlines() if x.startswith("LR")]
    assert read("full", ".fa") != read("full_auto", ".fa") or read("full", ".edits.tsv") != read("full_auto", ".edits.tsv")   # auto strand turned some read
    assert len(read("full", ".edits.tsv").splitlines()) == len(pieces) + 1 and len(read("full", ".stats_basics.txt").splitlines()) > len(reads) // 2
    assert b"correcting on 2 GPU(s)" in runs["full2"].stdout

    # the reports of the preparation itself, against the reference
    name_of = lambda b: bc_names[int(b) - 1] if b else "-"
    lens = np.array([len(x) for x in reads])
    d = ref["demux"]
    demux_tsv = ["read_name\traw_length\tbarcode\tstatus\thead_barcode\thead_err\thead_margin\thead_end\ttail_barcode\ttail_err\ttail_margin\ttail_end"]
    for nm, x, w in zip(names, reads, d):
        demux_tsv.append("\t".join([nm, str(len(x)), name_of(w["barcode"]), str(int(w["status"])), name_of(w["head_best"]), str(int(w["head_err"])), str(int(w["head_margin"])),
                                    str(int(w["head_end"])), name_of(w["tail_best"]), str(int(w["tail_err"])), str(int(w["tail_margin"])), str(int(w["tail_end"]))]))
    counts_tsv = ["barcode\treads\tbases"]
    for b in list(range(1, 97)) + [0]:
        mine = d["barcode"] == b
        counts_tsv.append("%s\t%d\t%d" % (bc_names[b - 1] if b else "unclassified", int(mine.sum()), int(lens[mine].sum())))
    cls, st = d["barcode"] > 0, d["status"]
    demux_line = "[TALC]: demux: %d reads, %d classified (%d both ends, %d head only, %d tail only), %d conflicts, %d without a barcode" % (
        len(d), int(cls.sum()), int((cls & (st == DR.BOTH)).sum()), int((cls & (st == DR.HEAD_ONLY)).sum()), int((cls & (st == DR.TAIL_ONLY)).sum()),
        int((st == DR.CONFLICT).sum()), int((~cls & (st != DR.CONFLICT)).sum()))
    u = ref["umi"]
    umi_tsv = ["read_name\tlength\tend\terr\tother_err\tstart\tstop\tumi\tkept_start\tkept_len"]
    for nm, x, w in zip(piece_names, came, u):
        umi_tsv.append("\t".join([nm, str(len(x)), str(int(w["end"])), str(int(w["err"])), "-" if w["other_err"] == 255 else str(int(w["other_err"])), str(int(w["start"])),
                                  str(int(w["stop"])), w["umi"].decode() if w["end"] else "-", str(int(w["kept_start"])), str(int(w["kept_len"]))]))
    both = u["other_err"] != 255
    umi_line = "[TALC]: umi: %d reads, %d at the head, %d at the tail, %d at both ends, %d without" % (
        len(u), int(((u["end"] == 1) & ~both).sum()), int(((u["end"] == 2) & ~both).sum()), int(both.sum()), int((u["end"] == 0).sum()))
    e = ref["ends"]
    ends_tsv = ["read_name\traw_length\thead_adapter\thead_adapter_len\thead_adapter_err\thead_poly\ttail_adapter\ttail_adapter_len\ttail_adapter_err\ttail_poly\tkept_start\tkept_len\torient"]
    for nm, x, w in zip(piece_names, came, e):
        ends_tsv.append("\t".join([nm, str(len(x))] + [str(int(w[f])) for f in ("head_adapter", "head_adapter_len", "head_adapter_err", "head_poly_len", "tail_adapter",
                                                                                  "tail_adapter_len", "tail_adapter_err", "tail_poly_len", "kept_start", "kept_len", "orient")]))
    ends_line = "[TALC]: read ends: %d reads, %d with an adapter, %d with a poly run, %d bases clipped" % (
        len(e), int(((e["head_adapter"] > 0) | (e["tail_adapter"] > 0)).sum()), int(((e["head_poly_len"] > 0) | (e["tail_poly_len"] > 0)).sum()),
        sum(len(x) for x in came) - int(e["kept_len"].sum()))
    hits = ref["hits"]
    chimera_tsv = ["read_name\traw_length\tadapter\tstrand\tstart\tend\terr"]
    chimera_tsv += ["\t".join([names[int(h["read"])], str(len(reads[int(h["read"])])), str(int(h["adapter"])), "-" if h["strand"] else "+", str(int(h["start"])),
                               str(int(h["end"])), str(int(h["err"]))]) for h in hits]
    pieces_tsv = ["piece_name\tread_name\tstart\tlen"] + ["\t".join([pn, names[int(p["read"])], str(int(p["start"])), str(int(p["len"]))]) for pn, p in zip(piece_names, pieces)]
    chimera_line = "[TALC]: chimeras: %d reads, %d hits in %d reads, %d pieces kept, %d pieces dropped (%d bases)" % (
        len(reads), len(hits), len(np.unique(hits["read"])), len(pieces), dropped, dropped_bases)
    for full in ("full", "full2", "full_auto"):
        for ext, lines in ((".demux.tsv", demux_tsv), (".demux_counts.tsv", counts_tsv), (".umi.tsv", umi_tsv), (".ends.tsv", ends_tsv), (".chimera.tsv", chimera_tsv),
                           (".chimera_pieces.tsv", pieces_tsv)):
            assert read(full, ext).decode().splitlines() == lines, (full, ext)
        out = runs[full].stdout.decode().splitlines()
        for line in (demux_line, umi_line, ends_line, chimera_line):
            assert out.count(line) == 1, (full, line, [x for x in out if x.startswith(line[:14])])
        # the per-barcode files: every record of <o>.fa, byte for byte and in order, in the file of its source read's barcode
        records = [b">" + x for x in read(full, ".fa").split(b">")[1:]]
        assert [x.split(b"\n")[0][1:].decode() for x in records] == piece_names
        dealt = {nm: b"" for nm in bc_names + ["unclassified"]}
        for rec, p in zip(records, pieces):
            dealt[name_of(d[int(p["read"])]["barcode"]).replace("-", "unclassified")] += rec
        assert sum(1 for v in dealt.values() if v) >= 20 and dealt["unclassified"]
        for nm, text in dealt.items():
            assert read(full, ".%s.fa" % nm) == text, (full, nm)
    for host in ("host", "host_auto"):
        assert not any(word in runs[host].stdout for word in (b"demux:", b"umi:", b"read ends:", b"chimeras:"))
