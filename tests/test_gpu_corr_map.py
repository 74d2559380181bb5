"""The correction map on the device (docs/correction_map.md; k_search's leave_outcome, k_pack_map, k_mask_case) against
the map rebuilt from the oracle's trace (tests/corr_map_ref.py).  Every map-on run is also held against a map-off run of
the same batch: same records, offsets, statuses and work counters."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import corr_map_ref as M
import parity_util as PU
from talc_amd import build as B
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALC = os.path.join(B.OUT, "talc")
TALC_REF = os.path.join(ROOT, "oracle", "_build", "talc_ref")
ERR_CAPACITY, ERR_STATE = -5, -6


def ctx_of(s):
    if s.pair.ctx is None:
        s.pair.upload(0)
    return s.pair.ctx


def run(ctx, bases, offs, on, mask=True):
    """One correction of a fresh batch with the map on or off: records, offsets, statuses, work counters, return code
    and, with the map, the segments, their offsets and the masked records."""
    ctx.record_map(on)
    b = ctx.batch(bases, offs)
    try:
        r = dict(rc=b.correct())
        r["out"], r["oo"], r["st"] = b.fetch_corrected()
        t = ctx.timing()
        r["work"] = (t.n_trail_steps, t.n_dp_cells)
        r["timing"] = t
        r["nseg"] = b.n_segments
        if on:
            r["segs"], r["so"] = b.fetch_map()
            if mask:
                r["masked"], moo, mst = b.fetch_corrected(soft_mask=True)
                assert np.array_equal(moo, r["oo"]) and np.array_equal(mst, r["st"])
        return r
    finally:
        b.close()
        ctx.record_map(False)


def same_records(a, b):
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["oo"], b["oo"]) and np.array_equal(a["st"], b["st"])
    assert a["rc"] == b["rc"]


def check_against(r, exp, what=""):
    """The device map of every read equals the expected one; the masked records are the expected pieces with the RAW
    ones in lower case (so: upper() is the plain record, and the lower-case positions are exactly the RAW out ranges)."""
    assert r["nseg"] == len(r["segs"]) == int(r["so"][-1]) == sum(len(e["segs"]) for e in exp)
    got = PU.seqs_of(r["out"], r["oo"])
    msk = PU.seqs_of(r["masked"], r["oo"]) if "masked" in r else None
    for i, e in enumerate(exp):
        g = r["segs"][int(r["so"][i]):int(r["so"][i + 1])]
        w = M.as_array(e["segs"])
        assert len(g) == len(w) and (g == w).all(), (what, i, [tuple(x) for x in g[:6].tolist()], e["segs"][:6],
                                                     np.nonzero(g != w)[0][:4].tolist() if len(g) == len(w) else (len(g), len(w)))
        assert int(r["st"][i]) == e["status"] and got[i] == e["out"], (what, i)
        if msk is not None:
            assert msk[i] == M.masked(e), (what, i)
            assert msk[i].upper() == got[i]
            low = np.zeros(len(got[i]) + 1, dtype=np.int64)
            for kind, rs, rl, os_, ol in e["segs"]:
                if kind == M.RAW:
                    low[os_] += 1
                    low[os_ + ol] -= 1
            assert [c.islower() for c in msk[i]] == (np.cumsum(low)[:-1] > 0).tolist()


def check_set(s, ctx, what):
    bases, offs = s.packed()
    off, on = run(ctx, bases, offs, False), run(ctx, bases, offs, True)
    assert off["nseg"] == 0
    same_records(on, off)
    assert on["work"] == off["work"] and on["work"][0] > 0
    check_against(on, s.exp, what)
    assert all(M.raw_overlaps([tuple(x) for x in on["segs"][int(on["so"][i]):int(on["so"][i + 1])].tolist()]) == 0 for i in range(len(s.exp)))
    return on


@pytest.mark.parametrize("name", list(M.SETS))
def test_map_equals_the_reference_map(name):
    s = M.map_set(name)
    c = s.counts()
    assert c["S"] and c["C"] and c["R"] and c["head_corrected"] and c["tail_corrected"]
    if name in ("default", "reverse"):
        assert c["zero_corrected"] and c["zero_raw"]
    if name == "paralog-maxb4":
        assert c["head_long"] + c["tail_long"]
    if name == "k31":
        assert c["head_long"] and c["tail_long"] and any(e["R"] == 1 for e in s.exp)
    check_set(s, ctx_of(s), name)


@pytest.mark.parametrize("graph", M.COMB_SETS)
def test_map_of_reads_with_more_than_64_regions(graph):
    s = M.comb_set(graph)
    assert len(s.exp) >= 10 and all(e["R"] >= 100 for e in s.exp)
    check_set(s, ctx_of(s), graph)


def test_map_of_edge_inputs():
    """The inputs of test_correction_edge_inputs: the empty read, L <= K, no solid k-mer, N runs."""
    s0 = M.map_set("default")
    r = PU.seqs_of(*s0.pair.reads(5000, 8))
    reads = ["", r[0][:21], r[0][:22], r[1].lower(), r[2][:400] + "N" + r[2][400:],
             r[3][:300] + "N" * 10 + r[3][300:900] + "RYKM" + r[3][900:], "ACGT" * 300, "A" * 500,
             "".join(random.Random(1).choice("ACGT") for _ in range(1500)), r[4], r[5][:60], r[6] + r[7]]
    s = M.MapSet(s0.pair, reads)
    st = [e["status"] for e in s.exp]
    assert st[0] == 1 and st[1] == 1 and 2 in st and 0 in st
    assert s.exp[0]["segs"] == [(M.RAW, 0, 0, 0, 0)]
    on = check_set(s, ctx_of(s0), "edge inputs")
    for i, e in enumerate(s.exp):
        if e["status"] != 0:
            assert int(on["so"][i + 1] - on["so"][i]) == 1


def test_map_survives_the_retry_pass_and_failed_reads(monkeypatch):
    """TALC_TEST_TINY_CAPS: reads overflow their scratch and are redone by the retry launches, which must leave the
    outcome as well.  With TALC_TEST_FAIL_RETRY_ALLOC those reads end as TALC_READ_ERROR: one RAW segment each."""
    s = M.map_set("default")
    bases, offs = s.packed()
    ref = run(ctx_of(s), bases, offs, False)
    monkeypatch.setenv("TALC_TEST_TINY_CAPS", "1")
    ctx2 = T.Context(s.pair.ttab, s.pair.p, 0)
    off, on = run(ctx2, bases, offs, False), run(ctx2, bases, offs, True)
    assert on["timing"].n_retried > 0 and on["timing"].n_failed == 0
    same_records(on, off)
    same_records(on, ref)
    assert on["work"] == off["work"]
    check_against(on, s.exp, "retry")
    ctx2.close()
    monkeypatch.setenv("TALC_TEST_FAIL_RETRY_ALLOC", "1")
    ctx3 = T.Context(s.pair.ttab, s.pair.p, 0)
    off, on = run(ctx3, bases, offs, False), run(ctx3, bases, offs, True)
    assert on["rc"] == T.WARN_READ_ERRORS and on["timing"].n_failed > 0
    same_records(on, off)
    exp = []
    for i, e in enumerate(s.exp):
        if on["st"][i] == T.READ_ERROR:
            L = len(s.reads[i])
            exp.append(dict(segs=[(M.RAW, 0, L, 0, L)], pieces=[M.dna5(s.reads[i])], out=M.dna5(s.reads[i]), status=T.READ_ERROR))
        else:
            exp.append(e)
    assert sum(1 for e in exp if e["status"] == T.READ_ERROR) == on["timing"].n_failed
    check_against(on, exp, "failed retry")
    ctx3.close()


def test_map_with_every_edge_published_as_a_task(monkeypatch):
    s = M.map_set("paralog-maxb4")
    ctx_of(s)                                        # (uploaded; the switches are read when a context is made)
    monkeypatch.setenv("TALC_EDGE_TASKS", "1")
    monkeypatch.setenv("TALC_EDGE_TASK_MIN", "0")
    ctx2 = T.Context(s.pair.ttab, s.pair.p, 0)
    bases, offs = s.packed()
    off, on = run(ctx2, bases, offs, False), run(ctx2, bases, offs, True)
    same_records(on, off)
    check_against(on, s.exp, "edge tasks")


def test_map_calls_report_capacity_and_state():
    s = M.map_set("default")
    ctx = ctx_of(s)
    bases, offs = PU.pack_reads(s.reads[:20])
    L = T.lib()
    ctx.record_map(True)
    b = ctx.batch(bases, offs)
    try:
        assert b.n_segments == 0
        so = np.zeros(21, dtype=np.uint64)
        assert L.talc_batch_fetch_map(ctx._h, b._h, None, 0, so.ctypes.data) == ERR_STATE       # not corrected yet
        b.correct()
        n = b.n_segments
        assert n == sum(len(e["segs"]) for e in s.exp[:20])
        assert L.talc_batch_fetch_map(ctx._h, b._h, None, 0, so.ctypes.data) == 0 and int(so[20]) == n   # offsets only
        segs = np.zeros(n, dtype=T.SEGMENT_DTYPE)
        assert L.talc_batch_fetch_map(ctx._h, b._h, segs.ctypes.data, n - 1, so.ctypes.data) == ERR_CAPACITY
        assert str(n).encode() in L.talc_last_error()
        assert L.talc_batch_fetch_map(ctx._h, b._h, segs.ctypes.data, n, None) == 0
        assert (segs[: len(s.exp[0]["segs"])] == M.as_array(s.exp[0]["segs"])).all()
    finally:
        b.close()
        ctx.record_map(False)


@pytest.mark.parametrize("where", ["host", "device"])
def test_record_calls_report_capacity_and_leave_the_buffer(where):
    """talc_batch_fetch_corrected / talc_batch_copy_corrected_device with room for one byte less than the records take:
    TALC_ERR_CAPACITY naming the total, offsets and statuses filled as by a full call, not a byte of the buffer written."""
    s = M.map_set("default")
    ctx = ctx_of(s)
    n = 20
    bases, offs = PU.pack_reads(s.reads[:n])
    L = T.lib()
    b = ctx.batch(bases, offs)
    hip = dev = None
    try:
        b.correct()
        want, woo, wst = b.fetch_corrected()
        total = int(woo[n])
        assert total == b.corrected_bytes > 1
        oo, st = np.zeros(n + 1, dtype=np.uint64), np.full(n, -1, dtype=np.int32)
        buf = np.full(total, 0xEE, dtype=np.uint8)
        if where == "host":
            call, ptr, read = L.talc_batch_fetch_corrected, buf.ctypes.data, lambda: buf
        else:   # a device buffer of the test's own, filled with the same sentinel
            hip, dev = PU._hip(), C.c_void_p()
            assert hip.hipMalloc(C.byref(dev), total) == 0
            assert hip.hipMemcpy(dev, buf.ctypes.data, total, 1) == 0      # (1: host to device)

            def read():
                back = np.zeros(total, dtype=np.uint8)
                assert hip.hipMemcpy(back.ctypes.data, dev, total, 2) == 0     # (2: device to host)
                return back
            call, ptr = L.talc_batch_copy_corrected_device, dev
        assert call(ctx._h, b._h, ptr, total - 1, oo.ctypes.data, st.ctypes.data) == ERR_CAPACITY
        assert str(total).encode() in L.talc_last_error()
        assert np.array_equal(oo, woo) and np.array_equal(st, wst)
        assert (read() == 0xEE).all()
        assert call(ctx._h, b._h, ptr, total, None, None) == 0
        assert np.array_equal(read(), want)
    finally:
        if dev:
            hip.hipFree(dev)
        b.close()


def test_one_context_with_the_map_off_on_and_off_again():
    """One context over batches of changing shape: the switch holds for the corrections that follow it, a correction
    without the map leaves none behind (TALC_ERR_STATE), also on a batch that had one."""
    s = M.map_set("default")
    ctx = ctx_of(s)
    L = T.lib()
    shapes = [(0, 50), (50, 200), (10, 13), (0, 120)]
    for lo, hi in shapes:
        bases, offs = PU.pack_reads(s.reads[lo:hi])
        off = run(ctx, bases, offs, False)
        on = run(ctx, bases, offs, True)
        same_records(on, off)
        check_against(on, s.exp[lo:hi], "shape %d..%d" % (lo, hi))
    bases, offs = PU.pack_reads(s.reads[:30])
    b = ctx.batch(bases, offs)
    try:
        b.correct()                                  # off
        with pytest.raises(T.TalcError, match="-6"):
            b.fetch_map()
        with pytest.raises(T.TalcError, match="-6"):
            b.fetch_corrected(soft_mask=True)
        ctx.record_map(True)
        b.correct()
        segs, so = b.fetch_map()
        assert int(so[-1]) == sum(len(e["segs"]) for e in s.exp[:30])
        ctx.record_map(False)
        b.correct()                                  # the same batch again, without
        assert b.n_segments == 0
        assert L.talc_batch_fetch_map(ctx._h, b._h, None, 0, so.ctypes.data) == ERR_STATE
    finally:
        b.close()
        ctx.record_map(False)


def cli(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_cli_map_file_and_masked_records(tmp_path, rev):
    S = Synth(target_kmers=150_000, k=21, seed=77)
    S.write_dump(str(tmp_path / "sr.dump"))
    S.write_fasta(str(tmp_path / "reads.fa"), 0, 60)
    lines = (tmp_path / "reads.fa").read_text().splitlines()
    names, reads = [x[1:] for x in lines[0::2]], lines[1::2]
    if rev:   # (k-mers are directional: -rev corrects the reads of the opposite strand)
        reads = [M.revcomp(r) for r in reads]
        (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, reads)))
    pair = PU.Pair(target_kmers=150_000, k=21, seed=77, reverse=int(rev))
    exp = [M.expected(pair.otab, r) for r in reads]
    assert sum(e["status"] == 0 for e in exp) >= 50
    args = [str(tmp_path / "reads.fa"), "-k", "21", "-SR", str(tmp_path / "sr.dump")] + (["-rev"] if rev else [])
    a = cli(TALC, args + ["--corr-map", "--soft-mask", "--batch-reads", "7", "-o", "gpu"], tmp_path)
    assert a.returncode == 0, a.stderr.decode()
    want_tsv = [l for n, e in zip(names, exp) for l in M.tsv_lines(n, e)]
    assert (tmp_path / "gpu.map.tsv").read_text().splitlines() == want_tsv
    assert any(l.split("\t")[1] == "R" for l in want_tsv) and any(len(e["segs"]) > len(M.tsv_lines("x", e)) for e in exp)
    want_fa = []
    for n, e in zip(names, exp):
        m = M.masked(e)
        want_fa += [">" + n] + [m[p:p + 70] for p in range(0, len(m), 70)]
    assert (tmp_path / "gpu.fa").read_text().splitlines() == want_fa
    # without the two options: the reference driver's files, and no map file
    p = cli(TALC, args + ["--batch-reads", "7", "-o", "plain"], tmp_path)
    b = cli(TALC_REF, args + ["-o", "ref", "-t", "8"], tmp_path)
    assert p.returncode == 0 and b.returncode == 0, (p.stderr.decode(), b.stderr.decode())
    for ext in (".fa", ".log", ".stats_basics.txt"):
        fp, fr = tmp_path / ("plain" + ext), tmp_path / ("ref" + ext)
        assert fp.exists() == fr.exists() and (not fp.exists() or fp.read_bytes() == fr.read_bytes()), ext
    assert (tmp_path / "plain.config.txt").read_bytes().replace(b"plain", b"ref") == (tmp_path / "ref.config.txt").read_bytes()
    assert (tmp_path / "gpu.config.txt").read_bytes().replace(b"gpu", b"ref") == (tmp_path / "ref.config.txt").read_bytes()
    assert (tmp_path / "gpu.fa").read_text().upper() == (tmp_path / "plain.fa").read_text().upper()
    assert not (tmp_path / "plain.map.tsv").exists()
