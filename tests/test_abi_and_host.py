"""CPU-side checks of the product boundary: the C-ABI library loads without a GPU, exports every
symbol include/talc_hip.h declares, fails loudly (no CPU fallback) when asked to compute, and
its host-side table builder agrees with the oracle's table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
from talc_amd import lib as T
from talc_amd.synth import Synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "talc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(talc_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no prototypes found in the header"
    L = T.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert set(T.ABI_SYMBOLS) == declared
    assert L.talc_abi_version() == 1
    # every call is bound with as many arguments as its prototype takes ((void): none), so ctypes refuses a wrong arity
    protos = re.findall(r"\b(talc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)
    assert {name for name, _ in protos} == declared
    wrong = {}
    for name, params in protos:
        want = 0 if params.strip() == "void" else params.count(",") + 1
        bound = getattr(L, name).argtypes
        if bound is None or len(bound) != want:
            wrong[name] = (want, bound)
    assert not wrong, wrong


def test_environment_is_read_in_one_place_and_documented():
    """talc_switches.h is the one file of the native sources that reads the environment, and the switches it reads are
    exactly the ones INTEGRATION.md "Library switches" lists (one list item per switch, its name first)."""
    csrc = os.path.join(ROOT, "talc_amd", "csrc")
    readers = sorted(f for f in os.listdir(csrc) if "getenv" in open(os.path.join(csrc, f), errors="replace").read())
    assert readers == ["talc_switches.h"]
    read = set(re.findall(r'"(TALC_[A-Z0-9_]+)"', open(os.path.join(csrc, "talc_switches.h")).read()))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc.split("## Library switches", 1)[1].split("\n## ", 1)[0]
    listed = set(re.findall(r"^- `(TALC_[A-Z0-9_]+)`", section, flags=re.M))
    assert read and read == listed, (sorted(read - listed), sorted(listed - read))


def test_device_memory_has_one_owner_and_one_way_to_fail():
    """talc_devmem.h is the one file of the native sources that allocates or frees device and page-locked memory (its
    owners' destructors give it back, so a failing call returns where it stands), and the C ABI layer has no other
    error idiom left beside HIPCHK: no local checking macros, no cleanup lambdas, no chains of `e == hipSuccess`."""
    csrc = os.path.join(ROOT, "talc_amd", "csrc")
    text = {f: open(os.path.join(csrc, f), errors="replace").read() for f in os.listdir(csrc)}
    calls = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(")
    users = sorted(f for f, t in text.items() if any(c in t for c in calls))
    assert users == ["talc_devmem.h"]
    layer = sorted(f for f in text if f == "talc_capi.hip" or (f.startswith("talc_capi_") and f.endswith(".inc")))
    assert len(layer) >= 5 and "talc_capi_counter.inc" in layer
    for f in layer:
        for idiom in ("BCHK", "CCHK", "auto cleanup", "auto drop", "== hipSuccess) e ="):
            assert idiom not in text[f], (f, idiom)


def test_poison_hooks_are_exported_and_take_only_what_the_header_allows():
    L = T.lib()
    for sym in ("talc_test_set_poison", "talc_test_get_poison", "talc_test_guard_report", "talc_test_cache_reuses", "talc_test_guard_selftest"):
        assert hasattr(L, sym) and sym in T.ABI_SYMBOLS, sym
    assert T.poison_setting() == (-1, 0)
    for byte, guard in ((-2, 0), (256, 256), (0, 100), (0, 255), (0, (1 << 20) + 256)):
        assert L.talc_test_set_poison(byte, guard) == -1 and T.poison_setting() == (-1, 0), (byte, guard)      # TALC_ERR_INVALID
    before = T.guard_report()
    try:
        assert L.talc_test_set_poison(0xA5, 512) == 0 and T.poison_setting() == (0xA5, 512)
        assert L.talc_test_set_poison(0, 0) == 0 and T.poison_setting() == (0, 0)                              # poison without red zones
    finally:
        assert L.talc_test_set_poison(-1, 4096) == 0
    assert T.poison_setting() == (-1, 0) and T.guard_report() == before


def test_alloc_failure_hooks_are_exported_refuse_unknown_kinds_and_report_without_a_device():
    L = T.lib()
    for sym in ("talc_test_fail_alloc", "talc_test_alloc_report"):
        assert hasattr(L, sym) and sym in T.ABI_SYMBOLS, sym
    assert L.talc_test_alloc_report(None) == -1
    before = T.alloc_report()
    assert before["kinds"] == 0                                  # off
    for kinds, skip, count, real in ((4, 0, 1, 0), (7, 0, 0, 0), (1, -1, 1, 0), (1, 0, 1, 2)):
        assert L.talc_test_fail_alloc(kinds, skip, count, real) == -1 and T.alloc_report() == before, (kinds, skip, count, real)   # TALC_ERR_INVALID
        assert L.talc_last_error()
    try:
        assert L.talc_test_fail_alloc(3, 5, 2, 1) == 0
        armed = T.alloc_report()
        assert armed == dict(device=0, pinned=0, injected=0, owner=0, bytes=0, runtime_code=0, live=before["live"], kinds=3)
    finally:
        assert L.talc_test_fail_alloc(0, 0, 0, 0) == 0
    assert T.alloc_report()["kinds"] == 0
    with pytest.raises(ZeroDivisionError):                        # the context manager switches off when its body raises
        with T.failing_allocs(T.KIND_PINNED, 0, 1):
            assert T.alloc_report()["kinds"] == 2
            1 // 0
    assert T.alloc_report()["kinds"] == 0
    with pytest.raises(T.TalcError) as e:                         # a setting the library refuses switches nothing on
        with T.failing_allocs(4, 0, 1):
            pass
    assert e.value.code == -1 and T.alloc_report()["kinds"] == 0


def test_retry_report_hook_is_exported_and_refuses_null_arguments():
    L = T.lib()
    assert hasattr(L, "talc_test_retry_report") and "talc_test_retry_report" in T.ABI_SYMBOLS
    out = np.zeros(4, dtype=np.uint32)
    assert L.talc_test_retry_report(None, out.ctypes.data) == -1 and L.talc_last_error()      # TALC_ERR_INVALID


def test_every_owner_must_have_its_result_looked_at(tmp_path):
    """The five allocating calls of talc_devmem.h are [[nodiscard]], and the library's build makes a dropped result an error:
    -Wno-unused-value, which the build passes, silences -Wunused-result too, so -Werror=unused-result stands behind it.  A
    two-line program that drops such a result is refused by the build's own flags, and compiles once it looks at it."""
    import subprocess
    from talc_amd import build as B
    text = open(os.path.join(ROOT, "talc_amd", "csrc", "talc_devmem.h")).read()
    assert len(re.findall(r"\[\[nodiscard\]\] hipError_t (alloc|ensure)\(", text)) == 5
    flags = [f for f in B.hip_command(str(tmp_path / "unused.so")) if f.startswith("-W")]
    assert "-Werror=unused-result" in flags and flags.index("-Werror=unused-result") > flags.index("-Wno-unused-value"), flags
    src = tmp_path / "drop.hip"
    for body, ok in (("f();", False), ("return f();", True)):
        src.write_text("[[nodiscard]] int f() { return 0; }\nint main() { %s }\n" % body)
        r = subprocess.run([B.HIPCC, "--offload-arch=" + B.ARCH, "-std=c++17", "-fsyntax-only", *flags, str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert (r.returncode == 0) == ok, (body, r.stdout.decode()[-600:])
        assert ok or b"unused-result" in r.stdout, r.stdout.decode()[-600:]


def test_poisoned_switches_off_again_when_its_body_raises():
    assert T.poison_setting() == (-1, 0)
    with pytest.raises(ZeroDivisionError):
        with T.poisoned(0xFF):
            assert T.poison_setting() == (0xFF, 256)
            1 // 0
    assert T.poison_setting() == (-1, 0)
    with T.poisoned(0x35, guard=1024):
        assert T.poison_setting() == (0x35, 1024)
    assert T.poison_setting() == (-1, 0)
    with pytest.raises(T.TalcError):                     # a setting the library refuses switches nothing on
        with T.poisoned(300):
            pass
    assert T.poison_setting() == (-1, 0)


def test_params_default_match_reference_defaults():
    p = T.default_params()
    q = O.params()
    for f in PU.PARAM_FIELDS:
        assert getattr(p, f) == getattr(q, f), f
    # main.cpp:115-116,142-183 / Explorer.cpp:85-97 / Jellyfish.cpp:64 / Read.cpp:361
    assert (p.k, p.min_count, p.alpha, p.window_size, p.sr_error_rate) == (21, 2, 2.57, 9, 0.025)
    assert (p.min_inner_score, p.min_border_score, p.max_nb_competing_paths) == (0.7, 0.7, 7)
    assert (p.min_start_anchors, p.max_start_anchors, p.max_in_count) == (3, 5, 100000)
    assert (p.max_nb_border_paths, p.max_nb_inner_paths, p.check_interval) == (75, 50, 6)
    assert (p.allowed_failure_rate, p.max_nb_border_failures, p.coloured_count_thr, p.max_border_length) == (0.3, 3, 10000, 500)


def test_invalid_parameters_are_rejected():
    for kw in (dict(k=17), dict(k=32), dict(min_count=0), dict(coloured_count_thr=70000)):
        p = T.default_params(**kw)
        with pytest.raises(T.TalcError):
            T.Table.from_arrays(np.zeros(1, np.uint64), np.ones(1, np.uint32), p)


@pytest.mark.parametrize("field,top", [("max_nb_competing_paths", 64), ("max_nb_inner_paths", 60), ("max_start_anchors", 64)])
def test_path_search_parameters_are_accepted_up_to_what_the_scratch_holds(field, top):
    """The three parameters that size k_search's per-wave scratch (a ballot of 64 lanes, TCAP slots, the aim lists): the
    largest value is accepted, the one above it and 0 are refused, and the message names the field."""
    one = (np.zeros(1, np.uint64), np.ones(1, np.uint32))
    for good in (1, top):
        T.Table.from_arrays(*one, T.default_params(**{field: good})).close()
    for bad in (0, top + 1, 0xFFFFFFFF):
        with pytest.raises(T.TalcError, match=field):
            T.Table.from_arrays(*one, T.default_params(**{field: bad}))


def test_refusals_name_the_field_and_unbounded_parameters_pass():
    one = (np.zeros(1, np.uint64), np.ones(1, np.uint32))
    for k in (17, 32):
        with pytest.raises(T.TalcError, match="k=%d" % k):
            T.Table.from_arrays(*one, T.default_params(k=k))
    with pytest.raises(T.TalcError, match="check_interval"):
        T.Table.from_arrays(*one, T.default_params(check_interval=0))
    # no upper bound: the border limit and the check interval (tests/param_limit_cases.py runs the search with 300 and 50);
    # min_start_anchors above max_start_anchors is a legal pair too
    T.Table.from_arrays(*one, T.default_params(max_nb_border_paths=1 << 30, check_interval=1 << 30, min_start_anchors=63, max_start_anchors=1)).close()


@pytest.mark.skipif(PU.T.device_count() > 0, reason="only meaningful on a host without a GPU")
def test_compute_fails_loudly_without_gpu():
    p = T.default_params()
    t = T.Table.from_arrays(np.arange(10, dtype=np.uint64), np.full(10, 5, np.uint32), p)
    with pytest.raises(T.TalcError):
        t.upload(0)
    with pytest.raises(T.TalcError):
        T.Context(t, p, 0)          # table not uploaded / no device: no silent CPU path
    with pytest.raises(T.TalcError):
        t.lookup(np.arange(3, dtype=np.uint64))


def test_host_table_equals_oracle_table_incl_duplicates_and_filter():
    rng = np.random.default_rng(3)
    p, q = PU.both_params(k=21)
    keys = rng.integers(0, 1 << 42, 50_000, dtype=np.uint64)
    counts = rng.integers(0, 40, 50_000).astype(np.uint32)       # some below MIN_COUNT
    # duplicates with different counts: the first line wins (std::map::insert, Jellyfish.cpp:262)
    keys = np.concatenate([keys, keys[:5000]])
    counts = np.concatenate([counts, (counts[:5000] + 7).astype(np.uint32)])
    ot = O.OracleTable(q, O.OracleTable.MAP)
    ot.insert_packed(keys, counts)
    tt = T.Table.from_arrays(keys, counts, p)
    assert len(ot) == len(tt)
    probe = np.concatenate([keys, rng.integers(0, 1 << 42, 20_000, dtype=np.uint64)])
    oc, oj = ot.lookup_packed(probe)
    tc, tj = tt.lookup_host(probe)
    assert (oc == tc).all() and (oj == tj).all()


def test_host_table_junction_colouring_and_decolouring():
    p, q = PU.both_params(k=21, use_junctions=1)
    S = Synth(target_kmers=60_000, k=21, seed=5)
    keys, counts = S.dump_arrays()
    jk, jc = S.junction_arrays()
    # add reverse-complement-only junction entries and homopolymers
    hom = np.array([0, (1 << 42) - 1, int("01" * 21, 2), int("10" * 21, 2)], dtype=np.uint64)
    keys = np.concatenate([keys, hom])
    counts = np.concatenate([counts, np.full(4, 50, np.uint32)])
    jk = np.concatenate([jk, hom])
    jc = np.concatenate([jc, np.full(4, 77, np.int64)])
    ot = O.OracleTable(q, O.OracleTable.MAP)
    ot.insert_packed(keys, counts)
    ot.colour_packed(jk, jc)
    ot.decolour()
    tt = T.Table.from_arrays(keys, counts, p)
    tt.colour(jk, jc)
    tt.decolour_repeats()

    def rc(km):
        r = 0
        for _ in range(21):
            r = (r << 2) | (3 - (km & 3))
            km >>= 2
        return r
    probe = np.concatenate([keys, jk, np.array([rc(int(x)) for x in jk[:2000]], dtype=np.uint64)])
    oc, oj = ot.lookup_packed(probe)
    tc, tj = tt.lookup_host(probe)
    assert (oc == tc).all() and (oj == tj).all()
    assert (oj > 0).sum() > 100                 # colours were applied
    assert (oj[len(keys) - 4:len(keys)] == 0).all()   # homopolymers un-coloured (utils.cpp:658-669)
    assert (oj < 10000).all()                   # colouredCountThr (Jellyfish.cpp:64,284)


def test_table_from_dump_files_matches_oracle(tmp_path):
    S = Synth(target_kmers=30_000, k=21, seed=6)
    dump, jd = str(tmp_path / "sr.dump"), str(tmp_path / "j.dump")
    S.write_dump(dump)
    S.write_junctions(jd)
    with open(dump, "a") as f:      # malformed / odd lines the reference tolerates
        f.write("ACGTNACGTACGTACGTACGT 9\n")    # N k-mer: never matchable by an ACGT read k-mer
        f.write("acgtacgtacgtacgtacgta 12\n")   # lower case is accepted by Dna5
        f.write("ACGT 5\n")                     # wrong length
        f.write("lonely\n")                     # one token: 'Error when building dBG...'
        f.write("\n")                           # blank line
        f.write("  GATTACAGATTACAGATTACA\t\t 41  trailing words\r\n")   # tabs, leading blanks, CRLF, extra tokens
        f.write("TTTTACAGATTACAGATTACA 7x\n")    # atoi stops at the first non-digit: 7
        f.write("CCCCACAGATTACAGATTACA +3\n")    # explicit sign
        f.write("AAAAACAGATTACAGATTACA 5")       # last line without a newline
    p, q = PU.both_params(k=21, use_junctions=1)
    ot = O.OracleTable(q, O.OracleTable.MAP)
    st_o = ot.build_from_files(dump, jd)
    tt = T.Table.from_files(dump, jd, p)
    assert tt.build_stats[0] == st_o[0] and tt.build_stats[1] == st_o[1]
    keys, counts = S.dump_arrays(release=False)
    lower = np.array([int("".join({"a": "00", "c": "01", "g": "10", "t": "11"}[c] for c in "acgtacgtacgtacgtacgta"), 2)], dtype=np.uint64)
    probe = np.concatenate([keys, lower])
    oc, oj = ot.lookup_packed(probe)
    tc, tj = tt.lookup_host(probe)
    assert (oc == tc).all() and (oj == tj).all()
    assert tc[-1] == 12
    def pk(t):
        return np.array([int("".join({"A": "00", "C": "01", "G": "10", "T": "11"}[c] for c in t), 2)], dtype=np.uint64)
    for text, want in (("GATTACAGATTACAGATTACA", 41), ("TTTTACAGATTACAGATTACA", 7), ("CCCCACAGATTACAGATTACA", 3),
                       ("AAAAACAGATTACAGATTACA", 5)):
        assert tt.lookup_host(pk(text))[0][0] == want == ot.lookup_packed(pk(text))[0][0], text
    # the oracle's map also holds the two unmatchable keys (N k-mer, short k-mer)
    assert len(ot) == len(tt) + 2


def test_synth_is_deterministic_and_sharded():
    a = Synth(target_kmers=40_000, k=21, seed=9)
    b = Synth(target_kmers=40_000, k=21, seed=9)
    ka, ca = a.dump_arrays()
    kb, cb = b.dump_arrays()
    assert (ka == kb).all() and (ca == cb).all()
    ba, oa = a.reads(0, 50)
    b1, o1 = b.reads(0, 20)
    b2, o2 = b.reads(20, 30)        # any rank can generate its own shard
    assert bytes(ba) == bytes(b1) + bytes(b2)
    assert (ca == 1).sum() > 0 and (ca >= 2).sum() > 30_000
    lens = np.diff(oa.astype(np.int64))
    assert lens.max() < 6000 and lens.mean() > 500


def test_bench_workload_is_derived_from_its_arguments():
    """bench.py names the workload it really ran: N = 1 is BASELINE config 2, N > 1 config 3 (the same 1 M reads for
    every N: strong scaling), --config forces one, and any overridden figure turns the label into "custom"."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    w1 = bench.resolve_workload(bench.parse([]), 1)
    assert (w1["config"], w1["reads"], w1["kmers"], w1["k"]) == (2, 100_000, 50_000_000, 21) and w1["label"].startswith("config2:")
    for n in (2, 4, 8):
        w = bench.resolve_workload(bench.parse(["--gpus", str(n)]), n)
        assert (w["config"], w["reads"], w["kmers"], w["k"], w["junctions"]) == (3, 1_000_000, 200_000_000, 21, False)
        assert w["label"].startswith("config3:") and "over %d GPU" % n in w["label"]
    w4 = bench.resolve_workload(bench.parse(["--config", "4"]), 1)
    assert w4["junctions"] and w4["label"].startswith("config4:") and "junction" in w4["label"]
    w5 = bench.resolve_workload(bench.parse(["--config", "5"]), 1)
    assert (w5["k"], w5["kmers"], w5["mixed"]) == (31, 500_000_000, True) and "20 kb" in w5["label"]
    wk = bench.resolve_workload(bench.parse(["--k", "31", "--reads", "5000"]), 1)
    assert wk["label"].startswith("custom (config2 with reads, k changed)") and wk["k"] == 31 and wk["reads"] == 5000
    assert "config2:" not in wk["label"]
