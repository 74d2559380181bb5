"""`bench.py --gpus N` is the path's parallelism switch, as `-t N` is the reference's (main.cpp:242,247): without a
launcher it starts its own N ranks from a process that stays off the GPU, relays rank 0's one JSON line and returns the
children's worst exit code; under a launcher whose WORLD_SIZE disagrees with --gpus it refuses to run."""
import importlib.util
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod_launch", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def test_world_size_that_differs_from_gpus_is_refused():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "1", "--warmup", "0"], env=_clean_env(WORLD_SIZE="2", RANK="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2 and p.stdout == b"" and b"--gpus 4 but WORLD_SIZE=2" in p.stderr
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "1", "--warmup", "0"], env=_clean_env(WORLD_SIZE="8", RANK="3"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2 and p.stdout == b""


def test_launcher_starts_n_ranks_and_relays_rank0s_line(tmp_path, capfd):
    """The launcher itself, with a stand-in for the rank program: N children with RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_ADDR = 127.0.0.1 / one MASTER_PORT, the arguments passed through, only rank 0's stdout relayed."""
    bench = _bench_module()
    script = ("import os, sys, json\n"
              "r = int(os.environ['RANK'])\n"
              "open(os.path.join(%r, 'rank%%d' %% r), 'w').write(json.dumps({k: os.environ.get(k) for k in "
              "('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')} | {'argv': sys.argv[1:]}))\n"
              "print('noise from rank %%d' %% r if r else json.dumps({'n_gpus': int(os.environ['WORLD_SIZE'])}))\n") % str(tmp_path)
    argv = ["--gpus", "3", "--steps", "1"]
    rc = bench.launch_ranks(bench.parse(argv), argv, child=[sys.executable, "-c", script])
    out = capfd.readouterr()
    assert rc == 0
    assert out.out.strip().splitlines() == ['{"n_gpus": 3}']
    seen = [json.load(open(tmp_path / ("rank%d" % r))) for r in range(3)]
    assert [s["RANK"] for s in seen] == ["0", "1", "2"] and [s["LOCAL_RANK"] for s in seen] == ["0", "1", "2"]
    assert all(s["WORLD_SIZE"] == "3" and s["MASTER_ADDR"] == "127.0.0.1" and s["argv"] == argv for s in seen)
    assert len({s["MASTER_PORT"] for s in seen}) == 1


def test_launcher_returns_the_worst_code_and_ends_the_survivors(capfd):
    """A rank that fails must not leave the others waiting in a collective: they are ended, the code is the failure's."""
    bench = _bench_module()
    script = ("import os, sys, time\n"
              "r = int(os.environ['RANK'])\n"
              "if r == 1: sys.exit(7)\n"
              "time.sleep(600)\n")
    argv = ["--gpus", "2"]
    t0 = time.time()
    rc = bench.launch_ranks(bench.parse(argv), argv, child=[sys.executable, "-c", script])
    assert rc == 7 and time.time() - t0 < 60
    assert capfd.readouterr().out == ""


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a GPU")
def test_bench_gpus_2_launches_its_own_ranks_rehearsal(tmp_path):
    """The command of the driver's N > 1 run, without torchrun, on the one-GPU box (TALC_BENCH_REHEARSAL=1: both ranks on
    device 0 over gloo): exactly one stdout line, n_gpus 2, every read of the workload gathered and merged on rank 0 (and
    dumped from there by --dump-outputs)."""
    import numpy as np
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--reads", "20000", "--kmers", "2000000", "--steps", "1", "--warmup", "0",
                        "--dump-outputs", str(tmp_path)],
                       env=_clean_env(TALC_BENCH_REHEARSAL="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["gathered_reads_on_rank0"] == 20000 and d["config"]["reads_total"] == 20000
    assert "own child ranks" in d["config"]["launched_by"] and "REHEARSAL" in d["data"]
    assert d["config"]["gather_host_reads_per_step_rank0"] == 2      # one host read per half-shard gather
    assert len(np.load(tmp_path / "status.npy")) == 20000 and len(np.load(tmp_path / "sample_reads.npy")) > 0


def test_dump_outputs_writes_the_records_as_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: every read's status, record offsets and record CRC-32, and a seeded sample of whole records, as
    float32 / float64 .npy files under the budget; the sample depends on the read indices and input lengths alone."""
    import zlib
    import numpy as np
    bench = _bench_module()
    args = bench.parse(["--gpus", "1"])
    assert args.full is False and args.dump_outputs is None
    assert bench.parse(["--full", "--dump-outputs", "d"]).full and bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"
    rng = np.random.default_rng(3)
    n = 3000
    in_len = rng.integers(200, 3000, n)
    rec_len = (in_len * rng.uniform(0.0, 1.3, n)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(rec_len)]).astype(np.uint64)
    records = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), int(offsets[-1]))
    status = rng.integers(0, 5, n).astype(np.int32)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 << 20)       # small enough that only a sample of records fits
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), records, offsets, status, in_len, lambda m: None)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"status", "offsets", "record_crc32", "sample_reads", "sample_records"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) - 128 for k in got) <= 2 << 20
    for k, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy")))
    assert np.array_equal(got["status"], status) and np.array_equal(got["offsets"], offsets.astype(np.float64))
    assert np.array_equal(got["record_crc32"], [zlib.crc32(records[int(offsets[i]):int(offsets[i + 1])]) for i in range(n)])
    sample = got["sample_reads"].astype(np.int64)
    assert 0 < len(sample) < n and np.all(np.diff(sample) > 0)
    want = np.concatenate([records[int(offsets[i]):int(offsets[i + 1])] for i in sample])
    assert np.array_equal(got["sample_records"], want.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a GPU")
def test_bench_plain_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain `bench.py --gpus 1` run: exactly --steps timed steps, the headline fields, none of the --full side legs;
    --dump-outputs of two runs with the same arguments holds the same records, and they agree with the line."""
    import numpy as np
    lines = []
    for d in ("a", "b"):
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--reads", "3000", "--kmers", "300000", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / d)], env=_clean_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        out = p.stdout.decode().strip().splitlines()
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "bases/s" and d["higher_is_better"] is True and d["dtype"] == "u8" and d["metric"].startswith("corrected")
    assert not {"cpu_baseline", "host_to_host", "paralog_workload", "end_to_end"} & set(d)
    names = ("status", "offsets", "record_crc32", "sample_reads", "sample_records")
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in names}
    for k in names:
        assert np.array_equal(a[k], np.load(tmp_path / "b" / (k + ".npy"))), k
    assert len(a["status"]) == 3000 and len(a["offsets"]) == 3001 and len(a["sample_reads"]) > 0
    hist = d["config"]["read_status_hist_rank0[corrected,short,no_solid,no_structure,error]"]
    assert np.bincount(a["status"].astype(np.int64), minlength=5).tolist() == hist
    s = a["sample_reads"].astype(np.int64)
    assert len(a["sample_records"]) == int((a["offsets"][s + 1] - a["offsets"][s]).sum())
