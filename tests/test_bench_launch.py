"""bench.py's launch contract (no GPU needed): `--gpus N` started plainly launches N ranks itself before any GPU
call and fails -- never silently runs fewer ranks; a WORLD_SIZE that contradicts --gpus is an error."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _has_gpu():
    import torch
    return torch.cuda.device_count() > 0


def test_world_size_contradicting_gpus_is_an_error():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8"], env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr and r.stdout.strip() == ""


@pytest.mark.skipif(_has_gpu(), reason="on a GPU box the gpu-marked test covers the self-launch")
def test_plain_start_with_gpus_2_fails_loudly_without_gpus():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1"], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "no fallback to fewer ranks" in r.stderr
    assert r.stdout.strip() == ""                        # no result line was printed
    # with the device-count check waived the launcher starts both ranks; each fails (no GPU), nothing falls back
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env=_env(RH_BENCH_SHARE_GPU0="1", RH_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "rank exit codes" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
def test_self_launch_on_one_gpu_box(tmp_path):
    """One GPU: `--gpus 2` must fail (rank 1 has no GPU); with the two ranks sharing GPU 0 over gloo the script launches
    itself and reports n_gpus = 2 and rccl_ranks_seen = 2."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("more than one GPU here")
    small = ["--steps", "3", "--warmup", "1", "--prewarm-ms", "0", "--workload", "cfg2", "--no-cpu", "--no-e2e", "--no-cfg2", "--no-cfg5",
             "--detail-out", str(tmp_path / "detail.json")]
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + small, env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "no fallback" in r.stderr and r.stdout.strip() == ""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + small, env=_env(RH_BENCH_SHARE_GPU0="1", RH_BENCH_BACKEND="gloo"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) < 4096
    line = json.loads(last)
    assert json.load(open(tmp_path / "detail.json"))["n_gpus"] == 2     # the full document went to the side file
    assert line["n_gpus"] == 2 and line["rccl_ranks_seen"] == 2 and line["config"]["candidates_per_step"] == 8192


def test_plain_and_full_options_parse():
    """--steps sets the timed steps and must be >= 1; --full and --dump-outputs are off unless given."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_bench_mod", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    a = b.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = b.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        b.parse(["--steps", "0"])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_counts(tmp_path):
    """A plain run prints the headline keys without the --full legs and writes the last timed step's counts and nothing
    else (a read-only checkout must do); the same arguments give the same counts (seeded inputs), and --oracle-check holds
    the dumped counts against the oracle."""
    import numpy as np
    detail = os.path.join(ROOT, "bench_detail.json")
    before = os.stat(detail).st_mtime_ns if os.path.exists(detail) else None
    base = ["--workload", "cfg2", "--warmup", "2"]
    lines = []
    for k, extra in enumerate((["--steps", "5", "--oracle-check", "64"], ["--steps", "3"])):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dump-outputs", str(tmp_path / ("d%d" % k))] + base + extra,
                           env=_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for line, steps in zip(lines, (5, 3)):
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["metric"] == "candidates_scored_per_sec"
        assert line["value"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["roofline"]["kernel"] is None and line["cpu_baseline"] is None and "masks_ms" not in line
        assert "detail" not in line
    assert (os.stat(detail).st_mtime_ns if os.path.exists(detail) else None) == before
    assert lines[0]["oracle_checked"] == 64
    c0, c1 = (np.load(tmp_path / ("d%d" % k) / "counts.npy") for k in (0, 1))
    assert c0.dtype == np.float64 and c0.shape == (4096,) and np.array_equal(c0, np.round(c0)) and c0.sum() > 4096 * 100
    assert np.array_equal(c0, c1)
