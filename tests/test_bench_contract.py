"""The bench.py output contract (one JSON line), checked on the line committed from the last GPU run of the round
(profiles/r02_h_bench_full.json) and on bench.py's own source (metric / config strings = BASELINE.json's)."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_fields():
    line = json.load(open(os.path.join(ROOT, "profiles", "r02_h_bench_full.json")))
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in line, k
    # (lines committed before the metric string was read from BASELINE.json spell the multiplication sign and the arrow in ASCII)
    norm = lambda t: t.replace("\u00d7", " x ").replace("\u2192", "->").replace("  ", " ")
    assert norm(line["metric"]) == norm(base["metric"]) and line["unit"] == "scans/s"
    import bench
    assert bench.baseline_metric() == base["metric"]
    assert line["n_gpus"] == 1 and line["higher_is_better"] is True and line["scaling"] == "weak" and line["vs_baseline"] is None
    assert line["dtype"] == "f64" and line["data"] == "synthetic" and "configs[1]" in line["config"]["workload"]
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]  # whole-job throughput = steps / timed region
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) < 1e-6 * r["achieved"]
    c = line["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["unit"] == line["unit"]
    # the extras the round-1 verdict asked for
    for k in ("configs", "mapping_mode", "inclusive_h2d", "pose_err_vs_oracle", "c5_batch"):
        assert k in line, k
    assert set(line["configs"]) == {"configs[0]", "configs[2]", "configs[3]"}
    assert line["c5_batch"]["jobs"] == 512 and line["c5_batch"]["converged_jobs"] == 512 and line["c5_batch"]["distinct_poses"] == 512
    assert line["pose_err_vs_oracle"]["dt_m"] < 1e-4 and line["pose_err_vs_oracle"]["dR_rad"] < 1e-4 and line["pose_err_vs_oracle"]["same_iterations"]


def test_bare_gpus_n_launches_its_own_ranks_and_fails_loudly_without_gpus():
    """`python bench.py --gpus 2` WITHOUT a launcher must start two ranks itself (torch.distributed.run) and, on this
    GPU-less box, exit non-zero -- never fall back to a quiet single-process run.  (The GPU box runs the same command to completion:
    tests/test_gpu_batch_ranks.py::test_bare_bench_gpus_2_reports_two_ranks.)"""
    import subprocess
    import sys

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["FLS_BENCH_SHARE_DEVICE"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--no-extras",
                        "--no-cpu-baseline", "--no-batch"], env=env, capture_output=True, text=True, timeout=600)
    assert "starting 2 ranks through torch.distributed.run" in p.stderr, p.stderr[-2000:]
    import torch
    if not torch.cuda.is_available():
        assert p.returncode != 0, "no GPU here: the ranks must fail loudly"
        assert '"n_gpus": 1' not in p.stdout


def test_launcher_rank_count_must_match_gpus_flag():
    """A launcher that started a different number of ranks than --gpus says is refused (rc 2), whatever the hardware."""
    import subprocess
    import sys

    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--no-batch", "--no-extras", "--no-cpu-baseline"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "refusing to run" in p.stderr, (p.returncode, p.stderr[-1000:])


def test_steps_below_one_is_refused():
    """--steps is the number of timed steps and ms_per_step divides by it: zero or fewer is an argument error, before anything touches a GPU."""
    import subprocess
    import sys

    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--no-batch", "--no-extras", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, (p.returncode, p.stderr[-1000:])


@pytest.mark.gpu
def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the pose, status and fls_stats fields of the last timed step as float64 .npy files; the line's steps / ms_per_step
    describe exactly the K timed steps asked for, and the dumped result is the one the line compares with the CPU oracle."""
    import subprocess
    import sys

    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-batch", "--no-extras",
                        "--no-cpu-baseline", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    files = {f.name: np.load(f) for f in out.iterdir()}
    assert {"pose.npy", "converged.npy", "stats_iterations.npy", "stats_n_valid.npy", "stats_sum_res.npy", "stats_last_dx.npy"} <= set(files)
    assert all(a.dtype == np.float64 for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64 << 20
    T = files["pose.npy"]
    assert T.shape == (4, 4) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) and np.allclose(T[:3, :3].T @ T[:3, :3], np.eye(3), atol=1e-9)
    assert files["stats_iterations.npy"][0] == line["config"]["gn_iterations"] and bool(files["converged.npy"][0]) == line["config"]["converged"]
    same = line["pose_err_vs_oracle"]["timed_step_vs_oracle_same_call_index"]
    assert same["dt_m"] < 1e-4 and same["dR_rad"] < 1e-4 and same["same_n_valid"]


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_computes_what_full_computes(tmp_path):
    """Without --full the line carries the headline only (no roofline, oracle comparison, configs, batch legs or CPU baselines), and the
    last timed step returns bit for bit what it returns in a --full run: the legs --full adds run after the timed steps."""
    import subprocess
    import sys

    lines, dumps = [], []
    for extra in ([], ["--full", "--no-batch", "--no-extras", "--no-cpu-baseline"]):
        out = tmp_path / ("full" if extra else "plain")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *extra,
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        got = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(got) == 1, p.stdout[-2000:]
        lines.append(json.loads(got[0]))
        dumps.append({f.name: np.load(f) for f in out.iterdir()})
    plain, full = lines
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "legs"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["higher_is_better"] is True and plain["dtype"] == "f64" and plain["unit"] == "scans/s"
    assert abs(plain["value"] - 1e3 / plain["ms_per_step"]) < 1e-6 * plain["value"]
    assert list(plain)[-1] == "legs" and "headline_us" in plain["legs"]
    for k in ("roofline", "roofline_fit_kernel", "pose_err_vs_oracle", "configs", "mapping_mode", "loop_closure", "inclusive_h2d", "c5_batch",
              "c5_batch_native", "cpu_baseline", "cpu_baseline_ref"):
        assert k not in plain, k
    assert "roofline" in full and "pose_err_vs_oracle" in full
    assert set(dumps[0]) == set(dumps[1]) and all(np.array_equal(dumps[0][n], dumps[1][n]) for n in dumps[0])
    assert plain["config"]["gn_iterations"] == full["config"]["gn_iterations"]
