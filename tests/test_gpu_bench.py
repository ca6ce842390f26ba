"""bench.py on the device: a plain run's `--dump-outputs` holds what its timed solve computed — the same arrays a
direct solve of the same seeded inputs returns (the line's `steps` outer iterations, the headline's parameters)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ilqgames_amd import abi, examples

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs_are_the_timed_solve(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import bench
    from ilqgames_amd import hip
    B, steps = 64, 3
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--batch", str(B), "--dump-outputs", str(d)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["dtype"] == "f64"
    assert "cpu_baseline" not in out and "configs" not in out  # --full only
    dumped = {k: np.load(d / (k + ".npy")) for k in bench.DUMP_ARRAYS + ("instances",)}
    assert np.array_equal(dumped["instances"], np.arange(B))
    spec, _ = bench._bench_spec(examples, bench.HEADLINE_CONFIG)
    res = hip.Problem(spec, abi.F64).solve(examples.jittered_x0(spec, B, seed=0), fixed_iters=steps)
    for k in bench.DUMP_ARRAYS:
        assert np.array_equal(dumped[k], res[k].cpu().numpy().astype(dumped[k].dtype)), k
    assert np.all(dumped["iters"] == steps)


def test_bench_steps_beyond_the_solvers_iteration_bound(tmp_path):
    """A plain run whose --steps and --warmup exceed what one solve may run (the headline's max_solver_iters = 100:
    102 rounds on the asynchronous launch sequence) times them as solves of 20 and dumps the last one."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import bench
    from ilqgames_amd import hip
    B, steps = 64, 250
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "130",
           "--batch", str(B), "--dump-outputs", str(d)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == steps and out["success_fraction"] == 1.0
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 * steps - B * steps) < 1e-6 * B * steps
    spec, _ = bench._bench_spec(examples, bench.HEADLINE_CONFIG)
    res = hip.Problem(spec, abi.F64).solve(examples.jittered_x0(spec, B, seed=0), fixed_iters=20)
    for k in bench.DUMP_ARRAYS:
        assert np.array_equal(np.load(d / (k + ".npy")), res[k].cpu().numpy().astype(np.float64)), k
