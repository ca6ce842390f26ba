"""The fused trial kernel's running reductions against the split passes' decision kernel, bit for bit.

A line-search trial of the fused kernel with a register-held static row stage leaves its per-row merit and cost
partials in LDS, the row wave carries the merit sum and the per-player totals (or extremes and their time steps) over
each chunk of rows it has finished, and only the last chunk is added behind the rollout (`partials_extend`,
csrc/ilqg_stages.hpp; `trial_part_instance`, csrc/ilqg_solve.hpp).  The split passes keep `merit_costs_reduce` over the
global partials: they are the reference here.  A sum cut at a row boundary and carried on is the same sequence of
additions, so nothing may move: xs, us, P, alpha, costs, iters, status and the solve state's back-track count are
compared with `np.array_equal`.

Horizons, for the layout of 64-row chunks (the kernels with running reductions take the chunk that is not full last,
the others first): 8 (one chunk, no prefix), 36, 64 (exactly one full chunk), 65 (a one-row chunk), 100 (64 + 36: the
headline), 129 (64 + 64 + 1: three chunks).  Every case asserts that the registered static structure still matches at
its horizon (`ILQG_SCHEDULE_STATIC_ROWS` on both sides) and that one side ran fused and the other split.  Which fused
kernels keep running reductions is a register-budget list (`fused_partials_room`, csrc/ilqg_solve.hpp): every fp32
kernel here, in fp64 the headline's shape; the fp64 cases of the other two scenes compare the unchanged path.

Scenes: the headline scene with the benchmark's line-search parameters; the reachability scene of baseline config 5
(max / min cost structures, `t_extreme`; its line search fails from the second iteration on, so the fused launch also
carries rejected trials); the n = 16 intersection with its own parameters, free-running with at most three back-tracking
steps and the hand-off switched off, so that rejected trials — costs held back, a second pass in the same launch, a line
search that gives up — stay inside the fused kernel.  There the split side runs without the speculative probes: the
sequential pass through `ilq_decide_kernel` is the form whose back-track count is defined the same way.

`forced_steps` keeps every pass in the fused kernel whatever `split_trial` says (the launcher), so that case compares
the static row stage (running reductions) with the interpreted one (`static_rows` off: `merit_costs_reduce`), which the
library documents as equal bit for bit.  The `resume` case starts the second solve from a carried merit value
(`sa.first == 2`)."""
import numpy as np
import pytest

from ilqgames_amd import abi, examples

pytestmark = pytest.mark.gpu

HORIZONS = [8, 36, 64, 65, 100, 129]
SCENES = ["modified_three_player_intersection", "three_player_collision_avoidance_reachability", "three_player_intersection"]
ARRAYS = ("xs", "us", "P", "alpha", "costs", "iters", "status")
B, K = 4, 3


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, cus = h.device_info()
    assert "gfx950" in name, name
    return h


def _spec(scene, T):
    spec = examples.CONFIGS[scene](T=T)
    if scene == "modified_three_player_intersection":  # bench.py's parameters for the headline
        spec.params.initial_alpha_scaling = 0.1
        spec.params.expected_decrease_fraction = 0.001
        spec.params.max_backtracking_steps = 100
    elif scene == "three_player_intersection":  # its own line search, cut short: rejected trials and a search that gives up
        spec.params.max_backtracking_steps = 3
        spec.params.max_solver_iters = 8
    return spec


def _x0(scene, spec):
    # (six instances from seed 3 for the free-running scene: at T = 100 the CPU oracle's line search gives up on two of them)
    return examples.jittered_x0(spec, 6, seed=3) if scene == "three_player_intersection" else examples.jittered_x0(spec, B, seed=7)


def _solve_kw(scene):
    """(keywords of the fused solve, keywords of the split solve)"""
    if scene == "three_player_intersection":
        return dict(split_trial=False, handoff=False), dict(split_trial=True, probe=False)
    return dict(split_trial=False, fixed_iters=K), dict(split_trial=True, fixed_iters=K)


def _run(hip, spec, dtype, x0, **kw):
    prob = hip.Problem(spec, dtype)
    bufs = prob.solve(x0 if dtype == abi.F64 else x0.astype(np.float32), **kw)
    out = {k: bufs[k].detach().cpu().numpy().copy() for k in ARRAYS}
    out["backtracks"] = prob.solve_state(bufs)["backtracks"].detach().cpu().numpy().copy()
    return out, prob.last_schedule(), prob, bufs


def _assert_equal(a, b, what):
    for k in ARRAYS + ("backtracks",):
        print(what, k, "equal" if np.array_equal(a[k], b[k], equal_nan=True) else "DIFFERENT")
    for k in ARRAYS + ("backtracks",):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("scene", SCENES)
def test_fused_running_reductions_equal_split_decision(hip, scene, T, dtype):
    spec = _spec(scene, T)
    x0 = _x0(scene, spec)
    kw_fused, kw_split = _solve_kw(scene)
    fused, sched_f, _, _ = _run(hip, spec, dtype, x0, **kw_fused)
    split, sched_s, _, _ = _run(hip, spec, dtype, x0, **kw_split)
    assert sched_f & abi.SCHEDULE_STATIC_ROWS and sched_s & abi.SCHEDULE_STATIC_ROWS, "the static structure no longer matches"
    assert not sched_f & abi.SCHEDULE_SPLIT_TRIAL and sched_s & abi.SCHEDULE_SPLIT_TRIAL
    print(scene, T, "iters", fused["iters"], "status", fused["status"], "backtracks", fused["backtracks"])
    _assert_equal(fused, split, "%s T=%d" % (scene, T))
    assert np.isfinite(fused["xs"]).all() and np.isfinite(fused["costs"]).all()


def test_rejected_trials_happen_inside_the_fused_launch(hip):
    """The free-running scene really exercises what it is there for: back-tracks in the fused kernel, and at least one
    instance whose line search gives up (status 0 with the last accepted iterate kept)."""
    spec = _spec("three_player_intersection", 100)
    x0 = _x0("three_player_intersection", spec)
    fused, sched, _, _ = _run(hip, spec, abi.F64, x0, **_solve_kw("three_player_intersection")[0])
    assert not sched & abi.SCHEDULE_SPLIT_TRIAL
    print("backtracks", fused["backtracks"], "status", fused["status"], "iters", fused["iters"])
    assert (fused["backtracks"] > 0).any() and (fused["status"] == 0).any()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_forced_steps_static_equals_interpreted(hip, dtype):
    spec = _spec("modified_three_player_intersection", 100)
    x0 = examples.jittered_x0(spec, B, seed=7)
    steps = np.tile(np.array([0.1, 0.05, 0.02]), (B, 1))
    steps = steps if dtype == abi.F64 else steps.astype(np.float32)
    a, sched_a, _, _ = _run(hip, spec, dtype, x0, fixed_iters=K, forced_steps=steps)
    b, sched_b, _, _ = _run(hip, spec, dtype, x0, fixed_iters=K, forced_steps=steps, static_rows=False)
    assert sched_a & abi.SCHEDULE_STATIC_ROWS and not sched_b & abi.SCHEDULE_STATIC_ROWS
    assert not sched_a & abi.SCHEDULE_SPLIT_TRIAL and not sched_b & abi.SCHEDULE_SPLIT_TRIAL
    _assert_equal(a, b, "forced steps")


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_resumed_solve_fused_equals_split(hip, dtype):
    """Two iterations, then two more with `resume` (the state's merit value is carried into the second solve)."""
    spec = _spec("modified_three_player_intersection", 100)
    x0 = examples.jittered_x0(spec, B, seed=7)
    outs = []
    for split in (False, True):
        _, _, prob, bufs = _run(hip, spec, dtype, x0, split_trial=split, fixed_iters=2)
        x = x0 if dtype == abi.F64 else x0.astype(np.float32)
        bufs = prob.solve(x, bufs=bufs, split_trial=split, fixed_iters=2, resume=True)
        assert bool(prob.last_schedule() & abi.SCHEDULE_SPLIT_TRIAL) == split and prob.last_schedule() & abi.SCHEDULE_STATIC_ROWS
        out = {k: bufs[k].detach().cpu().numpy().copy() for k in ARRAYS}
        out["backtracks"] = prob.solve_state(bufs)["backtracks"].detach().cpu().numpy().copy()
        outs.append(out)
    _assert_equal(outs[0], outs[1], "resume")
