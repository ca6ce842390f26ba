"""ilqg_solve_options::sweep_forms: the one-tile feedback sweeps run the m x m Nash solve of a step with DPP row
broadcasts (the pivot columns replicated in every 16-lane row, ilqgames_amd/csrc/ilqg_lq.hpp lu_solve_columns_rows)
instead of read-lane broadcasts over the scalar unit.  Only the way a value travels between lanes changes — every
floating-point operation and its order are the same — so a solve with the forms ON returns the bits of the same solve with
them OFF: every output array, free-running line searches included, in both precisions, for the headline shape
(14, 3, 2), an n = 16 shape (no spare tile column: alpha has its own store), a shape with one control per player
(m = 2: fourteen right-hand sides per row) and the single-wave sweep."""
import numpy as np
import pytest

from ilqgames_amd import abi, examples

pytestmark = pytest.mark.gpu

ARRAYS = ("xs", "us", "P", "alpha", "costs", "iters", "status", "converged")


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    return h


def _np(t):
    return t.detach().cpu().numpy()


def _solve(hip, prob, x0, **kw):
    import torch
    out = prob.solve(x0, **kw)
    torch.cuda.synchronize()
    return {q: _np(out[q]).copy() for q in ARRAYS}


def _assert_same_bits(a, b):
    for q in ARRAYS:
        assert np.all(np.isfinite(a[q])), q
        assert np.array_equal(a[q], b[q]), q


SCENES = ["modified_three_player_intersection",  # (14, 3, 2): the headline
          "three_player_intersection",           # (16, 3, 2): no spare tile column
          "dubins_origin"]                       # (6, 2, 1): one control per player


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_row_broadcast_solve_returns_the_bits_of_the_read_lane_solve(hip, scene, dtype):
    spec = examples.CONFIGS[scene]()
    B = 96
    x0 = examples.jittered_x0(spec, B, seed=11)
    prob = hip.Problem(spec, dtype)
    on = _solve(hip, prob, x0, fixed_iters=6, sweep_forms=True)
    off = _solve(hip, prob, x0, fixed_iters=6, sweep_forms=False)
    auto = _solve(hip, prob, x0, fixed_iters=6)
    assert np.any(on["P"] != 0)
    _assert_same_bits(on, off)
    _assert_same_bits(on, auto)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_free_running_headline_solve_takes_the_same_decisions_bit_for_bit(hip, dtype):
    spec = examples.modified_three_player_intersection()
    spec.params.initial_alpha_scaling = 0.1
    spec.params.expected_decrease_fraction = 0.001
    spec.params.max_backtracking_steps = 100
    spec.params.max_solver_iters = 12
    x0 = examples.jittered_x0(spec, 64, seed=5)
    prob = hip.Problem(spec, dtype)
    _assert_same_bits(_solve(hip, prob, x0, sweep_forms=True), _solve(hip, prob, x0, sweep_forms=False))


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_single_wave_sweep_has_both_forms_too(hip, dtype):
    spec = examples.modified_three_player_intersection()
    spec.params.expected_decrease_fraction = 0.001
    x0 = examples.jittered_x0(spec, 40, seed=7)
    prob = hip.Problem(spec, dtype)
    on = _solve(hip, prob, x0, fixed_iters=5, single_wave_sweep=True, sweep_forms=True)
    assert prob.last_schedule() & abi.SCHEDULE_SINGLE_WAVE_SWEEP
    off = _solve(hip, prob, x0, fixed_iters=5, single_wave_sweep=True, sweep_forms=False)
    assert prob.last_schedule() & abi.SCHEDULE_SINGLE_WAVE_SWEEP
    _assert_same_bits(on, off)


def test_large_fp32_batch_runs_the_packed_kernel_in_both_forms(hip):
    """1536 fp32 instances with the single-wave sweep pinned off: the 128-register build of the player-parallel sweep."""
    spec = examples.modified_three_player_intersection()
    spec.params.expected_decrease_fraction = 0.001
    x0 = examples.jittered_x0(spec, 1536, seed=2)
    prob = hip.Problem(spec, abi.F32)
    on = _solve(hip, prob, x0, fixed_iters=3, single_wave_sweep=False, sweep_forms=True)
    off = _solve(hip, prob, x0, fixed_iters=3, single_wave_sweep=False, sweep_forms=False)
    _assert_same_bits(on, off)
