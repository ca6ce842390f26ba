"""The player-parallel feedback sweep with B's constant entries in registers (ilqg_solve_options::sweep_forms ON / AUTO;
ilqgames_amd/csrc/ilqg_lq.hpp, BCONST) against the same sweep reading the B tile (sweep_forms OFF).  Every sum the
new forms replace had a single term that is not an exact zero, and F = A - B P on the vector unit is the matrix pipe's
fused multiply-add (scripts/ubench/mfma_round.hip), so ON returns the bits of OFF on every output array
(np.array_equal: a zero's sign is not compared).  tests/test_gpu_sweep_forms.py covers (14, 3, 2), (16, 3, 2) and
(6, 2, 1) with fixed iterations, the free-running headline and the 128-register fp32 kernel; here: the schedule bit, the
shapes that file does not have, a free-running solve per precision and a batch with per-instance subsystem parameters.
Eight instances and four fixed iterations unless a test says otherwise."""
import numpy as np
import pytest

from ilqgames_amd import abi, examples

pytestmark = pytest.mark.gpu

ARRAYS = ("xs", "us", "P", "alpha", "costs", "iters", "status", "converged")
B = 8


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    return h


def _solve(hip, prob, x0, **kw):
    import torch
    out = prob.solve(x0, **kw)
    torch.cuda.synchronize()
    return {q: out[q].detach().cpu().numpy().copy() for q in ARRAYS}, prob.last_schedule()


def _assert_same_bits(a, b):
    for q in ARRAYS:
        assert np.all(np.isfinite(a[q])), q
        assert np.array_equal(a[q], b[q]), q


def _on_off(hip, spec, dtype, x0=None, **kw):
    """(outputs, schedule) with the forms ON and OFF on one problem; asserts equal bits."""
    prob = kw.pop("prob", None) or hip.Problem(spec, dtype)
    x0 = examples.jittered_x0(spec, B, seed=23) if x0 is None else x0
    on, sched_on = _solve(hip, prob, x0, sweep_forms=True, **kw)
    off, sched_off = _solve(hip, prob, x0, sweep_forms=False, **kw)
    assert np.any(on["P"] != 0)
    _assert_same_bits(on, off)
    return on, sched_on, sched_off, prob, x0


# ---- (a) the schedule bit ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_constant_b_is_reported_for_a_problem_that_qualifies(hip, dtype):
    spec = examples.modified_three_player_intersection()
    assert hip.sweep_b_structure(spec, dtype)[0]
    on, sched_on, sched_off, prob, x0 = _on_off(hip, spec, dtype, fixed_iters=4)
    assert sched_on & abi.SCHEDULE_CONSTANT_B
    assert not sched_off & abi.SCHEDULE_CONSTANT_B
    assert sched_on & ~abi.SCHEDULE_CONSTANT_B == sched_off
    auto, sched_auto = _solve(hip, prob, x0, fixed_iters=4)
    assert sched_auto == sched_on
    _assert_same_bits(auto, on)
    # the single-wave sweep keeps the B tile: the bit says what ran
    _, sched_1w = _solve(hip, prob, x0, fixed_iters=4, single_wave_sweep=True)
    assert sched_1w & abi.SCHEDULE_SINGLE_WAVE_SWEEP and not sched_1w & abi.SCHEDULE_CONSTANT_B


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_air_3d_has_computed_entries_and_never_sets_the_bit(hip, dtype):
    spec = examples.air_3d()
    assert not hip.sweep_b_structure(spec, dtype)[0]
    _, sched_on, sched_off, prob, x0 = _on_off(hip, spec, dtype, fixed_iters=4)
    assert sched_on == sched_off and not sched_on & abi.SCHEDULE_CONSTANT_B
    assert not _solve(hip, prob, x0, fixed_iters=4)[1] & abi.SCHEDULE_CONSTANT_B


# ---- (b) ON == OFF where tests/test_gpu_sweep_forms.py has no case ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_config_5_scene_where_the_vector_column_is_the_last(hip, dtype):
    """(15, 3, 2): JB = 15, the tile has no zero column left — beta = -B alpha comes out of lane j = 15."""
    spec = examples.three_player_collision_avoidance_reachability()
    assert (spec.n, len(spec.subsystems), spec.udims[0]) == (15, 3, 2)
    _, sched_on, sched_off, _, _ = _on_off(hip, spec, dtype, fixed_iters=4)
    assert sched_on & abi.SCHEDULE_CONSTANT_B and not sched_off & abi.SCHEDULE_CONSTANT_B


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_two_player_shape(hip, dtype):
    """(10, 2, 2), two Car5D: two waves per instance, one helper wave; fp32 keeps rows 8, 9 of B in one lane group."""
    spec = examples.skeleton()
    assert (spec.n, len(spec.subsystems), spec.udims[0]) == (10, 2, 2)
    _, sched_on, sched_off, _, _ = _on_off(hip, spec, dtype, fixed_iters=4)
    assert sched_on & abi.SCHEDULE_CONSTANT_B and not sched_off & abi.SCHEDULE_CONSTANT_B


def test_roundabout_on_the_feedback_sweep_keeps_its_tiles(hip):
    """(24, 4, 2) runs the 2 x 2-tile sweep, which the forms do not reach: B qualifies on the host, the bit stays clear."""
    spec = examples.roundabout_merging(open_loop=False)
    assert hip.sweep_b_structure(spec)[0]
    _, sched_on, sched_off, _, _ = _on_off(hip, spec, abi.F64, fixed_iters=4)
    assert sched_on == sched_off and not sched_on & abi.SCHEDULE_CONSTANT_B


def test_mixed_dubins_car_scene_on_the_padded_sweep_is_not_constant(hip):
    """Control dimensions (1, 2): the run-time-dimensioned solve, its sweep on a padded specialised kernel whose B has a
    zero column — no compact rows, so the host says not constant and the padded sweep reads its B tile."""
    spec = examples.mixed_dubins_car_scene()
    assert not hip.sweep_b_structure(spec)[0]
    _, sched_on, sched_off, _, _ = _on_off(hip, spec, abi.F64, fixed_iters=4)
    assert sched_on & abi.SCHEDULE_GENERIC and sched_on & abi.SCHEDULE_PADDED_SWEEP
    assert sched_on == sched_off and not sched_on & abi.SCHEDULE_CONSTANT_B


# ---- (c) free-running, with line searches ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_free_running_headline_solve_takes_the_same_decisions(hip, dtype):
    spec = examples.modified_three_player_intersection()
    spec.params.initial_alpha_scaling = 0.1
    spec.params.expected_decrease_fraction = 0.001
    spec.params.max_backtracking_steps = 100
    spec.params.max_solver_iters = 12
    on, sched_on, _, _, _ = _on_off(hip, spec, dtype, x0=examples.jittered_x0(spec, B, seed=5))
    assert sched_on & abi.SCHEDULE_CONSTANT_B
    assert np.all(on["iters"] > 1)


# ---- (d) per-instance subsystem parameters enter A, never B ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_bound_wheelbases_leave_b_alone(hip, dtype):
    spec = examples.modified_three_player_intersection()
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_subsystem_params([0, 1])  # the two Car5D
    table = np.random.default_rng(9).uniform(2.5, 5.0, (B, 2)).astype(np.float32)
    prob.bind_instance_values(table)
    on, sched_on, _, _, x0 = _on_off(hip, spec, dtype, prob=prob, fixed_iters=4)
    assert sched_on & abi.SCHEDULE_CONSTANT_B
    prob.bind_instance_values(None)
    unbound, _ = _solve(hip, prob, x0, fixed_iters=4, sweep_forms=True)
    assert np.any(unbound["xs"] != on["xs"])  # the table was read
