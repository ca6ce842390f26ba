"""The C-term product of the one-tile feedback sweeps over the rows of present cost pairs only
(ilqg_solve_options::sweep_forms ON / AUTO; ilqgames_amd/csrc/ilqg_lq.hpp PAIRS, ilqg_lq_feedback1w.hpp ROWBC) against the
same sweeps with the full product (sweep_forms OFF).  Row jj MU + aa of the right operand [H | q] is an exact zero where
player w has no cost on player jj's controls, so a k block of [P | alpha]^T [H | q] without a row of a present pair adds
0 x p to every entry: ON does not issue the block's matrix instruction (a scalar mask per player wave, from the pair table)
and returns the bits of OFF on every output array (np.array_equal: a zero's sign is not compared).  The mask is an fp64
form: the fp32 kernels keep the full product (a branch in their loop moves the compiler's
packed arithmetic, and with it the bits) and are compared all the same.

Four instances, T = 6 (the prologue stages rows T-1, T-2 and T-3) and three iterations with forced step sizes, so every
instance takes the same path on both sides.  Cases: the headline scene (own pairs only: one k block of two in fp64)
on the player-parallel and the single-wave sweep; the same scene with one cross pair (and a coupling term, see
headline_coupled), whose mask has to widen; a two-player shape (10, 2, 2).  The cross-pair case is also held
against the CPU oracle.  tests/test_gpu_sweep_forms.py, which the ON / OFF comparisons follow, has no oracle comparison
of its own to take a tolerance from: the tolerances are those of tests/test_gpu_forced.py, which compares forced-step
solves with the oracle instance by instance (fp64 1e-9; fp32 2e-3 on the operating point, 1e-2 on P / alpha)."""
import numpy as np
import pytest

from ilqgames_amd import abi, examples
from helpers import rel_err

pytestmark = pytest.mark.gpu

ARRAYS = ("P", "alpha", "xs", "us", "costs")
B, T, K = 4, 6, 3
STEPS = np.tile(np.array([0.5, 0.25, 0.125]), (B, 1))  # [B][K]: inside what a back-tracking search accepts


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    return h


def headline():
    return examples.modified_three_player_intersection(T=T)


def headline_coupled(cross_pair):
    """The headline scene with player 0's cost on player 2's acceleration: the (0, 2) block, rows 4 and 5 of P — in fp64
    the other k block than player 0's own rows 0 and 1.  (The issue's example pair (0, 1) has rows 2 and 3, in the same
    fp64 block as the own pair: it would not widen the mask.)  In the headline scene the players are decoupled
    (block-diagonal dynamics, proximity weight 0), so P_2^T R_02 P_2 would stay in the block of Z_0 that belongs to player
    2's states and reach no output: a distance cost between players 0 and 2 couples the blocks.  With weights of 1000 the
    pair moves P by 1e-3 on a scale of 2.8 (the oracle, both precisions), so a dropped block changes the bits."""
    s = examples.modified_three_player_intersection(T=T)
    s.relative_distance(0, 1000.0, (0, 1), (10, 11))
    if cross_pair:
        s.quadratic(0, 1000.0, 1, 0.0, control_of=2)
    return s


def two_player():
    return examples.skeleton(T=T)


def _solve(hip, prob, x0, **kw):
    import torch
    out = prob.solve(x0, fixed_iters=K, forced_steps=STEPS, **kw)
    torch.cuda.synchronize()
    return {q: out[q].detach().cpu().numpy().copy() for q in ARRAYS}, prob.last_schedule()


def _on_off(hip, spec, dtype, **kw):
    prob = hip.Problem(spec, dtype)
    x0 = examples.jittered_x0(spec, B, seed=31)
    on, sched_on = _solve(hip, prob, x0, sweep_forms=True, **kw)
    off, sched_off = _solve(hip, prob, x0, sweep_forms=False, **kw)
    assert np.any(on["P"] != 0)
    for q in ARRAYS:
        assert np.all(np.isfinite(on[q])), q
        assert np.array_equal(on[q], off[q]), q
    return prob, x0, on, sched_on, sched_off


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("single_wave", [False, True])
def test_headline_scene_with_own_pairs_only(hip, dtype, single_wave):
    spec = headline()
    prob, _, _, sched_on, sched_off = _on_off(hip, spec, dtype, single_wave_sweep=single_wave)
    assert sorted(prob.pairs) == [(0, 0), (1, 1), (2, 2)]  # every player penalises its own controls only
    for sched in (sched_on, sched_off):
        assert bool(sched & abi.SCHEDULE_SINGLE_WAVE_SWEEP) == single_wave
    if not single_wave:
        assert sched_on & abi.SCHEDULE_CONSTANT_B and not sched_off & abi.SCHEDULE_CONSTANT_B


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_a_cross_pair_widens_the_mask(hip, oracle, dtype):
    """Player 0 (rows 0, 1 of P: fp64 block 0) also has the pair (0, 2) (rows 4, 5: block 1): its mask grows from one block
    to both, while players 1 and 2 keep one.  A mask built from the own pair alone would lose P_2^T R_02 P_2 from Z_0."""
    spec = headline_coupled(True)
    prob, x0, on, sched_on, _ = _on_off(hip, spec, dtype, single_wave_sweep=False)
    assert sorted(prob.pairs) == [(0, 0), (0, 2), (1, 1), (2, 2)]
    assert sched_on & abi.SCHEDULE_CONSTANT_B and not sched_on & abi.SCHEDULE_SINGLE_WAVE_SWEEP
    ref = oracle.OracleProblem(spec).solve(dtype, x0, fixed_iters=K, forced_steps=STEPS)
    tol_op, tol_st = (1e-9, 1e-9) if dtype == abi.F64 else (2e-3, 1e-2)
    errs = {"xs": rel_err(on["xs"], ref["xs"]), "P": rel_err(on["P"], ref["rawP"]), "alpha": rel_err(on["alpha"], ref["alpha"])}
    print("cross pair, %s: relative error against the oracle %s" % ("f64" if dtype == abi.F64 else "f32", errs))
    assert errs["xs"] < tol_op and errs["P"] < tol_st and errs["alpha"] < tol_st
    # the pair is felt: the same scene without it has another P
    without, _ = _solve(hip, hip.Problem(headline_coupled(False), dtype), x0, sweep_forms=True, single_wave_sweep=False)
    assert rel_err(without["P"], on["P"]) > 1e-4


def test_two_player_shape_with_a_spare_column(hip):
    """(10, 2, 2): two waves per instance, M = 4 — one k block in fp64, and both players' rows in it."""
    spec = two_player()
    assert (spec.n, len(spec.subsystems), spec.udims[0]) == (10, 2, 2)
    _, _, _, sched_on, _ = _on_off(hip, spec, abi.F64, single_wave_sweep=False)
    assert sched_on & abi.SCHEDULE_CONSTANT_B
