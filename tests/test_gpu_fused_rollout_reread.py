"""The fused trial kernel reads its arguments again behind the rollout (trial_args_again, csrc/ilqg_solve.hpp) and keeps
the step loop's constants and lane masks in the scalar registers that frees (rollout_instance's HOLD, csrc/ilqg_stages.hpp).

What that can break is what wave 0 derives a second time — buffer addresses, the workspace layout, the row stage's tables,
the instance's solver parameters — and a second rollout in the same launch, which starts from the re-read values.  The
split pass (rollout / rows / decision kernels) derives everything once per launch and runs the same functions, so the
checks are EXACT: the fused kernel against the split pass, every output array bit for bit, on the headline scene at the
horizons where the row stage's chunks fall differently, with line-search parameters that make the fused kernel back-track
inside the launch (the example's own 1.0 / 0.9; hand-off off, so the rejected steps stay in the fused kernel; rounds not
counted)."""
import numpy as np
import pytest

from ilqgames_amd import abi, examples
from instance_harness import KEYS, same_bits as _same_bits, to_numpy as _np

pytestmark = pytest.mark.gpu

B = 8
# 3: one short chunk; 64: exactly one full chunk; 65: a full chunk and a one-row last chunk that the two waves share;
# 100: the headline horizon
HORIZONS = (3, 64, 65, 100)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


def _scene(T):
    spec = examples.modified_three_player_intersection(T=T)
    assert (spec.params.initial_alpha_scaling, spec.params.expected_decrease_fraction) == (1.0, np.float32(0.9))  # the example's own
    spec.params.max_solver_iters = 6
    return spec


def _fused_and_split(prob, x0):
    outs = []
    for split in (False, True):
        o = prob.solve(x0, split_trial=split, handoff=False, counted=False)
        state = prob.solve_state(o)
        outs.append(({k: _np(o[k]).copy() for k in KEYS}, int(_np(state["backtracks"]).sum())))
    return outs


def _assert_same(fused, split):
    for k in KEYS:
        print(k, "equal" if _same_bits(fused[k], split[k]) else "DIFFERS")
    for k in KEYS:
        assert _same_bits(fused[k], split[k]), k


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("T", HORIZONS)
def test_fused_kernel_with_back_tracking_is_the_split_pass_bit_for_bit(hip, T, dtype):
    spec = _scene(T)
    prob = hip.Problem(spec, dtype)
    assert prob.row_program()[1] > 0, "the headline scene's row structure is a registered one at every horizon"
    x0 = examples.jittered_x0(spec, B, seed=3)
    (fused, rejected), (split, rejected_split) = _fused_and_split(prob, x0)
    print("T", T, "iters", fused["iters"], "rejected steps", rejected)
    assert rejected > 0 and rejected == rejected_split, "the line searches should back-track inside the launch"
    assert np.isfinite(fused["xs"]).all()
    _assert_same(fused, split)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_bound_solver_parameters_are_read_behind_the_rollout(hip, dtype):
    """Per-instance solver parameters (the decision section's solver_params_of, read behind the rollout and the row
    stage): two different step fractions in the batch, so the instances' line searches end at different depths."""
    spec = _scene(100)
    fields = ["geometric_alpha_scaling", "expected_decrease_fraction"]
    table = np.array([[0.5, 0.9], [0.7, 0.3]], dtype=np.float32)[np.arange(B) % 2]
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_solver_params(fields)
    prob.bind_instance_values(table)
    assert prob.row_program()[1] > 0, "the headline scene's row structure is a registered one"
    x0 = examples.jittered_x0(spec, B, seed=3)
    (fused, rejected), (split, rejected_split) = _fused_and_split(prob, x0)
    print("iters", fused["iters"], "rejected steps", rejected)
    assert rejected > 0 and rejected == rejected_split
    _assert_same(fused, split)
    # the two halves of the batch did take different parameters: the same batch under row 0 alone differs
    prob.bind_instance_values(np.ascontiguousarray(table[:1].repeat(B, axis=0)))
    uniform = {k: _np(v).copy() for k, v in prob.solve(x0, split_trial=False, handoff=False, counted=False).items() if k in KEYS}
    assert not _same_bits(uniform["xs"][1::2], fused["xs"][1::2])


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_bound_subsystem_parameters_take_the_bound_twin_of_the_fused_kernel(hip, dtype):
    """Per-instance subsystem parameters (two wheelbases in the batch): the problem's fused kernel is the BOUND twin,
    whose rollout reads the instance's row of the table (instance_values) in front of the step loop and whose row stage
    reads it behind the rollout, from the arguments read again."""
    spec = _scene(100)
    own = spec.subsystems[1][3]
    table = np.array([[own], [1.125 * own]], dtype=np.float32)[np.arange(B) % 2]
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_subsystem_params([1])  # player 2's wheelbase
    prob.bind_instance_values(table)
    assert prob.row_program()[1] > 0, "the headline scene's row structure is a registered one"
    x0 = examples.jittered_x0(spec, B, seed=3)
    (fused, rejected), (split, rejected_split) = _fused_and_split(prob, x0)
    print("iters", fused["iters"], "rejected steps", rejected)
    assert rejected > 0 and rejected == rejected_split
    _assert_same(fused, split)
    # the wheelbase did reach the odd instances: the same batch with nothing bound differs there
    plain = hip.Problem(spec, dtype).solve(x0, split_trial=False, handoff=False, counted=False)
    assert not _same_bits(_np(plain["xs"])[1::2], fused["xs"][1::2])
