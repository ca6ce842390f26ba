"""Per-instance subsystem parameters on the device (ilqg_problem_declare_instance_subsystem_params): a different
wheelbase or speed for each game of a batch.

As for the cost parameters (tests/test_gpu_instance_params.py; shared check: tests/instance_harness.py), the core checks are
EXACT: an instance of a heterogeneous batch must return the bits of the same instance solved in a problem created with
its param0 written into the descriptor — the values are floats on both paths and enter the arithmetic at the same place —
over every instance and every output array.  Only the stage kernels against the oracle have tolerances, those of
tests/test_gpu_parity.py::test_stage_kernels_match_oracle for the same arrays, and the closed-form Dubins displacement,
whose bound is worked out in its docstring.  Wheelbases are drawn from [2.5, 5.0] m, speeds from [0.5, 2.0] x the baked
value."""
import copy
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ilqgames_amd import abi, examples
from helpers import rel_err
from instance_harness import KEYS, check_baked_equals_bound, headline as _headline, same_bits as _same_bits, to_numpy as _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


WHEELBASE = (2.5, 5.0)
# two cost columns of tests/test_gpu_instance_params.py::HEADLINE_DECL, beside the two wheelbases
HEADLINE_COST_DECL = [("p1_nominal_speed", "value", 6.0, 10.0), ("p2_lane", "weight", 15.0, 35.0)]


def _sub_decl(spec, rows):
    """[(row, lo, hi)]: a wheelbase from [2.5, 5.0], a speed from [0.5, 2.0] x the baked one."""
    out = []
    for r in rows:
        kind, _, _, p0 = spec.subsystems[r]
        if kind in (abi.DYN_CAR_5D, abi.DYN_CAR_6D, abi.DYN_CAR_7D):
            out.append((r,) + WHEELBASE)
        else:
            assert kind in (abi.DYN_DUBINS_CAR, abi.DYN_DELAYED_DUBINS_CAR, abi.DYN_AIR_3D_EVADER, abi.DYN_AIR_3D_PURSUER)
            out.append((r, 0.5 * p0, 2.0 * p0))
    return out


def _draw(cost_decl, sub_decl, count, seed):
    """-> ([(name, field)], [rows], float32 [count][cost | subsystem] seeded values inside each entry's range)."""
    rng = np.random.default_rng(seed)
    lo = np.array([d[2] for d in cost_decl] + [d[1] for d in sub_decl])
    hi = np.array([d[3] for d in cost_decl] + [d[2] for d in sub_decl])
    vals = (lo + (hi - lo) * rng.random((count, len(lo)))).astype(np.float32)
    return [(d[0], d[1]) for d in cost_decl], [d[0] for d in sub_decl], vals


def _baked(spec, params, rows, row):
    """The spec with one parameter vector written into its terms and its subsystems."""
    s = copy.deepcopy(spec)
    for (name, field), v in zip(params, row[:len(params)]):
        s.terms[s.term_index(name)][field] = float(np.float32(v))
    for r, v in zip(rows, row[len(params):]):
        kind, xd, ud, _ = s.subsystems[r]
        s.subsystems[r] = (kind, xd, ud, float(np.float32(v)))
    return s


def _identity_row(spec, params, rows):
    return np.array([spec.terms[spec.term_index(n)][f] for n, f in params] + [spec.subsystems[r][3] for r in rows],
                    dtype=np.float32)


def _bound_problem(hip, spec, dtype, params, rows, table, subsystems_first=False):
    prob = hip.Problem(spec, dtype)
    if subsystems_first:  # either declaration may be made first: the cost columns come first in the table all the same
        prob.declare_instance_subsystem_params(rows)
    if params:
        prob.declare_instance_params(params)
    if not subsystems_first:
        prob.declare_instance_subsystem_params(rows)
    prob.bind_instance_values(table)
    return prob


def _check_baked_equals_bound(hip, spec, rows, dtype, cost_decl=(), BV=4, seed=5, subsystems_first=False, **kw):
    params, rows, vals = _draw(list(cost_decl), _sub_decl(spec, rows), BV, seed)
    return check_baked_equals_bound(hip, spec, dtype,
                                    lambda table: _bound_problem(hip, spec, dtype, params, rows, table, subsystems_first),
                                    lambda row: _baked(spec, params, rows, row), vals, seed=seed, **kw)[0]


# ---- 1. bound equals baked, bit for bit ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("static_rows", [None, False])
@pytest.mark.parametrize("split_trial", [True, False])
@pytest.mark.parametrize("fixed_iters", [0, 6])
def test_headline_scene_two_wheelbases_bound_equal_baked(hip, dtype, static_rows, split_trial, fixed_iters):
    """split_trial on: the paired rollout, two different instances in one wavefront; off: the fused kernel."""
    spec = _headline()
    if static_rows is None:
        assert hip.Problem(spec, dtype).row_program()[1] != 0, "the headline scene runs the static row code"
    _check_baked_equals_bound(hip, spec, [0, 1], dtype, deterministic=True, static_rows=static_rows,
                              split_trial=split_trial, fixed_iters=fixed_iters)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("subsystems_first", [False, True])
def test_cost_columns_come_first_whichever_is_declared_first(hip, dtype, subsystems_first):
    _check_baked_equals_bound(hip, _headline(), [1, 0], dtype, cost_decl=HEADLINE_COST_DECL, deterministic=True,
                              subsystems_first=subsystems_first)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("probe_lanes", [True, False])
def test_probing_rollouts_bound_equal_baked(hip, dtype, probe_lanes):
    """Free-running with the speculative line search: a lane per (candidate, subsystem), or two candidates per wavefront."""
    spec = examples.three_player_collision_avoidance_reachability()
    spec.params.max_solver_iters = 8
    prob = _check_baked_equals_bound(hip, spec, [0, 1, 2], dtype, B=12, whole_batch_partner=True, split_trial=True,
                                     probe=True, probe_lanes=probe_lanes)
    x0 = examples.jittered_x0(spec, 12, seed=6)
    o = prob.solve(x0, split_trial=True, probe=True, probe_lanes=probe_lanes)
    assert int(_np(prob.solve_state(o)["backtracks"]).sum()) > 0, "the line searches should back-track: nothing was probed"


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_roundabout_car6d_open_loop_bound_equals_baked(hip, dtype):
    spec = examples.roundabout_merging()
    spec.params.max_solver_iters = 12
    assert spec.n == 24 and spec.subsystems[0][0] == abi.DYN_CAR_6D
    _check_baked_equals_bound(hip, spec, [0, 1, 2, 3], dtype, B=8, deterministic=True)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("padded_sweep", [True, False])
def test_run_time_dimensioned_rollout_bound_equals_baked(hip, dtype, padded_sweep):
    spec = examples.mixed_dubins_car_scene()
    spec.params.max_solver_iters = 12
    assert [s[0] for s in spec.subsystems[:2]] == [abi.DYN_DUBINS_CAR, abi.DYN_CAR_5D]
    _check_baked_equals_bound(hip, spec, [0, 1], dtype, B=8, deterministic=True, padded_sweep=padded_sweep)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene,rows", [("dynamics_zoo_scene", [0]), ("delayed_dubins_scene", [0, 1]), ("air_3d", [0, 1])])
def test_plain_rk4_models_bound_equal_baked(hip, dtype, scene, rows):
    """Car7D (the control-dependent Jacobian entry), the delayed Dubins car, and Air3D with both speeds declared: the
    pursuer's enters the evader's rows (the row-pair value column) and the rollout as a second operand."""
    spec = getattr(examples, scene)()
    spec.params.max_solver_iters = 12
    _check_baked_equals_bound(hip, spec, rows, dtype, B=8, deterministic=True)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_large_batch_schedule_bound_equals_baked(hip, dtype):
    """Without `deterministic`, at five or more instances per CU (the single-wave sweep): the partner is a homogeneous
    batch of the same size."""
    _, cus = hip.device_info()
    B = 6 * cus
    spec = _headline()
    _check_baked_equals_bound(hip, spec, [0, 1], dtype, B=B, BV=2, whole_batch_partner=True, fixed_iters=4)
    prob = hip.Problem(spec, dtype)
    prob.solve(examples.jittered_x0(spec, B, seed=1), fixed_iters=1)
    assert prob.last_schedule() & abi.SCHEDULE_SINGLE_WAVE_SWEEP


# ---- 2. identity table ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene", ["headline", "air_3d"])
def test_identity_table_changes_nothing(hip, dtype, scene):
    spec = _headline() if scene == "headline" else examples.air_3d()
    spec.params.max_solver_iters = 10
    rows = [0, 1]
    B = 10
    x0 = examples.jittered_x0(spec, B, seed=9)
    prob = hip.Problem(spec, dtype)
    plain = {k: _np(v) for k, v in prob.solve(x0).items() if k in KEYS}
    prob.declare_instance_subsystem_params(rows)
    prob.bind_instance_values(np.tile(_identity_row(spec, [], rows), (B, 1)))
    bound = prob.solve(x0)
    for k in KEYS:
        assert _same_bits(_np(bound[k]), plain[k]), k
    prob.bind_instance_values(None)
    again = prob.solve(x0)
    for k in KEYS:
        assert _same_bits(_np(again[k]), plain[k]), k


# ---- 3. stage kernels against the oracle, a different vector per instance ----
@pytest.mark.parametrize("scene,rows", [("modified_three_player_intersection", [0, 1]), ("mixed_dubins_car_scene", [0, 1]),
                                        ("air_3d", [0, 1])])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_rollout_and_linearize_match_per_vector_oracles(hip, oracle, scene, rows, dtype):
    """rollout and linearize of a bound batch against one OracleProblem per parameter vector, at a random operating point
    and with the tolerances of test_stage_kernels_match_oracle (tests/test_gpu_parity.py:330,336) for the same arrays and
    precisions — independent of the device's own baked path."""
    from test_gpu_parity import _random_op
    spec = getattr(examples, scene)()
    rng = np.random.default_rng(7)
    B = 4
    x0, xs_ref, us_ref, P, alpha = _random_op(spec, rng, B)
    scale = np.array([1.0, 0.5, 0.25, 0.1])
    _, rows, vals = _draw([], _sub_decl(spec, rows), B, seed=21)
    hp = _bound_problem(hip, spec, dtype, [], rows, vals)
    xs_d, us_d = (_np(a) for a in hp.rollout(x0, xs_ref, us_ref, P, alpha, scale))
    plain = hip.Problem(spec, dtype)
    xs_p, _ = plain.rollout(x0, xs_ref, us_ref, P, alpha, scale)
    assert not _same_bits(xs_d, _np(xs_p)), "the drawn vectors should change the rollout"
    xs_o = np.zeros((B, spec.T, spec.n))
    us_o = np.zeros((B, spec.T, spec.m))
    ops = [oracle.OracleProblem(_baked(spec, [], rows, vals[b])) for b in range(B)]
    tol = 1e-9 if dtype == abi.F64 else 5e-4
    for b in range(B):
        sl = slice(b, b + 1)
        xs_o[sl], us_o[sl] = ops[b].rollout(dtype, x0[sl], xs_ref[sl], us_ref[sl], P[sl], alpha[sl], scale[sl])
        ex, eu = rel_err(xs_d[sl], xs_o[sl]), rel_err(us_d[sl], us_o[sl])
        print("instance %d rollout rel err xs %.3e us %.3e" % (b, ex, eu))
        assert ex < tol and eu < tol, b
    # downstream at the ORACLE's operating point so errors do not chain
    A_d, B_d = (_np(a) for a in hp.linearize(xs_o, us_o))
    A_p, B_p = (_np(a) for a in plain.linearize(xs_o, us_o))
    assert not (_same_bits(A_d, A_p) and _same_bits(B_d, B_p)), "the drawn vectors should change the linearisation"
    tol = 1e-12 if dtype == abi.F64 else 1e-5
    for b in range(B):
        sl = slice(b, b + 1)
        A_o, B_o = ops[b].linearize(dtype, xs_o[sl], us_o[sl])
        ea, eb = rel_err(A_d[sl], A_o), rel_err(B_d[sl], B_o)
        print("instance %d linearize rel err A %.3e B %.3e" % (b, ea, eb))
        assert ea < tol and eb < tol, b


# ---- 4. it acts ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_dubins_speed_column_scales_the_displacement(hip, dtype):
    """One Dubins car under zero strategies and references (P = alpha = u_ref = 0: omega = 0, the heading stays theta0)
    through ilqg_rollout_batch, its speed 0.5, 1 and 2 by instance: px[T-1] - px[0] = v (T-1) dt cos(theta0), py with the
    sine.  The RK4 is exact for a constant right-hand side up to rounding: ~200 sub-step additions of one rounding each,
    2e-14 / 1.2e-5 relative in the worst case; asserted at 1e-12 (fp64) and 1e-4 (fp32)."""
    theta0 = 0.6
    spec = examples.one_player_reachability(theta0=theta0)
    assert len(spec.subsystems) == 1 and spec.subsystems[0][0] == abi.DYN_DUBINS_CAR
    T, n, m, dt = spec.T, spec.n, spec.m, spec.dt
    speeds = np.array([[0.5], [1.0], [2.0]], dtype=np.float32)
    B = len(speeds)
    x0 = np.tile(np.asarray(spec.x0, dtype=np.float64), (B, 1))
    assert x0[0, 2] == theta0
    xs_ref = np.random.default_rng(3).standard_normal((B, T, n))  # arbitrary: P = 0 takes it out
    zeros = lambda *shape: np.zeros(shape)
    prob = _bound_problem(hip, spec, dtype, [], [0], speeds)
    xs, us = (_np(a).astype(np.float64) for a in prob.rollout(x0, xs_ref, zeros(B, T, m), zeros(B, T, m * n), zeros(B, T, m)))
    assert not us.any()
    tol = 1e-12 if dtype == abi.F64 else 1e-4
    for b in range(B):
        v = float(speeds[b, 0])
        for axis, f in ((0, np.cos), (1, np.sin)):
            want = v * (T - 1) * dt * f(theta0)
            got = xs[b, T - 1, axis] - xs[b, 0, axis]
            print("speed %.1f axis %d displacement %.15g expected %.15g rel err %.3e" % (v, axis, got, want, abs(got - want) / want))
            assert abs(got - want) <= tol * abs(want), (b, axis)


# ---- 5. solve_again under a mask after the values were rewritten on the device ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_solve_again_with_rewritten_values_and_mask(hip, dtype):
    import torch
    spec = _headline()
    spec.params.max_solver_iters = 8
    B, BV = 8, 4
    _, rows, vals = _draw([], _sub_decl(spec, [0, 1]), BV, seed=31)
    _, _, vals2 = _draw([], _sub_decl(spec, [0, 1]), BV, seed=32)
    which = np.arange(B) % BV
    x0 = examples.jittered_x0(spec, B, seed=33)
    x0b = examples.jittered_x0(spec, B, seed=34)
    active = np.array([1, 0, 1, 1, 0, 1, 1, 0], dtype=np.int32)
    act_d = torch.as_tensor(active, device="cuda")
    prob = hip.Problem(spec, dtype)
    prob.single_wave_sweep = False  # pinned: the slices below must run the batch's schedule
    prob.declare_instance_subsystem_params(rows)
    table = prob.bind_instance_values(torch.as_tensor(vals[which], device="cuda").contiguous())
    bufs = prob.solve(x0)
    first = {k: _np(bufs[k]).copy() for k in KEYS}
    table.copy_(torch.as_tensor(vals2[which], device="cuda"))  # rewritten in place, on the device
    prob.solve_again(x0b, bufs, active=act_d)
    out = {k: _np(bufs[k]) for k in KEYS}
    for b in np.nonzero(active == 0)[0]:
        for k in KEYS:
            assert _same_bits(out[k][b], first[k][b]), ("masked instance touched", b, k)
    for v in range(BV):
        sel = np.nonzero(which == v)[0]
        p1 = hip.Problem(_baked(spec, [], rows, vals[v]), dtype)
        p1.single_wave_sweep = False
        rb = p1.solve(x0[sel])
        for k in KEYS:
            assert _same_bits(first[k][sel], _np(rb[k])), (k, v)
        # the same solver state carried into a problem with the second vector: its workspace layout is the same
        p2 = hip.Problem(_baked(spec, [], rows, vals2[v]), dtype)
        p2.single_wave_sweep = False
        p2.solve_again(x0b[sel], rb, active=act_d[torch.as_tensor(sel, device="cuda")].contiguous())
        for k in KEYS:
            for j, b in enumerate(sel):
                if active[b]:
                    assert _same_bits(out[k][b], _np(rb[k])[j]), (k, b)


# ---- 6. strategy costs and the Nash checks ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene", ["reachability", "air_3d"])
def test_strategy_costs_and_nash_checks_bound_equal_baked(hip, dtype, scene):
    if scene == "reachability":
        spec, rows = examples.three_player_intersection_reachability(T=20), [0, 1]  # a max-over-time player: the sufficient check's copy
    else:
        spec, rows = examples.air_3d(T=20), [0, 1]  # the second operand of the evader's row
    spec.params.max_solver_iters = 6
    B = 4
    _, rows, vals = _draw([], _sub_decl(spec, rows), B, seed=41)
    x0 = examples.jittered_x0(spec, B, seed=42)
    prob = _bound_problem(hip, spec, dtype, [], rows, vals)
    sol = prob.solve(x0, deterministic=True)
    args = [sol[k] for k in ("xs", "us", "P", "alpha")]
    costs = _np(prob.strategy_costs(x0, *args))
    rk4 = _np(prob.strategy_costs(x0, *args, euler=False))
    ok, margin = (_np(a) for a in prob.check_local_nash(x0, *args, max_perturbation=0.1))
    psd = _np(prob.check_sufficient_nash(sol["xs"], sol["us"]))
    for b in range(B):
        ref = hip.Problem(_baked(spec, [], rows, vals[b]), dtype)
        a1 = [v[b:b + 1].contiguous() for v in args]
        assert _same_bits(costs[b:b + 1], _np(ref.strategy_costs(x0[b:b + 1], *a1))), b
        assert _same_bits(rk4[b:b + 1], _np(ref.strategy_costs(x0[b:b + 1], *a1, euler=False))), b
        ok1, margin1 = (_np(a) for a in ref.check_local_nash(x0[b:b + 1], *a1, max_perturbation=0.1))
        assert _same_bits(ok[b:b + 1], ok1) and _same_bits(margin[b:b + 1], margin1), b
        assert _same_bits(psd[b:b + 1], _np(ref.check_sufficient_nash(a1[0], a1[1]))), b
    plain = _np(hip.Problem(spec, dtype).strategy_costs(x0, *args))
    assert not _same_bits(plain, costs), "the drawn vectors should change the strategy costs"


# ---- 7. the receding-horizon entry points ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_receding_horizon_entry_points_bound_equal_per_vector_problems(hip, dtype):
    """ilqg_plan_integrate_batch, ilqg_receding_horizon_sync_batch and ilqg_receding_horizon_shift_batch on plans of the
    headline scene: a bound batch of four against four problems created with the vectors, bit for bit."""
    import torch
    spec = _headline()
    B = 4
    _, rows, vals = _draw([], _sub_decl(spec, [0, 1]), B, seed=51)
    x0 = examples.jittered_x0(spec, B, seed=52)
    prob = _bound_problem(hip, spec, dtype, [], rows, vals)
    plain = hip.Problem(spec, dtype)
    refs = [hip.Problem(_baked(spec, [], rows, vals[b]), dtype) for b in range(B)]
    sol = prob.solve(x0, fixed_iters=3, deterministic=True)
    plan = prob.new_plan(B)
    prob.solution_splice(plan, sol, torch.zeros(B, dtype=torch.float64, device="cuda"))
    one = lambda d, b: {k: v[b:b + 1].contiguous() for k, v in d.items() if hasattr(v, "shape")}
    tdt = hip.torch_dtype(dtype)
    x = (sol["xs"][:, 7, :] + 0.03 * torch.as_tensor(np.random.default_rng(53).standard_normal((B, spec.n)), device="cuda")).to(tdt).contiguous()

    def integrate(p, pl, xin):
        xc = xin.clone()
        act = torch.ones(xc.shape[0], dtype=torch.int32, device="cuda")
        p.plan_integrate(pl, 0.93, 1.37, 1.7, xc, act)
        return _np(xc), _np(act)

    def sync(p, pl, xin):
        bufs = p.alloc_solve_buffers(xin.shape[0])
        act = torch.ones(xin.shape[0], dtype=torch.int32, device="cuda")
        x0n, st0, first = p.receding_horizon_sync(pl, xin, 0.75, 0.25, bufs, act)
        return [_np(a) for a in (x0n, st0, first, act, bufs["xs"], bufs["us"], bufs["P"], bufs["alpha"])]

    def shift(p, s, xin):
        bufs = {k: s[k].clone() for k in ("xs", "us", "P", "alpha")}
        x0n, first, new_t0 = p.receding_horizon_shift(xin, 0.75, 0.25, 0.0, bufs)
        return [_np(x0n), _np(first), np.float64(new_t0)] + [_np(bufs[k]) for k in ("xs", "us", "P", "alpha")]

    for name, call, src in (("plan_integrate", integrate, plan), ("sync", sync, plan), ("shift", shift, sol)):
        got = call(prob, src, x)
        unbound = call(plain, src, x)
        assert any(not _same_bits(a, u) for a, u in zip(got, unbound)), (name, "the table must have acted")
        for b in range(B):
            want = call(refs[b], one(src, b), x[b:b + 1].contiguous())
            for q, (a, w) in enumerate(zip(got, want)):
                assert _same_bits(a[b:b + 1] if a.ndim else a, w), (name, b, q)


# ---- 8. errors, each before any kernel is launched ----
def test_declaration_and_binding_errors(hip):
    import torch
    spec = _headline()
    prob = hip.Problem(spec, abi.F64)
    B = 4
    x0 = examples.jittered_x0(spec, B, seed=1)
    with pytest.raises(hip.IlqgError) as e:  # refused declarations are errors on the handle too
        prob.declare_instance_subsystem_params([0, 2])
    assert e.value.status == abi.ERR_UNSUPPORTED and "subsystem 2" in str(e.value) and "UNICYCLE_4D" in str(e.value)
    with pytest.raises(ValueError):  # nothing declared: a table has no columns
        prob.bind_instance_values(np.zeros((B, 2), dtype=np.float32))
    prob.declare_instance_subsystem_params([0, 1])
    with pytest.raises(ValueError):  # both counts: two columns, not one
        prob.bind_instance_values(np.zeros((B, 1), dtype=np.float32))
    table = prob.bind_instance_values(torch.full((B, 2), 4.0, dtype=torch.float32, device="cuda"))
    for declare in (lambda: prob.declare_instance_subsystem_params([0]), lambda: prob.declare_instance_subsystem_params([]),
                    lambda: prob.declare_instance_params([("p1_nominal_speed", "value")])):
        with pytest.raises(hip.IlqgError) as e:  # declare while bound, either call
            declare()
        assert e.value.status == abi.ERR_INVALID and "bound" in str(e.value)
    # batch mismatch: the entry points that integrate or linearise read the table too
    bufs = prob.solve(x0, fixed_iters=1)
    x3 = torch.as_tensor(x0[:3], device="cuda").contiguous()
    a3 = [bufs[k][:3].contiguous() for k in ("xs", "us", "P", "alpha")]
    b3 = dict(zip(("xs", "us", "P", "alpha"), a3))
    plan4 = prob.new_plan(B)
    prob.solution_splice(plan4, bufs, torch.zeros(B, dtype=torch.float64, device="cuda"))
    plan3 = {k: v[:3].contiguous() for k, v in plan4.items()}
    act3 = torch.ones(3, dtype=torch.int32, device="cuda")
    calls = [lambda: prob.rollout(x3, a3[0], a3[1], a3[2], a3[3]), lambda: prob.linearize(a3[0], a3[1]),
             lambda: prob.receding_horizon_shift(x3, 0.75, 0.25, 0.0, b3),
             lambda: prob.receding_horizon_sync(plan3, x3, 0.75, 0.25, prob.alloc_solve_buffers(3), act3),
             lambda: prob.plan_integrate(plan3, 0.93, 1.37, 1.7, x3.clone(), act3),
             lambda: prob.solve(x3, fixed_iters=1), lambda: prob.total_costs(a3[0], a3[1])]
    for q, call in enumerate(calls):
        with pytest.raises(hip.IlqgError) as e:
            call()
        assert e.value.status == abi.ERR_INVALID and "batch of 4" in str(e.value), q
    prob.bind_instance_values(None)
    for call in calls:
        call()
    # with cost columns alone, what evaluates no cost stays unaffected
    prob.declare_instance_subsystem_params([])
    prob.declare_instance_params([("p1_nominal_speed", "value")])
    prob.bind_instance_values(torch.full((B, 1), 8.0, dtype=torch.float32, device="cuda"))
    for call in calls[:5]:
        call()
    with pytest.raises(hip.IlqgError):
        calls[5]()
    prob.bind_instance_values(None)
    prob.declare_instance_params([])
    with pytest.raises(hip.IlqgError):
        hip._check(hip.lib().ilqg_problem_bind_instance_values(prob.h, B, hip._ptr(table)))


def test_cost_and_subsystem_columns_together_may_not_exceed_the_maximum(hip):
    """One table holds both kinds of column: the headline scene with 128 more quadratic terms (256 declarable cost
    columns), in either order of declaration.  A sum of exactly ILQG_MAX_INSTANCE_PARAMS is accepted, one more is
    ILQG_ERR_INVALID with the limit named, and a refused call leaves the earlier declaration standing."""
    MAX = 256
    spec = _headline()
    extra = [spec.quadratic(0, 1.0, d % 5, 0.0) for d in range(MAX // 2)]
    cost = [(t, f) for t in extra for f in ("weight", "value")]
    assert len(cost) == MAX
    prob = hip.Problem(spec, abi.F64)

    def refused(call, cost_count, sub_count):
        with pytest.raises(hip.IlqgError) as e:
            call()
        msg = str(e.value)
        assert e.value.status == abi.ERR_INVALID and "ILQG_MAX_INSTANCE_PARAMS" in msg, msg
        assert "%d cost columns" % cost_count in msg and "%d subsystem columns" % sub_count in msg, msg

    # cost columns first
    prob.declare_instance_params(cost[:MAX - 1])
    prob.declare_instance_subsystem_params([1])              # 255 + 1: the table is full
    refused(lambda: prob.declare_instance_subsystem_params([0, 1]), MAX - 1, 2)
    assert prob.instance_subsystems == [1]
    prob.bind_instance_values(np.ones((2, MAX), dtype=np.float32))  # the earlier declaration stands: 256 columns
    prob.bind_instance_values(None)
    prob.declare_instance_subsystem_params([])
    prob.declare_instance_params(cost)                       # 256 + 0
    refused(lambda: prob.declare_instance_subsystem_params([0]), MAX, 1)
    # subsystem columns first
    prob.declare_instance_params([])
    prob.declare_instance_subsystem_params([0, 1])
    refused(lambda: prob.declare_instance_params(cost[:MAX - 1]), MAX - 1, 2)
    assert prob.instance_params == []
    prob.declare_instance_params(cost[:MAX - 2])             # 254 + 2
    prob.bind_instance_values(np.ones((2, MAX), dtype=np.float32))
    prob.bind_instance_values(None)


# ---- 9. the C++ mirror ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_host_mirror_solve_batch_with_subsystem_params(hip, dtype):
    """tests/host/instance_subsystem_params_demo.cpp solve: GameSolver::SolveBatch(x0s, instance_params) on the headline
    scene built with the mirrored classes, player 1's nominal speed and — AddSubsystem — the two cars' wheelbases per
    instance, rows [cost | subsystem | subsystem].  The harness solves the same inputs on the descriptor the C++ flattener
    produced: as one bound batch, and in one problem per vector created with it (a batch of the same size each: the same
    schedule).  The mirror's containers are float: the harness's outputs are rounded to float before the exact comparison."""
    exe = os.path.join(ROOT, "tests", "host", "_bin", "instance_subsystem_params_demo")
    assert os.path.exists(exe), "build() compiles tests/host/instance_subsystem_params_demo.cpp"
    B = 6
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.bin")
        subprocess.run([exe, "solve", "f64" if dtype == abi.F64 else "f32", str(B), out], check=True, timeout=300)
        raw = np.fromfile(out, dtype=np.float64)
    resolved = subprocess.check_output([exe, "resolve"], text=True, timeout=120).splitlines()
    term, field = int(resolved[0].split()[1]), int(resolved[0].split()[2])
    rows = [int(ln.split()[1]) for ln in resolved[1:3]]
    assert rows == [0, 1]
    spec = abi.ProblemSpec.from_dump("\n".join(resolved[7:]))
    assert spec.canonical() == _headline().canonical()
    n, m, T = spec.n, spec.m, spec.T
    count = 3
    at = 0

    def take(k, shape):
        nonlocal at
        a = raw[at:at + k].reshape(shape)
        at += k
        return a
    x0 = take(B * n, (B, n))
    vals = take(B * count, (B, count)).astype(np.float32)
    xs = take(B * T * n, (B, T, n)).astype(np.float32)
    us = take(B * T * m, (B, T, m)).astype(np.float32)
    assert at == raw.size
    assert np.all((vals[:, 1:] >= 2.5) & (vals[:, 1:] <= 5.0))
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_params([(term, field)])
    prob.declare_instance_subsystem_params(rows)
    prob.bind_instance_values(vals)
    sol = prob.solve(x0)
    assert int(_np(sol["iters"]).min()) > 0
    assert _same_bits(_np(sol["xs"]).astype(np.float32), xs)
    assert _same_bits(_np(sol["us"]).astype(np.float32), us)
    for b in range(B):
        s = copy.deepcopy(spec)
        s.terms[term]["value" if field == abi.PARAM_VALUE else "weight"] = float(vals[b, 0])
        for r, v in zip(rows, vals[b, 1:]):
            kind, xd, ud, _ = s.subsystems[r]
            s.subsystems[r] = (kind, xd, ud, float(v))
        ref = hip.Problem(s, dtype).solve(x0)
        assert _same_bits(_np(ref["xs"])[b].astype(np.float32), xs[b]), b
        assert _same_bits(_np(ref["us"])[b].astype(np.float32), us[b]), b
    plain = hip.Problem(spec, dtype).solve(x0)
    assert not _same_bits(_np(plain["xs"]).astype(np.float32), xs), "the table must have acted"
