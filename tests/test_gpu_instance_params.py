"""Per-instance cost parameters on the device (ilqg_problem_declare_instance_params / ilqg_problem_bind_instance_values).

The core checks are EXACT: an instance of a heterogeneous batch must return the bits of the same instance solved in a
problem created with its parameter vector written into the descriptor (the values are floats on both paths and enter
the arithmetic at the same place), so nothing here has a tolerance except the stage kernels against the oracle, which
take the tolerances of tests/test_gpu_parity.py::test_stage_kernels_match_oracle (restated there, lines 336-349).
Every comparison runs over every instance and every output array."""
import copy

import numpy as np
import pytest

from ilqgames_amd import abi, examples
from helpers import rel_err
from instance_harness import KEYS, check_baked_equals_bound, headline as _headline, same_bits as _same_bits, to_numpy as _np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


# ---- scenes: what varies per instance, and the range each value is drawn from ----
HEADLINE_DECL = [("p1_nominal_speed", "value", 6.0, 10.0), ("p2_nominal_speed", "value", 4.0, 8.0),
                 ("p3_nominal_speed", "weight", 5.0, 20.0), ("p1_lane", "weight", 15.0, 35.0),
                 ("p2_lane", "weight", 15.0, 35.0),
                 # the scene bakes proximity weight 0: a non-zero override must work
                 ("p1_proximity_p2", "weight", 5.0, 30.0), ("p2_proximity_p1", "weight", 5.0, 30.0),
                 ("p1_proximity_p2", "value", 4.0, 8.0)]
ROUNDABOUT_DECL = [("p1_nominal_speed", "value", 6.0, 11.0), ("p3_nominal_speed", "value", 6.0, 11.0),
                   ("p2_lane", "weight", 15.0, 35.0), ("p4_proximity_p1", "weight", 50.0, 150.0),
                   ("p1_proximity_p2", "value", 4.0, 7.0)]
AVOIDANCE_DECL = [("p1_u0_max", "value", 0.5, 1.0), ("p2_u1_max", "value", 0.05, 0.1),  # constraint thresholds
                  ("p3_u0_min", "value", -1.0, -0.5), ("p1_distance_child0", "value", 2.0, 4.0)]
REACHABILITY_DECL = [("p1_distance_p2", "value", 4.0, 8.0), ("p1_distance_p3", "value", 4.0, 8.0),  # EXTREME_VALUE children
                     ("p2_nominal_speed", "value", 4.0, 8.0), ("p3_proximity_p1", "weight", 5.0, 30.0)]
MIXED_DECL = [("p1_goal_x", "value", 8.0, 16.0), ("p1_goal_y", "value", 1.0, 5.0), ("p2_nominal_speed", "value", 4.0, 8.0),
              ("p1_proximity_p2", "weight", 10.0, 30.0), ("p2_lane", "weight", 5.0, 15.0)]


def _draw(decl, count, seed):
    """-> ([(name, field)], float32 [count][len(decl)] seeded values inside each entry's range)."""
    rng = np.random.default_rng(seed)
    lo = np.array([d[2] for d in decl])
    hi = np.array([d[3] for d in decl])
    vals = (lo + (hi - lo) * rng.random((count, len(decl)))).astype(np.float32)
    return [(d[0], d[1]) for d in decl], vals


def _baked(spec, params, row):
    """The spec with one parameter vector written into its terms."""
    s = copy.deepcopy(spec)
    for (name, field), v in zip(params, row):
        s.terms[s.term_index(name)][field] = float(np.float32(v))
    return s


def _identity_row(spec, params):
    return np.array([spec.terms[spec.term_index(n)][f] for n, f in params], dtype=np.float32)


def _bound_problem(hip, spec, dtype, params, table):
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_params(params)
    prob.bind_instance_values(table)
    return prob


def _check_baked_equals_bound(hip, spec, decl, dtype, BV=4, seed=5, **kw):
    params, vals = _draw(decl, BV, seed)
    check_baked_equals_bound(hip, spec, dtype, lambda table: _bound_problem(hip, spec, dtype, params, table),
                             lambda row: _baked(spec, params, row), vals, seed=seed, **kw)


# ---- 1. baked equals bound, bit for bit ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("static_rows", [None, False])
@pytest.mark.parametrize("split_trial", [True, False])
@pytest.mark.parametrize("fixed_iters", [0, 6])
def test_headline_scene_bound_equals_baked(hip, dtype, static_rows, split_trial, fixed_iters):
    spec = _headline()
    if static_rows is None:
        assert hip.Problem(spec, dtype).row_program()[1] != 0, "the headline scene runs the static row code"
    _check_baked_equals_bound(hip, spec, HEADLINE_DECL, dtype, deterministic=True, static_rows=static_rows,
                              split_trial=split_trial, fixed_iters=fixed_iters)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_roundabout_open_loop_bound_equals_baked(hip, dtype):
    spec = examples.roundabout_merging()
    spec.params.max_solver_iters = 12
    _check_baked_equals_bound(hip, spec, ROUNDABOUT_DECL, dtype, B=8, deterministic=True)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_augmented_lagrangian_with_overridden_thresholds_bound_equals_baked(hip, dtype):
    """The multiplier update and the constraint error of the exit path read the term table in LDS."""
    spec = examples.three_player_collision_avoidance_reachability()
    spec.params.max_solver_iters = 12
    spec.params.unconstrained_solver_max_iters = 4
    _check_baked_equals_bound(hip, spec, AVOIDANCE_DECL, dtype, B=8, deterministic=True, augmented_lagrangian=True)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_extreme_value_children_bound_equals_baked(hip, dtype):
    spec = examples.three_player_intersection_reachability()
    spec.params.max_solver_iters = 12
    _check_baked_equals_bound(hip, spec, REACHABILITY_DECL, dtype, B=8, deterministic=True)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("padded_sweep", [True, False])
def test_run_time_dimensioned_kernels_bound_equals_baked(hip, dtype, padded_sweep):
    spec = examples.mixed_dubins_car_scene()
    spec.params.max_solver_iters = 12
    _check_baked_equals_bound(hip, spec, MIXED_DECL, dtype, B=8, deterministic=True, padded_sweep=padded_sweep)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_large_batch_schedule_bound_equals_baked(hip, dtype):
    """Without `deterministic`, at five or more instances per CU (the single-wave sweep): the partner is a homogeneous
    batch of the same size."""
    _, cus = hip.device_info()
    B = 6 * cus
    spec = _headline()
    _check_baked_equals_bound(hip, spec, HEADLINE_DECL, dtype, B=B, BV=2, whole_batch_partner=True, fixed_iters=4)
    prob = hip.Problem(spec, dtype)
    prob.solve(examples.jittered_x0(spec, B, seed=1), fixed_iters=1)
    assert prob.last_schedule() & abi.SCHEDULE_SINGLE_WAVE_SWEEP


# ---- 2. identity override ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene", ["headline", "avoidance"])
def test_identity_override_changes_nothing(hip, dtype, scene):
    spec, decl, kw = (_headline(), HEADLINE_DECL, {}) if scene == "headline" else \
        (examples.three_player_collision_avoidance_reachability(), AVOIDANCE_DECL, dict(augmented_lagrangian=True))
    spec.params.max_solver_iters = 10
    spec.params.unconstrained_solver_max_iters = 4
    B = 10
    params = [(d[0], d[1]) for d in decl]
    x0 = examples.jittered_x0(spec, B, seed=9)
    prob = hip.Problem(spec, dtype)
    plain = {k: _np(v) for k, v in prob.solve(x0, **kw).items() if k in KEYS}
    prob.declare_instance_params(params)
    prob.bind_instance_values(np.tile(_identity_row(spec, params), (B, 1)))
    bound = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(bound[k]), plain[k]), k
    prob.bind_instance_values(None)
    again = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(again[k]), plain[k]), k


# ---- 3. stage kernels against the oracle, a different vector per instance ----
@pytest.mark.parametrize("scene,decl", [("modified_three_player_intersection", HEADLINE_DECL),
                                        ("roundabout_merging", ROUNDABOUT_DECL),
                                        ("three_player_collision_avoidance_reachability", AVOIDANCE_DECL)])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_stage_kernels_match_per_vector_oracles(hip, oracle, scene, decl, dtype):
    """quadraticize (lambdas, mu, t_extreme) and total costs of a bound batch against one OracleProblem per parameter
    vector, at the oracle's operating point and with the tolerances of test_stage_kernels_match_oracle
    (tests/test_gpu_parity.py:344-349) for the same scenes and dtypes — independent of the device's own baked path."""
    from test_gpu_parity import _random_op
    spec = examples.CONFIGS[scene]()
    rng = np.random.default_rng(7)
    B = 4
    x0, xs_ref, us_ref, P, alpha = _random_op(spec, rng, B)
    scale = np.array([1.0, 0.5, 0.25, 0.1])
    params, vals = _draw(decl, B, seed=21)
    xs_o, us_o = oracle.OracleProblem(spec).rollout(dtype, x0, xs_ref, us_ref, P, alpha, scale)
    nc = spec.num_constraints
    lam = np.abs(rng.standard_normal((B, max(nc, 1), spec.T))) if nc else None
    mu = np.array([10.0, 11.0, 12.1, 5.0]) if nc else None
    te = rng.integers(0, spec.T, size=(B, len(spec.subsystems))).astype(np.int32)
    hp = _bound_problem(hip, spec, dtype, params, vals)
    quad_d = [_np(a) for a in hp.quadraticize(xs_o, us_o, lam, mu, te)]
    c_d, te_d = hp.total_costs(xs_o, us_o)
    plain = hip.Problem(spec, dtype)
    quad_plain = [_np(a) for a in plain.quadraticize(xs_o, us_o, lam, mu, te)]
    assert any(not _same_bits(a, b) for a, b in zip(quad_d, quad_plain)), "the drawn vectors should change the quadraticisation"
    tol = 1e-9 if dtype == abi.F64 else 2e-3
    for b in range(B):
        op = oracle.OracleProblem(_baked(spec, params, vals[b]))
        sl = slice(b, b + 1)
        quad_o = op.quadraticize(dtype, xs_o[sl], us_o[sl], None if lam is None else lam[sl],
                                 None if mu is None else mu[sl], te[sl])
        for name, a, o in zip("QlRr", quad_d, quad_o):
            err = rel_err(a[sl], o)
            print("instance %d %s rel err %.3e" % (b, name, err))
            assert err < tol, (b, name)
        c_o, te_o = op.total_costs(dtype, xs_o[sl], us_o[sl])
        err = rel_err(_np(c_d)[sl], c_o)
        print("instance %d total costs rel err %.3e" % (b, err))
        assert err < (1e-10 if dtype == abi.F64 else 1e-4), b
        assert np.array_equal(_np(te_d)[sl], te_o)


# ---- 4. it acts ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_nominal_speed_override_moves_the_player(hip, dtype):
    """Two instances of the headline scene, same x0, 20 fixed iterations from a zero warm start; player 1's nominal
    speed (term 11 of the spec: quadratic(0, 10.0, P1V, 8.0)) overridden to 6 and to 10.  The oracle, one problem per
    value, ends player 1 at y = 11.82, v = 5.005 for 6 and y = 16.25, v = 7.016 for 10; asserted here: the ordering with
    half of that gap as margin."""
    spec = _headline()
    assert spec.term_index("p1_nominal_speed") == 11
    x0 = np.tile(np.asarray(spec.x0, dtype=np.float64), (2, 1))
    prob = _bound_problem(hip, spec, dtype, [("p1_nominal_speed", "value")], np.array([[6.0], [10.0]], dtype=np.float32))
    xs = _np(prob.solve(x0, fixed_iters=20)["xs"]).astype(np.float64)
    P1Y, P1V = 1, 4
    print("final y", xs[:, -1, P1Y], "final v", xs[:, -1, P1V])
    assert xs[1, -1, P1Y] - xs[0, -1, P1Y] > 2.2
    assert xs[1, -1, P1V] - xs[0, -1, P1V] > 1.0


# ---- 5. solve_again under a mask after the values were rewritten on the device ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_solve_again_with_rewritten_values_and_mask(hip, dtype):
    import torch
    spec = _headline()
    spec.params.max_solver_iters = 8
    B, BV = 8, 4
    params, vals = _draw(HEADLINE_DECL, BV, seed=31)
    _, vals2 = _draw(HEADLINE_DECL, BV, seed=32)
    which = np.arange(B) % BV
    x0 = examples.jittered_x0(spec, B, seed=33)
    x0b = examples.jittered_x0(spec, B, seed=34)
    active = np.array([1, 0, 1, 1, 0, 1, 1, 0], dtype=np.int32)
    act_d = torch.as_tensor(active, device="cuda")
    prob = hip.Problem(spec, dtype)
    prob.single_wave_sweep = False  # pinned: the slices below must run the batch's schedule
    prob.declare_instance_params(params)
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
        p1 = hip.Problem(_baked(spec, params, vals[v]), dtype)
        p1.single_wave_sweep = False
        rb = p1.solve(x0[sel])
        for k in KEYS:
            assert _same_bits(first[k][sel], _np(rb[k])), (k, v)
        # the same solver state carried into a problem with the second vector: its workspace layout is the same
        p2 = hip.Problem(_baked(spec, params, vals2[v]), dtype)
        p2.single_wave_sweep = False
        p2.solve_again(x0b[sel], rb, active=act_d[torch.as_tensor(sel, device="cuda")].contiguous())
        for k in KEYS:
            for j, b in enumerate(sel):
                if active[b]:
                    assert _same_bits(out[k][b], _np(rb[k])[j]), (k, b)


# ---- 6. strategy costs and the Nash checks ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_strategy_costs_and_nash_checks_bound_equal_baked(hip, dtype):
    spec = examples.three_player_intersection_reachability(T=20)  # a max-over-time player: the sufficient check's copy
    spec.params.max_solver_iters = 6
    B = 4
    params, vals = _draw(REACHABILITY_DECL, B, seed=41)
    x0 = examples.jittered_x0(spec, B, seed=42)
    prob = _bound_problem(hip, spec, dtype, params, vals)
    sol = prob.solve(x0, deterministic=True)
    args = [sol[k] for k in ("xs", "us", "P", "alpha")]
    costs = _np(prob.strategy_costs(x0, *args))
    ok, margin = (_np(a) for a in prob.check_local_nash(x0, *args, max_perturbation=0.1))
    psd = _np(prob.check_sufficient_nash(sol["xs"], sol["us"]))
    costs_all = []
    for b in range(B):
        ref = hip.Problem(_baked(spec, params, vals[b]), dtype)
        a1 = [v[b:b + 1].contiguous() for v in args]
        c = _np(ref.strategy_costs(x0[b:b + 1], *a1))
        costs_all.append(c)
        assert _same_bits(costs[b:b + 1], c), b
        ok1, margin1 = (_np(a) for a in ref.check_local_nash(x0[b:b + 1], *a1, max_perturbation=0.1))
        assert _same_bits(ok[b:b + 1], ok1) and _same_bits(margin[b:b + 1], margin1), b
        assert _same_bits(psd[b:b + 1], _np(ref.check_sufficient_nash(a1[0], a1[1]))), b
    plain = _np(hip.Problem(spec, dtype).strategy_costs(x0, *args))
    assert not _same_bits(plain, costs), "the drawn vectors should change the strategy costs"


# ---- 7. errors, each before any kernel is launched ----
def test_declaration_and_binding_errors(hip):
    import torch
    spec = _headline()
    prob = hip.Problem(spec, abi.F64)
    B = 4
    x0 = examples.jittered_x0(spec, B, seed=1)
    table = torch.zeros((B, 1), dtype=torch.float32, device="cuda")
    with pytest.raises(hip.IlqgError) as e:  # bind without declare
        hip._check(hip.lib().ilqg_problem_bind_instance_values(prob.h, B, hip._ptr(table)))
    assert e.value.status == abi.ERR_INVALID and "declare" in str(e.value)
    with pytest.raises(hip.IlqgError) as e:  # refused declarations are errors on the handle too
        prob.declare_instance_params([("p1_nominal_speed", "value"), ("p1_nominal_speed", "value")])
    assert e.value.status == abi.ERR_UNSUPPORTED and "term 11" in str(e.value)
    prob.declare_instance_params([("p1_nominal_speed", "value")])
    prob.bind_instance_values(table.fill_(8.0))
    with pytest.raises(hip.IlqgError) as e:  # declare while bound
        prob.declare_instance_params([("p2_nominal_speed", "value")])
    assert e.value.status == abi.ERR_INVALID and "bound" in str(e.value)
    # batch mismatch: every cost-evaluating entry point
    x3 = x0[:3]
    bufs = prob.solve(x0, fixed_iters=1)
    a3 = [bufs[k][:3].contiguous() for k in ("xs", "us", "P", "alpha")]
    calls = [lambda: prob.solve(x3, fixed_iters=1), lambda: prob.quadraticize(a3[0], a3[1]),
             lambda: prob.total_costs(a3[0], a3[1]), lambda: prob.strategy_costs(x3, *a3),
             lambda: prob.check_local_nash(x3, *a3, max_perturbation=0.1), lambda: prob.check_sufficient_nash(a3[0], a3[1]),
             lambda: prob.solve_again(x3, prob.alloc_solve_buffers(3))]
    for q, call in enumerate(calls):
        with pytest.raises(hip.IlqgError) as e:
            call()
        assert e.value.status == abi.ERR_INVALID and "batch of 4" in str(e.value), q
    prob.linearize(a3[0], a3[1])  # evaluates no cost: unaffected
    prob.bind_instance_values(None)
    prob.solve(x3, fixed_iters=1)
    prob.declare_instance_params([])
    with pytest.raises(hip.IlqgError):
        hip._check(hip.lib().ilqg_problem_bind_instance_values(prob.h, B, hip._ptr(table)))


# ---- 8. the C++ mirror ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_host_mirror_solve_batch_with_instance_params(hip, dtype):
    """tests/host/instance_params_demo.cpp: GameSolver::SolveBatch(x0s, instance_params) on the headline scene built with
    the mirrored classes, its inputs and outputs written as raw arrays; the Python harness solves the same inputs on the
    descriptor the C++ flattener produced (its dump), declared by the indices the flattener resolved.  The mirror's
    containers are float, as the reference's: the harness's outputs are rounded to float before the exact comparison."""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "host", "_bin", "instance_params_demo")
    assert os.path.exists(exe), "build() compiles tests/host/instance_params_demo.cpp"
    B = 6
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.bin")
        subprocess.run([exe, "solve", "f64" if dtype == abi.F64 else "f32", str(B), out], check=True, timeout=300)
        raw = np.fromfile(out, dtype=np.float64)
    lines = subprocess.check_output([exe, "resolve"], text=True, timeout=120).splitlines()
    params = [tuple(int(v) for v in ln.split()) for ln in lines[:3]]
    spec = abi.ProblemSpec.from_dump("\n".join(lines[4:]))
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
    xs = take(B * T * n, (B, T, n))
    us = take(B * T * m, (B, T, m))
    assert at == raw.size
    prob = _bound_problem(hip, spec, dtype, params, vals)
    sol = prob.solve(x0)
    assert int(_np(sol["iters"]).min()) > 0
    assert _same_bits(_np(sol["xs"]).astype(np.float32), xs.astype(np.float32))
    assert _same_bits(_np(sol["us"]).astype(np.float32), us.astype(np.float32))
    plain = hip.Problem(spec, dtype).solve(x0)
    assert not _same_bits(_np(plain["xs"]).astype(np.float32), xs.astype(np.float32)), "the table must have acted"
