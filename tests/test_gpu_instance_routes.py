"""Per-instance routes on the device (ilqg_problem_declare_instance_routes / ilqg_problem_bind_instance_routes).

The core checks are EXACT: an instance of a heterogeneous batch must return the bits of the same instance solved in a
problem created with its polylines written into the descriptor (the points are floats on both paths, and the device
builds an instance's segments with the function the host builder calls), so nothing here has a tolerance except the
stage kernels against the oracle, which take the tolerances tests/test_gpu_instance_params.py takes for the same
comparison.  Every comparison runs over every instance and every output array."""
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


# ---- scenes: which points of which polyline move, and by how much at most (metres, each coordinate) ----
HEADLINE_ROUTES = [(1, (1, 2, 3, 4, 5), 1.5)]  # player 2's turn lane: the end of the straight and the bend
ZOO_ROUTES = [(2, (1, 2, 3), 1.0)]             # the wall of the signed-distance constraint: its bulge into lane 1
MIXED_ROUTES = [(0, (1, 2), 1.5)]              # the car's lane: its two inner vertices
REACH3_ROUTES = [(0, (0, 1, 2, 3), 1.0)]       # T = 20: player 2 is still on the straight, which moves sideways


def _displaced(spec, decl, count, seed):
    """-> (polylines, float32 [count][P][2]): the declared polylines' points, the listed ones displaced by a seeded draw."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(count):
        row = []
        for q, idx, amp in decl:
            pts = np.array(spec.polylines[q], dtype=np.float64)
            pts[list(idx)] += amp * (2.0 * rng.random((len(idx), 2)) - 1.0)
            row.append(pts)
        rows.append(np.concatenate(row))
    return [d[0] for d in decl], np.array(rows).astype(np.float32)


def _circles(spec, radii):
    """Route vectors of a scene whose polyline 0 is a circle about the origin: one radius each."""
    n = len(spec.polylines[0]) - 1
    return [0], np.array([examples.draw_circle((0.0, 0.0), r, n) for r in radii]).astype(np.float32)


def _baked(spec, polylines, row):
    """The spec with one route vector written into its polylines."""
    s = copy.deepcopy(spec)
    at = 0
    for q in polylines:
        k = len(s.polylines[q])
        s.polylines[q] = [(float(x), float(y)) for x, y in row[at:at + k]]
        at += k
    assert at == len(row)
    return s


def _identity_row(spec, polylines):
    return np.concatenate([np.array(spec.polylines[q], dtype=np.float32) for q in polylines])


def _bound_problem(hip, spec, dtype, polylines, table):
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_routes(polylines)
    prob.bind_instance_routes(table)
    return prob


def _check_baked_equals_bound(hip, spec, routes, dtype, BV=4, **kw):
    """routes: (polylines, float32 [BV][P][2]); instance b takes route vector b % BV."""
    polylines, vecs = routes
    assert len(vecs) == BV
    return check_baked_equals_bound(hip, spec, dtype, lambda table: _bound_problem(hip, spec, dtype, polylines, table),
                                    lambda row: _baked(spec, polylines, row), vecs, **kw)


def _vertex_hits(oracle, pts, xy, dtype):
    """How many of the positions xy [K][2] have their closest point of the polyline on one of its vertices."""
    return sum(1 for q in xy if oracle.polyline_closest_point(pts, (float(q[0]), float(q[1])), dtype)["is_vertex"])


# ---- 1. bound equals baked, bit for bit ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("static_rows", [None, False])
@pytest.mark.parametrize("split_trial", [True, False])
@pytest.mark.parametrize("fixed_iters", [0, 6])
def test_headline_scene_turn_lanes_bound_equal_baked(hip, oracle, dtype, static_rows, split_trial, fixed_iters):
    """Player 2's lane carries a QUADRATIC_POLYLINE2 and both SEMIQUADRATIC_POLYLINE2 terms.  A wrong base or stride shows
    at vertices and shortcuts: at least one instance's player 2 must have its closest lane point on a vertex (counted on the
    CPU with the oracle's Polyline2::ClosestPoint over the returned trajectories)."""
    spec = _headline()
    assert len(spec.polylines) == 3 and len(spec.polylines[1]) == 7
    if static_rows is None:
        assert hip.Problem(spec, dtype).row_program()[1] != 0, "the headline scene runs the static row code"
    routes = _displaced(spec, HEADLINE_ROUTES, 4, seed=3)
    _, out, _, which = _check_baked_equals_bound(hip, spec, routes, dtype, deterministic=True, static_rows=static_rows,
                                                 split_trial=split_trial, fixed_iters=fixed_iters)
    hits = sum(_vertex_hits(oracle, routes[1][which[b]], out["xs"][b][:, 5:7], dtype) for b in range(len(which)))
    print("rows of player 2 closest to a vertex of their own lane:", hits)
    assert hits > 0


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("probe_lanes", [True, False])
def test_reachability_target_radius_with_probing_bound_equals_baked(hip, dtype, probe_lanes):
    """POLYLINE2_SIGNED_DISTANCE of both players on a circle whose radius differs per instance, free-running with the
    speculative line search in both forms of its rollouts; the probing rows read the instance's table through the list
    slot's instance id."""
    spec = examples.two_player_reachability()
    spec.params.max_solver_iters = 8
    prob, _, x0, _ = _check_baked_equals_bound(hip, spec, _circles(spec, [0.5, 1.0, 1.5, 2.5]), dtype, B=12,
                                               whole_batch_partner=True, split_trial=True, probe=True,
                                               probe_lanes=probe_lanes)
    o = prob.solve(x0, split_trial=True, probe=True, probe_lanes=probe_lanes)
    assert int(_np(prob.solve_state(o)["backtracks"]).sum()) > 0, "the line searches should back-track: nothing was probed"


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_augmented_lagrangian_wall_constraint_bound_equals_baked(hip, dtype):
    """cost_zoo_scene's CONSTRAINT_POLYLINE2_SIGNED_DISTANCE on the `wall` polyline: the multiplier update and the
    constraint error of the exit path read the segment table from their LDS copy."""
    spec = examples.cost_zoo_scene()
    spec.params.max_solver_iters = 12
    spec.params.unconstrained_solver_max_iters = 4
    assert len(spec.polylines[2]) == 5
    _check_baked_equals_bound(hip, spec, _displaced(spec, ZOO_ROUTES, 4, seed=11), dtype, B=8, deterministic=True,
                              augmented_lagrangian=True)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("padded_sweep", [True, False])
def test_run_time_dimensioned_kernels_bound_equal_baked(hip, dtype, padded_sweep):
    spec = examples.mixed_dubins_car_scene()
    spec.params.max_solver_iters = 12
    _check_baked_equals_bound(hip, spec, _displaced(spec, MIXED_ROUTES, 4, seed=13), dtype, B=8, deterministic=True,
                              padded_sweep=padded_sweep)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_large_batch_schedule_bound_equals_baked(hip, dtype):
    """Without `deterministic`, at five or more instances per CU (the single-wave sweep, pinned): the partner is a
    homogeneous batch of the same size."""
    _, cus = hip.device_info()
    B = 6 * cus
    spec = _headline()
    _check_baked_equals_bound(hip, spec, _displaced(spec, HEADLINE_ROUTES, 2, seed=3), dtype, B=B, BV=2,
                              whole_batch_partner=True, fixed_iters=4, single_wave_sweep=True)
    prob = hip.Problem(spec, dtype)
    prob.solve(examples.jittered_x0(spec, B, seed=1), fixed_iters=1, single_wave_sweep=True)
    assert prob.last_schedule() & abi.SCHEDULE_SINGLE_WAVE_SWEEP


# ---- 2. routes and a value table together, bound in either order ----
VALUE_DECL = [("p2_nominal_speed", "value"), ("p2_lane", "weight")]
VALUE_ROWS = np.array([[4.5, 18.0], [7.5, 33.0], [6.0, 25.0]], dtype=np.float32)  # three vectors against four routes


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("routes_first", [True, False])
@pytest.mark.parametrize("static_rows", [None, False])
def test_routes_and_values_bound_together(hip, dtype, routes_first, static_rows):
    """Twelve instances, four routes against three value vectors: every instance its own combination.  The partner of
    route v is a problem created with it that binds the value rows of v's instances."""
    spec = _headline()
    B, kw = 12, dict(deterministic=True, static_rows=static_rows, fixed_iters=6)
    polylines, vecs = _displaced(spec, HEADLINE_ROUTES, 4, seed=3)
    which = np.arange(B) % 4
    values = VALUE_ROWS[np.arange(B) % 3]
    x0 = examples.jittered_x0(spec, B, seed=6)
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_params(VALUE_DECL)
    prob.declare_instance_routes(polylines)
    if routes_first:
        prob.bind_instance_routes(vecs[which])
    prob.bind_instance_values(values)
    if not routes_first:
        prob.bind_instance_routes(vecs[which])
    out = {k: _np(v) for k, v in prob.solve(x0, **kw).items() if k in KEYS}
    for v in range(4):
        sel = np.nonzero(which == v)[0]
        ref_prob = hip.Problem(_baked(spec, polylines, vecs[v]), dtype)
        ref_prob.declare_instance_params(VALUE_DECL)
        ref_prob.bind_instance_values(values[sel])
        ref = ref_prob.solve(x0[sel], **kw)
        for k in KEYS:
            assert _same_bits(out[k][sel], _np(ref[k])), (k, v)
    # unbinding one leaves the other bound
    prob.bind_instance_values(None)
    routes_only = _np(prob.solve(x0, **kw)["xs"])
    ref = _bound_problem(hip, spec, dtype, polylines, vecs[which]).solve(x0, **kw)
    assert _same_bits(routes_only, _np(ref["xs"])) and not _same_bits(routes_only, out["xs"])


# ---- 3. a table whose every row is the baked route ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene", ["headline", "zoo", "mixed"])
def test_identity_table_changes_nothing(hip, dtype, scene):
    spec, polylines, kw = {"headline": (_headline(), [1, 0], {}),
                           "zoo": (examples.cost_zoo_scene(), [2, 1], dict(augmented_lagrangian=True)),
                           "mixed": (examples.mixed_dubins_car_scene(), [0], {})}[scene]
    spec.params.max_solver_iters = 10
    spec.params.unconstrained_solver_max_iters = 4
    B = 10
    x0 = examples.jittered_x0(spec, B, seed=9)
    prob = hip.Problem(spec, dtype)
    plain = {k: _np(v) for k, v in prob.solve(x0, **kw).items() if k in KEYS}
    prob.declare_instance_routes(polylines)
    prob.bind_instance_routes(np.tile(_identity_row(spec, polylines), (B, 1, 1)))
    bound = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(bound[k]), plain[k]), k
    prob.bind_instance_routes(None)
    again = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(again[k]), plain[k]), k


# ---- 4. stage kernels against the oracle, a different route per instance ----
@pytest.mark.parametrize("scene,decl", [("modified_three_player_intersection", HEADLINE_ROUTES),
                                        ("cost_zoo_scene", ZOO_ROUTES)])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_stage_kernels_match_per_route_oracles(hip, oracle, scene, decl, dtype):
    """quadraticize (lambdas, mu, t_extreme) and total costs of a bound batch against one OracleProblem per route vector,
    at the oracle's operating point, with the tolerances of
    tests/test_gpu_instance_params.py::test_stage_kernels_match_per_vector_oracles."""
    from test_gpu_parity import _random_op
    spec = examples.CONFIGS[scene]() if scene in examples.CONFIGS else getattr(examples, scene)()
    rng = np.random.default_rng(7)
    B = 4
    x0, xs_ref, us_ref, P, alpha = _random_op(spec, rng, B)
    scale = np.array([1.0, 0.5, 0.25, 0.1])
    polylines, vecs = _displaced(spec, decl, B, seed=21)
    xs_o, us_o = oracle.OracleProblem(spec).rollout(dtype, x0, xs_ref, us_ref, P, alpha, scale)
    nc = spec.num_constraints
    lam = np.abs(rng.standard_normal((B, max(nc, 1), spec.T))) if nc else None
    mu = np.array([10.0, 11.0, 12.1, 5.0]) if nc else None
    te = rng.integers(0, spec.T, size=(B, len(spec.subsystems))).astype(np.int32)
    hp = _bound_problem(hip, spec, dtype, polylines, vecs)
    quad_d = [_np(a) for a in hp.quadraticize(xs_o, us_o, lam, mu, te)]
    c_d, te_d = hp.total_costs(xs_o, us_o)
    plain = hip.Problem(spec, dtype)
    quad_plain = [_np(a) for a in plain.quadraticize(xs_o, us_o, lam, mu, te)]
    assert any(not _same_bits(a, b) for a, b in zip(quad_d, quad_plain)), "the routes should change the quadraticisation"
    tol = 1e-9 if dtype == abi.F64 else 2e-3
    for b in range(B):
        op = oracle.OracleProblem(_baked(spec, polylines, vecs[b]))
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


# ---- 5. solve_again under a mask after the points were rewritten and bound again ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_solve_again_after_rebinding_rewritten_points_under_a_mask(hip, dtype):
    import torch
    spec = _headline()
    spec.params.max_solver_iters = 8
    B, BV = 8, 4
    polylines, vecs = _displaced(spec, HEADLINE_ROUTES, BV, seed=31)
    _, vecs2 = _displaced(spec, HEADLINE_ROUTES, BV, seed=32)
    which = np.arange(B) % BV
    x0 = examples.jittered_x0(spec, B, seed=33)
    x0b = examples.jittered_x0(spec, B, seed=34)
    active = np.array([1, 0, 1, 1, 0, 1, 1, 0], dtype=np.int32)
    act_d = torch.as_tensor(active, device="cuda")
    prob = hip.Problem(spec, dtype)
    prob.single_wave_sweep = False  # pinned: the slices below must run the batch's schedule
    prob.declare_instance_routes(polylines)
    table = prob.bind_instance_routes(torch.as_tensor(vecs[which], device="cuda").contiguous())
    bufs = prob.solve(x0)
    first = {k: _np(bufs[k]).copy() for k in KEYS}
    table.copy_(torch.as_tensor(vecs2[which], device="cuda"))  # rewritten on the device: consumed by the next bind
    prob.bind_instance_routes(table)
    prob.solve_again(x0b, bufs, active=act_d)
    out = {k: _np(bufs[k]) for k in KEYS}
    for b in np.nonzero(active == 0)[0]:
        for k in KEYS:
            assert _same_bits(out[k][b], first[k][b]), ("masked instance touched", b, k)
    changed = False
    for v in range(BV):
        sel = np.nonzero(which == v)[0]
        p1 = hip.Problem(_baked(spec, polylines, vecs[v]), dtype)
        p1.single_wave_sweep = False
        rb = p1.solve(x0[sel])
        for k in KEYS:
            assert _same_bits(first[k][sel], _np(rb[k])), (k, v)
        # the same solver state carried into a problem with the second route: its workspace layout is the same
        p2 = hip.Problem(_baked(spec, polylines, vecs2[v]), dtype)
        p2.single_wave_sweep = False
        p2.solve_again(x0b[sel], rb, active=act_d[torch.as_tensor(sel, device="cuda")].contiguous())
        for k in KEYS:
            for j, b in enumerate(sel):
                if active[b]:
                    assert _same_bits(out[k][b], _np(rb[k])[j]), (k, b)
                    changed = changed or (k == "xs" and not _same_bits(out[k][b], first[k][b]))
    assert changed


# ---- 6. strategy costs and the Nash checks ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_strategy_costs_and_nash_checks_bound_equal_baked(hip, dtype):
    spec = examples.three_player_intersection_reachability(T=20)  # a max-over-time player: the sufficient check's copy
    spec.params.max_solver_iters = 6
    B = 4
    polylines, vecs = _displaced(spec, REACH3_ROUTES, B, seed=41)
    x0 = examples.jittered_x0(spec, B, seed=42)
    prob = _bound_problem(hip, spec, dtype, polylines, vecs)
    sol = prob.solve(x0, deterministic=True)
    args = [sol[k] for k in ("xs", "us", "P", "alpha")]
    costs = _np(prob.strategy_costs(x0, *args))
    ok, margin = (_np(a) for a in prob.check_local_nash(x0, *args, max_perturbation=0.1))
    psd = _np(prob.check_sufficient_nash(sol["xs"], sol["us"]))
    for b in range(B):
        ref = hip.Problem(_baked(spec, polylines, vecs[b]), dtype)
        a1 = [v[b:b + 1].contiguous() for v in args]
        assert _same_bits(costs[b:b + 1], _np(ref.strategy_costs(x0[b:b + 1], *a1))), b
        ok1, margin1 = (_np(a) for a in ref.check_local_nash(x0[b:b + 1], *a1, max_perturbation=0.1))
        assert _same_bits(ok[b:b + 1], ok1) and _same_bits(margin[b:b + 1], margin1), b
        assert _same_bits(psd[b:b + 1], _np(ref.check_sufficient_nash(a1[0], a1[1]))), b
    plain = _np(hip.Problem(spec, dtype).strategy_costs(x0, *args))
    assert not _same_bits(plain, costs), "the routes should change the strategy costs"


# ---- 7. errors, each before any kernel is launched ----
def test_declaration_and_binding_errors(hip):
    import torch
    spec = _headline()
    prob = hip.Problem(spec, abi.F64)
    B = 4
    x0 = examples.jittered_x0(spec, B, seed=1)
    table = torch.as_tensor(np.tile(_identity_row(spec, [1]), (B, 1, 1)), device="cuda").contiguous()
    st = hip.C.c_void_p(0)
    with pytest.raises(hip.IlqgError) as e:  # bind without declare
        hip._check(hip.lib().ilqg_problem_bind_instance_routes(prob.h, B, hip._ptr(table), st))
    assert e.value.status == abi.ERR_INVALID and "declare" in str(e.value)
    for bad, word in (([3], "out of range"), ([-1], "out of range"), ([1, 0, 1], "twice")):
        with pytest.raises(hip.IlqgError) as e:  # refused declarations are errors on the handle too
            prob.declare_instance_routes(bad)
        assert e.value.status == abi.ERR_UNSUPPORTED and "polyline %d" % bad[-1] in str(e.value) and word in str(e.value)
    prob.declare_instance_routes([1])
    with pytest.raises(hip.IlqgError) as e:
        hip._check(hip.lib().ilqg_problem_bind_instance_routes(prob.h, 0, hip._ptr(table), st))
    assert e.value.status == abi.ERR_INVALID and "batch" in str(e.value)
    prob.bind_instance_routes(table)
    with pytest.raises(hip.IlqgError) as e:  # declare while bound
        prob.declare_instance_routes([0])
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
    prob.linearize(a3[0], a3[1])  # evaluates no cost: ignores the binding
    # a value table for another batch beside the routes, and the other way round
    prob.declare_instance_params([("p1_nominal_speed", "value")])
    with pytest.raises(hip.IlqgError) as e:
        prob.bind_instance_values(np.full((3, 1), 8.0, dtype=np.float32))
    assert e.value.status == abi.ERR_INVALID and "batch of 4" in str(e.value)
    prob.bind_instance_routes(None)
    prob.bind_instance_values(np.full((3, 1), 8.0, dtype=np.float32))
    with pytest.raises(hip.IlqgError) as e:
        prob.bind_instance_routes(table)
    assert e.value.status == abi.ERR_INVALID and "batch of 3" in str(e.value)
    prob.bind_instance_values(None)
    prob.solve(x3, fixed_iters=1)
    prob.declare_instance_routes([])
    with pytest.raises(hip.IlqgError):
        hip._check(hip.lib().ilqg_problem_bind_instance_routes(prob.h, B, hip._ptr(table), st))


def test_route_progress_polyline_is_refused_on_the_handle(hip):
    """A ROUTE_PROGRESS term tabulates its nominals from the baked polyline: its polyline is refused, naming the term;
    another polyline of the same problem is accepted."""
    spec = _headline()
    term = spec.route_progress(0, 5.0, 4.0, 0, (0, 1), 10.0)
    prob = hip.Problem(spec, abi.F64)
    with pytest.raises(hip.IlqgError) as e:
        prob.declare_instance_routes([1, 0])
    assert e.value.status == abi.ERR_UNSUPPORTED and "term %d" % term in str(e.value) and "ROUTE_PROGRESS" in str(e.value)
    prob.declare_instance_routes([1, 2])


# ---- 8. the C++ mirror ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_host_mirror_solve_batch_with_instance_routes(hip, dtype):
    """tests/host/instance_routes_demo.cpp: GameSolver::SolveBatch(x0s, instance_params) with AddRoute on the headline scene
    built with the mirrored classes, its inputs and outputs written as raw arrays; the Python harness solves the same
    inputs on the descriptor the C++ flattener produced, with the polyline the flattener resolved.  The mirror's
    containers are float, as the reference's: the harness's outputs are rounded to float before the exact comparison."""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "host", "_bin", "instance_routes_demo")
    assert os.path.exists(exe), "build() compiles tests/host/instance_routes_demo.cpp"
    B = 6
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.bin")
        subprocess.run([exe, "solve", "f64" if dtype == abi.F64 else "f32", str(B), out], check=True, timeout=300)
        raw = np.fromfile(out, dtype=np.float64)
    lines = subprocess.check_output([exe, "resolve"], text=True, timeout=120).splitlines()
    polyline = int(lines[0].split()[1])
    spec = abi.ProblemSpec.from_dump("\n".join(lines[lines.index("dump") + 1:]))
    assert spec.canonical() == _headline().canonical()
    n, m, T = spec.n, spec.m, spec.T
    P = len(spec.polylines[polyline])
    at = 0

    def take(k, shape):
        nonlocal at
        a = raw[at:at + k].reshape(shape)
        at += k
        return a
    x0 = take(B * n, (B, n))
    pts = take(B * P * 2, (B, P, 2)).astype(np.float32)
    xs = take(B * T * n, (B, T, n))
    us = take(B * T * m, (B, T, m))
    assert at == raw.size
    prob = _bound_problem(hip, spec, dtype, [polyline], pts)
    sol = prob.solve(x0)
    assert int(_np(sol["iters"]).min()) > 0
    assert _same_bits(_np(sol["xs"]).astype(np.float32), xs.astype(np.float32))
    assert _same_bits(_np(sol["us"]).astype(np.float32), us.astype(np.float32))
    plain = hip.Problem(spec, dtype).solve(x0)
    assert not _same_bits(_np(plain["xs"]).astype(np.float32), xs.astype(np.float32)), "the routes must have acted"
