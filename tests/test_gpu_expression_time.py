"""The time as an input of expression programs (ILQG_EXPR_PUSH_TIME) on the device.

1. Row k of a time-reading problem carries the bits of row k of the same problem with the time leaf replaced by the
   constant t_k (dt = 0.125: every t_k is exact in float32) — Q, l, R, r, and A, B of a time-reading model row.
2. examples.time_expression_twin against the built-in NominalPathLengthCost: stage parity and a forced-step solve under
   the project's conditioning probe.
3. The whole solve against the independent numpy reference of tests/lq_time_games.py, after every forced iteration, at
   100 x the committed gaps, on the pinned schedules of tests/test_gpu_lq_games.py.
4. The multiplier update of AugmentedLagrangianSolver on a moving keep-out zone: lambda + mu g(t_k, x_k), per (slot, k).
5. The paths around the solve: schedules, strategy costs and the Nash check (feedback and open loop), per-instance
   parameters, the FinalTimeCost gate, a receding-horizon replan, and the refusal of the plan kernels for a model that
   reads the time.
T = 8 or 12 and B = 3 throughout.  No oracle: it does not know the opcode."""
import copy
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import lq_games as G
import lq_time_games as TG
from ilqgames_amd import abi, examples
from ilqgames_amd.abi import Expr
from helpers import GOLDEN, rel_err
from instance_harness import KEYS, check_baked_equals_bound, same_bits, to_numpy as _np
from test_gpu_lq_games import PINNED, PINS, _device_iterations

pytestmark = pytest.mark.gpu

T, B = 12, 3
TIME, CONST = abi.EXPR_PUSH_TIME, abi.EXPR_PUSH_CONST
EXPRESSION_KINDS = (abi.COST_EXPRESSION, abi.CONSTRAINT_EXPRESSION, abi.DYN_ROW_EXPRESSION)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


def _tol(dtype):
    return 1e-9 if dtype == abi.F64 else 2e-4


def _operating_points(spec, dtype, seed=21):
    """Random operating points around jittered initial states -> (xs, us) as numpy arrays of the dtype."""
    NT = np.float64 if dtype == abi.F64 else np.float32
    rng = np.random.default_rng(seed)
    x0 = examples.jittered_x0(spec, B, seed=seed)
    xs = np.tile(x0[:, None, :], (1, spec.T, 1)) + 0.3 * rng.standard_normal((B, spec.T, spec.n))
    us = 0.2 * rng.standard_normal((B, spec.T, spec.m))
    return xs.astype(NT), us.astype(NT)


def _multipliers(nc, horizon, seed=3):
    rng = np.random.default_rng(seed)
    lam = np.abs(rng.standard_normal((B, nc, horizon)))
    lam[:, :, ::3] = 0.0
    return lam, np.array([10.0, 11.0, 12.1])


# ------------------------------------------------------------------------------------------------
# 1. the exact test against per-step constant programs
# ------------------------------------------------------------------------------------------------
def frozen(spec, t):
    """`spec` with every time leaf of every program replaced by PUSH_CONST t (t exact in float32)."""
    assert float(np.float32(t)) == float(t)
    s = copy.deepcopy(spec)
    count = 0
    for term in s.terms:
        if term["kind"] not in EXPRESSION_KINDS:
            continue
        off = term["polyline"]
        for i in range(int(s.dense_params[off])):
            if int(s.dense_params[off + 1 + 2 * i]) == TIME:
                s.dense_params[off + 1 + 2 * i], s.dense_params[off + 2 + 2 * i] = float(CONST), float(t)
                count += 1
    return s, count


def timed_cars(cars, horizon, dt):
    """`cars` gusting cars (examples.gusting_car_rows: the heading rate reads the time) — two: the specialised (8, 2, 1)
    kernels, three: the run-time-dimensioned ones — with time-reading terms of every other role: car 1 keeps away from a
    walking pedestrian (a Gaussian bump cost and a keep-out constraint over two states), car 2 follows a reference x_ref(t)
    on one state, and its curvature is penalised about a swaying nominal with a weight that grows with the time (a
    control cost, so R and r read the time)."""
    x, y, w, v, t = Expr.x(), Expr.y(), Expr.weight(), Expr.value(), Expr.time()
    s = abi.ProblemSpec(horizon, dt)
    for _ in range(cars):
        s.add_expression_player(4, 1, examples.gusting_car_rows(), param0=examples.COASTING_CAR_DRAG,
                                weights=[1.0, 1.0, examples.GUSTING_CAR_AMPLITUDE, 1.0])
    for i in range(cars):
        s.quadratic(i, 1.0, 0, 0.0, control_of=i)
        s.quadratic(i, 1.0, 4 * i, 0.0)
    dx, dy = examples.moving_obstacle_offset(x, 1.0, -2.0), examples.moving_obstacle_offset(y, 0.5, 1.0)
    s.name_term("bump", s.expression(0, ((dx.square() + dy.square()) * -0.5 / v.square()).exp() * w, (0, 1), weight=8.0, value=2.0))
    s.name_term("keep_out", s.expression_constraint(0, v.square() - dx.square() - dy.square(), (0, 1), value=1.5))
    s.name_term("reference", s.expression(1, 0.5 * w * (x - v * t).square(), (4,), weight=3.0, value=1.5))
    s.name_term("sway", s.expression(1, (w + t) * (x - (v * t).sin()).square(), (0,), weight=2.0, value=3.0, control_of=1))
    s.x0 = [0.5 * q for q in range(4 * cars)]
    s.position_dims = [(4 * i, 4 * i + 1) for i in range(cars)]
    s.heading_dims, s.speed_dims = [4 * i + 2 for i in range(cars)], [4 * i + 3 for i in range(cars)]
    return s


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("cars", [2, 3], ids=["8_2_1", "run_time_dims"])
def test_row_k_carries_the_bits_of_the_program_with_the_constant_t_k(hip, dtype, cars):
    horizon, dt = 8, 0.125
    spec = timed_cars(cars, horizon, dt)
    prob = hip.Problem(spec, dtype)
    generic = cars == 3
    xs, us = _operating_points(spec, dtype)
    lam, mu = _multipliers(spec.num_constraints, horizon)
    got = [_np(a) for a in prob.quadraticize(xs, us, lam, mu)] + [_np(a) for a in prob.linearize(xs, us)]
    costs = _np(prob.total_costs(xs, us)[0])
    at_zero = None
    moved = set()
    for k in range(horizon):
        const, count = frozen(spec, k * dt)
        assert count == cars + 7  # a leaf per heading row; two each in the bump, the disc and the sway, one in the reference
        cp = hip.Problem(const, dtype)
        want = [_np(a) for a in cp.quadraticize(xs, us, lam, mu)] + [_np(a) for a in cp.linearize(xs, us)]
        if k == 0:
            at_zero = want
        for name, a, b, z in zip(("Q", "l", "R", "r", "A", "B"), got, want, at_zero):
            assert same_bits(a[:, k], b[:, k]), (name, k)
            if k > 0 and not same_bits(a[:, k], z[:, k]):
                moved.add(name)
    # every array but the two a time-reading row cannot reach: the gust has no derivative, so A and B are the cars' own
    assert moved == {"Q", "l", "R", "r"}, moved
    assert np.isfinite(costs).all()
    # the schedule the shape stands for
    out = prob.solve(np.tile(np.asarray(spec.x0), (B, 1)), fixed_iters=1)
    assert bool(prob.last_schedule() & abi.SCHEDULE_GENERIC) == generic
    assert np.all(np.isfinite(_np(out["xs"])))


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_a_model_row_that_multiplies_the_state_by_the_time_puts_it_into_A_and_B(hip, dtype):
    """x sin(t) + u cos(t) and x y t (tests/test_expression_time.py's model, here on the device): row k of A and B is
    that of the model with the constant t_k, and the entries are I + dt J at t_k."""
    horizon, dt = 8, 0.125
    NT = np.float64 if dtype == abi.F64 else np.float32
    x, y, t = Expr.x(), Expr.y(), Expr.time()
    s = abi.ProblemSpec(horizon, dt)
    for _ in range(2):
        s.add_expression_player(2, 1, [(x * t.sin() + y * t.cos(), 0, 2), (x * y * t, 0, 1)])
        s.quadratic(len(s.subsystems) - 1, 1.0, 0, 0.0, control_of=len(s.subsystems) - 1)
    s.x0 = [0.5, -0.25, 1.0, 0.75]
    rng = np.random.default_rng(5)
    xs, us = rng.uniform(-1.5, 1.5, (B, horizon, 4)).astype(NT), rng.uniform(-1, 1, (B, horizon, 2)).astype(NT)
    A, Bm = [_np(a) for a in hip.Problem(s, dtype).linearize(xs, us)]
    for k in range(horizon):
        Ak, Bk = [_np(a) for a in hip.Problem(frozen(s, k * dt)[0], dtype).linearize(xs, us)]
        assert same_bits(A[:, k], Ak[:, k]) and same_bits(Bm[:, k], Bk[:, k]), k
        tk = k * dt
        for b in range(B):
            want = np.eye(4)
            for o in (0, 2):
                want[o, o] += dt * np.sin(tk)
                want[o + 1, o], want[o + 1, o + 1] = dt * xs[b, k, o + 1] * tk, 1.0 + dt * xs[b, k, o] * tk
            a = A[b, k].reshape(4, 4).T  # column-major words
            assert np.abs(a - want).max() <= (1e-12 if dtype == abi.F64 else 1e-5), (k, b)
            bw = np.zeros((4, 2))
            bw[0, 0] = bw[2, 1] = dt * np.cos(tk)
            assert np.abs(Bm[b, k].reshape(2, 4).T - bw).max() <= (1e-12 if dtype == abi.F64 else 1e-5), (k, b)


# ------------------------------------------------------------------------------------------------
# 2. the twin against NominalPathLengthCost
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_twin_quadraticizes_and_costs_like_the_built_in_kind(hip, dtype):
    """dynamics_zoo_scene and examples.time_expression_twin of it (NominalPathLengthCost as 0.5 w (x - t v)^2 through the
    time leaf; RouteProgressCost stays) at 3 jittered operating points: Q, l, R, r and the total costs to the project's
    parity bars against each array's largest entry."""
    spec = examples.dynamics_zoo_scene(T=T)
    twin, count = examples.time_expression_twin(spec)
    assert count == 1
    orig_p, twin_p = hip.Problem(spec, dtype), hip.Problem(twin, dtype)
    xs, us = _operating_points(spec, dtype)
    tol = _tol(dtype)
    for name, a, b in zip("QlRr", twin_p.quadraticize(xs, us), orig_p.quadraticize(xs, us)):
        err = rel_err(_np(a), _np(b))
        print(dtype, name, "%.3e" % err)
        assert err < tol, (name, err)
    c_t, c_o = _np(twin_p.total_costs(xs, us)[0]), _np(orig_p.total_costs(xs, us)[0])
    print(dtype, "costs %.3e" % rel_err(c_t, c_o))
    assert rel_err(c_t, c_o) < tol and np.all(np.isfinite(c_t))
    # the term is at work and reads the time: with its leaf frozen at t = 0 the gradient is another one
    dim = next(t["idx"][0] for t in spec.terms if t["kind"] == abi.COST_NOMINAL_PATH_LENGTH)
    still = _np(hip.Problem(frozen(twin, 0.0)[0], dtype).quadraticize(xs, us)[1])[:, :, 1, dim]
    moving = _np(twin_p.quadraticize(xs, us)[1])[:, :, 1, dim]
    assert same_bits(still[:, 0], moving[:, 0]) and np.abs(still[:, 1:] - moving[:, 1:]).min() > 0.1  # w v t_k = 0.25 k


def _probe_ratios(ref, nud, out):
    ratios = {}
    for k in ("xs", "us", "P", "alpha"):
        r, n_, o = _np(ref[k]), _np(nud[k]), _np(out[k])
        for b in range(r.shape[0]):
            probe = max(rel_err(n_[b], r[b]), 1e-12)
            ratios[(k, b)] = rel_err(o[b], r[b]) / probe
            print("instance %d %-5s twin %.3e  nudged %.3e  ratio %.1e" % (b, k, rel_err(o[b], r[b]), probe, ratios[(k, b)]))
    return ratios


def test_twin_solves_like_the_built_in_kind_within_the_measured_conditioning(hip):
    """The scene and its twin under forced steps (3 iterations of 0.1, fp64), and the original once more from x0 nudged by
    1e-12 relative (DESIGN.md section 2's conditioning probe).  Per instance and per output the twin may be at most 10 x
    as far from the original as the nudged run is, floor 1e-12 relative.  Every instance counts."""
    spec = examples.dynamics_zoo_scene(T=T)
    twin, _ = examples.time_expression_twin(spec)
    K = 3
    x0 = examples.jittered_x0(spec, B, seed=31)
    nudged_x0 = x0 * (1.0 + 1e-12 * np.random.default_rng(5).standard_normal(x0.shape))
    kw = dict(fixed_iters=K, forced_steps=np.full((B, K), 0.1))
    ref = hip.Problem(spec, abi.F64).solve(x0, **kw)
    nud = hip.Problem(spec, abi.F64).solve(nudged_x0, **kw)
    out = hip.Problem(twin, abi.F64).solve(x0, **kw)
    ratios = _probe_ratios(ref, nud, out)
    assert np.array_equal(_np(out["iters"]), _np(ref["iters"]))
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 10.0, (worst, ratios[worst])


# ------------------------------------------------------------------------------------------------
# 3. the solve against the independent numpy reference
# ------------------------------------------------------------------------------------------------
TIME_PINS = {"8_2_1": PINS["8_2_1_computed_b"], "14_3_2": PINS["14_3_2"], "8_2_1_open_loop": PINS["8_2_1_open_loop"]}
assert set(TIME_PINS) == set(TG.GAMES)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(TG.GAMES))
def test_every_instance_matches_the_reference_after_every_iteration_on_every_pinned_schedule(hip, name, precision):
    """tests/test_gpu_lq_games.py's comparison on the games of tests/lq_time_games.py: tracking terms 0.5 w (x - v t)^2 on
    two players and a forcing a sin(omega t) on one rate.  After every forced iteration every instance is compared on
    every output at 100 x the committed gap of that game (tests/golden/lq_time_games.json), floored at 100 ulp."""
    committed = json.load(open(os.path.join(GOLDEN, "lq_time_games.json")))
    game = TG.GAMES[name]()
    dtype = abi.F64 if precision == "f64" else abi.F32
    ref = TG.cached_run(name, "float64" if precision == "f64" else "float32")
    x0 = game.x0(TG.B, TG.SEED)
    prob = hip.Problem(game.spec, dtype)
    bars = {q: G.bar(committed, name, q, precision) for q in G.OUTPUTS}
    gap = committed[name]["gap64" if precision == "f64" else "gap32"]
    worst, failures = {}, []
    for pin, want, (also_set, also_clear) in TIME_PINS[name]:
        dev, sched = _device_iterations(prob, x0, **pin)
        print("%s %s pin %s: schedule 0x%x" % (name, precision, pin, sched))
        if sched & PINNED != want or sched & also_set != also_set or sched & also_clear:
            failures.append((pin, "schedule 0x%x" % sched))
        for k in range(len(G.STEPS)):
            for q in G.OUTPUTS:
                err = G.errors(q, dev[k], ref[k], ref[0])
                assert err.shape == (TG.B,)
                worst[q] = max(worst.get(q, 0.0), float(err.max()) / max(gap[q], G.EPS[precision]))
                if not err.max() <= bars[q]:
                    failures.append((pin, k + 1, q, float(err.max()), bars[q]))
    print("%s %s: largest device-to-reference distance in units of the committed gap: %s" % (
        name, precision, " ".join("%s %.1f" % (q, worst[q]) for q in G.OUTPUTS)))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------
# 4. the multiplier update on a moving keep-out zone
# ------------------------------------------------------------------------------------------------
def ws_layout(n, m, N, horizon, Rsz, rsz, num_constraints):
    """csrc/ilqg_solve.hpp's WsLayout of a feedback augmented-Lagrangian solve, in elements: where an instance's solver
    state and its multipliers lie in its slice of the workspace.  (Checked below against ilqg_solve_state_batch.)"""
    o = 0
    at = {}
    for name, cnt in (("xs1", horizon * n), ("us1", horizon * m), ("P1", horizon * m * n), ("al1", horizon * m),
                      ("A", horizon * n * n), ("B", horizon * n * m), ("Q", horizon * N * n * n), ("l", horizon * N * n),
                      ("R", horizon * Rsz), ("r", horizon * rsz), ("lqscr", horizon * (N * (n + 1) + n)), ("dx", horizon * n),
                      ("mpart", horizon * N * 2), ("cpart", horizon * N), ("ints", 2 * 8), ("state", 32),
                      ("lambdas", num_constraints * horizon), ("wxs", horizon * n), ("wus", horizon * m),
                      ("wP", horizon * m * n), ("wal", horizon * m)):
        at[name] = o
        o += (cnt + 3) & ~3
    at["total"] = o
    return at


def keep_out_g(x, y, t, radius, NT):
    """moving_obstacle_scene's keep-out program at (x, y, t), operation by operation in NT."""
    (cx, cy), (vx, vy) = examples.MOVING_OBSTACLE_START, examples.MOVING_OBSTACLE_VELOCITY
    f = lambda c: NT(np.float32(c))  # noqa: E731  an immediate is a float
    dx = (NT(x) - f(cx)) - f(vx) * NT(t)
    dy = (NT(y) - f(cy)) - f(vy) * NT(t)
    v = NT(np.float32(radius))
    return (v * v - dx * dx) - dy * dy


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_multipliers_after_one_outer_iteration_are_lambda_plus_mu_g_at_t_k(hip, dtype):
    """AugmentedLagrangianSolver on moving_obstacle_scene, cut to one multiplier update: the first inner solve takes its
    two iterations (unconstrained_solver_max_iters = 2, a convergence tolerance it cannot meet), the update follows, and
    the second inner solve fills the log (max_solver_iters = 4).  The multipliers the workspace then holds equal, per
    (slot, k), max(0, 0 + mu g(t_k, x_k)) on the last iterate of the first inner solve — restated in numpy in the solve's
    scalar type, with the reference's TimeIndex aliasing — to a few ulp (the update may contract to an FMA).  With g
    evaluated at t = 0 for every step, what the update did before it was handed the step, they do not."""
    import torch
    NT = np.float64 if dtype == abi.F64 else np.float32
    spec = examples.moving_obstacle_scene(T=T)
    J = 2
    spec.params.unconstrained_solver_max_iters = J
    spec.params.convergence_tolerance = 1e-9
    spec.params.max_solver_iters = J + 2
    spec.params.geometric_lambda_downscaling = spec.params.geometric_mu_downscaling = 1.0  # (a failed second inner solve
    #                                                                       would otherwise scale what is compared)
    prob = hip.Problem(spec, dtype)
    x0 = examples.jittered_x0(spec, B, seed=13)  # (every instance's coasting path crosses the zone about step 10)
    bufs = prob.solve(x0, augmented_lagrangian=True, deterministic=True, log_capacity=8)
    torch.cuda.synchronize()
    count = _np(bufs["log"]["count"])
    assert np.all(count >= J + 2) and np.all(count <= 2 * J + 2), count
    L = ws_layout(spec.n, spec.m, 2, T, prob.Rsz, prob.rsz, spec.num_constraints)
    assert prob.workspace_bytes(B) >= B * L["total"] * np.dtype(NT).itemsize
    ws = _np(bufs["ws"])[:B * L["total"] * np.dtype(NT).itemsize].view(NT).reshape(B, L["total"])
    # the restated layout is the library's: the state slot holds what ilqg_solve_state_batch reports
    words = 16 * 4 // np.dtype(NT).itemsize  # SolveState's sixteen ints
    state = prob.solve_state(bufs, augmented_lagrangian=True)
    assert same_bits(ws[:, L["state"] + words + 0], _np(state["step"]))  # (the accepted step it reports: acc_scale)
    assert same_bits(ws[:, L["state"] + words + 2], _np(state["last_merit"]))
    assert same_bits(ws[:, L["state"] + words + 3], _np(state["expected_decrease"]))
    # ... and its integers say which log entry the update saw: two inner solves, the first with its J accepted iterations
    ints = np.ascontiguousarray(ws[:, L["state"]:L["state"] + words]).view(np.int32).reshape(B, 16)
    accepted_last, logged, inner_calls = ints[:, 7], ints[:, 10], ints[:, 11]
    assert np.all(inner_calls == 2) and np.array_equal(logged, _np(bufs["iters"])), (inner_calls, logged, count)
    assert np.all(logged - 2 - accepted_last == J), (logged, accepted_last)
    mu_after = ws[:, L["state"] + words + 5]
    mu0 = NT(10.0)  # Constraint::mu_ = kDefaultMu
    assert np.all(mu_after == mu0 * NT(np.float32(spec.params.geometric_mu_scaling)))
    lam = ws[:, L["lambdas"]:L["lambdas"] + spec.num_constraints * T].reshape(B, spec.num_constraints, T)
    slot = spec.terms[spec.term_index("p1_pedestrian_keep_out")]["constraint_slot"]
    radius = spec.terms[spec.term_index("p1_pedestrian_keep_out")]["value"]
    xs = _np(bufs["log"]["xs"])[:, J]  # the last iterate of the first inner solve
    dt = spec.dt
    # Constraint::IncrementLambda at TimeIndex(t0 + dt float(k)): now and then a step lands on its predecessor's slot
    tidx = [int((dt * float(np.float32(k))) / dt) for k in range(T)]
    want, want_t0, g_all = np.zeros((B, T), NT), np.zeros((B, T), NT), np.zeros((B, T))
    for b in range(B):
        for k in range(T):
            for w, t in ((want, NT(np.float64(k) * dt)), (want_t0, NT(0))):
                g = keep_out_g(xs[b, k, 0], xs[b, k, 1], t, radius, NT)
                nl = w[b, tidx[k]] + mu0 * g
                w[b, tidx[k]] = nl if nl > 0 else NT(0)
            g_all[b, k] = float(keep_out_g(xs[b, k, 0], xs[b, k, 1], NT(np.float64(k) * dt), radius, NT))
    print(dtype, "g", g_all[0], "lambda", lam[0, slot])
    # not vacuous: the zone is entered at steps past the second (in every instance, as the scene and the seed are chosen)
    assert np.any(g_all[:, 2:] > 0), g_all
    assert all(np.any(g_all[b, 2:] > 0) for b in range(B)), g_all
    ulp = np.finfo(NT).eps
    assert np.abs(lam[:, slot] - want).max() <= 8 * ulp * np.abs(want).max(), (lam[:, slot], want)
    assert np.abs(want_t0 - want).max() > 1e-3 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------
# 5. the paths around the solve
# ------------------------------------------------------------------------------------------------
def _free_running(hip, spec, dtype, x0, **kw):
    prob = hip.Problem(spec, dtype)
    out = prob.solve(x0, deterministic=True, **kw)
    return prob, {k: _np(v) for k, v in out.items() if k in KEYS}


def test_every_schedule_of_the_solve_returns_the_same_bits(hip):
    spec = examples.moving_obstacle_scene(T=T)
    spec.params.max_solver_iters = 20
    x0 = examples.jittered_x0(spec, B, seed=41)
    for al in (False, True):
        prob, ref = _free_running(hip, spec, abi.F64, x0, augmented_lagrangian=al)
        assert int(ref["iters"].min()) > 1 and np.all(np.isfinite(ref["xs"]))
        seen = set()
        for kw in (dict(split_trial=True), dict(split_trial=False), dict(compact_rows=False), dict(compact_rows=True),
                   dict(split_trial=True, compact_rows=False), dict(static_rows=True), dict(handoff=False),
                   dict(generic_kernels=True)):
            p, out = _free_running(hip, spec, abi.F64, x0, augmented_lagrangian=al, **kw)
            seen.add(p.last_schedule() & (abi.SCHEDULE_SPLIT_TRIAL | abi.SCHEDULE_COMPACT_ROWS | abi.SCHEDULE_GENERIC))
            if "split_trial" in kw:
                assert bool(p.last_schedule() & abi.SCHEDULE_SPLIT_TRIAL) == kw["split_trial"]
            if "compact_rows" in kw:
                assert bool(p.last_schedule() & abi.SCHEDULE_COMPACT_ROWS) == kw["compact_rows"]
            if "generic_kernels" in kw:  # other kernels, other roundings: finite, and close
                assert p.last_schedule() & abi.SCHEDULE_GENERIC
                assert np.all(np.isfinite(out["xs"]))
                continue
            for k in KEYS:
                assert same_bits(out[k], ref[k]), (al, kw, k)
        assert len(seen) >= 3


@pytest.mark.parametrize("scene", ["moving_obstacle_scene", "gusting_car_scene"])
def test_equilibrium_checks_evaluate_the_time_reading_terms(hip, scene):
    """ilqg_strategy_costs_batch replays the converged gains with the feed-forward zeroed under the RK4 — for the gusting
    car with the gust at the stage times, as the solve's own rollout has it: it retraces the operating point, so its sums
    (term_evaluate_leaf at step k) are the row stage's total costs to accumulation error (1e-9)."""
    spec = getattr(examples, scene)(T=T)
    spec.params.max_solver_iters = 30
    x0 = examples.jittered_x0(spec, B, seed=47)
    prob = hip.Problem(spec, abi.F64)
    out = prob.solve(x0, deterministic=True)
    xs, us, P = _np(out["xs"]), _np(out["us"]), _np(out["P"])
    zero = np.zeros_like(_np(out["alpha"]))
    replay = _np(prob.strategy_costs(x0, xs, us, P, zero, euler=False))
    total = _np(prob.total_costs(xs, us)[0])
    assert np.all(np.isfinite(total)) and rel_err(replay, total) < 1e-9, (replay, total)
    # the time is part of both sums: the same trajectory costs something else with the clock stopped at t = 0
    still = hip.Problem(frozen(spec, 0.0)[0], abi.F64)
    if scene == "moving_obstacle_scene":
        assert rel_err(_np(still.total_costs(xs, us)[0]), total) > 1e-6
        assert rel_err(_np(still.strategy_costs(x0, xs, us, P, zero, euler=False)), replay) > 1e-6
    else:  # a stopped gust is no gust: the replay leaves the operating point
        assert rel_err(_np(still.strategy_costs(x0, xs, us, P, zero, euler=False)), replay) > 1e-6
    ok, margin = prob.check_local_nash(x0, xs, us, P, _np(out["alpha"]), 1e-2)
    assert np.all(np.isfinite(_np(margin))) and _np(ok).shape == (B,)


@pytest.mark.parametrize("euler", [False, True])
def test_open_loop_strategy_costs_evaluate_state_costs_at_the_next_step_s_time(hip, euler):
    """ComputeStrategyCosts' open-loop form on the tracking game of tests/lq_time_games.py against numpy: u_k = us_k, the
    forced rollout (RK4 at the stage times, or Euler at t_k), control costs at step k and state costs — the tracking
    terms' per-step linear parts among them — at step k + 1, for k < T - 1."""
    game = TG.build("8_2_1", open_loop=True)
    tb = TG.TimeTables(game, np.float64)
    rng = np.random.default_rng(71)
    x0 = game.x0(B, 11)
    us = rng.uniform(-1, 1, (B, game.T, game.m))
    horizon, z = game.T, np.zeros
    want = np.zeros((B, game.N))
    for b in range(B):
        xs, _ = TG.rollout(game, tb, x0[b], z((horizon, game.n)), us[b], z((horizon, game.m, game.n)), z((horizon, game.m)),
                           "euler" if euler else "rk4")
        for k in range(horizon - 1):
            for i in range(game.N):
                x = xs[k + 1]
                c = 0.5 * x @ (tb.Hx[k + 1, i] @ x) + tb.gx[k + 1, i] @ x + tb.cx[k + 1, i]
                for (a, j) in game.pairs:
                    if a == i:
                        uj = us[b, k, game.uoff[j]:game.uoff[j + 1]]
                        c += 0.5 * uj @ (tb.Hu[(a, j)][k] @ uj) + tb.gu[(a, j)][k] @ uj + tb.cu[(a, j)][k]
                want[b, i] += c
    prob = hip.Problem(game.spec, abi.F64)
    got = _np(prob.strategy_costs(x0, z((B, horizon, game.n)), us, z((B, horizon, game.m * game.n)), z((B, horizon, game.m)),
                                  open_loop=True, euler=euler))
    print("open loop, euler", euler, "%.3e" % rel_err(got, want))
    assert rel_err(got, want) < 1e-9
    # ... where the tracking terms taken at step k's time would be another sum: w v dt x_{k+1} apart per step
    apart = np.zeros((B, game.N))
    for b in range(B):
        xs, _ = TG.rollout(game, tb, x0[b], z((horizon, game.n)), us[b], z((horizon, game.m, game.n)), z((horizon, game.m)),
                           "euler" if euler else "rk4")
        for (i, dim, w, v) in game.tracks:
            apart[b, i] = sum((tb.gx[k + 1, i][dim] - tb.gx[k, i][dim]) * xs[k + 1, dim] for k in range(horizon - 1))
    assert np.abs(apart[:, :2]).min() > 1e-6 * np.abs(want).max()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_weight_and_value_of_a_time_reading_cost_per_instance_equal_baked(hip, dtype):
    spec = examples.moving_obstacle_scene(T=T)
    spec.params.max_solver_iters = 10
    params = [("p1_pedestrian_bump", "weight"), ("p1_pedestrian_bump", "value"), ("p2_pedestrian_bump", "weight")]
    vectors = np.array([[40.0, 2.0, 40.0], [80.0, 1.5, 10.0], [10.0, 3.0, 60.0]], np.float32)

    def bound(table):
        prob = hip.Problem(spec, dtype)
        prob.declare_instance_params(params)
        prob.bind_instance_values(table)
        return prob

    def baked(row):
        s = copy.deepcopy(spec)
        for (name, field), v in zip(params, row):
            s.terms[s.term_index(name)][field] = float(np.float32(v))
        return s

    check_baked_equals_bound(hip, spec, dtype, bound, baked, vectors, B=B, deterministic=True)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_final_time_gate_in_front_of_a_time_reading_term(hip, dtype):
    spec = examples.moving_obstacle_scene(T=T)
    gated = copy.deepcopy(spec)
    bump = gated.term_index("p1_pedestrian_bump")
    gated.final_time(0.6, bump)
    k0 = gated.terms[bump]["first_step"]
    assert k0 == T // 2
    without = copy.deepcopy(spec)
    without.terms[bump]["weight"] = 0.0  # exp(...) w: every entry of the term an exact zero
    xs, us = _operating_points(spec, dtype)
    xs[:, :, 0:2] = np.asarray(examples.MOVING_OBSTACLE_START) + 0.5 * xs[:, :, 0:2] / np.abs(xs[:, :, 0:2]).max()  # near the bump
    lam, mu = _multipliers(spec.num_constraints, T)
    Qg, lg, _, _ = [_np(a) for a in hip.Problem(gated, dtype).quadraticize(xs, us, lam, mu)]
    Qw, lw, _, _ = [_np(a) for a in hip.Problem(without, dtype).quadraticize(xs, us, lam, mu)]
    Qs, ls, _, _ = [_np(a) for a in hip.Problem(spec, dtype).quadraticize(xs, us, lam, mu)]
    assert same_bits(Qg[:, :k0], Qw[:, :k0]) and same_bits(lg[:, :k0], lw[:, :k0])     # exactly nothing before the step
    assert same_bits(Qg[:, k0:], Qs[:, k0:]) and same_bits(lg[:, k0:], ls[:, k0:])     # and the whole term from it on,
    assert not same_bits(Qs[:, :k0], Qw[:, :k0])
    # ... at the time of its own step, not counted from the gate
    Qf = _np(hip.Problem(frozen(gated, 0.0)[0], dtype).quadraticize(xs, us, lam, mu)[0])
    assert not same_bits(Qg[:, k0:], Qf[:, k0:])
    # the value-only path gates it the same way (ComputeStrategyCosts against the row stage's sums)
    prob = hip.Problem(gated, dtype)
    x0 = examples.jittered_x0(spec, B, seed=3)
    out = prob.solve(x0, deterministic=True, fixed_iters=2)
    replay = _np(prob.strategy_costs(x0, _np(out["xs"]), _np(out["us"]), _np(out["P"]), np.zeros_like(_np(out["alpha"])), euler=False))
    assert rel_err(replay, _np(prob.total_costs(_np(out["xs"]), _np(out["us"]))[0])) < (1e-9 if dtype == abi.F64 else 2e-4)


def _tracking_scene():
    """dynamics_zoo_scene without its RouteProgressCost terms (the receding-horizon entry points refuse those): the
    NominalPathLengthCost stays, and with it the time dependence."""
    spec = examples.dynamics_zoo_scene(T=T)
    spec.terms = [t for t in spec.terms if t["kind"] != abi.COST_ROUTE_PROGRESS]
    assert sum(t["kind"] == abi.COST_NOMINAL_PATH_LENGTH for t in spec.terms) == 1
    return spec


def test_a_receding_horizon_replan_reads_the_window_relative_time(hip):
    """One replan — a solve, ilqg_receding_horizon_shift_batch, the next solve from the shifted warm start — of the scene
    with NominalPathLengthCost and of its twin through the time leaf, under forced steps: a time-reading cost is allowed
    there and sees what the built-in kind sees, the time relative to the new window.  The twin's second solve may be at most
    10 x as far from the original's as the original's is from its own run nudged by 1e-12 (floor 1e-12 relative)."""
    spec = _tracking_scene()
    twin, count = examples.time_expression_twin(spec)
    assert count == 1
    K = 3
    x0 = examples.jittered_x0(spec, B, seed=31)
    kw = dict(fixed_iters=K, forced_steps=np.full((B, K), 0.1))

    def replan(s, start):
        prob = hip.Problem(s, abi.F64)
        bufs = prob.solve(start, **kw)
        x_now = _np(bufs["xs"])[:, 2].copy()
        x_next, first, new_t0 = prob.receding_horizon_shift(x_now, 0.2, 0.15, 0.0, bufs)
        assert new_t0 > 0.2
        return prob.solve(_np(x_next), bufs=bufs, **kw)

    ref = replan(spec, x0)
    nud = replan(spec, x0 * (1.0 + 1e-12 * np.random.default_rng(5).standard_normal(x0.shape)))
    out = replan(twin, x0)
    assert np.all(np.isfinite(_np(out["xs"])))
    ratios = _probe_ratios(ref, nud, out)
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 10.0, (worst, ratios[worst])


def test_plan_kernels_refuse_a_model_that_reads_the_time_and_no_other(hip):
    """ilqg_receding_horizon_shift_batch, ilqg_receding_horizon_sync_batch and ilqg_plan_integrate_batch: a problem with an
    expression subsystem whose rows read the time is refused (ILQG_ERR_UNSUPPORTED, the message names the subsystem); the
    coasting car, the same model without the gust, and a problem whose costs and constraints read the time are not."""
    import torch
    gust = examples.gusting_car_scene(T=T)
    prob = hip.Problem(gust, abi.F64)
    x0 = examples.jittered_x0(gust, B, seed=59)
    bufs = prob.solve(x0, fixed_iters=1)
    plan = prob.new_plan(B)
    act = torch.ones(B, dtype=torch.int32, device="cuda")
    xd = torch.from_numpy(x0.copy()).cuda()
    for call in (lambda: prob.receding_horizon_shift(x0, 0.2, 0.15, 0.0, bufs),
                 lambda: prob.plan_integrate(plan, 0.0, 0.1, 0.05, xd, act),
                 lambda: prob.receding_horizon_sync(plan, xd, 0.1, 0.05, prob.alloc_solve_buffers(B), act)):
        with pytest.raises(hip.IlqgError) as e:
            call()
        assert e.value.status == abi.ERR_UNSUPPORTED
        assert "subsystem 0 is an expression subsystem whose rows read the time (ILQG_EXPR_PUSH_TIME)" in str(e.value)
    for spec in (examples.coasting_car_scene(T=T), examples.moving_obstacle_scene(T=T)):
        p = hip.Problem(spec, abi.F64)
        start = examples.jittered_x0(spec, B, seed=59)
        b = p.solve(start, fixed_iters=1)
        x_next, _, new_t0 = p.receding_horizon_shift(_np(b["xs"])[:, 2].copy(), 0.2, 0.15, 0.0, b)
        assert np.all(np.isfinite(_np(x_next))) and new_t0 > 0.2


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_host_mirror_solves_the_gusting_car_scene(hip, dtype):
    """tests/host/gusting_car_demo.cpp: GameSolver::SolveBatch on tests/host/gusting_car_scene.h, the model whose heading
    rate reads host::Expr::Time(), built with the mirrored classes; the Python harness solves the description the C++
    flattener produced (its dump) from the same initial states.  The mirror's containers are float, as the reference's:
    the harness's outputs are rounded to float before the exact comparison."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "host", "_bin", "gusting_car_demo")
    assert os.path.exists(exe), "build() compiles tests/host/gusting_car_demo.cpp"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.bin")
        subprocess.run([exe, "solve", "f64" if dtype == abi.F64 else "f32", str(B), out], check=True, timeout=300)
        raw = np.fromfile(out, dtype=np.float64)
    spec = abi.ProblemSpec.from_dump(subprocess.check_output([exe, "dump"], text=True, timeout=120))
    n, m, horizon = spec.n, spec.m, spec.T
    assert raw.size == B * n + B * horizon * (n + m)
    x0 = raw[:B * n].reshape(B, n)
    xs = raw[B * n:B * n + B * horizon * n].reshape(B, horizon, n)
    us = raw[B * n + B * horizon * n:].reshape(B, horizon, m)
    sol = hip.Problem(spec, dtype).solve(x0)
    assert int(_np(sol["iters"]).min()) > 0
    assert same_bits(_np(sol["xs"]).astype(np.float32), xs.astype(np.float32))
    assert same_bits(_np(sol["us"]).astype(np.float32), us.astype(np.float32))
    # the gust acted: with the clock stopped at t = 0 the same description solves to another trajectory
    still = hip.Problem(frozen(spec, 0.0)[0], dtype).solve(x0)
    assert not same_bits(_np(still["xs"]).astype(np.float32), xs.astype(np.float32))
