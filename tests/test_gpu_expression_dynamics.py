"""Expression dynamics (ILQG_DYN_EXPRESSION) on the device: rollout and linearisation of the twins against the built-in
kinds they restate, of the coasting car against a numpy integrator and its analytic Jacobians, the trajectory's bits
across every path that integrates, the whole solve against the built-in kinds under the project's conditioning probe,
every schedule of the solve bit for bit, a per-instance drag coefficient, and the equilibrium and receding-horizon paths.
No oracle: it does not know the kind.  T = 12, B = 3; stage parity bars of tests/test_gpu_expression_cost.py: 1e-9 (fp64)
and 2e-4 (fp32) of each array's largest entry."""
import copy

import numpy as np
import pytest

from ilqgames_amd import abi, examples
from helpers import rel_err
from instance_harness import KEYS, check_baked_equals_bound, same_bits, to_numpy as _np
from test_expression_dynamics import coasting_rates, np_rk4_step

pytestmark = pytest.mark.gpu

T, B = 12, 3


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


def _strategies(spec, seed=21):
    """Jittered initial states and small random strategies about a noisy reference."""
    rng = np.random.default_rng(seed)
    n, m = spec.n, spec.m
    x0 = examples.jittered_x0(spec, B, seed=seed)
    xs_ref = np.tile(x0[:, None, :], (1, spec.T, 1)) + 0.05 * rng.standard_normal((B, spec.T, n))
    us_ref = 0.1 * rng.standard_normal((B, spec.T, m))
    P = 0.002 * rng.standard_normal((B, spec.T, m * n))
    alpha = 0.05 * rng.standard_normal((B, spec.T, m))
    return x0, xs_ref, us_ref, P, alpha


# ---- 1. twins against the built-in kinds, stage level ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene,restated,generic", [("delayed_dubins_scene", 2, False), ("dynamics_zoo_scene", 3, False),
                                                    ("mixed_dubins_car_scene", 2, True), ("three_unicycle_scene", 3, True)])
def test_twin_rolls_out_and_linearizes_like_the_built_in_kinds(hip, dtype, scene, restated, generic):
    """A scene and its twin (examples.expression_dynamics_twin) under the same strategies, and their linearisations at
    the original's operating point.  delayed_dubins_scene: the specialised (8, 2, 1) kernels, dynamics_zoo_scene (Car7D,
    Unicycle5D, ...): (17, 3, 2); mixed_dubins_car_scene (control dimensions 1 and 2; the original takes the
    stage-parallel integrator, RK4 up to roundings) and three_unicycle_scene: the run-time-dimensioned path."""
    spec = getattr(examples, scene)(T=T)
    twin, count = examples.expression_dynamics_twin(spec)
    assert count == restated == len(spec.subsystems)
    orig_p, twin_p = hip.Problem(spec, dtype), hip.Problem(twin, dtype)
    assert twin_p.row_program()[1] == 0
    x0, xs_ref, us_ref, P, alpha = _strategies(spec)
    scale = np.array([1.0, 0.5, 0.25])
    xs_o, us_o = [_np(a) for a in orig_p.rollout(x0, xs_ref, us_ref, P, alpha, scale)]
    xs_t, us_t = [_np(a) for a in twin_p.rollout(x0, xs_ref, us_ref, P, alpha, scale)]
    A_o, B_o = [_np(a) for a in orig_p.linearize(xs_o, us_o)]
    A_t, B_t = [_np(a) for a in twin_p.linearize(xs_o, us_o)]
    for name, a, b in (("xs", xs_t, xs_o), ("us", us_t, us_o), ("A", A_t, A_o), ("B", B_t, B_o)):
        err = rel_err(a, b)
        print(scene, dtype, name, "%.3e" % err)
        assert err < _tol(dtype), (name, err)
    assert np.all(np.isfinite(xs_t)) and np.abs(xs_t[:, -1] - xs_t[:, 0]).max() > 1e-2
    # the solves of the two run on the same kernels' shapes: specialised where the original is, generic where it is
    out = twin_p.solve(x0, fixed_iters=1)
    assert bool(twin_p.last_schedule() & abi.SCHEDULE_GENERIC) == generic
    assert np.all(np.isfinite(_np(out["xs"])))


# ---- 2. the coasting car against numpy ----
def _np_rollout(spec, NT, x0, xs_ref, us_ref, P, alpha, scale):
    """Strategy::operator() and the RK4 with two half-steps, in the arithmetic of NT."""
    n, m, c = spec.n, spec.m, NT(np.float32(spec.subsystems[0][3]))
    xs, us = np.zeros((B, spec.T, n), NT), np.zeros((B, spec.T, m), NT)
    for b in range(B):
        x = x0[b].astype(NT)
        for k in range(spec.T):
            xs[b, k] = x
            dx = x - xs_ref[b, k].astype(NT)
            Pk = P[b, k].astype(NT).reshape(n, m).T  # word t + m c: row t, column c
            u = (us_ref[b, k].astype(NT) - Pk @ dx) - NT(scale[b]) * alpha[b, k].astype(NT)
            us[b, k] = u
            if k + 1 < spec.T:
                x = np.concatenate([np_rk4_step(lambda s, v: coasting_rates(s, v, c), x[4 * i:4 * i + 4], u[i:i + 1], spec.dt, NT)
                                    for i in range(2)]).astype(NT)
    return xs, us


def _np_linearize(spec, NT, xs, us):
    n, m, dt, c = spec.n, spec.m, NT(spec.dt), NT(np.float32(spec.subsystems[0][3]))
    A, Bm = np.zeros(xs.shape[:2] + (n, n), NT), np.zeros(xs.shape[:2] + (n, m), NT)
    for b in range(xs.shape[0]):
        for k in range(xs.shape[1]):
            A[b, k] = np.eye(n, dtype=NT)
            for i in range(2):
                o = 4 * i
                th, v, kap = NT(xs[b, k, o + 2]), NT(xs[b, k, o + 3]), NT(us[b, k, i])
                A[b, k, o + 0, o + 2] = -v * np.sin(th) * dt
                A[b, k, o + 0, o + 3] = np.cos(th) * dt
                A[b, k, o + 1, o + 2] = v * np.cos(th) * dt
                A[b, k, o + 1, o + 3] = np.sin(th) * dt
                A[b, k, o + 2, o + 3] = kap * dt
                Bm[b, k, o + 2, i] = v * dt
                A[b, k, o + 3, o + 3] = NT(1) + (-(c * (NT(2) * v))) * dt
    # column-major words, as the device stores them
    return A.transpose(0, 1, 3, 2).reshape(xs.shape[:2] + (n * n,)), Bm.transpose(0, 1, 3, 2).reshape(xs.shape[:2] + (n * m,))


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_coasting_car_matches_the_numpy_integrator_and_the_analytic_jacobians(hip, dtype):
    NT = np.float64 if dtype == abi.F64 else np.float32
    spec = examples.coasting_car_scene(T=T)
    prob = hip.Problem(spec, dtype)
    x0, xs_ref, us_ref, P, alpha = _strategies(spec, seed=23)
    us_ref = us_ref + 0.3  # a curvature the cars really steer by
    scale = np.array([1.0, 0.5, 0.25])
    cast = lambda a: a.astype(NT)  # noqa: E731  (what the device is handed)
    xs, us = [_np(a) for a in prob.rollout(x0, xs_ref, us_ref, P, alpha, scale)]
    xs_w, us_w = _np_rollout(spec, NT, cast(x0), cast(xs_ref), cast(us_ref), cast(P), cast(alpha), cast(scale))
    for name, a, b in (("xs", xs, xs_w), ("us", us, us_w)):
        print(dtype, name, "%.3e" % rel_err(a, b))
        assert rel_err(a, b) < _tol(dtype), name
    A, Bm = [_np(a) for a in prob.linearize(xs, us)]
    A_w, B_w = _np_linearize(spec, NT, xs, us)
    for name, a, b in (("A", A, A_w), ("B", Bm, B_w)):
        print(dtype, name, "%.3e" % rel_err(a, b))
        assert rel_err(a, b) < _tol(dtype), name
    # the computed entries are there: the heading row's A and B entries, the drag on the diagonal, the position rows
    n = spec.n
    for i in range(2):
        o = 4 * i
        assert np.abs(A[:, :, (o + 2) + n * (o + 3)]).min() > 1e-3       # dt kappa
        assert np.abs(Bm[:, :, (o + 2) + n * i]).min() > 1e-2           # dt v
        assert np.all(A[:, :, (o + 3) + n * (o + 3)] < 1.0 - 1e-3)      # 1 - 2 c v dt
        assert np.abs(A[:, :, (o + 0) + n * (o + 2)]).max() > 1e-2 and np.abs(A[:, :, (o + 1) + n * (o + 3)]).max() > 1e-2
    assert np.abs(xs[:, -1, 3] - xs[:, 0, 3]).min() > 1e-2, "the cars lose speed"


# ---- 3. path independence ----
def test_coasting_car_trajectory_has_the_same_bits_on_every_path(hip):
    """One iteration of the solve accepts the trajectory that the stage rollout integrates from the solve's own initial
    operating point and returned strategies — on the specialised kernels with the fused and the split trial pass, on the
    run-time-dimensioned kernels, and with a forced step (which takes the fused pass): the stage entry point is the
    run-time-dimensioned rollout kernel, the solves' are the fused kernel's wave 0, the split pass's kernel and the
    generic one's.  The solve returns alpha scaled by the accepted step; every step a line search here can try is a power
    of two, so the scaling is exact and u = (u_ref - P dx) - 1 * (step alpha) has the bits of (u_ref - P dx) - step * alpha."""
    dtype = abi.F64
    spec = examples.coasting_car_scene(T=T)
    spec.params.initial_alpha_scaling = 0.125
    spec.params.geometric_alpha_scaling = 0.5
    x0 = examples.jittered_x0(spec, B, seed=29)
    prob = hip.Problem(spec, dtype)
    z = lambda *s: np.zeros(s)  # noqa: E731
    xs0, us0 = prob.rollout(x0, z(B, T, spec.n), z(B, T, spec.m), z(B, T, spec.m * spec.n), z(B, T, spec.m), np.ones(B))
    runs = {"fused": dict(split_trial=False), "split": dict(split_trial=True), "generic": dict(generic_kernels=True),
            "forced": dict(forced_steps=np.full((B, 1), 0.0625))}
    finals = {}
    for name, kw in runs.items():
        p = hip.Problem(spec, dtype)
        out = p.solve(x0, fixed_iters=1, **kw)
        sched = p.last_schedule()
        assert bool(sched & abi.SCHEDULE_GENERIC) == (name == "generic"), name
        if name in ("fused", "split"):
            assert bool(sched & abi.SCHEDULE_SPLIT_TRIAL) == (name == "split"), name
        step = _np(p.solve_state(out)["step"])
        assert np.all(step > 0) and np.all(np.log2(step) == np.round(np.log2(step))), (name, step)
        assert name != "forced" or np.all(step == 0.0625)
        xs, us = prob.rollout(x0, xs0, us0, out["P"], out["alpha"], np.ones(B))
        assert same_bits(_np(out["xs"]), _np(xs)) and same_bits(_np(out["us"]), _np(us)), name
        finals[name] = _np(out["xs"])
    assert same_bits(finals["fused"], finals["split"])
    assert np.abs(finals["fused"] - _np(xs0)).max() > 1e-6, "the iteration moved the operating point"


# ---- 4. the whole solve, twin against original ----
def test_twin_solves_like_the_built_in_kinds_within_the_measured_conditioning(hip):
    """delayed_dubins_scene and its twin under forced steps (3 iterations of 0.1, fp64), and the original once more from
    x0 nudged by 1e-12 relative (DESIGN.md section 2's conditioning probe).  Per instance and per output the twin may be
    at most 10 x as far from the original as the nudged run is, floor 1e-12 relative."""
    spec = examples.delayed_dubins_scene(T=T)
    twin, _ = examples.expression_dynamics_twin(spec)
    K = 3
    x0 = examples.jittered_x0(spec, B, seed=31)
    steps = np.full((B, K), 0.1)
    nudged_x0 = x0 * (1.0 + 1e-12 * np.random.default_rng(5).standard_normal(x0.shape))
    kw = dict(fixed_iters=K, forced_steps=steps)
    ref = hip.Problem(spec, abi.F64).solve(x0, **kw)
    nud = hip.Problem(spec, abi.F64).solve(nudged_x0, **kw)
    out = hip.Problem(twin, abi.F64).solve(x0, **kw)
    ratios = {}
    for k in ("xs", "us", "P", "alpha"):
        r, n_, o = _np(ref[k]), _np(nud[k]), _np(out[k])
        for b in range(B):
            probe = max(rel_err(n_[b], r[b]), 1e-12)
            dev = rel_err(o[b], r[b])
            ratios[(k, b)] = dev / probe
            print("instance %d %-5s twin %.3e  nudged %.3e  ratio %.1e" % (b, k, dev, probe, dev / probe))
    assert np.array_equal(_np(out["iters"]), _np(ref["iters"]))
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 10.0, (worst, ratios[worst])
    # free-running: both converge, in the same number of iterations
    free_o = hip.Problem(spec, abi.F64).solve(x0, deterministic=True)
    free_t = hip.Problem(twin, abi.F64).solve(x0, deterministic=True)
    assert np.all(_np(free_o["converged"]) == 1) and np.all(_np(free_t["converged"]) == 1)
    assert np.array_equal(_np(free_t["iters"]), _np(free_o["iters"]))


# ---- 5. every schedule runs it ----
def _free_running(hip, spec, dtype, x0, **kw):
    prob = hip.Problem(spec, dtype)
    out = prob.solve(x0, deterministic=True, **kw)
    return prob, {k: _np(v) for k, v in out.items() if k in KEYS}


def test_every_schedule_of_the_solve_returns_the_same_bits(hip):
    spec = examples.coasting_car_scene(T=T)
    spec.params.max_solver_iters = 30
    x0 = examples.jittered_x0(spec, B, seed=41)
    prob, ref = _free_running(hip, spec, abi.F64, x0)
    assert int(ref["iters"].min()) > 1 and np.all(np.isfinite(ref["xs"]))
    assert not prob.last_schedule() & abi.SCHEDULE_STATIC_ROWS, "static_rows = AUTO resolves to no registered structure"
    assert prob.row_program()[1] == 0
    seen = set()
    for kw in (dict(split_trial=True), dict(split_trial=False), dict(round_bursts=True), dict(round_bursts=False),
               dict(handoff=True), dict(handoff=False), dict(probe=True, split_trial=True), dict(probe=False, split_trial=True),
               dict(compact_rows=True), dict(compact_rows=False), dict(split_trial=True, compact_rows=False), dict(static_rows=None)):
        p, out = _free_running(hip, spec, abi.F64, x0, **kw)
        sched = p.last_schedule()
        seen.add(sched & (abi.SCHEDULE_SPLIT_TRIAL | abi.SCHEDULE_COMPACT_ROWS))
        assert not sched & abi.SCHEDULE_STATIC_ROWS and not sched & abi.SCHEDULE_GENERIC
        if "split_trial" in kw:  # the pin is honoured and reported
            assert bool(sched & abi.SCHEDULE_SPLIT_TRIAL) == kw["split_trial"]
        if "compact_rows" in kw and not kw["compact_rows"]:
            assert not sched & abi.SCHEDULE_COMPACT_ROWS
        for k in KEYS:
            assert same_bits(out[k], ref[k]), (kw, k)
    assert len(seen) >= 2


# ---- 6. a per-instance drag coefficient ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("split_trial", [True, False])
def test_drag_per_instance_equals_baked(hip, dtype, split_trial):
    spec = examples.coasting_car_scene(T=T)
    spec.params.max_solver_iters = 10
    vectors = np.array([[0.05, 0.05], [0.2, 0.0], [0.0, 0.4], [0.1, 0.3]], np.float32)

    def bound(table):
        prob = hip.Problem(spec, dtype)
        prob.declare_instance_subsystem_params([0, 1])
        prob.bind_instance_values(table)
        return prob

    def baked(row):
        s = copy.deepcopy(spec)
        for i, v in enumerate(row):
            s.subsystems[i] = s.subsystems[i][:3] + (float(np.float32(v)),)
        return s

    prob, _, x0, which = check_baked_equals_bound(hip, spec, dtype, bound, baked, vectors, B=4, deterministic=True,
                                                  split_trial=split_trial)
    # the stage entry points read the instance's coefficient too
    x0, xs_ref, us_ref, P, alpha = _strategies(spec, seed=27)
    x0, xs_ref, us_ref, P, alpha = [np.concatenate([a, a[:1]]) for a in (x0, xs_ref, us_ref, P, alpha)]  # B = 4
    xs, us = [_np(a) for a in prob.rollout(x0, xs_ref, us_ref, P, alpha, np.ones(4))]
    A, Bm = [_np(a) for a in prob.linearize(xs, us)]
    for b in range(4):
        ref = hip.Problem(baked(vectors[which[b]]), dtype)
        sl = slice(b, b + 1)
        xs_b, us_b = [_np(a) for a in ref.rollout(x0[sl], xs_ref[sl], us_ref[sl], P[sl], alpha[sl], np.ones(1))]
        A_b, B_b = [_np(a) for a in ref.linearize(xs[sl], us[sl])]
        assert same_bits(xs[sl], xs_b) and same_bits(us[sl], us_b) and same_bits(A[sl], A_b) and same_bits(Bm[sl], B_b), b
    assert not same_bits(xs[0], xs[1]) and not same_bits(A[0], A[1])


# ---- 7. the equilibrium and receding-horizon paths ----
def test_equilibrium_checks_integrate_the_coasting_car(hip):
    """ilqg_strategy_costs_batch replays the converged gains with the feed-forward zeroed under the RK4: it retraces the
    operating point, so its sums are the row stage's total costs to accumulation error (1e-9); the Euler form runs too."""
    spec = examples.coasting_car_scene(T=T)
    spec.params.max_solver_iters = 30
    x0 = examples.jittered_x0(spec, B, seed=47)
    prob = hip.Problem(spec, abi.F64)
    out = prob.solve(x0, deterministic=True)
    xs, us, P = _np(out["xs"]), _np(out["us"]), _np(out["P"])
    replay = _np(prob.strategy_costs(x0, xs, us, P, np.zeros_like(_np(out["alpha"])), euler=False))
    total = _np(prob.total_costs(xs, us)[0])
    assert np.all(np.isfinite(total)) and rel_err(replay, total) < 1e-9, (replay, total)
    euler = _np(prob.strategy_costs(x0, xs, us, P, np.zeros_like(_np(out["alpha"])), euler=True))
    assert np.all(np.isfinite(euler)) and rel_err(euler, total) > 1e-9, "the Euler steps are another integrator"
    ok, margin = prob.check_local_nash(x0, xs, us, P, _np(out["alpha"]), 1e-2)
    assert np.all(np.isfinite(_np(margin))) and _np(ok).shape == (B,)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_plan_integrate_matches_the_numpy_integrator(hip, dtype):
    """A partial first step, whole steps and a partial last step under a stored plan with zero gains and zero feed-forward:
    the controls are the plan's, the integrator the RK4 with two half-steps over each interval."""
    import torch
    NT = np.float64 if dtype == abi.F64 else np.float32
    spec = examples.coasting_car_scene(T=T)
    prob = hip.Problem(spec, dtype)
    c = NT(np.float32(spec.subsystems[0][3]))
    rng = np.random.default_rng(53)
    plan = prob.new_plan(B)
    rows = plan["xs"].shape[1]
    us_plan = (0.3 + 0.1 * rng.standard_normal((B, rows, spec.m))).astype(NT)
    plan["us"].copy_(torch.from_numpy(us_plan))
    plan["len"].fill_(rows)
    x = examples.jittered_x0(spec, B, seed=53).astype(NT)
    t_from, t_to = 0.23, 0.67  # steps 2 (partial), 3 .. 5 (whole), 6 (partial)
    xd = torch.from_numpy(x.copy()).cuda()
    act = torch.ones(B, dtype=torch.int32, device="cuda")
    prob.plan_integrate(plan, t_from, t_to, 0.5, xd, act)
    assert np.all(_np(act) == 1)
    dt = spec.dt
    pieces = [(2, 0.3 - t_from), (3, dt), (4, dt), (5, dt), (6, t_to - 0.6)]
    want = x.copy()
    for b in range(B):
        for k, interval in pieces:
            want[b] = np.concatenate([np_rk4_step(lambda s, v: coasting_rates(s, v, c), want[b, 4 * i:4 * i + 4],
                                                  us_plan[b, k, i:i + 1], interval, NT) for i in range(2)])
    print(dtype, "plan_integrate %.3e" % rel_err(_np(xd), want))
    assert rel_err(_np(xd), want) < _tol(dtype)
    assert np.abs(_np(xd) - x).max() > 1e-2


def test_receding_horizon_shift_returns_finite_plans(hip):
    spec = examples.coasting_car_scene(T=T)
    spec.params.max_solver_iters = 10
    prob = hip.Problem(spec, abi.F64)
    x0 = examples.jittered_x0(spec, B, seed=59)
    bufs = prob.solve(x0, deterministic=True)
    x_now = _np(bufs["xs"])[:, 2] + 0.01
    x_next, first, new_t0 = prob.receding_horizon_shift(x_now, 0.2, 0.15, 0.0, bufs)
    assert np.all(np.isfinite(_np(x_next))) and np.isfinite(new_t0) and new_t0 > 0.2
    for k in ("xs", "us", "P", "alpha"):
        assert np.all(np.isfinite(_np(bufs[k]))), k
    again = prob.solve(_np(x_next), bufs=bufs, deterministic=True)
    assert np.all(np.isfinite(_np(again["xs"])))
