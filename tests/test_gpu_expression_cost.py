"""Expression costs (ILQG_COST_EXPRESSION) on the device: the row stage against the built-in kinds they restate and
against a numpy restatement, the whole solve against the built-in kinds under the project's conditioning probe, every
schedule of the solve against the others bit for bit, per-instance parameters, the value-only path of the equilibrium
checks, and the FinalTimeCost gate.  No oracle: it does not know the kind."""
import copy

import numpy as np
import pytest

from ilqgames_amd import abi, examples
from helpers import rel_err
from instance_harness import KEYS, check_baked_equals_bound, same_bits, to_numpy as _np
from test_expression_cost import np_jet

pytestmark = pytest.mark.gpu

T = 12


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


def _operating_points(hip, spec, dtype, B=3, seed=21):
    """Jittered initial states rolled out under small random strategies (on the device, by the scene WITHOUT any change:
    the dynamics are the same for a scene and its twin) -> (xs, us) as numpy arrays of the dtype."""
    rng = np.random.default_rng(seed)
    n, m = spec.n, spec.m
    x0 = examples.jittered_x0(spec, B, seed=seed)
    xs_ref = np.tile(x0[:, None, :], (1, spec.T, 1)) + 0.05 * rng.standard_normal((B, spec.T, n))
    us_ref = 0.1 * rng.standard_normal((B, spec.T, m))
    P = 0.002 * rng.standard_normal((B, spec.T, m * n))
    alpha = 0.05 * rng.standard_normal((B, spec.T, m))
    xs, us = hip.Problem(spec, dtype).rollout(x0, xs_ref, us_ref, P, alpha, np.ones(B))
    return _np(xs), _np(us)


# ---- 1. stage parity with the built-in kinds ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene,replaced", [("cost_zoo_scene", 10), ("mixed_dubins_car_scene", 7)])
def test_twin_quadraticizes_and_costs_like_the_built_in_kinds(hip, dtype, scene, replaced):
    """The scene and its twin (examples.expression_twin: every single-dimension QuadraticCost, every CurvatureCost and every
    SemiquadraticNormCost on a state pair restated as an expression) at 3 jittered operating points: Q, l, R, r and the
    total costs to the project's parity bars against each array's largest entry — the formulas differ by a few roundings
    per entry.  cost_zoo_scene runs the specialised (10, 2, 2) kernels, mixed_dubins_car_scene the run-time-dimensioned ones."""
    spec = getattr(examples, scene)(T=T)
    twin, count = examples.expression_twin(spec)
    assert count == replaced
    orig_p, twin_p = hip.Problem(spec, dtype), hip.Problem(twin, dtype)
    assert twin_p.row_program()[1] == 0
    xs, us = _operating_points(hip, spec, dtype)
    nc = spec.num_constraints
    rng = np.random.default_rng(3)
    lam = np.abs(rng.standard_normal((3, max(nc, 1), T))) if nc else None
    mu = np.array([10.0, 11.0, 12.1]) if nc else None
    tol = 1e-9 if dtype == abi.F64 else 2e-4
    for name, a, b in zip("QlRr", twin_p.quadraticize(xs, us, lam, mu), orig_p.quadraticize(xs, us, lam, mu)):
        err = rel_err(_np(a), _np(b))
        print(scene, dtype, name, "%.3e" % err)
        assert err < tol, (name, err)
    c_t, c_o = _np(twin_p.total_costs(xs, us)[0]), _np(orig_p.total_costs(xs, us)[0])
    print(scene, dtype, "costs %.3e" % rel_err(c_t, c_o))
    assert rel_err(c_t, c_o) < tol
    assert np.all(np.isfinite(c_t))


# ---- 2. stage parity with the numpy restatement ----
def _without_expressions(spec):
    s = copy.deepcopy(spec)
    keep = [q for q, t in enumerate(s.terms) if t["kind"] != abi.COST_EXPRESSION]
    s.terms = [s.terms[q] for q in keep]
    s.term_names = {}
    s.dense_params = []
    return s


def _numpy_contributions(spec, xs, us, NT, only=None):
    """What the expression costs of `spec` (`only`: of these term indices) add to Q [B][T][N][n*n] (column-major), l [B][T][N][n], R, r (by the problem's
    control pairs: only the pair (1, 1) occurs here) and the per-player total costs, by np_jet in the dtype."""
    B, n = xs.shape[0], spec.n
    dQ, dl = np.zeros((B, spec.T, 2, n * n)), np.zeros((B, spec.T, 2, n))
    dR, dr = {}, {}
    dc = np.zeros((B, 2))
    for q, t in enumerate(spec.terms):
        if t["kind"] != abi.COST_EXPRESSION or (only is not None and q not in only):
            continue
        L = int(spec.dense_params[t["polyline"]])
        blk = spec.dense_params[t["polyline"] + 1:t["polyline"] + 1 + 2 * L]
        program = [(int(blk[2 * e]), blk[2 * e + 1]) for e in range(L)]
        i, ix, iy = t["player"], t["idx"][0], t["idx"][1]
        on_state = t["role"] == abi.ROLE_STATE_COST
        vec = xs if on_state else us[:, :, sum(spec.udims[:t["arg"]]):]
        for b in range(B):
            for k in range(t.get("first_step", 0), spec.T):
                x, y = vec[b, k, ix], (vec[b, k, iy] if iy >= 0 else 0.0)
                f, fx, fy, fxx, fyy, fxy = [float(c) for c in np_jet(program, NT(np.float32(t["weight"])),
                                                                     NT(np.float32(t["value"])), NT(x), NT(y), NT)]
                dc[b, i] += f
                if on_state:
                    dl[b, k, i, ix] += fx
                    dQ[b, k, i, ix + n * ix] += fxx
                    if iy >= 0:
                        dl[b, k, i, iy] += fy
                        dQ[b, k, i, iy + n * iy] += fyy
                        dQ[b, k, i, ix + n * iy] += fxy
                        dQ[b, k, i, iy + n * ix] += fxy
                else:
                    mj = spec.udims[t["arg"]]
                    key = (i, t["arg"])
                    dR.setdefault(key, np.zeros((B, spec.T, mj * mj)))[b, k, ix + mj * ix] += fxx
                    dr.setdefault(key, np.zeros((B, spec.T, mj)))[b, k, ix] += fx
    return dQ, dl, dR, dr, dc


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_bump_and_barrier_match_the_numpy_restatement(hip, dtype):
    """examples.expression_scene (a Gaussian bump over a player's own position, a log barrier on a speed, a one-sided
    control penalty) against the same scene without them plus np_jet's entries: Q, l, R, r and the costs, same bars."""
    NT = np.float64 if dtype == abi.F64 else np.float32
    spec = examples.expression_scene(T=T)
    base = _without_expressions(spec)
    xs, us = _operating_points(hip, base, dtype)
    with_p, base_p = hip.Problem(spec, dtype), hip.Problem(base, dtype)
    assert with_p.pairs == base_p.pairs
    dQ, dl, dR, dr, dc = _numpy_contributions(spec, xs, us, NT)
    assert np.abs(dQ).max() > 1e-3 and np.abs(dl).max() > 1e-3 and len(dR) == 1
    Q, l, R, r = [_np(a).astype(np.float64) for a in with_p.quadraticize(xs, us)]
    Q0, l0, R0, r0 = [_np(a).astype(np.float64) for a in base_p.quadraticize(xs, us)]
    for (i, j), blk in dR.items():
        q = with_p.pairs.index((i, j))
        roff = sum(spec.udims[b] ** 2 for _, b in with_p.pairs[:q])
        goff = sum(spec.udims[b] for _, b in with_p.pairs[:q])
        R0[:, :, roff:roff + blk.shape[2]] += blk
        r0[:, :, goff:goff + dr[(i, j)].shape[2]] += dr[(i, j)]
    tol = 1e-9 if dtype == abi.F64 else 2e-4
    for name, a, b in (("Q", Q, Q0 + dQ), ("l", l, l0 + dl), ("R", R, R0), ("r", r, r0)):
        print(dtype, name, "%.3e" % rel_err(a, b))
        assert rel_err(a, b) < tol, name
    c, c0 = _np(with_p.total_costs(xs, us)[0]), _np(base_p.total_costs(xs, us)[0])
    assert rel_err(c, c0 + dc) < tol


# ---- 3. the whole solve ----
def test_twin_solves_like_the_built_in_kinds_within_the_measured_conditioning(hip, capsys):
    """cost_zoo_scene and its twin under forced steps (3 iterations of 0.1, B = 4, fp64), and the original once more from
    x0 nudged by 1e-12 relative (DESIGN.md section 2's conditioning probe).  Per instance and per output the twin may
    be at most 10 x as far from the original as the nudged run is, floor 1e-12 relative: the expression formulas perturb
    Q / l entries by a few roundings, a hundred times less than the nudge.  Every instance counts."""
    spec = examples.cost_zoo_scene(T=T)
    twin, _ = examples.expression_twin(spec)
    B, K = 4, 3
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


# ---- 4. every schedule runs it ----
def _free_running(hip, spec, dtype, x0, **kw):
    prob = hip.Problem(spec, dtype)
    out = prob.solve(x0, deterministic=True, **kw)
    return prob, {k: _np(v) for k, v in out.items() if k in KEYS}


def test_every_schedule_of_the_solve_returns_the_same_bits(hip):
    spec = examples.expression_scene(T=T)
    spec.params.max_solver_iters = 30
    x0 = examples.jittered_x0(spec, 4, seed=41)
    prob, ref = _free_running(hip, spec, abi.F64, x0)
    assert int(ref["iters"].min()) > 1 and np.all(np.isfinite(ref["xs"]))
    assert not prob.last_schedule() & abi.SCHEDULE_STATIC_ROWS, "static_rows = AUTO falls back to the interpreter"
    assert prob.last_schedule() & abi.SCHEDULE_COMPACT_ROWS, "the stack's scratch keeps the scene on compact rows"
    seen = set()
    for kw in (dict(split_trial=True), dict(split_trial=False), dict(compact_rows=False), dict(compact_rows=True),
               dict(split_trial=True, compact_rows=False), dict(static_rows=True), dict(handoff=False)):
        p, out = _free_running(hip, spec, abi.F64, x0, **kw)
        seen.add(p.last_schedule() & (abi.SCHEDULE_SPLIT_TRIAL | abi.SCHEDULE_COMPACT_ROWS))
        if "split_trial" in kw:  # the pin is honoured and reported
            assert bool(p.last_schedule() & abi.SCHEDULE_SPLIT_TRIAL) == kw["split_trial"]
        if "compact_rows" in kw:
            assert bool(p.last_schedule() & abi.SCHEDULE_COMPACT_ROWS) == kw["compact_rows"]
        for k in KEYS:
            assert same_bits(out[k], ref[k]), (kw, k)
    assert len(seen) >= 3


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_probing_line_search_backtracks_through_the_gradient_only_pass(hip, dtype):
    """A deliberately large first step: the line search back-tracks, and with probe = ON the candidates' merits come from
    the gradient-only row pass (its scratch holds gradient slots and the stack, nothing else).  Same bits as probe = OFF."""
    spec = examples.expression_scene(T=T)
    spec.params.max_solver_iters = 3
    spec.params.initial_alpha_scaling = 4.0
    x0 = examples.jittered_x0(spec, 4, seed=43)
    prob, on = _free_running(hip, spec, dtype, x0, probe=True, split_trial=True)
    state = prob.solve_state(prob.solve(x0, deterministic=True, probe=True, split_trial=True))
    _, off = _free_running(hip, spec, dtype, x0, probe=False, split_trial=True)
    for k in KEYS:
        assert same_bits(on[k], off[k]), k
    print("backtracks", _np(state["backtracks"]), "last step", _np(state["step"]))
    assert int(_np(state["backtracks"]).max()) > 0 or float(_np(state["step"]).min()) < 4.0, "no step was rejected"
    assert np.all(np.isfinite(on["xs"]))


# ---- 5. per-instance parameters ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("split_trial", [True, False])
def test_bump_weight_and_width_per_instance_equal_baked(hip, dtype, split_trial):
    spec = examples.expression_scene(T=T)
    spec.params.max_solver_iters = 10
    params = [("p1_bump", "weight"), ("p1_bump", "value"), ("p2_speed_barrier", "value"), ("p2_acceleration_cap", "weight")]
    vectors = np.array([[30.0, 2.0, 15.0, 20.0], [60.0, 1.5, 12.0, 5.0], [10.0, 3.0, 20.0, 40.0], [45.0, 2.5, 14.0, 0.0]], np.float32)

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

    check_baked_equals_bound(hip, spec, dtype, bound, baked, vectors, B=4, deterministic=True, split_trial=split_trial)


# ---- 6. the value-only path ----
def test_equilibrium_checks_evaluate_expression_costs(hip):
    """ilqg_strategy_costs_batch replays a strategy and sums the costs with term_evaluate_leaf, the row stage's
    cost pass sums them for ilqg_total_costs_batch: the converged gains with the feed-forward zeroed retrace the operating
    point under the solver's own integrator, so the two agree to accumulation error (1e-9)."""
    spec = examples.expression_scene(T=T)
    spec.params.max_solver_iters = 30
    B = 4
    x0 = examples.jittered_x0(spec, B, seed=47)
    prob = hip.Problem(spec, abi.F64)
    out = prob.solve(x0, deterministic=True)
    xs, us, P = _np(out["xs"]), _np(out["us"]), _np(out["P"])
    replay = _np(prob.strategy_costs(x0, xs, us, P, np.zeros_like(_np(out["alpha"])), euler=False))
    total = _np(prob.total_costs(xs, us)[0])
    assert np.all(np.isfinite(total)) and rel_err(replay, total) < 1e-9, (replay, total)
    # ... and the expression costs are part of both sums
    plain = _np(hip.Problem(_without_expressions(spec), abi.F64).total_costs(xs, us)[0])
    assert np.all(np.abs(total - plain) > 1e-6 * np.abs(total))
    ok, margin = prob.check_local_nash(x0, xs, us, P, _np(out["alpha"]), 1e-2)
    assert np.all(np.isfinite(_np(margin))) and _np(ok).shape == (B,)


# ---- 7. the FinalTimeCost gate ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_final_time_gate_zeroes_the_bump_before_its_first_step(hip, dtype):
    NT = np.float64 if dtype == abi.F64 else np.float32
    spec = examples.expression_scene(T=T)
    gated = copy.deepcopy(spec)
    bump = gated.term_index("p1_bump")
    gated.final_time(0.6, bump)
    k0 = gated.terms[bump]["first_step"]
    assert k0 == T // 2
    without = copy.deepcopy(spec)
    without.terms[bump]["weight"] = 0.0  # w exp(...): every entry of the term an exact zero
    xs, us = _operating_points(hip, _without_expressions(spec), dtype)
    Qg, lg, _, _ = [_np(a) for a in hip.Problem(gated, dtype).quadraticize(xs, us)]
    Qw, lw, _, _ = [_np(a) for a in hip.Problem(without, dtype).quadraticize(xs, us)]
    Qs, ls, _, _ = [_np(a) for a in hip.Problem(spec, dtype).quadraticize(xs, us)]
    assert same_bits(Qg[:, :k0], Qw[:, :k0]) and same_bits(lg[:, :k0], lw[:, :k0])     # exactly nothing before the step
    assert same_bits(Qg[:, k0:], Qs[:, k0:]) and same_bits(lg[:, k0:], ls[:, k0:])     # and the whole term from it on
    assert not same_bits(Qs[:, :k0], Qw[:, :k0])
    # the cost: the gated scene's total is the ungated one's minus the bump's values before the step
    _, _, _, _, dc_all = _numpy_contributions(spec, xs, us, NT, only=(bump,))
    _, _, _, _, dc_late = _numpy_contributions(gated, xs, us, NT, only=(bump,))
    cg = _np(hip.Problem(gated, dtype).total_costs(xs, us)[0]).astype(np.float64)
    cs = _np(hip.Problem(spec, dtype).total_costs(xs, us)[0]).astype(np.float64)
    tol = 1e-9 if dtype == abi.F64 else 2e-4
    assert np.all(dc_all[:, 0] - dc_late[:, 0] > 0)
    # (a difference of two totals: it carries the totals' rounding)
    assert np.max(np.abs((cs - cg) - (dc_all - dc_late))) < tol * np.abs(cs).max()
