"""Expression terms between players and as constraints on the device (include/ilqg.h: relative inputs of the expression
kinds, ILQG_CONSTRAINT_EXPRESSION): the row stage against the built-in kinds they restate and against a numpy restatement
written by hand, every schedule of the solve against the others bit for bit, forced-step and free-running solves against
the built-in kinds under the project's conditioning probe, per-instance thresholds and weights, the equality flag and the
value-only paths.  No oracle: it does not know the encodings."""
import copy

import numpy as np
import pytest

from ilqgames_amd import abi, examples
from helpers import rel_err
from instance_harness import KEYS, check_baked_equals_bound, same_bits, to_numpy as _np
from test_expression_roles import constraint_mu, game_scene_formulas, numpy_contributions, upper_bound, without_expressions

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


def _tol(dtype):
    return 1e-9 if dtype == abi.F64 else 2e-4


def _close_x0(spec, B, seed, centre=(0.0, 0.0), radius=(1.2, 2.6)):
    """Initial states with the players on a ring about `centre` (+- 0.5 m), each at its own radius and a jittered angle:
    every pair of players 1.5 .. 5 m apart, so that proximity costs, clearances and repulsions are at work and none sits on
    the singularity of a distance at zero."""
    rng = np.random.default_rng(seed)
    x0 = examples.jittered_x0(spec, B, seed=seed)
    N = len(spec.position_dims)
    for b in range(B):
        c = np.asarray(centre) + rng.uniform(-0.5, 0.5, 2)
        for i, (xi, yi) in enumerate(spec.position_dims):
            ang = 2 * np.pi * i / N + rng.uniform(-0.4, 0.4)
            r = rng.uniform(*radius)
            x0[b, xi], x0[b, yi] = c[0] + r * np.cos(ang), c[1] + r * np.sin(ang)
    return x0


def _operating_points(hip, spec, dtype, x0, seed=21, us_scale=0.1):
    """x0 rolled out under small random strategies (on the device, by the scene given: the dynamics are the same for a
    scene and its twin) -> (xs, us) as numpy arrays of the dtype."""
    rng = np.random.default_rng(seed)
    n, m, B = spec.n, spec.m, x0.shape[0]
    xs_ref = np.tile(x0[:, None, :], (1, spec.T, 1)) + 0.05 * rng.standard_normal((B, spec.T, n))
    us_ref = us_scale * rng.standard_normal((B, spec.T, m))
    P = 0.002 * rng.standard_normal((B, spec.T, m * n))
    alpha = 0.05 * rng.standard_normal((B, spec.T, m))
    xs, us = hip.Problem(spec, dtype).rollout(x0, xs_ref, us_ref, P, alpha, np.ones(B))
    return _np(xs), _np(us)


def _multipliers(B, nc, seed=3):
    """lambdas >= 0 with every third step and one whole instance at zero (the inactive-inequality gate of Constraint::Mu
    then decides by g alone), mu per instance"""
    rng = np.random.default_rng(seed)
    lam = np.abs(rng.standard_normal((B, max(nc, 1), T)))
    lam[:, :, ::3] = 0.0
    lam[B - 1] = 0.0
    return lam, rng.uniform(5.0, 20.0, B)


# ---- 1. stage parity with the built-in kinds ----
SCENES = {
    "skeleton": (lambda: examples.skeleton(T=T), 8),
    "three_player_intersection": (lambda: examples.three_player_intersection(T=T), 15),
    "mixed_dubins_car_scene_constrained": (lambda: examples.mixed_dubins_car_scene(T=T, constrained=True), 12),
}


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene", list(SCENES))
def test_twin_quadraticizes_and_costs_like_the_built_in_kinds(hip, dtype, scene):
    """A scene and its twin (examples.expression_game_twin: proximity, relative-distance, difference and signed-distance costs
    over relative inputs, proximity and single-dimension constraints as expression constraints) at 4 operating points with
    the players 1.5 .. 5 m apart, under multipliers that leave some constraints active and some not: Q, l, R, r and the
    total costs to the project's parity bars against each array's largest entry.  skeleton runs the (10, 2, 2) kernels,
    three_player_intersection (six proximity constraints) the (16, 3, 2) ones, the constrained mixed scene the
    run-time-dimensioned ones with a state, a control and a relative constraint at once."""
    make, replaced = SCENES[scene]
    spec = make()
    twin, count = examples.expression_game_twin(spec)
    assert count == replaced
    if scene == "three_player_intersection":
        assert sum(t["kind"] == abi.CONSTRAINT_EXPRESSION for t in twin.terms) == 6
    orig_p, twin_p = hip.Problem(spec, dtype), hip.Problem(twin, dtype)
    assert twin_p.row_program()[1] == 0
    B = 4
    xs, us = _operating_points(hip, spec, dtype, _close_x0(spec, B, seed=61), us_scale=0.8)
    nc = spec.num_constraints
    lam, mu = _multipliers(B, nc) if nc else (None, None)
    for name, a, b in zip("QlRr", twin_p.quadraticize(xs, us, lam, mu), orig_p.quadraticize(xs, us, lam, mu)):
        err = rel_err(_np(a), _np(b))
        print(scene, dtype, name, "%.3e" % err)
        assert err < _tol(dtype), (name, err)
    if nc:  # the constraints are at work: without multipliers and penalty the arrays are others
        Q0 = _np(orig_p.quadraticize(xs, us, 0.0 * lam, 0.0 * mu)[0])
        assert rel_err(Q0, _np(orig_p.quadraticize(xs, us, lam, mu)[0])) > 1e-3
    c_t, c_o = _np(twin_p.total_costs(xs, us)[0]), _np(orig_p.total_costs(xs, us)[0])
    print(scene, dtype, "costs %.3e" % rel_err(c_t, c_o))
    assert rel_err(c_t, c_o) < _tol(dtype)
    assert np.all(np.isfinite(c_t))


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_single_dimension_constraint_twins_return_the_bits_of_the_built_in_kind(hip, dtype):
    """x - v and v - x as expression constraints perform the operations of SingleDimensionConstraint (a difference, then
    Constraint::ModifyDerivatives on g' = +-1, g'' = 0): with only those two terms of the constrained mixed scene replaced —
    one on the state, one on a control — every array equals the original's bit for bit."""
    spec = examples.mixed_dubins_car_scene(T=T, constrained=True)
    full, _ = examples.expression_game_twin(spec)
    twin = copy.deepcopy(spec)
    twin.dense_params = list(full.dense_params)
    swapped = 0
    for q, t in enumerate(spec.terms):
        if t["kind"] == abi.CONSTRAINT_SINGLE_DIMENSION:
            twin.terms[q] = copy.deepcopy(full.terms[q])
            swapped += 1
    assert swapped == 2 and {t["role"] for t in twin.terms if t["kind"] == abi.CONSTRAINT_EXPRESSION} == \
        {abi.ROLE_STATE_CONSTRAINT, abi.ROLE_CONTROL_CONSTRAINT}
    B = 4
    xs, us = _operating_points(hip, spec, dtype, _close_x0(spec, B, seed=62), us_scale=0.8)
    lam, mu = _multipliers(B, spec.num_constraints)
    got = hip.Problem(twin, dtype).quadraticize(xs, us, lam, mu)
    want = hip.Problem(spec, dtype).quadraticize(xs, us, lam, mu)
    identical = [same_bits(_np(a), _np(b)) for a, b in zip(got, want)]
    print("single-dimension twins bit-identical (Q, l, R, r):", identical)
    assert all(identical)


# ---- 2. stage parity with the numpy restatement ----
def _game_points(hip, spec, dtype, B=4, seed=63):
    """Operating points of expression_game_scene with car 1 about the rim of its keep-out disc and car 2 within a few
    metres of it: every term at work, the constraints on both sides of zero."""
    cx, cy = examples.EXPRESSION_DISC_CENTRE
    x0 = _close_x0(spec, B, seed, centre=(cx - 3.5, cy), radius=(1.0, 2.2))
    return _operating_points(hip, without_expressions(spec), dtype, x0, seed=seed, us_scale=1.2)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_game_scene_matches_the_numpy_restatement(hip, dtype):
    """examples.expression_game_scene against the same scene without its expression terms plus the hand-written numpy
    formulas (tests/test_expression_roles.py: derivatives by hand, checked there against central differences) under given
    lambdas and mu: Q, l, R, r and the costs.  The keep-out disc is gated (first step 3): nothing of it before."""
    NT = np.float64 if dtype == abi.F64 else np.float32
    spec = examples.expression_game_scene(T=T)
    base = without_expressions(spec)
    xs, us = _game_points(hip, spec, dtype)
    B = xs.shape[0]
    lam, mu = _multipliers(B, spec.num_constraints, seed=9)
    with_p, base_p = hip.Problem(spec, dtype), hip.Problem(base, dtype)
    assert with_p.pairs == base_p.pairs
    dQ, dl, dR, dr, dc, gs = numpy_contributions(spec, game_scene_formulas(), xs, us, lam, mu, NT)
    for name, g in gs.items():  # both sides of zero, and both branches of the gate
        live = g[:, spec.terms[spec.term_index(name)]["first_step"]:]
        print(name, "g in [%.3f, %.3f]" % (live.min(), live.max()))
    assert gs["p1_keep_out"].max() > 0 > gs["p1_keep_out"].min() and gs["p2_clearance"].max() > 0 > gs["p2_clearance"].min()
    assert np.all(gs["p1_keep_out"][:, :3] == 0)
    Q, l, R, r = [_np(a).astype(np.float64) for a in with_p.quadraticize(xs, us, lam, mu)]
    Q0, l0, R0, r0 = [_np(a).astype(np.float64) for a in base_p.quadraticize(xs, us)]
    assert list(dR) == [(0, 0)]
    for (i, j), blk in dR.items():
        q = with_p.pairs.index((i, j))
        roff = sum(spec.udims[b] ** 2 for _, b in with_p.pairs[:q])
        goff = sum(spec.udims[b] for _, b in with_p.pairs[:q])
        R0[:, :, roff:roff + blk.shape[2]] += blk
        r0[:, :, goff:goff + dr[(i, j)].shape[2]] += dr[(i, j)]
    for name, a, b in (("Q", Q, Q0 + dQ), ("l", l, l0 + dl), ("R", R, R0), ("r", r, r0)):
        print(dtype, name, "%.3e" % rel_err(a, b))
        assert rel_err(a, b) < _tol(dtype), name
    assert np.abs(dQ).max() > 1e-2 * np.abs(Q).max() and np.abs(dl).max() > 1e-2 * np.abs(l).max()
    # the gate: before its first step the disc adds exactly nothing — the scene without it returns the same bits there
    k0 = spec.terms[spec.term_index("p1_keep_out")]["first_step"]
    no_disc = copy.deepcopy(spec)
    no_disc.terms[no_disc.term_index("p1_keep_out")]["first_step"] = T
    Qn, ln, _, _ = [_np(a) for a in hip.Problem(no_disc, dtype).quadraticize(xs, us, lam, mu)]
    Qw, lw, _, _ = [_np(a) for a in with_p.quadraticize(xs, us, lam, mu)]
    assert same_bits(Qn[:, :k0], Qw[:, :k0]) and same_bits(ln[:, :k0], lw[:, :k0]) and not same_bits(Qn[:, k0:], Qw[:, k0:])
    # the costs: the relative costs' values and nothing of the constraints
    c, c0 = _np(with_p.total_costs(xs, us)[0]), _np(base_p.total_costs(xs, us)[0])
    assert np.all(np.abs(dc) > 1e-3) and rel_err(c, c0 + dc) < _tol(dtype)


def _without_constraints(spec):
    s = copy.deepcopy(spec)
    keep = [q for q, t in enumerate(spec.terms) if t["kind"] != abi.CONSTRAINT_EXPRESSION]
    s.terms = [s.terms[q] for q in keep]
    s.term_names = {k: keep.index(v) for k, v in spec.term_names.items() if v in keep}
    s._num_constraints = 0
    return s


# ---- 3. every schedule runs it ----
def _solve_x0(spec, B, seed):
    """car 1 heading for its keep-out disc, car 2 a few metres ahead of it: the constraints are violated on the way"""
    x0 = examples.jittered_x0(spec, B, seed=seed)
    rng = np.random.default_rng(seed)
    x0[:, 0], x0[:, 1] = 1.0 + rng.uniform(-0.3, 0.3, B), -4.0 + rng.uniform(-0.5, 0.5, B)
    x0[:, 5], x0[:, 6] = -2.5 + rng.uniform(-0.5, 0.5, B), 3.0 + rng.uniform(-0.5, 0.5, B)
    return x0


def _free_running(hip, spec, dtype, x0, **kw):
    prob = hip.Problem(spec, dtype)
    out = prob.solve(x0, deterministic=True, **kw)
    return prob, {k: _np(v) for k, v in out.items() if k in KEYS}


@pytest.mark.parametrize("al", [False, True], ids=["ilq", "augmented_lagrangian"])
def test_every_schedule_of_the_solve_returns_the_same_bits(hip, al):
    spec = examples.expression_game_scene(T=T)
    spec.params.max_solver_iters = 20
    x0 = _solve_x0(spec, 4, seed=41)
    prob, ref = _free_running(hip, spec, abi.F64, x0, augmented_lagrangian=al)
    assert int(ref["iters"].min()) > 1 and np.all(np.isfinite(ref["xs"]))
    assert prob.last_schedule() & abi.SCHEDULE_COMPACT_ROWS, "the stack's scratch keeps the scene on compact rows"
    seen = set()
    for kw in (dict(split_trial=True), dict(split_trial=False), dict(compact_rows=False), dict(compact_rows=True),
               dict(probe=True, split_trial=True), dict(probe=False, split_trial=True)):
        p, out = _free_running(hip, spec, abi.F64, x0, augmented_lagrangian=al, **kw)
        seen.add(p.last_schedule() & (abi.SCHEDULE_SPLIT_TRIAL | abi.SCHEDULE_COMPACT_ROWS))
        for k in KEYS:
            assert same_bits(out[k], ref[k]), (kw, k)
    assert len(seen) >= 3
    # The run-time-dimensioned kernels forced onto the shape (their row kernel and their probing one, the two generic forms
    # of kExprProg): the same bits with probe ON and OFF.  Their sweep is another kernel than the specialised solve's
    # (all-LDS, another order of sums), so against `ref` they are held to the decisions and to 1e-6, as the project
    # holds the two paths to the oracle and not to one another.
    pg, gen_on = _free_running(hip, spec, abi.F64, x0, augmented_lagrangian=al, generic_kernels=True, probe=True)
    _, gen_off = _free_running(hip, spec, abi.F64, x0, augmented_lagrangian=al, generic_kernels=True, probe=False)
    assert pg.last_schedule() & abi.SCHEDULE_GENERIC
    for k in KEYS:
        assert same_bits(gen_on[k], gen_off[k]), ("generic_kernels", k)
    agree = (gen_on["iters"] == ref["iters"]) & (gen_on["status"] == ref["status"])
    print("generic against specialised: same decisions in %d of %d instances, xs differ by %s" %
          (agree.sum(), len(agree), [float("%.2e" % rel_err(gen_on["xs"][b], ref["xs"][b])) for b in range(len(agree))]))
    assert agree.any()
    for b in np.nonzero(agree)[0]:
        assert rel_err(gen_on["xs"][b], ref["xs"][b]) < 1e-6, b


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_probing_line_search_backtracks_through_the_gradient_only_pass(hip, dtype):
    """A deliberately large first step: the line search back-tracks, and with probe = ON the candidates' merits come from
    the gradient-only row pass, where a constraint forms (lambda + mu g) g' alone.  Same bits as probe = OFF."""
    spec = examples.expression_game_scene(T=T)
    spec.params.max_solver_iters = 3
    spec.params.initial_alpha_scaling = 4.0
    x0 = _solve_x0(spec, 4, seed=43)
    prob, on = _free_running(hip, spec, dtype, x0, probe=True, split_trial=True)
    state = prob.solve_state(prob.solve(x0, deterministic=True, probe=True, split_trial=True))
    _, off = _free_running(hip, spec, dtype, x0, probe=False, split_trial=True)
    for k in KEYS:
        assert same_bits(on[k], off[k]), k
    print("backtracks", _np(state["backtracks"]), "last step", _np(state["step"]))
    assert int(_np(state["backtracks"]).max()) > 0 or float(_np(state["step"]).min()) < 4.0, "no step was rejected"
    assert np.all(np.isfinite(on["xs"]))


# ---- 4. forced-step solves against the built-in kinds ----
@pytest.mark.parametrize("scene", ["skeleton", "three_player_intersection"])
def test_twin_solves_like_the_built_in_kinds_within_the_measured_conditioning(hip, capsys, scene):
    """A scene and its twin under forced steps (3 iterations of 0.1, B = 4, fp64), and the original once more from x0
    nudged by 1e-12 relative (DESIGN.md section 2's conditioning probe).  Per instance and per output the twin may be at
    most 10 x as far from the original as the nudged run is, floor 1e-12 relative.  three_player_intersection's six
    proximity constraints enter every iteration through their augmented-Lagrangian terms (lambda = 0, mu = 10), as the
    forced-step solves of tests/test_gpu_affine.py drive theirs.  The ratios are printed whatever pytest captures."""
    spec = SCENES[scene][0]()
    twin, _ = examples.expression_game_twin(spec)
    B, K = 4, 3
    x0 = _close_x0(spec, B, seed=31, radius=(2.0, 3.5))
    steps = np.full((B, K), 0.1)
    nudged_x0 = x0 * (1.0 + 1e-12 * np.random.default_rng(5).standard_normal(x0.shape))
    kw = dict(fixed_iters=K, forced_steps=steps)
    ref = hip.Problem(spec, abi.F64).solve(x0, **kw)
    nud = hip.Problem(spec, abi.F64).solve(nudged_x0, **kw)
    out = hip.Problem(twin, abi.F64).solve(x0, **kw)
    ratios = {}
    with capsys.disabled():
        for k in ("xs", "us", "P", "alpha"):
            r, n_, o = _np(ref[k]), _np(nud[k]), _np(out[k])
            for b in range(B):
                probe = max(rel_err(n_[b], r[b]), 1e-12)
                dev = rel_err(o[b], r[b])
                ratios[(k, b)] = dev / probe
                print("%s instance %d %-5s twin %.3e  nudged %.3e  ratio %.1e" % (scene, b, k, dev, probe, dev / probe))
    assert np.array_equal(_np(out["iters"]), _np(ref["iters"]))
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 10.0, (worst, ratios[worst])


# ---- 5. free-running augmented-Lagrangian solves ----
def _al_x0(spec, B, seed):
    """car 1 passing its keep-out disc at about its radius (some instances inside, some outside), car 2 well away"""
    x0 = examples.jittered_x0(spec, B, seed=seed)
    rng = np.random.default_rng(seed)
    x0[:, 0], x0[:, 1] = 0.7 + rng.uniform(-0.1, 0.1, B), -6.0 + rng.uniform(-0.5, 0.5, B)
    x0[:, 5], x0[:, 6] = -2.5 + rng.uniform(-0.5, 0.5, B), 8.0 + rng.uniform(-0.5, 0.5, B)
    return x0


def test_free_running_al_solve_meets_its_constraint_tolerance(hip, capsys):
    """AugmentedLagrangianSolver::Solve on expression_game_scene (B = 8): the multiplier update and the maximum constraint
    error come from the value-only evaluator.  For every instance reported successful g, recomputed in numpy on the
    returned trajectory, is at most constraint_error_tolerance (+ 1e-9: the device value is the same formula rounded
    differently); an instance the solver gives up on within max_solver_iters is reported as that, and its g is above the
    tolerance.  The acceleration bound written as the built-in SingleDimensionConstraint gives the same run bit for bit
    (the same operations in the row stage and in the multiplier update)."""
    spec = examples.expression_game_scene(T=T)
    B = 8
    x0 = _al_x0(spec, B, seed=71)
    prob = hip.Problem(spec, abi.F64)
    out = {k: _np(v) for k, v in prob.solve(x0, augmented_lagrangian=True, deterministic=True).items() if k in KEYS}
    xs, us, status = out["xs"], out["us"], out["status"]
    assert np.all(np.isfinite(xs))
    gs = numpy_contributions(spec, game_scene_formulas(), xs, us)[5]
    worst = np.max(np.stack([g.max(axis=1) for g in gs.values()]), axis=0)
    # what the constraints are there for: the same game without them drives through the disc
    free = hip.Problem(_without_constraints(spec), abi.F64).solve(x0)
    g_free = numpy_contributions(spec, game_scene_formulas(), _np(free["xs"]), _np(free["us"]))[5]
    worst_free = np.max(np.stack([g.max(axis=1) for g in g_free.values()]), axis=0)
    with capsys.disabled():
        print("AL solve of expression_game_scene: status", status, "iters", out["iters"], "max g", np.round(worst, 5),
              "max g without the constraints", np.round(worst_free, 3))
    tol = float(spec.params.constraint_error_tolerance)
    for b in range(B):
        if status[b] == 1:
            assert worst[b] <= tol + 1e-9, (b, worst[b])
        else:
            assert worst[b] > tol - 1e-9 or out["iters"][b] >= spec.params.max_solver_iters, (b, worst[b])
    assert np.any(worst_free > tol), "a constraint should bind in some instance"
    assert status.sum() > 0, "no instance was solved"
    built_in = copy.deepcopy(spec)
    q = built_in.term_index("p1_acceleration_max")
    built_in.terms[q] = dict(built_in.terms[q], kind=abi.CONSTRAINT_SINGLE_DIMENSION, idx=(1, 0, 0, 0), flags=abi.FLAG_ORIENTED, polyline=-1)
    ref = {k: _np(v) for k, v in hip.Problem(built_in, abi.F64).solve(x0, augmented_lagrangian=True, deterministic=True).items() if k in KEYS}
    for k in KEYS:
        assert same_bits(out[k], ref[k]), k


def test_free_running_al_solve_of_the_intersection_twin_decides_like_the_original(hip, capsys):
    """three_player_intersection against its twin, free-running AL solves: instances whose iteration count or success
    differs are counted, not compared — no more of them than instances of the ORIGINAL that differ from its own run from
    x0 nudged by 1e-12 relative; the others agree to 1e-6."""
    spec = examples.three_player_intersection(T=T)
    spec.params.max_solver_iters = 30
    twin, _ = examples.expression_game_twin(spec)
    B = 8
    x0 = _close_x0(spec, B, seed=73, radius=(2.5, 4.0))
    nudged_x0 = x0 * (1.0 + 1e-12 * np.random.default_rng(6).standard_normal(x0.shape))
    ref = {k: _np(v) for k, v in hip.Problem(spec, abi.F64).solve(x0, augmented_lagrangian=True).items() if k in KEYS}
    nud = {k: _np(v) for k, v in hip.Problem(spec, abi.F64).solve(nudged_x0, augmented_lagrangian=True).items() if k in KEYS}
    out = {k: _np(v) for k, v in hip.Problem(twin, abi.F64).solve(x0, augmented_lagrangian=True).items() if k in KEYS}
    differs = lambda a: (a["iters"] != ref["iters"]) | (a["status"] != ref["status"])  # noqa: E731
    n_twin, n_nudged = int(differs(out).sum()), int(differs(nud).sum())
    with capsys.disabled():
        print("AL solve of three_player_intersection: twin differs in %d instances, the nudged original in %d; iters %s"
              % (n_twin, n_nudged, ref["iters"]))
    assert n_twin <= n_nudged
    for b in np.nonzero(~differs(out) & ~differs(nud))[0]:
        assert rel_err(out["xs"][b], ref["xs"][b]) <= max(1e-6, 10 * rel_err(nud["xs"][b], ref["xs"][b])), b


# ---- 6. per-instance threshold and weight ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("split_trial", [True, False])
def test_clearance_and_repulsion_weight_per_instance_equal_baked(hip, dtype, split_trial):
    """The clearance constraint's threshold and the repulsion's weight per instance: a heterogeneous batch returns the bits
    of problems created with those values baked in — the AL solve (row stage, multiplier update and constraint error read
    the instance's values) and the stage call."""
    spec = examples.expression_game_scene(T=T)
    spec.params.max_solver_iters = 10
    spec.x0 = _solve_x0(spec, 1, seed=0)[0]  # (the harness jitters the scene's own x0: the cars within reach of one another)
    params = [("p2_clearance", "value"), ("p1_repulsion", "weight"), ("p2_repulsion", "weight")]
    vectors = np.array([[3.0, 40.0, 40.0], [4.5, 10.0, 80.0], [2.0, 90.0, 5.0], [6.0, 0.0, 20.0]], np.float32)

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

    prob, _, x0, which = check_baked_equals_bound(hip, spec, dtype, bound, baked, vectors, B=4, deterministic=True,
                                                  split_trial=split_trial, augmented_lagrangian=True)
    xs, us = _game_points(hip, spec, dtype, B=4)
    lam, mu = _multipliers(4, spec.num_constraints, seed=11)
    got = [_np(a) for a in prob.quadraticize(xs, us, lam, mu)]
    for v in range(len(vectors)):
        sel = np.nonzero(which == v)[0]
        want = hip.Problem(baked(vectors[v]), dtype).quadraticize(xs[sel], us[sel], lam[sel], mu[sel])
        for a, b in zip(got, want):
            assert same_bits(a[sel], _np(b)), v


# ---- 7. the equality flag ----
def _equality_scene():
    """expression_game_scene with an EQUALITY expression constraint on car 2's speed, x - v = 0 with v above the speeds
    the car starts at: g < 0 all along the first trajectory."""
    from ilqgames_amd.abi import Expr
    spec = examples.expression_game_scene(T=T)
    spec.name_term("p2_speed_equals", spec.expression_constraint(1, Expr.x() - Expr.value(), (9,), value=7.0, is_equality=True))
    return spec


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_equality_constraint_takes_no_inactive_gate(hip, dtype):
    """quadraticize with g < 0 and a multiplier at or next to zero: an inequality would take no penalty there
    (Constraint::Mu), the equality applies mu; a negative multiplier enters as it is.  Against numpy."""
    NT = np.float64 if dtype == abi.F64 else np.float32
    spec = _equality_scene()
    formulas = dict(game_scene_formulas(), p2_speed_equals=upper_bound)
    xs, us = _game_points(hip, spec, dtype)
    B = xs.shape[0]
    assert xs[:, :, 9].max() < 7.0 - 1e-3
    lam, mu = _multipliers(B, spec.num_constraints, seed=13)
    slot = spec.terms[spec.term_index("p2_speed_equals")]["constraint_slot"]
    lam[:, slot, 1::3] = 5e-5          # below the gate's 1e-4
    lam[:, slot, 2::3] *= -1.0         # a running equality multiplier of the other sign
    assert np.all(constraint_mu(lam[:, slot], xs[:, :, 9] - 7.0, mu[:, None], True) == mu[:, None])
    dQ, dl, dR, dr, _, _ = numpy_contributions(spec, formulas, xs, us, lam, mu, NT)
    Q, l, _, _ = [_np(a).astype(np.float64) for a in hip.Problem(spec, dtype).quadraticize(xs, us, lam, mu)]
    Q0, l0, _, _ = [_np(a).astype(np.float64) for a in hip.Problem(without_expressions(spec), dtype).quadraticize(xs, us)]
    assert rel_err(Q, Q0 + dQ) < _tol(dtype) and rel_err(l, l0 + dl) < _tol(dtype)
    # mu is at work where the inequality's gate would have closed: H(v2, v2) of player 2 holds it
    n = spec.n
    gated = (lam[:, slot] == 0.0) | (lam[:, slot] == 5e-5)
    assert np.all((Q - Q0)[:, :, 1, 9 + n * 9][gated] > 0.99 * np.broadcast_to(mu[:, None], gated.shape)[gated] + 1.99)
    # ... and the same term as an inequality does take the gate
    ineq = copy.deepcopy(spec)
    ineq.terms[ineq.term_index("p2_speed_equals")]["flags"] = 0
    Qi = _np(hip.Problem(ineq, dtype).quadraticize(xs, us, lam, mu)[0]).astype(np.float64)
    assert np.all(np.abs((Qi - Q0)[:, :, 1, 9 + n * 9][gated] - 2.0) < 1e-3)


def test_al_run_leaves_a_negative_equality_multiplier_unclipped(hip, capsys):
    """An AL run of the equality scene: the first multiplier update meets g < 0 and the multiplier goes negative — clipped
    at zero the constraint would stay an inactive inequality and the speed where the cruise cost leaves it.  The run pulls
    car 2's speed up to the constraint's value as its affine restatement (AffineScalarConstraint, e_9^T x = 7, is_equality)
    does, and the same term without the flag does not."""
    spec = _equality_scene()
    spec.params.max_solver_iters = 30
    affine = copy.deepcopy(spec)
    q = affine.term_index("p2_speed_equals")
    a = [0.0] * spec.n
    a[9] = 1.0
    slot = affine.terms[q]["constraint_slot"]
    affine.terms[q] = dict(affine.terms[q], kind=abi.CONSTRAINT_AFFINE_SCALAR, idx=(0, 0, 0, 0), polyline=len(affine.dense_params),
                           constraint_slot=slot)
    affine.dense_params += a + [7.0]
    ineq = copy.deepcopy(spec)
    ineq.terms[q]["flags"] = 0
    B = 4
    x0 = _solve_x0(spec, B, seed=75)
    runs = {name: {k: _np(v) for k, v in hip.Problem(s, abi.F64).solve(x0, augmented_lagrangian=True, deterministic=True).items() if k in KEYS}
            for name, s in (("equality", spec), ("affine", affine), ("inequality", ineq))}
    gap = {name: np.abs(r["xs"][:, -1, 9] - 7.0) for name, r in runs.items()}
    with capsys.disabled():
        print("equality AL run: final |v2 - 7| expression %s  affine %s  inequality %s; iters %s" %
              (np.round(gap["equality"], 4), np.round(gap["affine"], 4), np.round(gap["inequality"], 4), runs["equality"]["iters"]))
    assert np.all(gap["equality"] < gap["inequality"] - 0.1)
    same = (runs["equality"]["iters"] == runs["affine"]["iters"]) & (runs["equality"]["status"] == runs["affine"]["status"])
    assert same.any()
    for b in np.nonzero(same)[0]:
        assert rel_err(runs["equality"]["xs"][b], runs["affine"]["xs"][b]) < 1e-6, b


# ---- 8. the value-only paths ----
def test_equilibrium_checks_evaluate_relative_costs_and_ignore_constraints(hip):
    """ilqg_strategy_costs_batch replays a strategy and sums the costs with term_evaluate_leaf: with the scene's relative
    costs and without any expression term, at a nominal and at a moved strategy, the difference is numpy's sum of the
    relative costs over the replayed trajectory — nothing of the constraints.  ilqg_check_local_nash_batch perturbs and
    compares such sums: the scene without its constraints returns the same bits."""
    spec = examples.expression_game_scene(T=T)
    base = without_expressions(spec)
    costs_only = _without_constraints(spec)
    B = 4
    x0 = _solve_x0(spec, B, seed=77)
    prob, base_p, costs_p = hip.Problem(spec, abi.F64), hip.Problem(base, abi.F64), hip.Problem(costs_only, abi.F64)
    rng = np.random.default_rng(78)
    xs, us = _operating_points(hip, base, abi.F64, x0, seed=79, us_scale=0.3)
    P = 0.002 * rng.standard_normal((B, T, spec.m * spec.n))
    formulas = {k: f for k, f in game_scene_formulas().items() if k in costs_only.term_names}
    deltas = []
    for alpha in (np.zeros((B, T, spec.m)), 0.3 * rng.standard_normal((B, T, spec.m))):
        replay = _np(prob.strategy_costs(x0, xs, us, P, alpha, euler=False))
        plain = _np(base_p.strategy_costs(x0, xs, us, P, alpha, euler=False))
        rx, ru = [_np(a) for a in base_p.rollout(x0, xs, us, P, alpha, np.ones(B))]
        dc = numpy_contributions(spec, formulas, rx, ru)[4]
        assert np.all(np.abs(dc) > 1e-3)
        assert np.max(np.abs((replay - plain) - dc)) < 1e-9 * np.abs(replay).max(), (replay - plain, dc)
        assert same_bits(replay, _np(costs_p.strategy_costs(x0, xs, us, P, alpha, euler=False)))
        deltas.append(replay - plain)
    assert np.max(np.abs(deltas[1] - deltas[0])) > 1e-3, "the moved strategy should change the relative costs"
    out = prob.solve(x0, deterministic=True, fixed_iters=3)
    sx, su, sP, sa = [_np(out[k]) for k in ("xs", "us", "P", "alpha")]
    ok, margin = prob.check_local_nash(x0, sx, su, sP, sa, 1e-2)
    ok_c, margin_c = costs_p.check_local_nash(x0, sx, su, sP, sa, 1e-2)
    assert np.all(np.isfinite(_np(margin))) and same_bits(_np(margin), _np(margin_c)) and same_bits(_np(ok), _np(ok_c))
    ok_b, margin_b = base_p.check_local_nash(x0, sx, su, sP, sa, 1e-2)
    assert not same_bits(_np(margin), _np(margin_b))
