"""Expression terms as children of an ExtremeValueCost on the device: the restated children of the two reachability
scenes against the built-in SignedDistanceCost children, the sets no built-in kind expresses
(examples.shaped_reachability_scene) against a float64 numpy restatement (tests/shaped_children.py), the time an
expression child reads in the value-only walks, the whole solve against the built-in kinds under the project's
conditioning probe, every schedule of the solve against the others bit for bit, and per-instance faces and radii.  No
oracle: it does not know the kind."""
import copy

import numpy as np
import pytest

from ilqgames_amd import abi, examples
from helpers import rel_err
from instance_harness import KEYS, check_baked_equals_bound, same_bits, to_numpy as _np
import shaped_children as sc

pytestmark = pytest.mark.gpu

T = 12
LEAD = 1e-4  # the best child leads the runner-up by this much of the largest |child value|, or the comparison is void


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


def _tol(dtype):
    return 1e-9 if dtype == abi.F64 else 2e-4  # the project's parity bars (test_gpu_expression_cost.py)


def twin_points(spec, seed, B=3):
    """Plain seeded numpy, no rollout: jittered initial states held over the horizon plus noise."""
    rng = np.random.default_rng(seed)
    x0 = examples.jittered_x0(spec, B, seed)
    xs = np.tile(x0[:, None, :], (1, spec.T, 1)) + 0.05 * rng.standard_normal((B, spec.T, spec.n))
    us = 0.1 * rng.standard_normal((B, spec.T, spec.m))
    return xs, us


def shaped_points(spec, seed=51, B=4):
    """Operating points of shaped_reachability_scene that visit every child: both cars' positions are drawn about the box
    and the sets (4 m standard deviation), everything else as twin_points."""
    rng = np.random.default_rng(seed)
    xs, us = twin_points(spec, seed, B)
    xlo, xhi, ylo, yhi = examples.SHAPED_BOX
    for (px, py), (cx, cy) in zip(spec.position_dims, ((0.5 * (xlo + xhi), 0.5 * (ylo + yhi)), (-5.0, 1.0))):
        xs[..., px] = cx + 4.0 * rng.standard_normal((B, spec.T))
        xs[..., py] = cy + 4.0 * rng.standard_normal((B, spec.T))
    return xs, us


def with_structure(spec, structure):
    s = copy.deepcopy(spec)
    s.player_costs = [(a, b, structure) for a, b, _ in s.player_costs]
    return s


# ---- 1. the restated children against the built-in ones ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene,children", [("three_player_collision_avoidance_reachability", 6),
                                            ("three_player_intersection_reachability", 2)])
def test_twin_children_quadraticize_and_cost_like_the_signed_distance_children(hip, dtype, scene, children):
    """The scene and its twin (examples.reachability_twin: every SignedDistanceCost child restated as an expression child,
    role CHILD kept) at three seeded operating points each: the total costs and Q, l, R, r — quadraticised in full at the
    time of extreme the costs report — to the project's parity bars against each array's largest entry, and the same
    time_of_extreme.  The built-in child forms its distance with t_hypot, the restatement with sqrt(X^2 + Y^2), so a tie
    between children could fall either way: every child's value is computed here in float64, and at EVERY (instance,
    step, parent) the best must lead the runner-up by LEAD of the largest |child value| (measured without a device: the
    smallest lead is 3.5e-4 of it, collision-avoidance scene, seed 21; 0.39 in the intersection scene)."""
    spec = getattr(examples, scene)(T=T)
    twin, _ = examples.reachability_twin(spec)
    kids = [q for _, ks in sc.parents_of(twin) for q in ks]
    assert len(kids) == children and all(twin.terms[q]["kind"] == abi.COST_EXPRESSION and twin.terms[q]["role"] == abi.ROLE_CHILD
                                         for q in kids)
    orig_p, twin_p = hip.Problem(spec, dtype), hip.Problem(twin, dtype)
    assert twin_p.row_program()[1] == 0
    nc = spec.num_constraints
    tol = _tol(dtype)
    for seed in (21, 31, 41):
        xs, us = twin_points(spec, seed)
        values = sc.signed_distance_children(spec, xs)
        largest = max(np.abs(v).max() for v in values)
        lead = min(sc.lead_of_best(v, False).min() for v in values)
        print(scene, dtype, "seed", seed, "smallest lead %.3e of the largest child value" % (lead / largest))
        assert lead >= LEAD * largest, (seed, lead, largest)
        rng = np.random.default_rng(3)
        lam = np.abs(rng.standard_normal((3, max(nc, 1), T))) if nc else None
        mu = np.array([10.0, 11.0, 12.1]) if nc else None
        (c_t, te_t), (c_o, te_o) = twin_p.total_costs(xs, us), orig_p.total_costs(xs, us)
        c_t, c_o, te_t, te_o = _np(c_t), _np(c_o), _np(te_t), _np(te_o)
        print(scene, dtype, "seed", seed, "costs %.3e" % rel_err(c_t, c_o), "time_of_extreme", te_o.tolist())
        if not np.array_equal(te_t, te_o):
            print("time_of_extreme differs: twin", te_t.tolist(), "costs", c_t.tolist(), "built-in", c_o.tolist())
        assert np.array_equal(te_t, te_o)
        assert np.all(np.isfinite(c_t)) and rel_err(c_t, c_o) < tol
        for name, a, b in zip("QlRr", twin_p.quadraticize(xs, us, lam, mu, t_extreme=te_t), orig_p.quadraticize(xs, us, lam, mu, t_extreme=te_o)):
            err = rel_err(_np(a), _np(b))
            print(scene, dtype, "seed", seed, name, "%.3e" % err)
            assert err < tol, (seed, name, err)
        # the children are in what was compared: the parents' players have state-cost entries at their time of extreme
        l_o = _np(orig_p.quadraticize(xs, us, lam, mu, t_extreme=te_o)[1])
        for parent, _ in sc.parents_of(spec):
            i = spec.terms[parent]["player"]
            assert all(np.abs(l_o[b, te_o[b, i], i]).max() > 0.1 for b in range(3))


# ---- 2. the sets no built-in kind restates ----
def _check_the_points_visit_every_child(spec, xs):
    """In numpy: every one of the seven children is the active one at some (instance, step), the moving disc at a step
    k > 0, and no choice between children hangs on the last bits (LEAD, as in test 1)."""
    pars = sc.shaped_children(spec, xs)
    largest = max(np.abs(p["values"]).max() for p in pars)
    seen = {}
    for par in pars:
        best, _ = sc.first_strict(par["values"], par["is_min"])
        lead = sc.lead_of_best(par["values"], par["is_min"]).min()
        print("player", par["player"], "smallest lead %.3e of the largest child value" % (lead / largest))
        assert lead >= LEAD * largest
        for q, name in enumerate(par["names"]):
            seen[name] = np.argwhere(best == q)
    print({n: len(v) for n, v in seen.items()})
    assert sorted(seen) == sorted(examples.SHAPED_CHILDREN) and all(len(v) > 0 for v in seen.values()), {n: len(v) for n, v in seen.items()}
    assert np.any(seen["p2_moving_disc"][:, 1] > 0)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_shaped_sets_match_the_numpy_restatement(hip, dtype):
    """shaped_reachability_scene against the same scene without its two parents plus the float64 numpy restatement
    (analytic value, gradient and Hessian per child, first strict improvement per step, the parent's structure over
    time).  Time-additive copies of both scenes quadraticise every row in full: the differences of Q, l and of the total
    costs over all steps.  The scene itself (MIN and MAX over time): its totals and times of extreme against the
    restatement of the whole per-step cost, and Q, l at those times."""
    spec = examples.shaped_reachability_scene(T=T)
    base = sc.without_parents(spec)
    xs, us = shaped_points(spec)
    _check_the_points_visit_every_child(spec, xs)
    dQ, dl, value, _ = sc.shaped_contributions(spec, xs)
    assert np.abs(dQ).max() > 1e-2 and np.abs(dl).max() >= 1.0
    tol = _tol(dtype)
    # every row in full: the time-additive copies
    sum_p, sum_base_p = hip.Problem(with_structure(spec, abi.SUM), dtype), hip.Problem(with_structure(base, abi.SUM), dtype)
    assert sum_p.row_program()[1] == 0
    Q, l, R, r = [_np(a).astype(np.float64) for a in sum_p.quadraticize(xs, us)]
    Q0, l0, R0, r0 = [_np(a).astype(np.float64) for a in sum_base_p.quadraticize(xs, us)]
    for name, a, b in (("Q", Q, Q0 + dQ), ("l", l, l0 + dl), ("R", R, R0), ("r", r, r0)):
        print(dtype, "sum", name, "%.3e" % rel_err(a, b))
        assert rel_err(a, b) < tol, name
    c, c0 = _np(sum_p.total_costs(xs, us)[0]).astype(np.float64), _np(sum_base_p.total_costs(xs, us)[0]).astype(np.float64)
    print(dtype, "sum costs %.3e" % rel_err(c, c0 + value.sum(axis=1)))
    assert rel_err(c, c0 + value.sum(axis=1)) < tol
    assert np.all(np.abs(value.sum(axis=1)) > 1e-3 * np.abs(c))
    # the scene's own structures: min / max over time of the whole per-step cost
    prob, base_p = hip.Problem(spec, dtype), hip.Problem(base, dtype)
    want_c, want_te = sc.over_time(spec, sc.quadratic_step_costs(spec, xs, us) + value)
    got_c, got_te = prob.total_costs(xs, us)
    got_c, got_te = _np(got_c), _np(got_te)
    print(dtype, "costs %.3e" % rel_err(got_c, want_c), "time_of_extreme", got_te.tolist())
    assert np.array_equal(got_te, want_te) and rel_err(got_c, want_c) < tol
    Q, l, _, _ = [_np(a).astype(np.float64) for a in prob.quadraticize(xs, us, t_extreme=got_te)]
    Q0, l0, _, _ = [_np(a).astype(np.float64) for a in base_p.quadraticize(xs, us, t_extreme=got_te)]
    at = np.zeros(xs.shape[:2] + (2, 1))  # 1 where player i's row is the one quadraticised in full
    for b in range(xs.shape[0]):
        for i in range(2):
            at[b, got_te[b, i], i] = 1.0
    assert rel_err(Q, Q0 + at * dQ) < tol and rel_err(l, l0 + at * dl) < tol
    assert np.abs(at * dl).max() >= 1.0


# ---- 3. the time in the value-only walks ----
def test_strategy_costs_evaluate_expression_children_at_their_step(hip):
    """ilqg_strategy_costs_batch replays a strategy and sums every player's per-step costs with the value-only walk
    (extreme_child); the row stage's cost pass sums the same per-step costs for the time-additive copy of the scene.  The
    converged gains with the feed-forward zeroed retrace the operating point under the solver's own integrator, so the two
    agree to accumulation error (1e-9, the bar of test_equilibrium_checks_evaluate_expression_costs) — if the walk hands
    the moving disc the time of its step.  In numpy: evaluated at t = 0 instead, the disc would move some instance's
    total by far more than that."""
    spec = examples.shaped_reachability_scene(T=T)
    spec.params.max_solver_iters = 30
    B = 4
    x0 = examples.jittered_x0(spec, B, seed=47)
    prob = hip.Problem(spec, abi.F64)
    out = prob.solve(x0, deterministic=True)
    xs, us, P = _np(out["xs"]), _np(out["us"]), _np(out["P"])
    assert np.all(np.isfinite(xs)) and np.all(np.isfinite(us))
    replay = _np(prob.strategy_costs(x0, xs, us, P, np.zeros_like(_np(out["alpha"])), euler=False))
    total = _np(hip.Problem(with_structure(spec, abi.SUM), abi.F64).total_costs(xs, us)[0])
    print("replay", replay.tolist(), "row stage", total.tolist(), "rel %.3e" % rel_err(replay, total))
    # what a walk that evaluated the children at step 0 would have summed for player 2
    at_step = sc.shaped_children(spec, xs)[1]
    at_zero = sc.shaped_children(spec, xs, time_of=lambda name, t: np.zeros_like(t))[1]
    assert at_step["names"][1] == "p2_moving_disc"
    moved = np.abs(sc.first_strict(at_zero["values"], False)[1].sum(axis=1) - sc.first_strict(at_step["values"], False)[1].sum(axis=1))
    print("a step-0 walk would move player 2's totals by", (moved / np.abs(total[:, 1])).tolist())
    assert np.any(moved > 1e-6 * np.abs(total[:, 1]))
    assert np.any(sc.first_strict(at_step["values"], False)[0][:, 1:] == 1), "the moving disc is active at a step k > 0"
    assert np.all(np.isfinite(total)) and rel_err(replay, total) < 1e-9, (replay, total)
    # the numpy restatement agrees with both sums
    want = (sc.quadratic_step_costs(spec, xs, us) + sc.shaped_contributions(spec, xs)[2]).sum(axis=1)
    assert rel_err(total, want) < 1e-9
    ok, margin = prob.check_local_nash(x0, xs, us, P, _np(out["alpha"]), 1e-2)
    assert np.all(np.isfinite(_np(margin))) and _np(ok).shape == (B,)


# ---- 4. the whole solve ----
def test_twin_solves_like_the_signed_distance_children_within_the_measured_conditioning(hip):
    """The collision-avoidance reachability scene and its twin under forced steps (3 iterations of 0.1, B = 4, fp64), and
    the original once more from x0 nudged by 1e-12 relative (DESIGN.md section 2's conditioning probe).  Per instance and
    per output the twin may be at most 10 x as far from the original as the nudged run is, floor 1e-12 relative.  Every
    instance counts, and the iteration counts are equal."""
    spec = examples.three_player_collision_avoidance_reachability(T=T)
    twin, _ = examples.reachability_twin(spec)
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


# ---- 5. every schedule runs it ----
def _free_running(hip, spec, dtype, x0, **kw):
    prob = hip.Problem(spec, dtype)
    out = prob.solve(x0, deterministic=True, **kw)
    return prob, {k: _np(v) for k, v in out.items() if k in KEYS}


def _schedule_scene():
    spec = examples.shaped_reachability_scene(T=T)
    spec.params.max_solver_iters = 30
    return spec, examples.jittered_x0(spec, 4, seed=41)


def test_every_schedule_of_the_solve_returns_the_same_bits(hip):
    spec, x0 = _schedule_scene()
    prob, ref = _free_running(hip, spec, abi.F64, x0)
    assert int(ref["iters"].min()) > 1 and np.all(np.isfinite(ref["xs"]))
    assert not prob.last_schedule() & abi.SCHEDULE_STATIC_ROWS, "static_rows = AUTO falls back to the interpreter"
    # a step is rejected somewhere: the line search's gradient-only row pass runs the children
    state = prob.solve_state(prob.solve(x0, deterministic=True))
    print("iters", ref["iters"].tolist(), "backtracks", _np(state["backtracks"]).tolist())
    assert int(_np(state["backtracks"]).max()) > 0, "no step was rejected"
    seen = set()
    for kw in (dict(split_trial=True), dict(split_trial=False), dict(compact_rows=False), dict(compact_rows=True),
               dict(split_trial=True, compact_rows=False), dict(static_rows=True), dict(handoff=False),
               dict(probe=True, split_trial=True), dict(probe=False, split_trial=True)):
        p, out = _free_running(hip, spec, abi.F64, x0, **kw)
        seen.add(p.last_schedule() & (abi.SCHEDULE_SPLIT_TRIAL | abi.SCHEDULE_COMPACT_ROWS))
        if "split_trial" in kw:  # the pin is honoured and reported
            assert bool(p.last_schedule() & abi.SCHEDULE_SPLIT_TRIAL) == kw["split_trial"]
        if "compact_rows" in kw:
            assert bool(p.last_schedule() & abi.SCHEDULE_COMPACT_ROWS) == kw["compact_rows"]
        assert not p.last_schedule() & abi.SCHEDULE_STATIC_ROWS
        for k in KEYS:
            assert same_bits(out[k], ref[k]), (kw, k)
    assert len(seen) >= 3


def test_generic_kernels_solve_the_shaped_scene_like_the_specialised_ones(hip):
    """One pass with generic_kernels = ON: the run-time-dimensioned kernels run the same row program; their sweeps order
    the arithmetic differently, so the bar is 1e-9 and the iteration counts are equal."""
    spec, x0 = _schedule_scene()
    _, ref = _free_running(hip, spec, abi.F64, x0)
    p, out = _free_running(hip, spec, abi.F64, x0, generic_kernels=True)
    assert p.last_schedule() & abi.SCHEDULE_GENERIC
    assert np.array_equal(out["iters"], ref["iters"])
    for k in ("xs", "us", "P", "alpha", "costs"):
        print(k, "%.3e" % rel_err(out[k], ref[k]))
        assert rel_err(out[k], ref[k]) < 1e-9, k


# ---- 6. per-instance faces and radii ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("split_trial", [True, False])
def test_box_faces_and_ellipse_radius_per_instance_equal_baked(hip, dtype, split_trial):
    spec = examples.shaped_reachability_scene(T=T)
    spec.params.max_solver_iters = 10
    params = [("p1_box_right", "value"), ("p1_box_left", "value"), ("p1_box_top", "value"), ("p1_box_bottom", "value"),
              ("p2_ellipse", "value")]
    vectors = np.array([[1.5, -1.5, 3.0, -1.0, 4.0], [3.0, 0.5, 1.0, -3.0, 6.0], [0.0, -4.0, 5.0, 2.0, 2.0], [2.5, -2.5, -2.0, -5.0, 8.0]],
                       np.float32)

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
