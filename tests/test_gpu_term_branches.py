"""Every built-in cost and constraint kind on the device against the oracle, point by point and branch by branch.

The cases, their points and the branch census are tests/term_cases.py's (one term per problem, 6 x 67 points, two
shapes); tests/test_term_branches.py establishes on the CPU that every branch of every kind is among them.  Four
tests, in this order below:
  1. ilqg_quadraticize_batch and ilqg_total_costs_batch (the row programs: term_compute_leaf behind the TERM op, the
     polyline search behind the CLOSEST op) against the oracle on those points;
  2. the same cases inside one iteration of a solve, so that the fused, split, probing, compact and run-time-dimensioned
     row paths see the same branches: split / probing / compact against the fused form bit for bit; the
     run-time-dimensioned kernels against the shape's own, and the shape's own against the oracle, per instance at the
     forced-step test's tolerances, and in fp32 the two kernel families within the fp32 oracle's own distance from
     the fp64 oracle;
  3. ilqg_total_costs_batch of a two-step problem standing still at each point: the value the row path returns for
     the cost kinds, per point (the 67-step totals of test 1 hold it only as a sum);
  4. ilqg_strategy_costs_batch on the same points: the value path of the COST kinds (term_evaluate_leaf_of), which no
     row path runs.  It returns the value of the same term_compute_leaf and runs the same polyline scan as the rows,
     so tests 3 and 4 reach one body through two wrappers and two kernels; what is this path's own is the wrapper
     (the search over the table in global memory, the step's nominal pair, the affine / expression dispatch).  Its
     constraint kinds run only in the multiplier update of an augmented-Lagrangian solve and are not compared here:
     their g is the function whose derivatives test 1 pins.

Every point is judged on its own scale s, the largest absolute entry of the fp64 oracle's (Q, l, R, r) rows of that
point, and its bound comes from the oracle alone:
  fp64      MARGIN x max(8 eps64, the largest change of the fp64 oracle's rows under four random one-ulp nudges of
            the point's state and control), relative to s;
  fp32      MARGIN x max(8 eps32, the fp32 oracle's distance from the fp64 oracle at that point), relative to s; points
            on which the two oracle precisions take different branches are left out (the census counts them);
  boundary  (dyadic points exactly on a threshold, exact arithmetic; the constraints' points with g next to
            float32(1e-4) and the edge multipliers among them, except the polyline constraint's, whose g passes
            through a square root) MARGIN x eps of the dtype, no allowance.
MARGIN = 8 is for what legitimately differs: the device's hypot, fmod and sqrt may be an ulp from glibc's and feed
formulas whose conditioning the spread measures; everything else is compiled with contraction off on both sides.
The totals of ilqg_total_costs_batch are sums over the 67 steps in another order than the oracle's: their allowance is
max(T eps, spread) of the sum of the steps' absolute costs (reassociating a T-term sum moves it by at most (T - 1) eps
of that)."""
import functools
import json
import os

import numpy as np
import pytest

from ilqgames_amd import abi
import term_cases as tc

pytestmark = pytest.mark.gpu

MARGIN = 8
# a kind may get a larger margin only for a cause read in the code and written down here, never above 64
KIND_MARGIN = {}
EPS = {abi.F64: 2.0 ** -52, abi.F32: 2.0 ** -23}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "term_branches.json")
CASES = [(name, shape) for shape in tc.SHAPES for name in tc.case_names(shape)]


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    return h


def _np(t):
    return t.detach().cpu().numpy()


def _rows(quad):
    """(Q, l, R, r) -> [B][T][everything of the point], float64."""
    return np.concatenate([np.asarray(a, np.float64).reshape(tc.B, tc.T, -1) for a in quad], axis=2)


def _nudged(rng, a):
    a = np.asarray(a, np.float64)
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


@functools.lru_cache(maxsize=None)
def reference(name, shape):
    """Everything the comparison needs from the oracle, computed once per case and shape on the CPU."""
    from oracle import pyoracle
    p = tc.case_points(name, shape)
    spec = p["spec"]
    op = pyoracle.OracleProblem(spec)
    args = (p["lam"], p["mu"], p["te"])
    rows = {d: _rows(op.quadraticize(d, p["xs"], p["us"], *args)) for d in (abi.F64, abi.F32)}
    costs = {d: op.total_costs(d, p["xs"], p["us"]) for d in (abi.F64, abi.F32)}
    scale = np.abs(rows[abi.F64]).max(axis=2)
    spread = np.zeros((tc.B, tc.T))
    cost_spread = np.zeros((tc.B, len(spec.subsystems)))
    for seed in range(4):
        rng = np.random.default_rng(1000 + seed)
        xs, us = _nudged(rng, p["xs"]), _nudged(rng, p["us"])
        spread = np.maximum(spread, np.abs(_rows(op.quadraticize(abi.F64, xs, us, *args)) - rows[abi.F64]).max(axis=2))
        cost_spread = np.maximum(cost_spread, np.abs(op.total_costs(abi.F64, xs, us)[0] - costs[abi.F64][0]))
    cost_scale = np.array([[sum(abs(op.player_value(i, p["xs"][b, k], p["us"][b, k], step=k)) for k in range(tc.T))
                            for i in range(len(spec.subsystems))] for b in range(tc.B)])
    agree = tc.case_census(name, shape)[1]
    return dict(p=p, rows=rows, costs=costs, scale=scale, spread=spread, cost_spread=cost_spread, cost_scale=cost_scale,
                agree=agree)


def point_bounds(ref, dtype, margin):
    """[B][T] absolute bound of every point, and the mask of the points compared."""
    eps = EPS[dtype]
    if dtype == abi.F64:
        allowance = np.maximum(8 * eps, ref["spread"] / ref["scale"])
        compared = np.ones((tc.B, tc.T), bool)
    else:
        allowance = np.maximum(8 * eps, np.abs(ref["rows"][abi.F32] - ref["rows"][abi.F64]).max(axis=2) / ref["scale"])
        compared = ref["agree"].copy()
    allowance = np.where(ref["p"]["exact"], eps, allowance)
    return margin * allowance * ref["scale"], compared


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,shape", CASES)
def test_device_rows_and_costs_match_oracle_per_point(hip, oracle, name, shape, dtype):
    ref = reference(name, shape)
    p = ref["p"]
    spec = p["spec"]
    eps = EPS[dtype]
    margin = max([MARGIN] + [KIND_MARGIN.get(spec.terms[ti]["kind"], MARGIN) for ti in tc.case_terms(spec)])
    assert margin <= 64
    hp = hip.Problem(spec, dtype)
    dev = _rows([_np(a) for a in hp.quadraticize(p["xs"], p["us"], p["lam"], p["mu"], p["te"])])
    want = ref["rows"][dtype]
    bound, compared = point_bounds(ref, dtype, margin)
    err = np.abs(dev - want).max(axis=2)
    worst = float((err / (eps * ref["scale"]))[compared].max())
    golden = json.load(open(GOLDEN))["points"]["%s:%s" % (name, shape)]
    floor = golden["points"] - (golden["differ"] if dtype == abi.F32 else 0)
    print("\nterm-branches %s %s %s: compared %d of %d points, largest error %.2f eps" %
          (name, shape, "f64" if dtype == abi.F64 else "f32", int(compared.sum()), tc.B * tc.T, worst))
    assert int(compared.sum()) >= floor
    bad = np.argwhere(compared & ~(err <= bound))
    assert not len(bad), "%d points over their bound, first (b, k) = %s: error %.3g eps, bound %.3g eps, flags %s" % (
        len(bad), tuple(bad[0]), err[tuple(bad[0])] / (eps * ref["scale"][tuple(bad[0])]),
        bound[tuple(bad[0])] / (eps * ref["scale"][tuple(bad[0])]),
        tc.classify(oracle, spec, dtype, p["xs"][tuple(bad[0])], p["us"][tuple(bad[0])],
                    None if p["lam"] is None else p["lam"][bad[0][0]], int(bad[0][1])))
    # entries the oracle has as exact zeros are exact zeros on the device, the sign included
    zero = (want == 0) & compared[:, :, None]
    assert np.all(dev[zero] == 0)
    assert np.array_equal(np.signbit(dev[zero]), np.signbit(want[zero]))
    # a FinalTimeCost writes nothing before its first step: the state rows of player 0 hold no other term
    for ti in tc.case_terms(spec):
        first = spec.terms[ti]["first_step"]
        if first > 0:
            q_and_l = spec.n * spec.n * len(spec.subsystems) + spec.n * len(spec.subsystems)
            assert not dev[:, :first, :q_and_l].any()
    # total costs: per instance; an fp32 instance holding a point the precisions classify differently is left out
    c_dev, te_dev = hp.total_costs(p["xs"], p["us"])
    c_want, te_want = ref["costs"][dtype]
    assert np.array_equal(_np(te_dev), te_want)
    if dtype == abi.F64:
        c_allow = np.maximum(tc.T * eps, ref["cost_spread"] / ref["cost_scale"])
    else:
        c_allow = np.maximum(tc.T * eps, np.abs(np.asarray(c_want, np.float64) - ref["costs"][abi.F64][0]) /
                             ref["cost_scale"])
    c_err = np.abs(_np(c_dev).astype(np.float64) - c_want)
    rows_ok = compared.all(axis=1)
    assert np.all((c_err <= margin * c_allow * ref["cost_scale"])[rows_ok]), (c_err / (eps * ref["cost_scale"]))[rows_ok]


# ---------------------------------------------------------------------------------------------------------------------
# the same branches through the row paths of a solve
# ---------------------------------------------------------------------------------------------------------------------
GAMES = [(name, shape) for shape in tc.SHAPES for name in tc.game_names(shape)]
KEYS = ("costs", "P", "alpha", "xs")


@functools.lru_cache(maxsize=None)
def game_reference(name, shape, dtype):
    """The oracle's iteration and the instances it resolves (conditioning() of test_gpu_forced.py), once per game.
    The draw of x0 is the committed one (tests/golden/term_branches.json), not re-selected here: the committed census
    of the coasting lines is then the census of what runs, whatever this host's libm does to a borderline draw."""
    from oracle import pyoracle
    g = tc.game_draw(name, shape, json.load(open(GOLDEN))["games"]["%s:%s" % (name, shape)]["draw"])
    mask, ref = tc.game_mask(pyoracle, g, dtype)
    return g, mask, ref


def sched_generic(schedules):
    return all(v & abi.SCHEDULE_GENERIC for v in schedules.values())


def _close(dev, want, f64, where):
    """The forced-step test's own tolerances and scales (test_gpu_forced.py), per instance."""
    from helpers import rel_err
    tol_op, tol_st = (1e-9, 1e-9) if f64 else (2e-3, 1e-2)
    for b in range(tc.GAME_B):
        at = "%s instance %d" % (where, b)
        assert rel_err(dev["xs"][b], want["xs"][b]) < tol_op, at
        assert rel_err(dev["P"][b], want["P"][b]) < tol_st, at
        assert rel_err(dev["alpha"][b], want["alpha"][b]) < tol_st, at
        scale = max(1.0, float(np.max(np.abs(want["xs"][b]))), float(np.max(np.abs(want["costs"][b]))))
        assert float(np.max(np.abs(dev["costs"][b].astype(np.float64) - want["costs"][b]))) < tol_op * scale, at


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,shape", GAMES)
def test_solve_row_paths_agree_on_every_branch(hip, oracle, name, shape, dtype):
    """One iteration from the zero warm start of the game that wraps the case (T = 24, B = 8): the rows are taken
    along the coasting lines from x0, whose branch census is committed.  Constraint cases run with lambda = 0,
    mu = 10 — the state every augmented-Lagrangian solve starts in.  Against the oracle and between the specialised
    and the run-time-dimensioned kernels the step is forced; every instance is compared."""
    g, mask, ref = game_reference(name, shape, dtype)
    assert np.all(ref["status"] == 1)
    assert mask.all(), "the oracle does not resolve instances %s of this game" % np.nonzero(~mask)[0]
    prob = hip.Problem(g["spec"], dtype)
    schedules = {}

    def run(forced=True, **kw):
        out = prob.solve(g["x0"], fixed_iters=1, forced_steps=g["steps"] if forced else None, **kw)
        assert np.all(_np(out["iters"]) == 1), kw
        assert not forced or np.all(_np(out["status"]) == 1), kw
        schedules[tuple(sorted(kw.items()))] = prob.last_schedule()
        return {k: _np(out[k]).copy() for k in KEYS}

    def same_bits(a, b, what):
        for k in KEYS:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)
    # Schedules against one another, bit for bit.  A forced step keeps the trial in the fused kernel, so the split and
    # the probing row kernels are reached with the line search running instead (the first iteration's rows are the same
    # coasting lines); compact rows are compared in both modes.
    fused = run(forced=False, split_trial=False)
    same_bits(run(forced=False, split_trial=True, probe=False), fused, "split_trial")
    same_bits(run(forced=False, split_trial=True, probe=True), fused, "probe")
    same_bits(run(forced=False, compact_rows=False), run(forced=False, compact_rows=True), "compact_rows, line search")
    same_bits(run(compact_rows=False), run(compact_rows=True), "compact_rows, forced step")
    if shape == "car_car":   # the specialised instantiation really took the paths asked for
        sched = lambda **kw: schedules[tuple(sorted(kw.items()))]  # noqa: E731
        assert not sched(split_trial=False) & abi.SCHEDULE_SPLIT_TRIAL
        assert sched(split_trial=True, probe=False) & abi.SCHEDULE_SPLIT_TRIAL
        assert sched(split_trial=True, probe=True) & abi.SCHEDULE_SPLIT_TRIAL
        assert sched(compact_rows=True) & abi.SCHEDULE_COMPACT_ROWS and not sched(compact_rows=False) & abi.SCHEDULE_COMPACT_ROWS
        assert not sched(compact_rows=True) & abi.SCHEDULE_GENERIC
    else:
        assert sched_generic(schedules)
    base = run()
    f64 = dtype == abi.F64
    generic = run(generic_kernels=True)
    _close(generic, base, f64, "generic against the shape's own kernels")
    if not f64:
        # fp32: the forced-step tolerances are whole-percent figures.  Two correct fp32 forms of the same iteration
        # are apart by what fp32 loses in it, which the oracle measures per instance: its own fp32 / fp64 distance.
        from helpers import rel_err
        exact = game_reference(name, shape, abi.F64)[2]
        for b in range(tc.GAME_B):
            for k, ko in (("xs", "xs"), ("P", "rawP"), ("alpha", "alpha"), ("costs", "costs")):
                allowance = max(8 * EPS[dtype], rel_err(ref[ko][b], exact[ko][b]))
                assert rel_err(generic[k][b], base[k][b]) <= MARGIN * allowance, (k, b)
    want = dict(xs=ref["xs"], P=ref["rawP"], alpha=ref["alpha"], costs=ref["costs"])
    _close(base, want, f64, "against the oracle")
    print("\nterm-branches game %s %s %s: schedules %s" % (name, shape, "f64" if f64 else "f32",
                                                          {k: hex(v) for k, v in schedules.items()}))


# ---------------------------------------------------------------------------------------------------------------------
# the value path (term_evaluate_leaf_of, polyline_closest): reached through ilqg_strategy_costs_batch
# ---------------------------------------------------------------------------------------------------------------------
# The rows and ilqg_total_costs_batch take a term's value from the row programs (term_compute_leaf behind the TERM op,
# the polyline scan behind the CLOSEST op).  The value path — a wrapper that runs the same scan over the table in global
# memory, fetches the step's nominal pair and returns the value of the same term_compute_leaf — runs in the
# strategy-cost / Nash-check kernel and in the multiplier update.  It is pinned here per point: every point is an
# instance of its own of a two-step problem (the shortest the library takes) rolled out with the Euler step, so its
# cost is the term at the point plus the term one Euler step on; judged on the sum of the two steps' absolute costs,
# with the same allowances as above (the step's sin / cos are the device's: the spread under one-ulp nudges covers it).
COST_CASES = [(name, shape) for name, shape in CASES if "constraint" not in name]


@functools.lru_cache(maxsize=None)
def strategy_reference(name, shape):
    from oracle import pyoracle
    p = tc.case_points(name, shape)
    spec = tc.make_spec(name, shape, horizon=2)
    op = pyoracle.OracleProblem(spec)
    n, m, N, count = spec.n, spec.m, len(spec.subsystems), tc.B * tc.T
    x0 = p["xs"].reshape(count, n)
    us = np.repeat(p["us"].reshape(count, 1, m), 2, axis=1)
    zeros = dict(xs=np.zeros((count, 2, n)), P=np.zeros((count, 2, m * n)), alpha=np.zeros((count, 2, m)))

    def costs(dtype, x0_, us_):
        return np.asarray(op.strategy_costs(dtype, x0_, zeros["xs"], us_, zeros["P"], zeros["alpha"]), np.float64)
    want = {d: costs(d, x0, us) for d in (abi.F64, abi.F32)}
    spread = np.zeros((count, N))
    for seed in range(4):
        rng = np.random.default_rng(2000 + seed)
        spread = np.maximum(spread, np.abs(costs(abi.F64, _nudged(rng, x0), _nudged(rng, us)) - want[abi.F64]))
    scale = np.zeros((count, N))
    for b in range(count):
        x1 = op.dynamics(abi.F64, x0[b], us[b, 0], euler=True)[1]
        for i in range(N):
            scale[b, i] = abs(op.player_value(i, x0[b], us[b, 0], step=0)) + abs(op.player_value(i, x1, us[b, 1], step=1))
    # the same two-step problem standing still at the point: ilqg_total_costs_batch then returns the ROW path's value of
    # the point (steps 0 and 1 of it), which the 67-step totals of the first test only hold as a sum
    still = np.repeat(x0.reshape(count, 1, n), 2, axis=1)
    row_want = {d: np.asarray(op.total_costs(d, still, us)[0], np.float64) for d in (abi.F64, abi.F32)}
    row_spread = np.zeros((count, N))
    for seed in range(4):
        rng = np.random.default_rng(3000 + seed)
        nudged = np.repeat(_nudged(rng, x0).reshape(count, 1, n), 2, axis=1)
        row_spread = np.maximum(row_spread, np.abs(op.total_costs(abi.F64, nudged, _nudged(rng, us))[0] - row_want[abi.F64]))
    row_scale = np.array([[abs(op.player_value(i, x0[b], us[b, 0], step=0)) + abs(op.player_value(i, x0[b], us[b, 1], step=1))
                           for i in range(N)] for b in range(count)])
    return dict(spec=spec, x0=x0, us=us, zeros=zeros, want=want, spread=spread, scale=scale, still=still,
                row_want=row_want, row_spread=row_spread, row_scale=row_scale,
                agree=tc.case_census(name, shape)[1].reshape(count))


def _judge_values(tag, name, shape, dtype, dev, want, want64, spread, scale, agree):
    """Per point and player: |dev - want| <= MARGIN x max(8 eps, the oracle's spread (fp64) or its fp32 / fp64 distance
    (fp32)) of `scale`; scale 0 (the steps cost nothing) demands the oracle's value exactly."""
    eps = EPS[dtype]

    def relative(a):
        return np.divide(a, scale, out=np.zeros_like(a), where=scale > 0)
    if dtype == abi.F64:
        allowance = np.maximum(8 * eps, relative(spread))
        compared = np.ones(len(dev), bool)
    else:
        allowance = np.maximum(8 * eps, relative(np.abs(want - want64)))
        compared = agree
    err = np.abs(dev - want)
    print("\n%s %s %s %s: compared %d of %d points, largest error %.2f eps" %
          (tag, name, shape, "f64" if dtype == abi.F64 else "f32", int(compared.sum()), len(dev),
           float(relative(err)[compared].max() / eps)))
    bad = np.argwhere(compared[:, None] & ~(err <= MARGIN * allowance * scale))
    assert not len(bad), "%d values over their bound, first (point, player) = %s: error %.3g eps" % (
        len(bad), tuple(bad[0]), relative(err)[tuple(bad[0])] / eps)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,shape", COST_CASES)
def test_row_path_values_match_oracle_per_point(hip, name, shape, dtype):
    """The value a row op returns (term_compute_leaf), per point: every point an instance of a two-step problem whose
    trajectory stands still at it, through ilqg_total_costs_batch."""
    ref = strategy_reference(name, shape)
    hp = hip.Problem(ref["spec"], dtype)
    dev = _np(hp.total_costs(ref["still"], ref["us"])[0]).astype(np.float64)
    _judge_values("term-row-values", name, shape, dtype, dev, ref["row_want"][dtype], ref["row_want"][abi.F64],
                  ref["row_spread"], ref["row_scale"], ref["agree"])


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,shape", COST_CASES)
def test_strategy_cost_values_match_oracle_per_point(hip, name, shape, dtype):
    ref = strategy_reference(name, shape)
    hp = hip.Problem(ref["spec"], dtype)
    z = ref["zeros"]
    dev = _np(hp.strategy_costs(ref["x0"], z["xs"], ref["us"], z["P"], z["alpha"])).astype(np.float64)
    _judge_values("term-values", name, shape, dtype, dev, ref["want"][dtype], ref["want"][abi.F64], ref["spread"],
                  ref["scale"], ref["agree"])
