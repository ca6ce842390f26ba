"""The numpy reference of tests/lq_games.py, checked on the CPU before it judges the device (tests/test_gpu_lq_games.py):
against the oracle on the one game both know, by the identities an exactly linear-quadratic game satisfies, its open-loop
sweep against one dense solve of the stacked first-order conditions, its hand-written matrices against central differences
of the programs, its conditioning under a nudge of x0 — every game, instance and iteration — and its distance from itself
in the next wider scalar type against the committed tests/golden/lq_games.json.

The identities.  The rollout is the ABI's RK4, the linearisation its Euler form, and the two maps differ by O((dt J)^2):
an LQ solve is exact for the rollout only where they are the same map.  So alpha_{k+1} = (1 - s_k) alpha_k is asserted
where that holds — every game without Gershgorin corrections under the reference's Euler rollout, and the `integrator`
game (J_x = 0) under the RK4 — and the RK4's departure from it on the damped chains is printed, not asserted: measured
max |alpha_k| / max |alpha_1| = 1, 0.493 .. 0.501, 0.368 .. 0.376, 0.0006 .. 0.0053 under steps (0.5, 0.25, 1, 0.5).
The gains need no such condition: A, B, Q and R do not depend on the operating point, so rawP has the same bits in every
iteration."""
import json
import os

import numpy as np
import pytest

import lq_games as G
from ilqgames_amd import abi
from helpers import GOLDEN
from test_expression_cost import np_jet

K = len(G.STEPS)
NO_CORRECTIONS = [g for g in G.GAMES if "gershgorin" not in g]


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return h


def committed():
    return json.load(open(os.path.join(GOLDEN, "lq_games.json")))


# ---- 1. against the oracle ----
@pytest.mark.parametrize("open_loop", [False, True], ids=["feedback", "open_loop"])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32], ids=["f64", "f32"])
def test_reference_matches_the_oracle_on_the_point_mass_game(oracle, dtype, open_loop):
    """Built-in quadratic / quadratic_difference costs on two point masses, after every forced iteration, every instance:
    1e-9 in fp64, the project's fp32 bars in fp32 (alpha on the scale of the first iteration's)."""
    game = G.build_point_mass(expression_costs=False, open_loop=open_loop)
    precision = "f64" if dtype == abi.F64 else "f32"
    NT = np.float64 if dtype == abi.F64 else np.float32
    x0 = game.x0(G.B, G.SEED)
    op = oracle.OracleProblem(game.spec)
    steps = np.tile(np.array(G.STEPS), (G.B, 1))
    mine = G.reference_run(game, x0, NT)
    first = None
    for k in range(1, K + 1):
        ref = op.solve(dtype, x0, fixed_iters=k, forced_steps=steps[:, :k], merit_log_len=k)
        assert np.all(ref["iters"] == k) and np.all(ref["status"] == 1)
        theirs = dict(xs=ref["xs"], us=ref["us"], P=ref["rawP"], alpha=ref["alpha"], costs=ref["costs"],
                      merit=ref["log"][:, k - 1, 0], expected_decrease=ref["log"][:, k - 1, 1])
        first = first or theirs
        for q in G.OUTPUTS:
            err = G.errors(q, mine[k - 1], theirs, first).max()
            print(precision, "open" if open_loop else "feedback", k, q, "%.2e" % err)
            assert err < G.PROJECT_BAR[precision][q], (k, q, err)
        if open_loop:
            assert not np.any(ref["rawP"]) and not np.any(mine[k - 1]["P"])


# ---- 2. what the builder promises ----
@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_the_gershgorin_step_fires_where_the_game_is_built_for_it_and_nowhere_else(name):
    game = G.GAMES[name]()
    count = sum(int(it["corrections"].sum()) for it in G.cached_run(name, "float64"))
    print(name, "Gershgorin corrections over %d instances x %d iterations: %d" % (G.B, K, count))
    if game.gershgorin:
        assert count > 0 and not game.open_loop
        per_iteration = [it["corrections"] for it in G.cached_run(name, "float64")]
        assert all(np.array_equal(c, per_iteration[0]) for c in per_iteration), "S does not depend on the operating point"
    else:
        assert count == 0


def test_the_library_sees_the_variant_of_b(hip):
    """ilqg_sweep_b_structure_build on the shapes with kernels of their own: one PUSH_X of a control is a constant entry
    dt, -(d x) + g u a computed one."""
    for shape in ("8_2_1", "17_3_2"):
        constant, entries = hip.sweep_b_structure(G.build(shape, "constant_b").spec)
        game = G.build(shape, "constant_b")
        assert constant and sorted((int(r), int(c)) for r, c, _, _ in entries) == sorted(zip(*np.nonzero(game.Ju)))
        assert set(entries[:, 2]) == {abi.B_ENTRY_DT}
        assert not hip.sweep_b_structure(G.build(shape, "computed_b").spec)[0]
    assert hip.sweep_b_structure(G.build_point_mass(expression_costs=True).spec)[0]
    for name in G.GAMES:  # every game is one the library accepts: its terms, its rows, its programs
        game = G.GAMES[name]()
        for ti, t in enumerate(game.spec.terms):
            if t["kind"] in (abi.COST_EXPRESSION, abi.DYN_ROW_EXPRESSION):
                hip.expression_check(game.spec, ti)


# ---- 3. the identities ----
def _alpha_ratios(run):
    a = np.array([np.abs(it["raw_alpha"]).max() for it in run])
    return a / a[0]


@pytest.mark.parametrize("name", NO_CORRECTIONS)
def test_exact_lq_identities(name):
    """Steps (0.5, 0.25, 1, 0.5): max |alpha_k| / max |alpha_1| = 1, 0.5, 0.375 and 0, the full step lands on the fixed
    point and the last step no longer moves the trajectory.  Bars: 1e-12 of the first alpha's / the trajectory's scale,
    4500 eps — each iteration is a sweep of T = 12 steps of n <= 24 wide sums through an elimination of condition < 10."""
    game = G.GAMES[name]()
    for b, x0 in enumerate(game.x0(3, G.SEED)):
        rk4 = G.solve(game, x0, G.STEPS, np.float64)
        exact = rk4 if game.shape == "integrator" else G.solve(game, x0, G.STEPS, np.float64, integrator="euler")
        for run in (rk4, exact):  # the gains: the same bits in every iteration, whatever the rollout
            assert all(np.array_equal(it["rawP"], run[0]["rawP"]) for it in run)
        print(name, b, "rk4", _alpha_ratios(rk4), "exact model", _alpha_ratios(exact))
        ratios = _alpha_ratios(exact)
        assert np.abs(ratios[:3] - [1.0, 0.5, 0.375]).max() < 1e-12 and ratios[3] < 1e-12
        a1 = exact[0]["raw_alpha"]
        for k, factor in ((1, 0.5), (2, 0.375)):  # entry by entry: alpha_{k+1} = (1 - s_k) alpha_k
            assert np.abs(exact[k]["raw_alpha"] - factor * a1).max() < 1e-12 * np.abs(a1).max()
        scale = np.abs(exact[2]["xs"]).max()
        assert np.abs(exact[3]["xs"] - exact[2]["xs"]).max() < 1e-12 * scale
        assert np.abs(exact[3]["us"] - exact[2]["us"]).max() < 1e-12 * max(1.0, np.abs(exact[2]["us"]).max())
        if game.shape != "integrator":  # the RK4 is another map than I + dt J: close to the identity, not on it
            assert 1e-5 < _alpha_ratios(rk4)[3] < 0.05


# ---- 4. open loop: the sweep against the stacked first-order conditions ----
@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_open_loop_sweep_equals_the_dense_kkt_solve(name):
    """Every game's LQ problem at its initial operating point, from a random initial deviation: the sweep's alpha and
    states against one dense solve, 1e-10 of their largest entry (the stacked matrix's condition number is printed)."""
    game = G.GAMES[name]()
    tb = G.Tables(game, np.float64)
    x0 = game.x0(1, G.SEED)[0]
    xs, us = G._start(game, tb, x0, "rk4")
    lq = G.lq_inputs(game, tb, xs, us)
    dx0 = np.random.default_rng(3).uniform(-0.5, 0.5, game.n)
    P, alpha, dxs, _ = G.open_loop_sweep(game, lq, dx0, np.float64)
    alpha_kkt, dxs_kkt = G.open_loop_kkt(game, lq, dx0)
    ea = np.abs(alpha - alpha_kkt).max() / np.abs(alpha_kkt).max()
    ex = np.abs(dxs - dxs_kkt).max() / np.abs(dxs_kkt).max()
    print(name, "alpha %.2e  dx %.2e" % (ea, ex))
    assert not np.any(P) and np.abs(alpha_kkt).max() > 1e-2
    assert ea < 1e-10 and ex < 1e-10


# ---- 5. the programs are the matrices ----
def _program_value(t, v, param0=0.0):
    """The term's program at the argument vector v (over t["idx"]), plain numpy (np_jet's value)."""
    k = len(t["dims"])
    ins = [v[a] - (v[k + a] if t["relative_to"] else 0.0) for a in range(k)]
    return float(np_jet(t["program"], t["weight"], t["value"], ins[0], ins[1] if k > 1 else 0.0, np.float64)[0])


@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_central_differences_of_the_programs_reproduce_the_hand_written_matrices(name):
    """Values, gradients and Hessians of every cost program (second-order central differences, exact for a quadratic up to
    rounding: steps of 1/2, dyadic points), and the Jacobian rows of every rate program."""
    game = G.GAMES[name]()
    rng = np.random.default_rng(11)
    h = 0.5
    checked = 0
    for t in game.terms:
        if t["program"] is None:
            continue
        d = len(t["idx"])
        v = np.round(rng.uniform(-2, 2, d) * 8) / 8
        f = lambda w: _program_value(t, w)  # noqa: E731
        E = np.eye(d) * h
        assert abs(f(v) - (0.5 * v @ t["H"] @ v + t["g"] @ v + t["c"])) < 1e-13
        grad = np.array([(f(v + E[a]) - f(v - E[a])) / (2 * h) for a in range(d)])
        hess = np.array([[(f(v + E[a] + E[b]) - f(v + E[a] - E[b]) - f(v - E[a] + E[b]) + f(v - E[a] - E[b])) / (4 * h * h)
                          for b in range(d)] for a in range(d)])
        assert np.abs(grad - (t["H"] @ v + t["g"])).max() < 1e-13 and np.abs(hess - t["H"]).max() < 1e-13
        checked += 1
    assert checked or name == "point_mass"
    spec = game.spec
    for i, (kind, xdim, udim, param0) in enumerate(spec.subsystems):
        if kind != abi.DYN_EXPRESSION:
            continue
        rows = [t for t in spec.terms if t["kind"] == abi.DYN_ROW_EXPRESSION and t["player"] == i]
        assert sorted(t["idx"][0] for t in rows) == list(range(xdim))
        for t in rows:
            r, xin, yin = t["idx"][0], t["idx"][1], t["idx"][2]
            cnt = int(spec.dense_params[t["polyline"]])
            words = spec.dense_params[t["polyline"] + 1:t["polyline"] + 1 + 2 * cnt]
            program = [(int(words[2 * a]), words[2 * a + 1]) for a in range(cnt)]
            z = np.round(rng.uniform(-2, 2, xdim + udim) * 8) / 8  # the subsystem's own [x | u]
            rate = lambda w: float(np_jet(program, t["weight"], param0, w[xin], w[yin] if yin >= 0 else 0.0, np.float64)[0])  # noqa: E731
            row = np.array([(rate(z + h * e) - rate(z - h * e)) / (2 * h) for e in np.eye(xdim + udim)])
            want = np.concatenate([game.Jx[game.xoff[i] + r, game.xoff[i]:game.xoff[i + 1]],
                                   game.Ju[game.xoff[i] + r, game.uoff[i]:game.uoff[i + 1]]])
            assert np.abs(row - want).max() < 1e-13, (i, r)
            assert abs(rate(z) - want @ z) < 1e-13


def test_a_final_time_gate_is_part_of_the_matrices():
    for name in G.GAMES:
        game = G.GAMES[name]()
        gated = [t for t in game.terms if t["first_step"] > 0]
        assert gated and all(0 < t["first_step"] < game.T - 1 for t in gated)
        tb = G.Tables(game, np.float64)
        i = gated[0]["player"]
        assert not np.array_equal(tb.Hx[0, i], tb.Hx[game.T - 1, i])


# ---- 6. conditions on the inputs: nothing is skipped ----
@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_a_nudge_of_x0_moves_no_output_of_any_instance_or_iteration(name):
    """x0 + 1e-12 noise moves no output by more than 1e-10 relative (alpha on the scale of the first iteration's): the
    amplification every (instance, iteration) pair of the device comparison may count on, so that none is left out."""
    ref, nud = G.cached_run(name, "float64"), G.cached_run(name, "float64", nudged=True)
    worst = 0.0
    for k in range(K):
        for q in G.OUTPUTS:
            err = G.errors(q, nud[k], ref[k], ref[0])
            assert err.shape == (G.B,)
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-10, (name, k, q, err)
    print(name, "amplification of a 1e-12 nudge: %.2f" % (worst / 1e-12))


# ---- 7. the committed gaps ----
@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_committed_gaps_are_the_reference_s_own(name):
    """tests/golden/lq_games.json within a factor of 2 of what this machine computes (both floored at one ulp of the
    narrower type: a gap of 0 or of a fraction of an ulp is rounding luck), and every bar made of them no looser than the
    project's existing ones."""
    want, got = committed()[name], G.gaps(name)
    for key, precision in (("gap64", "f64"), ("gap32", "f32")):
        for q in G.OUTPUTS:
            a, b = max(want[key][q], G.EPS[precision]), max(got[key][q], G.EPS[precision])
            assert 0.5 <= a / b <= 2.0, (name, key, q, want[key][q], got[key][q])
            assert G.bar(committed(), name, q, precision) <= G.PROJECT_BAR[precision][q]
    assert set(committed()) == set(G.GAMES)


# ---- 7b. the comparison notices the handling errors it was written for ----
def _drop_off_diagonal_r_ij(game):
    for t in game.terms:
        if t["on"] != "x" and t["on"] != t["player"]:
            t["H"] = np.diag(np.diag(t["H"]))


def _drop_cross_player_q(game):
    owner = lambda e: max(i for i in range(game.N) if game.xoff[i] <= e)  # noqa: E731
    for t in game.terms:
        if t["on"] == "x":
            for a, ea in enumerate(t["idx"]):
                for b, eb in enumerate(t["idx"]):
                    if owner(ea) != owner(eb):
                        t["H"][a, b] = 0.0


def _constant_entry_for_a_computed_b(game):
    game.Ju[game.Ju != 0] = 1.0


@pytest.mark.parametrize("name,mutate", [("17_3_2", _drop_off_diagonal_r_ij), ("14_3_2", _drop_off_diagonal_r_ij),
                                         ("8_2_1_computed_b", _drop_cross_player_q), ("point_mass_expression", _drop_cross_player_q),
                                         ("8_2_1_computed_b", _constant_entry_for_a_computed_b),
                                         ("17_3_2", _constant_entry_for_a_computed_b)])
def test_the_bars_tell_a_solve_that_mishandles_one_kind_of_entry(name, mutate):
    """A solve that drops the off-diagonal entries of R_ij (i != j), drops the Q entries that couple two players' states,
    or takes dt for a computed entry of B — restated by changing the hand-written matrices — lands at least 1e6 bars away
    from the reference after the first iteration, in fp64 and in fp32, on the gains or the feed-forward terms."""
    game = G.GAMES[name]()
    mutate(game)
    x0 = game.x0(2, G.SEED)
    for type_name, precision in (("float64", "f64"), ("float32", "f32")):
        ref = G.cached_run(name, type_name)
        ref2 = [{q: v[:2] for q, v in it.items()} for it in ref]
        wrong = G.reference_run(game, x0, G.TYPES[type_name])
        ratios = {q: float(G.errors(q, wrong[0], ref2[0], ref2[0]).max()) / G.bar(committed(), name, q, precision) for q in ("P", "alpha")}
        print(name, mutate.__name__, precision, ratios)
        assert max(ratios.values()) > (1e6 if precision == "f64" else 10.0), ratios


# ---- 8. the free-running reference: what the device's line search is held to ----
def test_free_running_reference_matches_the_oracle_where_its_decisions_are_stable(oracle):
    """solve_free against the oracle's free-running ILQSolver::Solve on the point-mass game (a shorter first step than the
    device comparison's, so that the search has decisions to make): wherever no Armijo or convergence test of the
    reference sits within 1e-6 relative of its threshold, the same outcome, iteration count and operating point."""
    game = G.build_point_mass(expression_costs=False)
    G.free_running(game.spec, initial=0.75)
    x0 = game.x0(G.B, G.SEED)
    ref = oracle.OracleProblem(game.spec).solve(abi.F64, x0)
    stable = 0
    for b in range(G.B):
        res = G.solve_free(game, x0[b], np.float64, initial=0.75)
        if res["margin"] <= 1e-6:
            continue
        stable += 1
        assert (res["iters"], int(res["ok"]), int(res["converged"])) == (ref["iters"][b], ref["status"][b], ref["converged"][b])
        assert np.abs(res["xs"] - ref["xs"][b]).max() < 1e-9 * np.abs(ref["xs"][b]).max()
        assert np.abs(res["costs"] - ref["costs"][b]).max() < 1e-9 * np.abs(ref["costs"][b]).max()
    assert stable >= G.B // 2 and ref["iters"].max() > 3


@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_free_running_reference_ends_finite_and_the_gershgorin_games_make_stable_decisions(name):
    """With a first step of 1 a game without corrections lands next to its fixed point at once, and the second iteration's
    Armijo test compares two numbers that agree to ~1e-6 (the RK4 / Euler mismatch): whether that search then fails is
    rounding luck, which is why the device comparison asserts outcomes only above a margin of 1e-6.  The games with
    Gershgorin corrections take damped steps: 10 to 30 iterations, every decision with a margin."""
    game = G.GAMES[name]()
    results = [G.solve_free(game, x0, np.float64) for x0 in game.x0(G.B, G.SEED)]
    assert all(np.all(np.isfinite(r["xs"])) and 1 < r["iters"] < 100 for r in results)
    stable = [r for r in results if r["margin"] > 1e-6]
    print(name, [(r["iters"], r["ok"], r["converged"], "%.0e" % r["margin"]) for r in results])
    if game.gershgorin:
        assert len(stable) >= G.B - 1 and sum(r["converged"] and r["iters"] >= 10 for r in stable) >= G.B // 2
