"""The device against an independent numpy solve on exactly linear-quadratic games made of the expression kinds
(tests/lq_games.py; the reference's own checks are tests/test_lq_games.py).

T = 12, B = 8, K = 4 forced iterations with steps (0.5, 0.25, 1, 0.5) for every instance, both precisions.  After every
iteration every instance is compared on xs, us, P, alpha, costs, last_merit and expected_decrease — no skip mask: the
conditioning test of tests/test_lq_games.py holds for every (instance, iteration) pair.  Per output the bar is 100 x the
committed gap of that game (tests/golden/lq_games.json: gap64 for fp64, gap32 for fp32), floored at 100 ulp, and never
looser than the project's existing bars.  Each schedule pin is confirmed through last_schedule().

What the shapes can reach (csrc/ilqg_api.hip's schedule): the single-wave sweep and the constant-B form exist for two
controls per player and fewer than 16 states, so of these games the point masses with expression costs, (8, 2, 2), take
them; on (8, 2, 1) those pins are honoured as "not available" (the bits stay clear) and the solve is compared all the same.
A forced step always takes the fused trial kernel, so split_trial shows in the free-running solves only.

Reference-free checks on the same solves: the gains of iterations 1 to 4 agree to the bar on every game.  alpha_{k+1} =
(1 - s_k) alpha_k and a trajectory at rest after the full step hold where the RK4 rollout is the map the Euler
linearisation describes — the `integrator` game (J_x = 0); on the damped chains the two differ by O((dt J)^2) and the
device's alpha follows the reference's 1, 0.493 .. 0.501, 0.368 .. 0.376, 0.0006 .. 0.0053 (compared above, to the bar).
"""
import json
import os

import numpy as np
import pytest

import lq_games as G
from ilqgames_amd import abi
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

K = len(G.STEPS)
S = abi
PINNED = S.SCHEDULE_SINGLE_WAVE_SWEEP | S.SCHEDULE_CONSTANT_B | S.SCHEDULE_PADDED_SWEEP | S.SCHEDULE_GENERIC | S.SCHEDULE_OPEN_LOOP

# the pins of each game: (solve options, the PINNED bits last_schedule() must then show, further bits (set, clear))
_PLAIN_8_2_1 = [
    (dict(), 0, (0, 0)),
    (dict(single_wave_sweep=True, adjoint_expected_decrease=True), 0, (0, S.SCHEDULE_ADJOINT_DECREASE)),  # no such sweep: MU = 1
    (dict(single_wave_sweep=True, adjoint_expected_decrease=False), 0, (0, S.SCHEDULE_ADJOINT_DECREASE)),
    (dict(sweep_forms=True), 0, (0, 0)),
    (dict(sweep_forms=False), 0, (0, 0)),
    (dict(split_trial=True), 0, (0, S.SCHEDULE_SPLIT_TRIAL)),   # (a forced step takes the fused kernel)
    (dict(split_trial=False), 0, (0, S.SCHEDULE_SPLIT_TRIAL)),
    (dict(compact_rows=True), 0, (S.SCHEDULE_COMPACT_ROWS, 0)),
    (dict(compact_rows=False), 0, (0, S.SCHEDULE_COMPACT_ROWS)),
    (dict(generic_kernels=True), S.SCHEDULE_GENERIC, (0, 0)),
]
_RUN_TIME_DIMS = [
    (dict(), S.SCHEDULE_GENERIC | S.SCHEDULE_PADDED_SWEEP, (0, 0)),
    (dict(padded_sweep=True), S.SCHEDULE_GENERIC | S.SCHEDULE_PADDED_SWEEP, (0, 0)),
    (dict(padded_sweep=False), S.SCHEDULE_GENERIC, (0, 0)),
]
_OL = S.SCHEDULE_OPEN_LOOP
PINS = {
    "8_2_1_constant_b": _PLAIN_8_2_1,
    "8_2_1_computed_b": _PLAIN_8_2_1,
    "8_2_1_gershgorin": _PLAIN_8_2_1,
    "17_3_2": [(dict(), 0, (0, 0)), (dict(generic_kernels=True), S.SCHEDULE_GENERIC, (0, 0))],
    "17_3_2_gershgorin": [(dict(), 0, (0, 0)), (dict(generic_kernels=True), S.SCHEDULE_GENERIC, (0, 0))],
    "14_3_2": _RUN_TIME_DIMS,
    "14_3_2_gershgorin": _RUN_TIME_DIMS,
    "9_mixed": _RUN_TIME_DIMS,
    "9_mixed_gershgorin": _RUN_TIME_DIMS,
    "point_mass_expression": [
        (dict(), S.SCHEDULE_CONSTANT_B, (S.SCHEDULE_COMPACT_ROWS, 0)),
        (dict(single_wave_sweep=True, adjoint_expected_decrease=True), S.SCHEDULE_SINGLE_WAVE_SWEEP, (S.SCHEDULE_ADJOINT_DECREASE, 0)),
        (dict(single_wave_sweep=True, adjoint_expected_decrease=False), S.SCHEDULE_SINGLE_WAVE_SWEEP, (0, S.SCHEDULE_ADJOINT_DECREASE)),
        (dict(single_wave_sweep=False), S.SCHEDULE_CONSTANT_B, (0, 0)),
        (dict(sweep_forms=False), 0, (S.SCHEDULE_COMPACT_ROWS, 0)),
        (dict(compact_rows=False), 0, (0, S.SCHEDULE_COMPACT_ROWS)),
        (dict(generic_kernels=True), S.SCHEDULE_GENERIC, (0, 0)),
    ],
    # (an expression subsystem runs the plain RK4, which (24, 4, 2) does not carry: the run-time-dimensioned path, its
    # sweep padded onto the two-tile open-loop kernel or all in LDS)
    "24_4_2_open_loop": [(dict(), S.SCHEDULE_GENERIC | S.SCHEDULE_PADDED_SWEEP | _OL, (0, 0)),
                         (dict(generic_kernels=True, padded_sweep=False), S.SCHEDULE_GENERIC | _OL, (0, 0))],
    "8_2_1_open_loop": [(dict(), _OL, (0, 0)), (dict(compact_rows=False), _OL, (0, S.SCHEDULE_COMPACT_ROWS)),
                        (dict(generic_kernels=True), S.SCHEDULE_GENERIC | _OL, (0, 0))],
    "integrator": [(dict(), S.SCHEDULE_GENERIC | S.SCHEDULE_PADDED_SWEEP, (0, 0)), (dict(padded_sweep=False), S.SCHEDULE_GENERIC, (0, 0))],
}
assert set(PINS) == set(G.GAMES)


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


@pytest.fixture(scope="module")
def committed():
    return json.load(open(os.path.join(GOLDEN, "lq_games.json")))


def _np(t):
    return t.detach().cpu().numpy()


def _device_iterations(prob, x0, **pin):
    """-> one dict of OUTPUTS per iteration k = 1 .. K (the solve with fixed_iters = k), and the schedule of the last."""
    steps = np.tile(np.array(G.STEPS), (x0.shape[0], 1))
    out = []
    for k in range(1, K + 1):
        bufs = prob.solve(x0, fixed_iters=k, forced_steps=steps[:, :k], **pin)
        st = prob.solve_state(bufs)
        assert np.all(_np(bufs["iters"]) == k) and np.all(_np(bufs["status"]) == 1)
        d = {q: _np(bufs[q]).astype(np.float64) for q in ("xs", "us", "P", "alpha", "costs")}
        d["merit"], d["expected_decrease"] = _np(st["last_merit"]).astype(np.float64), _np(st["expected_decrease"]).astype(np.float64)
        assert np.allclose(_np(st["step"]), G.STEPS[k - 1])
        out.append(d)
    return out, prob.last_schedule()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_every_instance_matches_the_reference_after_every_iteration_on_every_pinned_schedule(hip, committed, name, precision):
    game = G.GAMES[name]()
    dtype = abi.F64 if precision == "f64" else abi.F32
    ref = G.cached_run(name, "float64" if precision == "f64" else "float32")
    x0 = game.x0(G.B, G.SEED)
    prob = hip.Problem(game.spec, dtype)
    bars = {q: G.bar(committed, name, q, precision) for q in G.OUTPUTS}
    gap = committed[name]["gap64" if precision == "f64" else "gap32"]
    worst, failures, pairs = {}, [], 0
    for pin, want, (also_set, also_clear) in PINS[name]:
        dev, sched = _device_iterations(prob, x0, **pin)
        print("%s %s pin %s: schedule 0x%x" % (name, precision, pin, sched))
        if sched & PINNED != want or sched & also_set != also_set or sched & also_clear:
            failures.append((pin, "schedule 0x%x" % sched, "wanted 0x%x of the pinned bits, set 0x%x, clear 0x%x" % (want, also_set, also_clear)))
        for k in range(K):
            for q in G.OUTPUTS:
                err = G.errors(q, dev[k], ref[k], ref[0])
                assert err.shape == (G.B,)  # all B instances, nothing masked
                ratio = float(err.max()) / max(gap[q], G.EPS[precision])
                worst[q] = max(worst.get(q, 0.0), ratio)
                if not err.max() <= bars[q]:
                    failures.append((pin, k + 1, q, float(err.max()), bars[q]))
            pairs += G.B
        # reference-free: A, B, Q, R do not depend on the operating point, so the gains of iterations 1 .. 4 agree
        for k in range(1, K):
            scale = max(np.abs(dev[0]["P"]).max(), 1e-30)
            assert np.abs(dev[k]["P"] - dev[0]["P"]).max() <= bars["P"] * scale, (pin, k)
        if game.shape == "integrator":  # ... and where the rollout is the linearisation's map, the LQ solve is exact
            a = [np.abs(d["alpha"]).reshape(G.B, -1).max(axis=1) / s for d, s in zip(dev, G.STEPS)]  # the raw alpha
            assert np.abs(a[1] / a[0] - 0.5).max() <= bars["alpha"] and np.abs(a[2] / a[0] - 0.375).max() <= bars["alpha"]
            assert (a[3] / a[0]).max() <= bars["alpha"]
            scale = np.abs(dev[2]["xs"]).reshape(G.B, -1).max(axis=1)
            assert (np.abs(dev[3]["xs"] - dev[2]["xs"]).reshape(G.B, -1).max(axis=1) / scale).max() <= bars["xs"]
    assert pairs == len(PINS[name]) * G.B * K
    print("%s %s: largest device-to-reference distance in units of the committed gap: %s" % (
        name, precision, " ".join("%s %.1f" % (q, worst[q]) for q in G.OUTPUTS)))
    assert not failures, failures


@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_free_running_solve_makes_the_reference_s_decisions(hip, committed, name):
    """initial_alpha_scaling = 1, geometric_alpha_scaling = 0.5, expected_decrease_fraction = 0.001, deterministic, fp64,
    once fused and once with split passes.  Wherever no Armijo or convergence test of the reference sits within 1e-6
    relative of its threshold (checked here, on the CPU), the device ends with the reference's outcome — converged, or a
    line search that gave up — after the same number of iterations at the same operating point; elsewhere (a first step of
    1 lands next to the fixed point, and the next Armijo test then compares two numbers that agree to ~1e-6) it ends
    finite next to it.  The games with Gershgorin corrections take 10 to 30 damped iterations, each decision with a margin."""
    game = G.GAMES[name]()
    G.free_running(game.spec)
    x0 = game.x0(G.B, G.SEED)
    ref = [G.solve_free(game, x0[b], np.float64) for b in range(G.B)]
    stable = [b for b in range(G.B) if ref[b]["margin"] > 1e-6]
    prob = hip.Problem(game.spec, abi.F64)
    failures, worst = [], {}
    for pin in (dict(split_trial=False), dict(split_trial=True)):
        out = prob.solve(x0, deterministic=True, **pin)
        sched = prob.last_schedule()
        if not sched & S.SCHEDULE_GENERIC:
            assert bool(sched & S.SCHEDULE_SPLIT_TRIAL) == pin["split_trial"]
        assert bool(sched & S.SCHEDULE_OPEN_LOOP) == game.open_loop
        xs, us, costs = _np(out["xs"]), _np(out["us"]), _np(out["costs"])
        assert np.all(np.isfinite(xs)) and np.all(np.isfinite(us))
        print(name, pin, "device iters", _np(out["iters"]), "reference", [r["iters"] for r in ref], "stable", stable)
        for b in range(G.B):
            r = ref[b]
            if b in stable:
                got = (int(_np(out["iters"])[b]), int(_np(out["status"])[b]), int(_np(out["converged"])[b]))
                if got != (r["iters"], int(r["ok"]), int(r["converged"])):
                    failures.append((pin, b, "outcome", got, (r["iters"], int(r["ok"]), int(r["converged"]))))
                    continue
                for q, a, w in (("xs", xs[b], r["xs"]), ("us", us[b], r["us"]), ("costs", costs[b], r["costs"])):
                    err = np.abs(a - w).max() / max(np.abs(w).max(), 1e-30)
                    worst[q] = max(worst.get(q, 0.0), err / G.bar(committed, name, q, "f64"))
                    if not err <= G.bar(committed, name, q, "f64"):  # the forced iterations' bar: the iteration contracts
                        failures.append((pin, b, q, err))
            else:  # next to the fixed point either way: one more accepted step moves it by the mismatch, O((dt J)^2)
                assert np.abs(xs[b] - r["xs"]).max() <= 0.05 * np.abs(r["xs"]).max(), (pin, b)
    print(name, "free-running: largest distance from the reference in units of the forced-step bar:", worst)
    assert not failures, failures
    if game.gershgorin:
        assert len(stable) >= G.B - 1


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(G.GAMES))
def test_stage_entry_points_return_the_hand_written_matrices(hip, name, precision):
    """ilqg_linearize_batch against I + dt J and ilqg_quadraticize_batch against the hand-written Hessians and gradients
    at a random operating point: the column-major / pair layout of dense R_ij, Q entries that couple two players, computed
    B entries.  The matrices' entries are dyadic: exact; the gradients to 100 ulp of their largest entry."""
    game = G.GAMES[name]()
    dtype, NT = (abi.F64, np.float64) if precision == "f64" else (abi.F32, np.float32)
    tb = G.Tables(game, NT)
    rng = np.random.default_rng(19)
    xs = rng.uniform(-2, 2, (2, game.T, game.n)).astype(NT)
    us = rng.uniform(-1, 1, (2, game.T, game.m)).astype(NT)
    prob = hip.Problem(game.spec, dtype)
    assert prob.pairs == game.pairs
    A, Bm = [_np(a) for a in prob.linearize(xs, us)]
    Q, l, R, r = [_np(a) for a in prob.quadraticize(xs, us)]
    cm = lambda M: np.swapaxes(M, -1, -2).reshape(M.shape[:-2] + (-1,))  # noqa: E731  column-major words
    assert np.array_equal(A, np.broadcast_to(cm(tb.A), A.shape)) and np.array_equal(Bm, np.broadcast_to(cm(tb.B), Bm.shape))
    assert np.array_equal(Q, np.broadcast_to(cm(tb.Hx), Q.shape))
    tol = 100 * G.EPS[precision]
    for b in range(2):
        lq = G.lq_inputs(game, tb, xs[b], us[b])
        assert np.abs(l[b] - lq["l"]).max() <= tol * np.abs(lq["l"]).max()
        Ro = ro = 0
        for (i, j) in game.pairs:
            mj = game.ms[j]
            assert np.array_equal(R[b][:, Ro:Ro + mj * mj], cm(tb.Hu[(i, j)])), (i, j)
            assert np.abs(r[b][:, ro:ro + mj] - lq["r"][(i, j)]).max() <= tol * max(1.0, np.abs(lq["r"][(i, j)]).max()), (i, j)
            Ro, ro = Ro + mj * mj, ro + mj
        assert Ro == R.shape[-1] and ro == r.shape[-1]
    costs = _np(prob.total_costs(xs, us)[0])
    want = np.stack([G.total_costs(game, tb, xs[b], us[b]) for b in range(2)])
    assert np.abs(costs - want).max() <= 10 * tol * np.abs(want).max()
