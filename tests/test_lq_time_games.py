"""The numpy reference of tests/lq_time_games.py, checked on the CPU: with the nominal speeds and the forcing zero it is
tests/lq_games.py's reference to the last bit; the time-dependent parts are in the matrices and in the rollout where they
belong; the committed gaps (tests/golden/lq_time_games.json) are this machine's."""
import json
import os

import numpy as np
import pytest

import lq_games as G
import lq_time_games as TG
from helpers import GOLDEN


def _committed():
    return json.load(open(os.path.join(GOLDEN, "lq_time_games.json")))


@pytest.mark.parametrize("type_name", ["float64", "float32"])
@pytest.mark.parametrize("shape,open_loop", [("8_2_1", False), ("14_3_2", False), ("8_2_1", True)])
def test_without_speed_and_forcing_the_reference_is_lq_games_own(shape, open_loop, type_name):
    """v = 0, a = 0: the tracking terms are 0.5 w x^2 and the forcing adds zeros, so every array of every iteration equals
    lq_games.solve's on the game that holds the plain quadratics, bit for bit."""
    NT = G.TYPES[type_name]
    timed = TG.build(shape, v=(0.0, 0.0), a=0.0, open_loop=open_loop)
    plain = TG.plain_twin(shape, open_loop=open_loop)
    for x0 in timed.x0(2, TG.SEED):
        got, want = TG.solve(timed, x0, TG.STEPS, NT), G.solve(plain, x0, G.STEPS, NT)
        for k in range(len(TG.STEPS)):
            for q in ("xs", "us", "rawP", "alpha", "costs", "merit", "expected_decrease"):
                assert np.array_equal(np.asarray(got[k][q]), np.asarray(want[k][q])), (k, q)


def test_the_tracking_terms_fill_the_per_step_tables():
    game = TG.build("8_2_1")
    tb, plain = TG.TimeTables(game, np.float64), G.Tables(game, np.float64)
    assert np.array_equal(tb.Hx, plain.Hx) and np.array_equal(tb.A, plain.A) and np.array_equal(tb.B, plain.B)
    for (i, dim, w, v) in game.tracks:
        for k in range(game.T):
            t = k * game.dt
            assert tb.gx[k, i][dim] - plain.gx[k, i][dim] == pytest.approx(-w * v * t, abs=1e-15)
            # the cost of that step, as a function of the tracked state alone: 0.5 w (x - v t)^2
            x = np.zeros(game.n)
            x[dim] = 1.25
            q = lambda tab: 0.5 * x @ (tab.Hx[k, i] @ x) + tab.gx[k, i] @ x + tab.cx[k, i]  # noqa: E731
            assert q(tb) - q(plain) == pytest.approx(0.5 * w * (1.25 - v * t) ** 2 - 0.5 * w * 1.25 ** 2, abs=1e-14)
    assert len(game.tracks) == 2 and game.tracks[0][0] != game.tracks[1][0]


def test_the_forcing_enters_the_rollout_at_the_stage_times():
    """One step of the forced row alone against scipy-free quadrature: with every other rate zeroed the row integrates
    a sin(omega t) over the step, and the RK4 with the stage times is Simpson's rule on each half-step of h = dt / 2: its
    error is at most h^5 / 2880 times the largest fourth derivative, h^5 a omega^4 / 2880 per half-step, summed over the
    2 (T - 1) half-steps (3.5e-8 here).  Stages all taken at t_k would be the rectangle rule, off by about
    a omega dt / 2 per unit time: 1e-2."""
    game = TG.build("8_2_1")
    r, a, om = game.forcing
    tb = TG.TimeTables(game, np.float64)
    tb.Jx, tb.Ju = np.zeros_like(tb.Jx), np.zeros_like(tb.Ju)
    T, z = game.T, np.zeros
    xs, _ = TG.rollout(game, tb, z(game.n), z((T, game.n)), z((T, game.m)), z((T, game.m, game.n)), z((T, game.m)))
    want = np.array([a * (1.0 - np.cos(om * k * game.dt)) / om for k in range(T)])
    h = game.dt / 2.0
    assert np.max(np.abs(xs[:, r] - want)) <= 2 * (T - 1) * h ** 5 * a * om ** 4 / 2880.0
    assert np.max(np.abs(xs[:, r])) > 0.1 and np.all(np.delete(xs, r, axis=1) == 0.0)


def test_speed_and_forcing_move_every_output():
    """The comparison is not vacuous: against the game without them every output of the first iteration moves by far more
    than any bar."""
    game, still = TG.build("8_2_1"), TG.build("8_2_1", v=(0.0, 0.0), a=0.0)
    x0 = game.x0(1, TG.SEED)[0]
    a, b = TG.solve(game, x0, TG.STEPS, np.float64)[0], TG.solve(still, x0, TG.STEPS, np.float64)[0]
    for q in ("xs", "us", "alpha", "costs", "merit"):
        assert np.max(np.abs(np.asarray(a[q]) - np.asarray(b[q]))) > 1e-3 * np.max(np.abs(np.asarray(b[q]))), q


@pytest.mark.parametrize("name", sorted(TG.GAMES))
def test_committed_gaps_are_the_reference_s_own(name):
    """tests/golden/lq_time_games.json within a factor of 2 of what this machine computes (both floored at one ulp of the
    type), and the bars made of it inside the project's existing ones."""
    want, got = _committed()[name], TG.gaps(name)
    for key, precision in (("gap64", "f64"), ("gap32", "f32")):
        for q in TG.OUTPUTS:
            a, b = max(want[key][q], G.EPS[precision]), max(got[key][q], G.EPS[precision])
            assert 0.5 <= a / b <= 2.0, (name, key, q, want[key][q], got[key][q])
            assert G.bar(_committed(), name, q, precision) <= G.PROJECT_BAR[precision][q]
    assert set(_committed()) == set(TG.GAMES)
