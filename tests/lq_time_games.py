"""Linear-quadratic games whose costs and rates read the time (ILQG_EXPR_PUSH_TIME), and an iLQ iteration on them in plain
numpy: tests/lq_games.py's games, builder, sweeps, elimination and cost sums by import, and beside them

  * a tracking term 0.5 w (x - v t)^2 on one state of each of two players, written with the time leaf.  Its Hessian w is
    constant; its linear part g_k = -w v t_k and its constant c_k = 0.5 w (v t_k)^2 change with the step and are filled
    into a Tables subclass, per step;
  * a forcing a sin(omega t) on one rate of player 0.  It has no derivative in x or u, so A and B stay lq_games' constant
    matrices; the rollout evaluates it at the RK4's stage times (MultiPlayerDynamicalSystem::Integrate: the two half-steps
    of h = dt / 2 evaluate at t0, t0 + h/2, t0 + h/2, t0 + h, with t0 = k dt and then k dt + h);
  * the forced-step loop of lq_games.solve over that rollout.

t_k = double(k) * dt rounded once to the scalar type, a stage time likewise.  With v = 0 and a = 0 the game is lq_games'
own with a plain 0.5 w x^2 in the tracking terms' place, and solve() here returns lq_games.solve's numbers exactly
(tests/test_lq_time_games.py): what entitles this module to judge the device is that identity plus lq_games' own checks."""
import numpy as np

import lq_games as G
from ilqgames_amd import abi
from ilqgames_amd.abi import Expr

STEPS = G.STEPS
OUTPUTS = G.OUTPUTS
TRACK_W = 0.75                       # the tracking weight, a multiple of 1/8 like every coefficient of lq_games
TRACK_V = (0.5, -0.25)               # the nominal speeds of the two tracking players
FORCING_A, FORCING_OMEGA = 0.375, 2.5
FORCED_ROW = 0                       # of player 0: a row in the middle of a chain, -(d x_0) + g x_1


def tracked_dims(game):
    """The state each of the two tracking players follows: its second one."""
    return [game.xoff[i] + 1 for i in range(2)]


def build(shape, v=TRACK_V, a=FORCING_A, omega=FORCING_OMEGA, open_loop=False, T=12, dt=0.1):
    """lq_games.build(shape, "computed_b") with the two tracking terms and the forcing.  game.tracks: [(player, dim, w, v)],
    game.forcing: (state row, a, omega)."""
    game = G.build(shape, "computed_b", T=T, dt=dt, open_loop=open_loop)
    spec = game.spec
    game.tracks = []
    for i, dim in enumerate(tracked_dims(game)):
        prog = 0.5 * Expr.weight() * (Expr.x() - Expr.value() * Expr.time()).square()
        ti = spec.expression(i, prog, (dim,), weight=TRACK_W, value=v[i])
        # for lq_games.Tables: the constant part of the term, its Hessian; the per-step parts are TimeTables'
        game.terms.append(dict(player=i, on="x", idx=[dim], H=np.array([[TRACK_W]]), g=np.zeros(1), c=0.0, first_step=0,
                               program=prog.program(), weight=TRACK_W, value=v[i], dims=[dim], relative_to=[], term=ti))
        game.tracks.append((i, dim, TRACK_W, v[i]))
    # the forcing: the row's program with a sin(omega t) behind it, a = the row term's weight
    r = FORCED_ROW
    d, g = -game.Jx[r, r], game.Jx[r, r + 1]
    assert d > 0 and g > 0 and game.Ju[r].max() == 0
    ti = next(q for q, t in enumerate(spec.terms) if t["role"] == abi.ROLE_DYNAMICS_ROW and t["player"] == 0 and t["idx"][0] == r)
    assert spec.terms[ti]["idx"][1:3] == (r, r + 1)
    prog = -(Expr.const(d) * Expr.x()) + Expr.const(g) * Expr.y() + Expr.weight() * (Expr.const(omega) * Expr.time()).sin()
    spec.terms[ti].update(polyline=len(spec.dense_params), weight=a)
    spec.dense_params += abi.expr_block(prog.program())
    game.forcing = (r, a, omega)
    return game


def plain_twin(shape, open_loop=False, T=12, dt=0.1):
    """lq_games' own game with 0.5 w x^2 where build() has its tracking terms: what build(v = 0, a = 0) must equal."""
    game = G.build(shape, "computed_b", T=T, dt=dt, open_loop=open_loop)
    for i, dim in enumerate(tracked_dims(game)):
        G._add(game, i, G._single(TRACK_W, 0.0), (dim,))
    return game


def time_of(k, dt, NT):
    return NT(np.float64(k) * np.float64(dt))  # formed in double, rounded once


class TimeTables(G.Tables):
    """lq_games.Tables plus the tracking terms' per-step linear parts and constants."""

    def __init__(self, game, NT):
        super().__init__(game, NT)
        for (i, dim, w, v) in game.tracks:
            for k in range(game.T):
                nominal = NT(v) * time_of(k, game.dt, NT)
                self.gx[k, i][dim] += -(NT(w) * nominal)
                self.cx[k, i] += NT(0.5) * NT(w) * (nominal * nominal)


def rollout(game, tb, x0, xs_ref, us_ref, P, alpha, integrator="rk4"):
    """lq_games.rollout with the forcing in the rates, evaluated at the stage times."""
    NT, T = tb.NT, game.T
    r, a, omega = game.forcing
    xs, us = np.zeros((T, game.n), NT), np.zeros((T, game.m), NT)
    x = np.array(x0, NT)
    h = NT(game.dt / 2.0)
    hd = np.float64(game.dt) / 2.0
    e = np.zeros(game.n, NT)
    e[r] = NT(1)

    def f(x, u, t):
        return tb.Jx @ x + tb.Ju @ u + e * (NT(a) * np.sin(NT(omega) * NT(t)))

    for k in range(T):
        xs[k] = x
        u = us_ref[k] - P[k] @ (x - xs_ref[k]) - alpha[k]
        us[k] = u
        if k + 1 < T:
            tk = np.float64(k) * np.float64(game.dt)
            if integrator == "euler":
                x = x + NT(game.dt) * f(x, u, tk)
                continue
            for s in range(2):
                t0 = tk + s * hd
                k1 = h * f(x, u, t0)
                k2 = h * f(x + NT(0.5) * k1, u, t0 + 0.5 * hd)
                k3 = h * f(x + NT(0.5) * k2, u, t0 + 0.5 * hd)
                k4 = h * f(x + k3, u, t0 + hd)
                x = x + (k1 + NT(2.0) * (k2 + k3) + k4) / NT(6.0)
    return xs, us


def solve(game, x0, steps, NT, integrator="rk4"):
    """lq_games.solve's forced-step loop (ILQSolver::Solve) over TimeTables and the forced rollout: one dict per iteration."""
    tb = TimeTables(game, NT)
    x0 = np.array(x0, NT)
    T, z = game.T, np.zeros
    start = z((T, game.n), NT)
    start[0] = x0
    xs, us = rollout(game, tb, x0, start, z((T, game.m), NT), z((T, game.m, game.n), NT), z((T, game.m), NT), integrator)
    lq = G.lq_inputs(game, tb, xs, us)
    out = []
    for s in steps:
        P, alpha, dxs, corrections = (G.open_loop_sweep if game.open_loop else G.feedback_sweep)(game, lq, x0 - xs[0], NT)
        ed = G.expected_decrease(game, lq, alpha, dxs)
        scaled = alpha * NT(s)
        xs, us = rollout(game, tb, xs[0], xs, us, P, scaled, integrator)
        lq = G.lq_inputs(game, tb, xs, us)
        out.append(dict(xs=xs, us=us, rawP=P, alpha=scaled, raw_alpha=alpha, costs=G.total_costs(game, tb, xs, us),
                        merit=G.merit(game, lq), expected_decrease=ed, corrections=corrections, dxs=dxs))
    return out


# ---- the games of the comparison ----
GAMES = {
    "8_2_1": lambda: build("8_2_1"),
    "14_3_2": lambda: build("14_3_2"),
    "8_2_1_open_loop": lambda: build("8_2_1", open_loop=True),
}
B, SEED = 3, 7
_RUNS = {}


def reference_run(game, x0, NT, steps=STEPS):
    """solve() for every instance of x0 [B][n], in lq_games.reference_run's layout."""
    runs = [solve(game, x0[b], steps, NT) for b in range(x0.shape[0])]
    out = []
    for k in range(len(steps)):
        d = {q: np.stack([np.asarray(r[k][q]) for r in runs]) for q in ("xs", "us", "alpha", "costs", "merit", "expected_decrease")}
        d["P"] = np.stack([G.flat(r[k]["rawP"]) for r in runs])
        d["corrections"] = np.array([r[k]["corrections"] for r in runs])
        out.append(d)
    return out


def cached_run(name, type_name):
    if (name, type_name) not in _RUNS:
        game = GAMES[name]()
        _RUNS[(name, type_name)] = reference_run(game, game.x0(B, SEED), G.TYPES[type_name])
    return _RUNS[(name, type_name)]


def gaps(name):
    """lq_games.gaps for these games: how far the reference is from itself in the next wider scalar type, per output."""
    r32, r64, rld = (cached_run(name, t) for t in ("float32", "float64", "longdouble"))
    out = {"gap64": {}, "gap32": {}}
    for q in OUTPUTS:
        out["gap64"][q] = max(float(G.errors(q, r64[k], rld[k], rld[0]).max()) for k in range(len(STEPS)))
        out["gap32"][q] = max(float(G.errors(q, r32[k], r64[k], r64[0]).max()) for k in range(len(STEPS)))
    return out
