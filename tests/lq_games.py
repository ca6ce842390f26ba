"""Exactly linear-quadratic games out of the expression kinds, and an iLQ iteration on them in plain numpy.

Every player of a game from build() is an expression subsystem (abi.DYN_EXPRESSION) whose rates are linear programs, every
cost an abi.COST_EXPRESSION program that is an exact quadratic with a positive semi-definite Hessian, so the builder that
writes a program also writes down, by hand, the entries it stands for: J_x, J_u of the rates, and per term a small Hessian
H, a linear part g and a constant c over the entries of the state (or of one player's control) it reads,
    term(v) = 0.5 v^T H v + g^T v + c.
Every coefficient is a multiple of 1/8, so its float32 slot in the ABI holds it exactly.  No GPU, no oracle, no shared
evaluator: solve() restates the loop of ILQSolver::Solve with forced steps (the semantics oracle/ilqg_oracle.hpp SolveILQ
documents) on those matrices in the scalar type NT (float32, float64 or longdouble), with a hand-written elimination,
because numpy.linalg refuses longdouble.  build_point_mass() is the one game the oracle knows too: what entitles this
reference to judge the device is its agreement with the oracle there (tests/test_lq_games.py).

The rollout is the ABI's RK4 with two half-steps, the linearisation its Euler form A = I + dt J_x, B = dt J_u.  The two
differ by O((dt J)^2), so the LQ model of an iteration is not the derivative of the rollout: with integrator="euler"
solve() rolls out with the model the linearisation is exact for, and only then (or where J_x = 0, the `integrator` shape)
is each LQ solve in deviation coordinates exact and alpha_{k+1} = (1 - s_k) alpha_k an identity.
"""
import numpy as np

from ilqgames_amd import abi
from ilqgames_amd.abi import Expr

STEPS = (0.5, 0.25, 1.0, 0.5)  # the forced steps of every comparison: two short ones, the full step, one more
MIN_EVAL = np.float32(1e-3)     # LQFeedbackSolver's Gershgorin floor, a float literal there

# (xdim, udim) per player
SHAPES = {
    "8_2_1": [(4, 1), (4, 1)],                 # the specialised plain-RK4 kernels, m = 2
    "17_3_2": [(6, 2), (6, 2), (5, 2)],        # the 16 < n <= 31 sweep inside a solve
    "14_3_2": [(5, 2), (5, 2), (4, 2)],        # run-time-dimensioned, padded onto the headline sweep
    "9_mixed": [(4, 1), (5, 2)],               # mixed control dimensions, padded onto (10, 2, 2)
    "24_4_2": [(6, 2), (6, 2), (6, 2), (6, 2)],  # two tiles (the open-loop sweep)
    "integrator": [(2, 2), (2, 2)],            # J_x = 0: the RK4 and the Euler step are the same map
}


class Game:
    """spec (abi.ProblemSpec), dims, Jx (n, n), Ju (n, m), terms [dict(player, on = 'x' | control player j, idx, H, g, c,
    first_step, program, weight, value, dims, relative_to)], pairs (first-touch order), open_loop."""

    def x0(self, B=8, seed=7):
        return np.random.default_rng(seed).uniform(-2.0, 2.0, (B, self.n))


# ---- the hand-written quadratics: (program, weight, value, H, g, c) over the listed inputs ----
def _single(w, v):
    """0.5 w (x - v)^2"""
    prog = 0.5 * Expr.weight() * (Expr.x() - Expr.value()).square()
    return prog, w, v, [[w]], [-w * v], 0.5 * w * v * v


def _pair(a, b, c):
    """a x^2 + b x y + c y^2, positive semi-definite for 4 a c >= b^2"""
    assert a >= 0 and c >= 0 and 4 * a * c >= b * b
    x, y = Expr.x(), Expr.y()
    prog = Expr.const(a) * x.square() + Expr.const(b) * (x * y) + Expr.const(c) * y.square()
    return prog, 1.0, 0.0, [[2 * a, b], [b, 2 * c]], [0.0, 0.0], 0.0


def _relative(term, count):
    """The same program over differences: inputs (x, x') -> x - x' and (x, y, x', y') -> (x - x', y - y')."""
    prog, w, v, H, g, c = term
    if count == 1:  # over [x, x']: fxx (1, -1; -1, 1), fx (1, -1)
        h, g0 = H[0][0], g[0]
        return prog, w, v, [[h, -h], [-h, h]], [g0, -g0], c
    (hxx, hxy), (_, hyy) = H  # over [x, y, x', y']
    H4 = [[hxx, hxy, -hxx, -hxy], [hxy, hyy, -hxy, -hyy], [-hxx, -hxy, hxx, hxy], [-hxy, -hyy, hxy, hyy]]
    return prog, w, v, H4, [g[0], g[1], -g[0], -g[1]], c


def _add(game, player, term, dims, relative_to=None, control_of=None, final_time=None, builtin=None):
    prog, w, v, H, g, c = term
    spec = game.spec
    if builtin is not None:
        ti = builtin(spec)
    else:
        ti = spec.expression(player, prog, dims, weight=w, value=v, control_of=control_of, relative_to=relative_to)
    if final_time is not None:
        spec.final_time(final_time, ti)
    idx = list(dims) + list(relative_to or ())
    H, g = np.array(H, np.float64), np.array(g, np.float64)
    assert H.shape == (len(idx), len(idx)) and np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() > -1e-12
    for q in list(H.ravel()) + [w, v]:
        assert q * 8 == round(q * 8), q  # what the ABI's float32 slots hold: multiples of 1/8
    game.terms.append(dict(player=player, on="x" if control_of is None else control_of, idx=idx, H=H, g=g, c=float(c),
                           first_step=spec.terms[ti]["first_step"], program=None if builtin else prog.program(),
                           weight=w, value=v, dims=list(dims), relative_to=list(relative_to or ()), term=ti))
    return ti


def _finish(game, open_loop):
    spec = game.spec
    spec.params.open_loop = 1 if open_loop else 0
    game.open_loop = bool(open_loop)
    game.n, game.m, game.N, game.T, game.dt = spec.n, spec.m, len(spec.subsystems), spec.T, spec.dt
    game.ms = list(spec.udims)
    game.xoff = [spec.xoff(i) for i in range(game.N + 1)]
    game.uoff = [sum(game.ms[:i]) for i in range(game.N + 1)]
    game.pairs = spec.pairs()
    assert all((i, i) in game.pairs for i in range(game.N))
    spec.x0 = [0.0] * game.n
    return game


def build(shape, variant="computed_b", T=12, dt=0.1, gershgorin=False, open_loop=False):
    """The game of `shape` (a key of SHAPES).  variant: how a control enters its row — "constant_b": the row's whole
    program is one PUSH_X of the control (the ABI's constant entry dt), "computed_b": -(d x) + g u.  gershgorin: the
    players' own control Hessians lose their diagonal dominance (off-diagonal entries as large as the diagonal, small
    weights) and the players couple strongly, so that the sweep's Gershgorin step fires."""
    assert variant in ("constant_b", "computed_b")
    game = Game()
    game.shape, game.variant, game.gershgorin = shape, variant, gershgorin
    game.terms = []
    spec = game.spec = abi.ProblemSpec(T, dt)
    players = SHAPES[shape]
    n, m = sum(p[0] for p in players), sum(p[1] for p in players)
    Jx, Ju = np.zeros((n, n)), np.zeros((n, m))
    xo = uo = 0
    for i, (xdim, udim) in enumerate(players):
        # damped chains, one per control: xdot_r = -d x_r + g x_{r+1}, the last row of a chain takes the control
        ends = [xdim - 1] if udim == 1 else [(xdim + 1) // 2 - 1, xdim - 1]
        rows = []
        for r in range(xdim):
            d, g = (1 + (3 * r + i) % 4) / 8.0, (4 + 2 * ((r + 2 * i) % 4)) / 8.0
            if shape == "integrator":
                assert variant == "constant_b"
            if r in ends:
                c = ends.index(r)
                if variant == "constant_b":
                    rows.append((Expr.x(), xdim + c, None))
                    Ju[xo + r, uo + c] = 1.0
                else:
                    rows.append((-(Expr.const(d) * Expr.x()) + Expr.const(g) * Expr.y(), r, xdim + c))
                    Jx[xo + r, xo + r], Ju[xo + r, uo + c] = -d, g
            else:
                rows.append((-(Expr.const(d) * Expr.x()) + Expr.const(g) * Expr.y(), r, r + 1))
                Jx[xo + r, xo + r], Jx[xo + r, xo + r + 1] = -d, g
        spec.add_expression_player(xdim, udim, rows)
        xo, uo = xo + xdim, uo + udim
    game.Jx, game.Ju = Jx, Ju
    N = len(players)
    xoff = [sum(p[0] for p in players[:i]) for i in range(N + 1)]
    for i, (xdim, udim) in enumerate(players):
        # (one-dimensional controls have no off-diagonal R_ii: there a column of S loses its dominance to the OTHER
        # player's row, whose value function couples the two controlled states much more strongly than the player's own)
        couple = ((16.0 if i % 2 else 1.0) if gershgorin else 0.25)
        j = (i + 1) % N
        o, oj, xj = xoff[i], xoff[j], players[j][0]
        ctrl = [o + e for e in ([xdim - 1] if udim == 1 else [(xdim + 1) // 2 - 1, xdim - 1])]  # the controlled rows
        ctrl_j = oj + players[j][0] - 1
        for r in range(xdim):  # single entries: every own state is drawn to a value
            _add(game, i, _single((4 + 2 * ((r + i) % 3)) / 8.0, ((r + 2 * i) % 5 - 2) / 4.0), (o + r,))
        _add(game, i, _pair(0.5, 0.5, 0.375), (o, o + 1))                        # two states of one player
        _add(game, i, _pair(couple, -2 * couple, couple), (ctrl[-1], ctrl_j))    # states of two players (plain PAIR2)
        if xdim >= 4 and xj >= 4:
            _add(game, i, _relative(_single(0.75, 0.5), 1), (o + 2,), relative_to=(oj + 1,), final_time=0.55)
            _add(game, i, _relative(_pair(0.375, -0.25, 0.25), 2), (o, o + 3), relative_to=(oj + 2, oj + 3))
        else:
            _add(game, i, _relative(_single(0.75, 0.5), 1), (o,), relative_to=(oj + 1,), final_time=0.55)
        # the player's own control: both entries of a two-dimensional one (off-diagonal R_ii)
        if udim == 2:
            _add(game, i, _pair(0.25, 0.375, 0.25) if gershgorin else _pair(1.0, 0.5, 0.75), (0, 1), control_of=i)
        else:
            _add(game, i, _single(0.125 if gershgorin else 1.0, 0.0), (0,), control_of=i)
        # another player's control (R_ij, off-diagonal where it has two entries)
        if players[j][1] == 2:
            _add(game, i, _pair(0.25, 0.25, 0.125), (0, 1), control_of=j)
        else:
            _add(game, i, _single(0.25, 0.25), (0,), control_of=j)
    return _finish(game, open_loop)


def build_point_mass(expression_costs=False, T=12, dt=0.1, open_loop=False):
    """Two DYN_POINT_MASS_2D players, (8, 2, 2): the linear model the oracle knows.  With built-in quadratic /
    quadratic_difference costs only (the oracle cross-check), or with the expression costs of build() added (the device's
    non-plain-RK4 specialised kernels and its constant-B forms)."""
    game = Game()
    game.shape, game.variant, game.gershgorin = "point_mass", "constant_b", False
    game.terms = []
    spec = game.spec = abi.ProblemSpec(T, dt)
    Jx, Ju = np.zeros((8, 8)), np.zeros((8, 4))
    for i in range(2):
        spec.add_player(abi.DYN_POINT_MASS_2D)
        o = 4 * i
        Jx[o, o + 2] = Jx[o + 1, o + 3] = 1.0
        Ju[o + 2, 2 * i] = Ju[o + 3, 2 * i + 1] = 1.0
    game.Jx, game.Ju = Jx, Ju
    for i in range(2):
        j, o, oj = 1 - i, 4 * i, 4 * (1 - i)
        for r in range(4):
            w, v = (4 + 2 * ((r + i) % 3)) / 8.0, ((r + 2 * i) % 5 - 2) / 4.0
            _add(game, i, _single(w, v), (o + r,), builtin=lambda s, w=w, v=v, r=r: s.quadratic(i, w, o + r, v))
        # 0.5 w ((x0 - x0')^2 + (x1 - x1')^2)
        wd = 0.75
        H = np.kron(np.array([[1, -1], [-1, 1]]), np.eye(2)) * wd
        _add(game, i, (None, wd, 0.0, H.tolist(), [0.0] * 4, 0.0), (o, o + 1), relative_to=(oj, oj + 1),
             builtin=lambda s: s.quadratic_difference(i, wd, (o, o + 1), (oj, oj + 1)))
        _add(game, i, (None, 0.5, 0.0, (H * (0.5 / wd)).tolist(), [0.0] * 4, 0.0), (o + 2, o + 3), relative_to=(oj + 2, oj + 3),
             builtin=lambda s: s.final_time(0.55, s.quadratic_difference(i, 0.5, (o + 2, o + 3), (oj + 2, oj + 3))))
        for c in range(2):
            w = 1.0 + 0.5 * c
            _add(game, i, _single(w, 0.0), (c,), control_of=i, builtin=lambda s, w=w, c=c: s.quadratic(i, w, c, 0.0, control_of=i))
        _add(game, i, _single(0.25, 0.25), (1,), control_of=j, builtin=lambda s: s.quadratic(i, 0.25, 1, 0.25, control_of=j))
        if expression_costs:
            _add(game, i, _pair(0.5, 0.5, 0.375), (o, o + 2))
            _add(game, i, _pair(0.25, -0.5, 0.25), (o + 3, oj + 3))
            _add(game, i, _relative(_single(0.75, 0.5), 1), (o + 1,), relative_to=(oj + 1,), final_time=0.35)
            _add(game, i, _relative(_pair(0.375, -0.25, 0.25), 2), (o, o + 3), relative_to=(oj + 2, oj + 1))
            _add(game, i, _pair(1.0, 0.5, 0.75), (0, 1), control_of=i)
            _add(game, i, _pair(0.25, 0.25, 0.125), (0, 1), control_of=j)
    return _finish(game, open_loop)


# ------------------------------------------------------------------------------------------------
# the numpy reference
# ------------------------------------------------------------------------------------------------
def eliminate(A, B, NT):
    """A^-1 B by Gaussian elimination with partial pivoting, every operation in NT."""
    A, B = np.array(A, NT), np.array(B, NT)
    k = A.shape[0]
    for c in range(k):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]], B[[c, p]] = A[[p, c]], B[[p, c]]
        for r in range(c + 1, k):
            f = A[r, c] / A[c, c]
            if f != 0:
                A[r, c:] = A[r, c:] - f * A[c, c:]
                B[r] = B[r] - f * B[c]
    X = np.zeros_like(B)
    for r in range(k - 1, -1, -1):
        X[r] = (B[r] - A[r, r + 1:] @ X[r + 1:]) / A[r, r]
    return X


class Tables:
    """The game's matrices in NT: A, B (constant), per step and player the summed Hessians / linear parts / constants of
    the active terms, over the state (Hx, gx, cx) and per pair over the control (Hu, gu, cu)."""

    def __init__(self, game, NT):
        T, N, n = game.T, game.N, game.n
        self.NT = NT
        # A = I + dt J_x, B = dt J_u as the ABI forms them: each entry T(double(d) * dt), a diagonal entry T(1) + that
        self.A = np.eye(n, dtype=NT) + (game.Jx * np.float64(game.dt)).astype(NT)
        self.B = (game.Ju * np.float64(game.dt)).astype(NT)
        self.Jx, self.Ju = game.Jx.astype(NT), game.Ju.astype(NT)
        self.Hx, self.gx, self.cx = np.zeros((T, N, n, n), NT), np.zeros((T, N, n), NT), np.zeros((T, N), NT)
        self.Hu = {p: np.zeros((T, game.ms[p[1]], game.ms[p[1]]), NT) for p in game.pairs}
        self.gu = {p: np.zeros((T, game.ms[p[1]]), NT) for p in game.pairs}
        self.cu = {p: np.zeros(T, NT) for p in game.pairs}
        for t in game.terms:
            i, idx = t["player"], np.array(t["idx"])
            for k in range(t["first_step"], T):
                if t["on"] == "x":
                    self.Hx[k, i][np.ix_(idx, idx)] += t["H"].astype(NT)
                    self.gx[k, i][idx] += t["g"].astype(NT)
                    self.cx[k, i] += NT(t["c"])
                else:
                    p = (i, t["on"])
                    self.Hu[p][k][np.ix_(idx, idx)] += t["H"].astype(NT)
                    self.gu[p][k][idx] += t["g"].astype(NT)
                    self.cu[p][k] += NT(t["c"])


def rollout(game, tb, x0, xs_ref, us_ref, P, alpha, integrator="rk4"):
    """u_k = u_ref_k - P_k (x_k - x_ref_k) - alpha_k; the ABI's RK4 with two half-steps of dt / 2 (or one Euler step)."""
    NT, T = tb.NT, game.T
    xs, us = np.zeros((T, game.n), NT), np.zeros((T, game.m), NT)
    x = np.array(x0, NT)
    h = NT(game.dt / 2.0)
    f = lambda x, u: tb.Jx @ x + tb.Ju @ u  # noqa: E731
    for k in range(T):
        xs[k] = x
        u = us_ref[k] - P[k] @ (x - xs_ref[k]) - alpha[k]
        us[k] = u
        if k + 1 < T:
            if integrator == "euler":
                x = x + NT(game.dt) * f(x, u)
                continue
            for _ in range(2):
                k1 = h * f(x, u)
                k2 = h * f(x + NT(0.5) * k1, u)
                k3 = h * f(x + NT(0.5) * k2, u)
                k4 = h * f(x + k3, u)
                x = x + (k1 + NT(2.0) * (k2 + k3) + k4) / NT(6.0)
    return xs, us


def lq_inputs(game, tb, xs, us):
    """The linearisation (constant) and the quadraticisation at an operating point: gradients of the hand-written
    quadratics, l = H x + g, r = H u_j + g."""
    T, N = game.T, game.N
    l = np.einsum("kiab,kb->kia", tb.Hx, xs) + tb.gx
    r = {}
    for (i, j) in game.pairs:
        uj = us[:, game.uoff[j]:game.uoff[j + 1]]
        r[(i, j)] = np.einsum("kab,kb->ka", tb.Hu[(i, j)], uj) + tb.gu[(i, j)]
    return dict(A=np.broadcast_to(tb.A, (T,) + tb.A.shape), B=np.broadcast_to(tb.B, (T,) + tb.B.shape), Q=tb.Hx, l=l,
                R=tb.Hu, r=r)


def total_costs(game, tb, xs, us):
    NT = tb.NT
    out = np.zeros(game.N, NT)
    for k in range(game.T):
        for i in range(game.N):
            c = NT(0.5) * (xs[k] @ (tb.Hx[k, i] @ xs[k])) + tb.gx[k, i] @ xs[k] + tb.cx[k, i]
            for (a, j) in game.pairs:
                if a == i:
                    uj = us[k, game.uoff[j]:game.uoff[j + 1]]
                    c = c + NT(0.5) * (uj @ (tb.Hu[(a, j)][k] @ uj)) + tb.gu[(a, j)][k] @ uj + tb.cu[(a, j)][k]
            out[i] += c
    return out


def merit(game, lq):
    """MeritFunction: 0.5 (sum |r_ii|^2 + sum over k > 0 of |l_i|^2)."""
    s = sum((lq["r"][(i, i)] ** 2).sum() for i in range(game.N)) + (lq["l"][1:] ** 2).sum()
    return type(s)(0.5) * s


def expected_decrease(game, lq, alpha, dxs):
    ed = 0
    for k in range(game.T):
        for i in range(game.N):
            ai = alpha[k, game.uoff[i]:game.uoff[i + 1]]
            ed = ed - (ai @ lq["R"][(i, i)][k]) @ lq["r"][(i, i)][k]
            if k > 0:
                ed = ed - (dxs[k] @ lq["Q"][k, i]) @ lq["l"][k, i]
    return ed


def feedback_sweep(game, lq, dx0, NT):
    """LQFeedbackSolver: the coupled Riccati recursion with the Gershgorin step on S.  -> P, alpha, dxs, corrections."""
    T, N, n, m = game.T, game.N, game.n, game.m
    sl = [slice(game.uoff[i], game.uoff[i + 1]) for i in range(N)]
    Z = [np.array(lq["Q"][T - 1, i], NT) for i in range(N)]
    zeta = [np.array(lq["l"][T - 1, i], NT) for i in range(N)]
    P, alpha = np.zeros((T, m, n), NT), np.zeros((T, m), NT)
    corrections = 0
    floor = NT(MIN_EVAL)
    for k in range(T - 2, -1, -1):
        A, B = lq["A"][k], lq["B"][k]
        S, Y = np.zeros((m, m), NT), np.zeros((m, n + 1), NT)
        for i in range(N):
            BiZ = B[:, sl[i]].T @ Z[i]
            S[sl[i]] = BiZ @ B
            S[sl[i], sl[i]] += lq["R"][(i, i)][k]
            Y[sl[i], :n] = BiZ @ A
            Y[sl[i], n] = B[:, sl[i]].T @ zeta[i] + lq["r"][(i, i)][k]
        for c in range(m):
            radius = np.abs(S[:, c]).sum() - np.abs(S[c, c])
            if S[c, c] - radius < floor:
                S[c, c] += radius + floor
                corrections += 1
        X = eliminate(S, Y, NT)
        P[k], alpha[k] = X[:, :n], X[:, n]
        F = A - B @ P[k]
        beta = -(B @ alpha[k])
        for i in range(N):
            z = F.T @ (Z[i] @ beta + zeta[i]) + lq["l"][k, i]
            Zn = F.T @ (Z[i] @ F) + lq["Q"][k, i]
            for (a, j) in game.pairs:
                if a == i:
                    Rij = lq["R"][(a, j)][k]
                    z = z + P[k][sl[j]].T @ (Rij @ alpha[k][sl[j]] - lq["r"][(a, j)][k])
                    Zn = Zn + P[k][sl[j]].T @ (Rij @ P[k][sl[j]])
            Z[i], zeta[i] = Zn, z
    dxs = np.zeros((T, n), NT)
    x = np.array(dx0, NT)
    for k in range(T):  # the forward pass carries no feedback term
        dxs[k] = x
        x = lq["A"][k] @ x - lq["B"][k] @ alpha[k]
    return P, alpha, dxs, corrections


def open_loop_sweep(game, lq, dx0, NT):
    """LQOpenLoopSolver: value functions M, m backwards through Lambda = I + sum B_i R_ii^-1 B_i^T M_i, states and
    feed-forward terms forwards.  -> P (zero), alpha, dxs, 0."""
    T, N, n, m = game.T, game.N, game.n, game.m
    sl = [slice(game.uoff[i], game.uoff[i + 1]) for i in range(N)]
    M = [np.array(lq["Q"][T - 1, i], NT) for i in range(N)]
    mv = [np.array(lq["l"][T - 1, i], NT) for i in range(N)]
    keep = [None] * T
    for k in range(T - 2, -1, -1):
        A, B = lq["A"][k], lq["B"][k]
        Lam = np.eye(n, dtype=NT)
        inter = np.zeros(n, NT)
        wB, wr = [], []
        for i in range(N):
            Bi = B[:, sl[i]]
            sol = eliminate(lq["R"][(i, i)][k], np.concatenate([Bi.T, lq["r"][(i, i)][k][:, None]], axis=1), NT)
            wB.append(sol[:, :n])
            wr.append(sol[:, n])
            Lam = Lam + (Bi @ wB[i]) @ M[i]
            inter = inter - Bi @ (wB[i] @ mv[i] + wr[i])
        sol = eliminate(Lam, np.concatenate([A, inter[:, None]], axis=1), NT)
        LinvA, lc = sol[:, :n], sol[:, n]
        keep[k] = (Lam, inter, wB, wr, [Mi.copy() for Mi in M], [v.copy() for v in mv])
        for i in range(N):
            Mn = A.T @ (M[i] @ LinvA) + lq["Q"][k, i]
            mn = A.T @ (M[i] @ lc + mv[i]) + lq["l"][k, i]
            M[i], mv[i] = Mn, mn
    P, alpha, dxs = np.zeros((T, m, n), NT), np.zeros((T, m), NT), np.zeros((T, n), NT)
    x = np.array(dx0, NT)
    for k in range(T - 1):
        dxs[k] = x
        Lam, inter, wB, wr, Mk, mk = keep[k]
        x = eliminate(Lam, (lq["A"][k] @ x + inter)[:, None], NT)[:, 0]
        for i in range(N):
            alpha[k, sl[i]] = wB[i] @ (Mk[i] @ x + mk[i]) + wr[i]
    dxs[T - 1] = x
    return P, alpha, dxs, 0


def open_loop_kkt(game, lq, dx0):
    """The open-loop Nash equilibrium of the LQ game by ONE dense solve (float64) of every player's first-order
    conditions stacked over the horizon — unknowns dx_1 .. dx_{T-1}, du_0 .. du_{T-2} and one costate chain
    lam^i_1 .. lam^i_{T-1} per player:
        dx_{k+1} = A_k dx_k + B_k du_k,
        R_ii du_i,k + r_ii,k + B_i,k^T lam^i_{k+1} = 0                      (k = 0 .. T-2),
        Q_i,k dx_k + l_i,k + A_k^T lam^i_{k+1} - lam^i_k = 0                (k = 1 .. T-1, lam^i_T = 0).
    -> alpha (T, m) with alpha_k = -du_k (row T-1 zero), dxs (T, n)."""
    T, N, n, m = game.T, game.N, game.n, game.m
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    X = lambda k: slice((k - 1) * n, k * n)                                  # noqa: E731  dx_k, k = 1 .. T-1
    U = lambda k: slice((T - 1) * n + k * m, (T - 1) * n + (k + 1) * m)      # noqa: E731  du_k, k = 0 .. T-2
    L0 = (T - 1) * (n + m)
    Lm = lambda i, k: slice(L0 + ((k - 1) * N + i) * n, L0 + ((k - 1) * N + i + 1) * n)  # noqa: E731  lam^i_k, k = 1 .. T-1
    size = L0 + (T - 1) * N * n
    K, rhs = np.zeros((size, size)), np.zeros(size)
    row = 0
    for k in range(T - 1):  # dynamics
        rs = slice(row, row + n)
        K[rs, X(k + 1)] = -np.eye(n)
        K[rs, U(k)] = f(lq["B"][k])
        if k == 0:
            rhs[rs] = -f(lq["A"][0]) @ f(dx0)
        else:
            K[rs, X(k)] = f(lq["A"][k])
        row += n
    for k in range(T - 1):  # controls
        for i in range(N):
            mi = game.ms[i]
            rs = slice(row, row + mi)
            ui = slice(U(k).start + game.uoff[i], U(k).start + game.uoff[i + 1])
            K[rs, ui] = f(lq["R"][(i, i)][k])
            K[rs, Lm(i, k + 1)] = f(lq["B"][k])[:, game.uoff[i]:game.uoff[i + 1]].T
            rhs[rs] = -f(lq["r"][(i, i)][k])
            row += mi
    for k in range(1, T):  # costates
        for i in range(N):
            rs = slice(row, row + n)
            K[rs, X(k)] = f(lq["Q"][k, i])
            K[rs, Lm(i, k)] = -np.eye(n)
            if k + 1 < T:
                K[rs, Lm(i, k + 1)] = f(lq["A"][k]).T
            rhs[rs] = -f(lq["l"][k, i])
            row += n
    assert row == size
    sol = np.linalg.solve(K, rhs)
    alpha, dxs = np.zeros((T, m)), np.zeros((T, n))
    dxs[0] = f(dx0)
    for k in range(1, T):
        dxs[k] = sol[X(k)]
    for k in range(T - 1):
        alpha[k] = -sol[U(k)]
    return alpha, dxs


def _start(game, tb, x0, integrator):
    """The initial rollout under zero strategies from the zero operating point with xs[0] = x0."""
    NT, T = tb.NT, game.T
    xs_ref = np.zeros((T, game.n), NT)
    xs_ref[0] = np.array(x0, NT)
    z = np.zeros
    return rollout(game, tb, x0, xs_ref, z((T, game.m), NT), z((T, game.m, game.n), NT), z((T, game.m), NT), integrator)


def solve(game, x0, steps, NT, open_loop=None, integrator="rk4"):
    """ILQSolver::Solve with forced steps for one instance, in NT.  -> one dict per iteration: xs, us, rawP (T, m, n), alpha
    (scaled by the step, as the device returns it), raw_alpha, costs, merit, expected_decrease, corrections (of this
    iteration's sweep), lq (the inputs of this iteration's LQ solve), dxs."""
    open_loop = game.open_loop if open_loop is None else open_loop
    tb = Tables(game, NT)
    x0 = np.array(x0, NT)
    xs, us = _start(game, tb, x0, integrator)
    lq = lq_inputs(game, tb, xs, us)
    out = []
    for s in steps:
        P, alpha, dxs, corrections = (open_loop_sweep if open_loop else feedback_sweep)(game, lq, x0 - xs[0], NT)
        ed = expected_decrease(game, lq, alpha, dxs)
        used = lq
        scaled = alpha * NT(s)
        xs, us = rollout(game, tb, xs[0], xs, us, P, scaled, integrator)
        lq = lq_inputs(game, tb, xs, us)
        out.append(dict(xs=xs, us=us, rawP=P, alpha=scaled, raw_alpha=alpha, costs=total_costs(game, tb, xs, us),
                        merit=merit(game, lq), expected_decrease=ed, corrections=corrections, lq=used, dxs=dxs))
    return out


def solve_free(game, x0, NT, initial=1.0, geometric=0.5, fraction=0.001, tolerance=0.1, max_iters=1000, max_backtracks=10):
    """ILQSolver::Solve with its line search.  -> dict(xs, us, rawP, alpha, costs, iters, converged, ok, margin): margin is
    the smallest relative distance of any decision (an Armijo test, a convergence test) from its threshold."""
    tb = Tables(game, NT)
    x0 = np.array(x0, NT)
    xs, us = _start(game, tb, x0, "rk4")
    lq = lq_inputs(game, tb, xs, us)
    last, iters, converged, ok, margin = NT(np.inf), 0, False, True, np.inf
    res = dict(xs=xs, us=us, rawP=None, alpha=None)
    sweep = open_loop_sweep if game.open_loop else feedback_sweep
    while iters < max_iters and not converged:
        iters += 1
        P, alpha, dxs, _ = sweep(game, lq, x0 - xs[0], NT)
        ed = expected_decrease(game, lq, alpha, dxs)
        step, accepted = NT(initial), False
        for _ in range(max_backtracks):
            txs, tus = rollout(game, tb, xs[0], xs, us, P, alpha * step, "rk4")
            tlq = lq_inputs(game, tb, txs, tus)
            mer = merit(game, tlq)
            bound = NT(fraction) * step * ed
            if np.isfinite(last):
                margin = min(margin, float(abs((last - mer) - bound) / max(abs(last), abs(mer), abs(bound))))
            if last - mer >= bound:
                if np.isfinite(last):
                    margin = min(margin, float(abs(abs(last - mer) - NT(tolerance)) / NT(tolerance)))
                converged = bool(mer <= last and abs(last - mer) < NT(tolerance))
                last, accepted = mer, True
                break
            step = step * NT(geometric)
        if not accepted:
            ok = False
            break
        xs, us, lq = txs, tus, tlq
        res = dict(xs=xs, us=us, rawP=P, alpha=alpha * step)
    res.update(costs=total_costs(game, tb, xs, us), iters=iters, converged=converged, ok=ok, margin=margin, merit=last)
    return res


def free_running(spec, initial=1.0):
    """The solver parameters of the free-running comparison, set on the spec (solve_free's defaults)."""
    spec.params.initial_alpha_scaling, spec.params.geometric_alpha_scaling = initial, 0.5
    spec.params.expected_decrease_fraction = 0.001
    return spec


def flat(P):
    """(..., m, n) gains as the device's column-major words [..., t + m c]."""
    return np.swapaxes(P, -1, -2).reshape(P.shape[:-2] + (-1,))


# ---- the games of the comparison: name -> builder ----
GAMES = {
    "8_2_1_constant_b": lambda: build("8_2_1", "constant_b"),
    "8_2_1_computed_b": lambda: build("8_2_1", "computed_b"),
    "8_2_1_gershgorin": lambda: build("8_2_1", "computed_b", gershgorin=True),
    "17_3_2": lambda: build("17_3_2", "computed_b"),
    "17_3_2_gershgorin": lambda: build("17_3_2", "constant_b", gershgorin=True),
    "14_3_2": lambda: build("14_3_2", "computed_b"),
    "14_3_2_gershgorin": lambda: build("14_3_2", "constant_b", gershgorin=True),
    "9_mixed": lambda: build("9_mixed", "computed_b"),
    "9_mixed_gershgorin": lambda: build("9_mixed", "constant_b", gershgorin=True),
    "point_mass_expression": lambda: build_point_mass(expression_costs=True),
    "24_4_2_open_loop": lambda: build("24_4_2", "computed_b", open_loop=True),
    "8_2_1_open_loop": lambda: build("8_2_1", "constant_b", open_loop=True),
    "integrator": lambda: build("integrator", "constant_b"),
}
OUTPUTS = ("xs", "us", "P", "alpha", "costs", "merit", "expected_decrease")


def reference_run(game, x0, NT, steps=STEPS):
    """solve() for every instance of x0 [B][n]: -> one dict per iteration of arrays [B][...] under the names of OUTPUTS
    (P as the device's words), float64 (or longdouble) copies of NT's results."""
    runs = [solve(game, x0[b], steps, NT) for b in range(x0.shape[0])]
    out = []
    for k in range(len(steps)):
        d = {q: np.stack([np.asarray(r[k][q]) for r in runs]) for q in ("xs", "us", "alpha", "costs", "merit", "expected_decrease")}
        d["P"] = np.stack([flat(r[k]["rawP"]) for r in runs])
        d["corrections"] = np.array([r[k]["corrections"] for r in runs])
        out.append(d)
    return out


def scale_of(name, ref_k, ref_1):
    """The scale an output's error is relative to, per instance: its own largest entry — alpha on the scale of the first
    iteration's (after a full step it is rounding noise), a scalar on max(1, |value|)."""
    a = np.abs(np.asarray(ref_1["alpha"] if name == "alpha" else ref_k[name], np.float64))
    if a.ndim == 1:
        return np.maximum(1.0, a)
    return np.maximum(a.reshape(a.shape[0], -1).max(axis=1), 1e-30)


def errors(name, got, ref_k, ref_1):
    """Per instance: max |got - ref| over the output's entries, relative to scale_of."""
    d = np.abs(np.asarray(got[name], np.longdouble) - np.asarray(ref_k[name], np.longdouble))
    d = d.reshape(d.shape[0], -1).max(axis=1)
    return (d / scale_of(name, ref_k, ref_1)).astype(np.float64)


# ---- the measured precision gaps (tests/golden/lq_games.json, written by tests/golden/make_lq_games.py) ----
B, SEED = 8, 7
TYPES = {"float32": np.float32, "float64": np.float64, "longdouble": np.longdouble}
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
# the project's existing bars (tests/test_gpu_forced.py): no bar derived from a gap may be looser
PROJECT_BAR = {"f64": dict.fromkeys(OUTPUTS, 1e-9),
               "f32": dict(xs=2e-3, us=2e-3, costs=2e-3, merit=2e-3, P=1e-2, alpha=1e-2, expected_decrease=1e-2)}
_RUNS = {}


def cached_run(name, type_name, nudged=False):
    """reference_run of GAMES[name] on its B instances in the named type, computed once per process and left unchanged."""
    key = (name, type_name, nudged)
    if key not in _RUNS:
        game = GAMES[name]()
        x0 = game.x0(B, SEED)
        if nudged:
            x0 = x0 + 1e-12 * np.random.default_rng(SEED + 1).standard_normal(x0.shape)
        _RUNS[key] = reference_run(game, x0, TYPES[type_name])
    return _RUNS[key]


def gaps(name):
    """-> {"gap64": {output: |float64 - longdouble|}, "gap32": {output: |float32 - float64|}}: the largest relative
    distance (errors()) over the B instances and the iterations, of the reference alone."""
    r32, r64, rld = (cached_run(name, t) for t in ("float32", "float64", "longdouble"))
    out = {"gap64": {}, "gap32": {}}
    for q in OUTPUTS:
        out["gap64"][q] = max(float(errors(q, r64[k], rld[k], rld[0]).max()) for k in range(len(STEPS)))
        out["gap32"][q] = max(float(errors(q, r32[k], r64[k], r64[0]).max()) for k in range(len(STEPS)))
    return out


def bar(committed, name, output, precision):
    """100 x the committed gap of that game and output, floored at 100 ulp of the type: the device sums in another order,
    contracts to FMA and takes its pivots' reciprocals within an ulp."""
    gap = committed[name]["gap64" if precision == "f64" else "gap32"][output]
    b = max(100.0 * gap, 100.0 * EPS[precision])
    assert b <= PROJECT_BAR[precision][output], (name, output, precision, b)
    return b
