"""The time as an input of expression programs (ILQG_EXPR_PUSH_TIME, include/ilqg.h) without a device: the validator, what
the host half of creation accepts, the evaluators (csrc/ilqg_expr.hpp, through the stand-alone
tests/host/expr_time_check.cpp) against a numpy restatement in which the time leaf is the constant t_k and against central
differences, a time-reading model's linearisation and RK4 step, and the C++ mirror (host::Expr::Time())."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from ilqgames_amd import abi, examples
from ilqgames_amd.abi import Expr
from test_expression_cost import np_jet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ilqgames_amd", "csrc")
X, Y, CONST, W, V, ADD, MUL, TIME = (abi.EXPR_PUSH_X, abi.EXPR_PUSH_Y, abi.EXPR_PUSH_CONST, abi.EXPR_PUSH_WEIGHT,
                                     abi.EXPR_PUSH_VALUE, abi.EXPR_ADD, abi.EXPR_MUL, abi.EXPR_PUSH_TIME)
T12 = 12


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        entry.build()
    return h


def test_the_enumerator_and_the_python_leaf():
    assert TIME == 18 and Expr.time().program() == [(18, 0.0)]
    text = open(os.path.join(ROOT, "include", "ilqg.h")).read()
    assert "ILQG_EXPR_PUSH_TIME = 18" in text


# ------------------------------------------------------------------------------------------------
# the stand-alone checker
# ------------------------------------------------------------------------------------------------
def _build_checker(out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off"] + list(extra) +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "host", "expr_time_check.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(str(tmp_path_factory.mktemp("exprtime") / "expr_time_check"))


def _jet_line(dtype, two, w, v, k, dt, block, pts):
    T = np.float32 if dtype == "f32" else np.float64
    flat = []
    for x, y in pts:
        flat += [repr(float(T(x))), repr(float(T(y)))]
    return " ".join(["jet", dtype, "1" if two else "0", repr(float(w)), repr(float(v)), str(int(k)), repr(float(dt)),
                     str(len(block))] + [str(b) if isinstance(b, str) else repr(float(b)) for b in block] +
                    [str(len(pts))] + flat)


def _parse_jets(out):
    cases = []
    for line in out.splitlines():
        tok = line.split()
        if tok[0] == "check":
            cases.append((tuple(int(t) for t in tok[1:4]), []))
        else:
            vals = [float.fromhex(t) for t in tok if t not in ("jet", "grad", "value", "|")]
            cases[-1][1].append(dict(jet=vals[0:6], grad=vals[6:9], value=vals[9]))
    return cases


def _run_jets(exe, lines):
    return _parse_jets(subprocess.run([exe], input="\n".join(lines) + "\n", text=True, capture_output=True, check=True).stdout)


# ---- the validator: (block words, two inputs, ExprFault, op at fault, final depth or None) ----
VALIDATOR = [
    ([1.0, TIME, 0.0], False, 0, -1),                                   # the leaf alone
    ([3.0, X, 0.0, TIME, 0.0, MUL, 0.0], False, 0, -1),                 # a push like the others: X T MUL
    ([4.0] + [TIME, 0.0] * 4, True, 6, -1),                             # four entries are allowed, four left are not
    ([5.0] + [TIME, 0.0] * 5, True, 5, 4),                              # a fifth entry: overflow at depth 4, at op 4
    ([5.0] + [X, 0.0] * 4 + [TIME, 0.0], True, 5, 4),                   # ... also behind four other pushes
    ([2.0, X, 0.0, TIME, 0.0], True, 6, -1),                            # two entries left
    ([2.0, TIME, 0.0, ADD, 0.0], True, 4, 1),                           # it is one entry, not two
    ([2.0, X, 0.0, 42.0, 0.0], True, 3, 1),                             # still unknown
    ([2.0, X, 0.0, 99.0, 0.0], True, 3, 1),
    ([2.0, X, 0.0, 19.0, 0.0], True, 3, 1),                             # the first opcode past the table
]


def test_validator_counts_the_time_leaf_as_a_push(checker):
    cases = _run_jets(checker, [_jet_line("f64", two, 1.0, 1.0, 3, 0.1, blk, [(0.5, 0.25)]) for blk, two, _, _ in VALIDATOR])
    assert len(cases) == len(VALIDATOR)
    for (blk, two, fault, op), (check, rows) in zip(VALIDATOR, cases):
        assert check[:2] == (fault, op), (blk, check)
        assert (len(rows) == 1) == (fault == 0)
    assert cases[2][0][2] == 4 and cases[5][0][2] == 2  # the final depths reported
    # the leaf alone is the time itself, with no derivative
    assert cases[0][1][0]["jet"] == [3 * 0.1, 0.0, 0.0, 0.0, 0.0, 0.0] and cases[0][1][0]["value"] == 3 * 0.1


def _scene_terms():
    """(spec, term, kind) of a time-reading term of each of the three kinds."""
    obstacle, gust = examples.moving_obstacle_scene(T=T12), examples.gusting_car_scene(T=T12)
    row = next(q for q, t in enumerate(gust.terms) if t["kind"] == abi.DYN_ROW_EXPRESSION and t["idx"][0] == 2)
    return [(obstacle, obstacle.term_index("p1_pedestrian_bump"), abi.COST_EXPRESSION),
            (obstacle, obstacle.term_index("p1_pedestrian_keep_out"), abi.CONSTRAINT_EXPRESSION),
            (gust, row, abi.DYN_ROW_EXPRESSION)]


def _reads_time(spec, term):
    off = spec.terms[term]["polyline"]
    L = int(spec.dense_params[off])
    return TIME in [int(spec.dense_params[off + 1 + 2 * i]) for i in range(L)]


def test_the_host_half_of_creation_accepts_the_opcode_in_all_three_kinds(hip):
    for spec, term, kind in _scene_terms():
        assert spec.terms[term]["kind"] == kind and _reads_time(spec, term)
        hip.expression_check(spec, term)      # raises where creation would refuse
        words, _ = hip.row_program_build(spec)  # the whole host half: tables and the row program
        assert len(words) > 0


@pytest.mark.parametrize("opcode", [42.0, 99.0, 19.0])
def test_unknown_opcodes_are_still_refused_in_all_three_kinds(hip, opcode):
    for spec, term, kind in _scene_terms():
        spec.terms[term]["polyline"] = len(spec.dense_params)
        spec.dense_params += [2.0, float(X), 0.0, opcode, 0.0]
        with pytest.raises(hip.IlqgError) as e:
            hip.expression_check(spec, term)
        assert e.value.status == abi.ERR_UNSUPPORTED and "op 1: unknown opcode" in str(e.value), kind


def test_depth_rules_reach_creation_s_messages(hip):
    for spec, term, kind in _scene_terms():
        spec.terms[term]["polyline"] = len(spec.dense_params)
        spec.dense_params += [5.0] + [float(TIME), 0.0] * 5
        with pytest.raises(hip.IlqgError) as e:
            hip.expression_check(spec, term)
        assert e.value.status == abi.ERR_UNSUPPORTED and "op 4: stack overflow" in str(e.value), kind
    for spec, term, kind in _scene_terms():
        spec.terms[term]["polyline"] = len(spec.dense_params)
        spec.dense_params += [2.0, float(X), 0.0, float(TIME), 0.0]
        with pytest.raises(hip.IlqgError) as e:
            hip.expression_check(spec, term)
        assert e.value.status == abi.ERR_INVALID and "ends with 2 entries on the stack" in str(e.value), kind


def test_time_expression_twin_replaces_the_nominal_path_length_cost_alone(hip):
    zoo = examples.dynamics_zoo_scene(T=T12)
    twin, replaced = examples.time_expression_twin(zoo)
    assert replaced == 1
    assert [t["kind"] for t in twin.terms].count(abi.COST_EXPRESSION) == 1
    assert [t["kind"] for t in twin.terms].count(abi.COST_NOMINAL_PATH_LENGTH) == 0
    assert [t["kind"] for t in twin.terms].count(abi.COST_ROUTE_PROGRESS) == 2  # RouteProgressCost is not twinned
    hip.row_program_build(twin)


# ------------------------------------------------------------------------------------------------
# the evaluator against the numpy restatement with the time leaf a constant
# ------------------------------------------------------------------------------------------------
def np_time_jet(program, w, v, x, y, t, T):
    """test_expression_cost.np_jet of `program` at time t: the time leaf becomes a constant that np_jet pushes exactly —
    PUSH_VALUE with value = t where the program does not read the value, else PUSH_CONST with t as its immediate (np_jet
    rounds an immediate to float32 as the block does, so t must then be a float32: the callers choose dt accordingly)."""
    ops = [op for op, _ in program]
    if V not in ops:
        return np_jet([(V, 0.0) if op == TIME else (op, imm) for op, imm in program], w, T(t), x, y, T)
    assert float(np.float32(t)) == float(t), "this program reads the value: its time must be exact in float32"
    return np_jet([(CONST, float(t)) if op == TIME else (op, imm) for op, imm in program], w, v, x, y, T)


x_, y_, w_, v_, t_ = Expr.x(), Expr.y(), Expr.weight(), Expr.value(), Expr.time()
_dx, _dy = examples.moving_obstacle_offset(x_, 3.0, -2.0), examples.moving_obstacle_offset(y_, -6.0, 1.0)
# (tree, two inputs, (weight, value), the box the points are drawn from)
EXACT = {  # pushes, ADD SUB MUL DIV NEG SQUARE SQRT HINGE only: IEEE operations in the same order round the same
    "tracking": (0.5 * w_ * (x_ - t_ * v_).square(), False, (10.0, 5.0), (-3.0, 12.0)),
    "leaf_plus_x": (t_ + x_, False, (1.0, 0.0), (-3.0, 3.0)),
    "x_times_t": (x_ * t_, False, (1.0, 0.0), (-3.0, 3.0)),
    "x_y_t": (x_ * y_ * t_ - w_ * t_ * t_, True, (2.0, 0.0), (-3.0, 3.0)),
    "square_of_offset_times_y": ((x_ - t_).square() * y_, True, (1.0, 0.0), (-3.0, 3.0)),
    "ramped_weight": (w_ * (t_ / (1.0 + t_)) * (x_.square() + y_.square()), True, (3.0, 0.0), (-2.0, 2.0)),
    "rational": (x_ / (1.0 + t_) + y_ * t_ * t_, True, (1.0, 0.0), (-3.0, 3.0)),
    "hinge_past_the_front": (0.5 * w_ * (x_ - v_ * t_).hinge().square(), False, (4.0, 2.0), (-1.0, 6.0)),
    "keep_out": (v_.square() - _dx.square() - _dy.square(), True, (1.0, 1.5), (-8.0, 8.0)),
    "growing_disc": ((x_.square() + y_.square() + t_).sqrt() - v_ * t_, True, (1.0, 0.5), (-3.0, 3.0)),
}
SMOOTH = {  # EXP LOG SIN COS
    "moving_bump": (((_dx.square() + _dy.square()) * -0.5 / v_.square()).exp() * w_, True, (40.0, 2.0), (-6.0, 6.0)),
    "discounted": ((-(v_ * t_)).exp() * w_ * x_.square(), False, (3.0, 0.7), (-3.0, 3.0)),
    "rotating": (t_.sin() * x_ + t_.cos() * y_, True, (1.0, 0.0), (-3.0, 3.0)),
    "composed": ((x_ * t_).sin() * (y_ - t_).cos(), True, (1.0, 0.0), (-2.0, 2.0)),
    "log_of_time": ((1.0 + t_ + x_.square()).log(), False, (1.0, 0.0), (-4.0, 4.0)),
}
CASES = dict(EXACT, **SMOOTH)
assert len(CASES) >= 12
FD_SKIP = {"hinge_past_the_front": lambda x, y, t: abs(x - 2.0 * t) < 0.1}
# dt = 0.125: every t_k is exact in float32, so each program can be restated in either precision; dt = 0.1 (fp32 only for
# the programs that read the value): t_k = T(double(k) * dt) is rounded, once
STEPS = (0, 1, 5, 11)


def _points(name, t, count=8):
    _, two, _, (lo, hi) = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    pts = []
    while len(pts) < count:
        x, y = rng.uniform(lo, hi, 2)
        if name in FD_SKIP and FD_SKIP[name](x, y, t):
            continue
        pts.append((float(x), float(y) if two else 0.0))
    return pts


def _time(k, dt, T):
    return T(float(k) * dt)  # formed in double, rounded once


def _dts(name, dtype):
    reads_value = V in [op for op, _ in CASES[name][0].program()]
    return (0.125,) if (reads_value and dtype == "f64") else (0.125, 0.1)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_arithmetic_programs_match_the_numpy_restatement_bit_for_bit(checker, dtype):
    T = np.float32 if dtype == "f32" else np.float64
    runs = [(n, k, dt) for n in sorted(EXACT) for dt in _dts(n, dtype) for k in STEPS]
    cases = _run_jets(checker, [_jet_line(dtype, EXACT[n][1], *EXACT[n][2], k, dt, abi.expr_block(EXACT[n][0].program()),
                                          _points(n, k * dt)) for n, k, dt in runs])
    assert len(cases) == len(runs)
    seen_time = set()
    for (name, k, dt), (check, rows) in zip(runs, cases):
        tree, two, (w, v), _ = EXACT[name]
        assert check == (0, -1, 1), name
        t = _time(k, dt, T)
        for (x, y), row in zip(_points(name, k * dt), rows):
            want = np_time_jet(tree.program(), T(w), T(v), T(x), T(y), t, T)
            got = [T(c) for c in row["jet"]]
            assert np.array(got, T).tobytes() == np.array(want, T).tobytes(), (name, k, dt, x, y, got, want)
            assert np.array(row["grad"], T).tobytes() == np.array(want[:3], T).tobytes(), name
            assert T(row["value"]).tobytes() == T(want[0]).tobytes(), name
            if k > 0 and want[0] != np_time_jet(tree.program(), T(w), T(v), T(x), T(y), T(0), T)[0]:
                seen_time.add(name)
    assert seen_time == set(EXACT), "every program's value depends on the time at some point"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_transcendental_programs_match_the_numpy_restatement(checker, dtype):
    """fp64: each libm call is good to a couple of ulp and at most 64 ops follow: 1e-12 of the jet's largest component.
    fp32: the same count in float — 64 roundings of 6e-8 are 4e-6, and these programs amplify an error of their argument
    by less than five (|d exp| <= exp <= 1 here, sin / cos are contractions): 2e-5."""
    T = np.float32 if dtype == "f32" else np.float64
    bar = 1e-12 if dtype == "f64" else 2e-5
    runs = [(n, k, dt) for n in sorted(SMOOTH) for dt in _dts(n, dtype) for k in STEPS]
    cases = _run_jets(checker, [_jet_line(dtype, SMOOTH[n][1], *SMOOTH[n][2], k, dt, abi.expr_block(SMOOTH[n][0].program()),
                                          _points(n, k * dt)) for n, k, dt in runs])
    for (name, k, dt), (check, rows) in zip(runs, cases):
        tree, two, (w, v), _ = SMOOTH[name]
        assert check == (0, -1, 1), name
        t = _time(k, dt, T)
        for (x, y), row in zip(_points(name, k * dt), rows):
            want = np.array(np_time_jet(tree.program(), T(w), T(v), T(x), T(y), t, T), np.float64)
            err = np.max(np.abs(np.array(row["jet"]) - want)) / max(np.max(np.abs(want)), 1e-300)  # (an all-zero jet: exact)
            assert err <= bar, (name, k, dt, x, y, err)
            assert abs(row["value"] - want[0]) <= bar * np.max(np.abs(want)), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_derivatives_in_x_and_y_match_central_differences(checker, name):
    """Central differences of the VALUE program (h = 1e-5, fp64) for the gradient and of the jet's gradient for the
    Hessian, both good to about h^2 + eps / h = 1e-10; the bar is 1e-7 of the largest entry, at steps 1, 5 and 11."""
    tree, two, (w, v), _ = CASES[name]
    block = abi.expr_block(tree.program())
    h, dt = 1e-5, 0.1
    for k in STEPS[1:]:
        pts = _points(name, k * dt)
        shifted = []
        for x, y in pts:
            shifted += [(x, y), (x + h, y), (x - h, y), (x, y + h), (x, y - h)]
        (check, rows), = _run_jets(checker, [_jet_line("f64", two, w, v, k, dt, block, shifted)])
        assert check == (0, -1, 1)
        for q, (x, y) in enumerate(pts):
            at, xp, xm, yp, ym = rows[5 * q:5 * q + 5]
            hx, hy = ((x + h) - (x - h)) / 2.0, ((y + h) - (y - h)) / 2.0
            grad_fd = np.array([(xp["value"] - xm["value"]) / (2 * hx), (yp["value"] - ym["value"]) / (2 * hy) if two else 0.0])
            grad, hess = np.array(at["jet"][1:3]), np.array(at["jet"][3:6])
            hess_fd = np.array([(xp["jet"][1] - xm["jet"][1]) / (2 * hx),
                                (yp["jet"][2] - ym["jet"][2]) / (2 * hy) if two else 0.0,
                                (yp["jet"][1] - ym["jet"][1]) / (2 * hy) if two else 0.0])
            scale_g = max(np.max(np.abs(grad)), 1e-300)
            scale_h = max(np.max(np.abs(hess)), 1e-300)
            assert np.max(np.abs(grad - grad_fd)) <= 1e-7 * scale_g, (name, k, x, y, grad, grad_fd)
            assert np.max(np.abs(hess - hess_fd)) <= 1e-7 * scale_h, (name, k, x, y, hess, hess_fd)
            if not two:
                assert at["jet"][2] == 0.0 and at["jet"][4] == 0.0 and at["jet"][5] == 0.0


# ------------------------------------------------------------------------------------------------
# a time-reading model: linearisation at t_k, RK4 at the stage times
# ------------------------------------------------------------------------------------------------
DT = 0.1
u_ = y_  # (a row's second input may be a control)
SWAY_ROWS = [(x_ * t_.sin() + u_ * t_.cos(), 0, 2), (x_ * y_ * t_, 0, 1)]  # xdim 2, udim 1
SWAY = (2, 1, SWAY_ROWS, 0.0, None)
GUST = (4, 1, examples.gusting_car_rows(), float(np.float32(examples.COASTING_CAR_DRAG)),
        [1.0, 1.0, float(np.float32(examples.GUSTING_CAR_AMPLITUDE)), 1.0])


def sway_rates(x, u, t):
    return np.array([x[0] * np.sin(t) + u[0] * np.cos(t), x[0] * x[1] * t])


def gust_rates(x, u, t):
    c, a, om = GUST[3], GUST[4][2], float(np.float32(examples.GUSTING_CAR_OMEGA))
    return np.array([x[3] * np.cos(x[2]), x[3] * np.sin(x[2]), x[3] * u[0] + a * np.sin(om * t), -(c * (x[3] * x[3]))])


def _model_text(model, k, pts):
    xdim, udim, rows, param, weights = model
    lines = ["model %d %d %r %r %d" % (xdim, udim, float(param), DT, k)]
    for r, (tree, xin, yin) in enumerate(rows):
        block = abi.expr_block(tree.program())
        lines.append(" ".join(["row", str(xin), str(-1 if yin is None else yin), repr(1.0 if weights is None else weights[r]),
                               str(len(block))] + [repr(float(b)) for b in block]))
    lines.append("points %d" % len(pts))
    lines += [" ".join(repr(float(v)) for v in p) for p in pts]
    return "\n".join(lines) + "\n"


def _run_model(exe, model, k, pts):
    xdim, udim = model[:2]
    out = subprocess.run([exe], input=_model_text(model, k, pts), text=True, capture_output=True, check=True).stdout
    checks, res = [], []
    for line in out.splitlines():
        tok = line.split()
        if tok[0] == "check":
            checks.append(tuple(int(t) for t in tok[1:5]))
            continue
        vals = [float.fromhex(t) for t in tok if t not in ("rate", "A", "B", "step", "euler", "|")]
        a0, b0, s0, e0 = xdim, xdim + xdim * xdim, xdim + xdim * xdim + xdim * udim, 2 * xdim + xdim * xdim + xdim * udim
        res.append(dict(rate=np.array(vals[:a0]), A=np.array(vals[a0:b0]).reshape(xdim, xdim),
                        B=np.array(vals[b0:s0]).reshape(xdim, udim), step=np.array(vals[s0:e0]), euler=np.array(vals[e0:])))
    assert checks == [(r, 0, -1, 1) for r in range(xdim)]
    return res


def _model_points(model, count=6):
    xdim, udim = model[:2]
    return np.random.default_rng(7 * xdim + udim).uniform(-1.5, 1.5, (count, xdim + udim))


@pytest.mark.parametrize("k", [0, 3, 11])
def test_linearisation_is_at_t_k_with_the_time_inside_A_and_B(checker, k):
    """A = I + dt J_x, B = dt J_u of x sin(t) + u cos(t) and of x y t, written out by hand: a handful of roundings per
    entry, 1e-14 of the largest."""
    pts = _model_points(SWAY)
    t = k * DT
    for p, at in zip(pts, _run_model(checker, SWAY, k, pts)):
        x, u = p[:2], p[2:]
        A = np.eye(2) + DT * np.array([[np.sin(t), 0.0], [x[1] * t, x[0] * t]])
        B = DT * np.array([[np.cos(t)], [0.0]])
        assert np.max(np.abs(at["rate"] - sway_rates(x, u, t))) <= 1e-14 * max(np.max(np.abs(p)), 1.0)
        assert np.max(np.abs(at["A"] - A)) <= 1e-14 * np.max(np.abs(A))
        assert np.max(np.abs(at["B"] - B)) <= 1e-14 * np.max(np.abs(B))
        if k > 0:
            assert at["A"][0, 0] != 1.0 and at["A"][1, 1] != 1.0  # the time is inside A ...
        else:
            assert at["A"][0, 0] == 1.0 and at["B"][0, 0] == DT   # ... and at t = 0 sin is 0, cos is 1


def np_rk4_step(rates, x, u, k, dt, staged=True):
    """MultiPlayerDynamicalSystem::Integrate's RK4 (src/multi_player_dynamical_system.cpp:66-72): two half-steps of
    h = dt / 2, the stages of a half-step that begins at t0 evaluated at t0, t0 + h/2, t0 + h/2, t0 + h.
    staged=False: every stage at t_k, what an integrator that ignored the stage times would compute."""
    x = np.array(x, np.float64)
    h = dt / 2.0
    for s in range(2):
        t0 = k * dt + s * h
        at = (lambda c: t0 + c * h) if staged else (lambda c: k * dt)
        k1 = h * rates(x, u, at(0.0))
        k2 = h * rates(x + 0.5 * k1, u, at(0.5))
        k3 = h * rates(x + 0.5 * k2, u, at(0.5))
        k4 = h * rates(x + k3, u, at(1.0))
        x = x + (k1 + 2.0 * (k2 + k3) + k4) / 6.0
    return x


@pytest.mark.parametrize("model,rates", [(SWAY, sway_rates), (GUST, gust_rates)], ids=["sway", "gusting_car"])
@pytest.mark.parametrize("k", [0, 4, 11])
def test_the_step_is_the_rk4_with_its_stages_at_the_stage_times(checker, model, rates, k):
    xdim = model[0]
    pts = _model_points(model)
    for p, at in zip(pts, _run_model(checker, model, k, pts)):
        x, u = p[:xdim], p[xdim:]
        want = np_rk4_step(rates, x, u, k, DT)
        assert np.max(np.abs(at["step"] - want)) <= 1e-14 * max(np.max(np.abs(want)), 1.0)
        # the stage times matter at this bar: with every stage at t_k the step is a different one
        assert np.max(np.abs(np_rk4_step(rates, x, u, k, DT, staged=False) - want)) >= 1e-6
        euler = x + DT * rates(x, u, k * DT)
        assert np.max(np.abs(at["euler"] - euler)) <= 1e-14 * max(np.max(np.abs(euler)), 1.0)


def test_stand_alone_checker_is_clean_under_the_host_sanitizers(tmp_path):
    exe = _build_checker(str(tmp_path / "expr_time_check_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    text = "\n".join(_jet_line("f32", two, 1.0, 1.0, 3, 0.1, blk, [(0.5, 0.25)]) for blk, two, _, _ in VALIDATOR) + "\n"
    text += "\n".join(_jet_line(d, CASES[n][1], *CASES[n][2], 5, 0.125, abi.expr_block(CASES[n][0].program()), _points(n, 0.625, 3))
                      for n in sorted(CASES) for d in ("f32", "f64")) + "\n"
    text += _model_text(SWAY, 3, _model_points(SWAY, 2)) + _model_text(GUST, 7, _model_points(GUST, 2))
    done = subprocess.run([exe], input=text, text=True, capture_output=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr
    assert done.stdout.count("jet") == 6 * len(CASES) + 2 and done.stdout.count("rate") == 4


# ------------------------------------------------------------------------------------------------
# the C++ mirror
# ------------------------------------------------------------------------------------------------
def _build_host_program(tmp_path, name, source, defines=()):
    entry.build_host()
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + entry.host_compile_flags() + list(defines) +
                          ["-I" + os.path.join(ROOT, "tests", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", source)] + entry.host_link_flags())
    return exe


def test_cpp_gusting_car_scene_flattens_like_examples_py(tmp_path):
    exe = _build_host_program(tmp_path, "dump_gusting_car_scene", "dump_example.cpp",
                              ['-DEXAMPLE_HEADER="gusting_car_scene.h"', "-DEXAMPLE_CLASS=GustingCarScene"])
    got = abi.ProblemSpec.from_dump(subprocess.check_output([exe], text=True))
    want = examples.gusting_car_scene()
    g, w = got.canonical(), want.canonical()
    for key in ("subsystems", "player_costs", "pairs", "T", "dt"):
        assert g[key] == w[key], key
    assert set(g["groups"]) == set(w["groups"]) and (0, abi.ROLE_DYNAMICS_ROW) in g["groups"]
    for key in w["groups"]:
        assert g["groups"][key] == w["groups"][key], key
    # the dense table itself: the eight programs, subsystem by subsystem, the time leaf in both heading rows
    assert [np.float32(v) for v in got.dense_params] == [np.float32(v) for v in want.dense_params]
    ops = []
    off = 0
    while off < len(got.dense_params):
        L = int(got.dense_params[off])
        ops.append([int(got.dense_params[off + 1 + 2 * i]) for i in range(L)])
        off += 1 + 2 * L
    assert len(ops) == 8 and [TIME in o for o in ops] == [False, False, True, False] * 2
    np.testing.assert_allclose(np.array(got.x0, np.float32), np.array(want.x0, np.float32), rtol=1e-6, atol=1e-6)


def test_the_mirror_refuses_plan_integration_of_a_time_reading_model(tmp_path):
    """The refusal of the plan kernels (include/ilqg.h), on the mirror's side: a CHECK that names the subsystem, in front
    of every device call.  (The C ABI's own refusal needs a problem handle: tests/test_gpu_expression_time.py.)"""
    exe = _build_host_program(tmp_path, "time_model_refusal_check", "time_model_refusal_check.cpp")
    done = subprocess.run([exe], text=True, capture_output=True)
    assert done.returncode != 0
    assert "initialized" in done.stdout and "integrated" not in done.stdout
    assert "subsystem 0 is an expression subsystem whose rows read the time (Expr::Time())" in done.stderr
