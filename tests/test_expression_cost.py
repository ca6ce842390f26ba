"""Expression costs (ILQG_COST_EXPRESSION, include/ilqg.h) without a device: what creation refuses, the evaluator
(csrc/ilqg_expr.hpp, through the stand-alone tests/host/expr_check.cpp) against a numpy restatement of the op table and
against finite differences, the row program, and the C++ mirror (ExpressionCost, host::Expr)."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from ilqgames_amd import abi, examples
from ilqgames_amd.abi import Expr
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ilqgames_amd", "csrc")
X, Y, CONST, W, V, ADD, SUB, MUL, DIV, NEG, SQUARE, SQRT, EXP, LOG, SIN, COS, HINGE = range(1, 18)
assert (X, HINGE) == (abi.EXPR_PUSH_X, abi.EXPR_HINGE)


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        entry.build()
    return h


# ------------------------------------------------------------------------------------------------
# the table of include/ilqg.h, restated: every product and sum a numpy scalar operation of the dtype
# ------------------------------------------------------------------------------------------------
def np_jet(program, w, v, x, y, T):
    """-> [f, fx, fy, fxx, fyy, fxy] of the postfix program [(opcode, imm), ...] in the arithmetic of T."""
    one, zero, two, half = T(1), T(0), T(2), T(0.5)
    stack = []
    with np.errstate(all="ignore"):
        for op, imm in program:
            if op == X:
                stack.append([T(x), one, zero, zero, zero, zero])
            elif op == Y:
                stack.append([T(y), zero, one, zero, zero, zero])
            elif op in (CONST, W, V):
                stack.append([T(np.float32(imm)) if op == CONST else T(w if op == W else v), zero, zero, zero, zero, zero])
            elif op in (ADD, SUB):
                b, a = stack.pop(), stack.pop()
                stack.append([p + q if op == ADD else p - q for p, q in zip(a, b)])
            elif op == MUL:
                b, a = stack.pop(), stack.pop()
                stack.append([a[0] * b[0],
                              a[1] * b[0] + a[0] * b[1],
                              a[2] * b[0] + a[0] * b[2],
                              (a[3] * b[0] + a[0] * b[3]) + two * (a[1] * b[1]),
                              (a[4] * b[0] + a[0] * b[4]) + two * (a[2] * b[2]),
                              (a[5] * b[0] + a[0] * b[5]) + (a[1] * b[2] + a[2] * b[1])])
            elif op == DIV:
                b, a = stack.pop(), stack.pop()
                q = a[0] / b[0]
                qx = (a[1] - q * b[1]) / b[0]
                qy = (a[2] - q * b[2]) / b[0]
                stack.append([q, qx, qy,
                              (a[3] - two * (qx * b[1]) - q * b[3]) / b[0],
                              (a[4] - two * (qy * b[2]) - q * b[4]) / b[0],
                              (a[5] - qx * b[2] - qy * b[1] - q * b[5]) / b[0]])
            elif op == HINGE:
                if not stack[-1][0] > zero:
                    stack[-1] = [zero] * 6
            else:
                a = stack.pop()
                f = a[0]
                if op == NEG:
                    g, g1, g2 = -f, T(-1), zero
                elif op == SQUARE:
                    g, g1, g2 = f * f, two * f, two
                elif op == SQRT:
                    g = np.sqrt(f)
                    g1 = half / g
                    g2 = T(-0.5) * g1 / f
                elif op == EXP:
                    g = g1 = g2 = np.exp(f)
                elif op == LOG:
                    g, g1 = np.log(f), one / f
                    g2 = -(g1 * g1)
                elif op == SIN:
                    g, g1, g2 = np.sin(f), np.cos(f), -np.sin(f)
                elif op == COS:
                    g, g1, g2 = np.cos(f), -np.sin(f), -np.cos(f)
                else:
                    raise ValueError(op)
                stack.append([g, g1 * a[1], g1 * a[2],
                              g2 * (a[1] * a[1]) + g1 * a[3],
                              g2 * (a[2] * a[2]) + g1 * a[4],
                              g2 * (a[1] * a[2]) + g1 * a[5]])
    assert len(stack) == 1
    return [T(c) for c in stack[0]]


# ---- test programs: (tree, two inputs, (weight, value), the box the points are drawn from) ----
x_, y_, w_, v_ = Expr.x(), Expr.y(), Expr.weight(), Expr.value()
EXACT = {  # pushes, ADD SUB MUL DIV NEG SQUARE SQRT HINGE only: IEEE operations in the same order round the same
    "quadratic": (0.5 * w_ * (x_ - v_).square(), False, (10.0, 8.0), (-3.0, 12.0)),
    "curvature": (0.5 * w_ * (x_ / y_).square(), True, (20.0, 0.0), (0.5, 9.0)),
    "hinged_norm": (0.5 * w_ * ((x_.square() + y_.square()).sqrt() - v_).hinge().square(), True, (0.5, 4.0), (-6.0, 6.0)),
    "hinged_norm_inside": (0.5 * w_ * (-((x_.square() + y_.square()).sqrt() - v_)).hinge().square(), True, (0.5, 4.0), (-6.0, 6.0)),
    "product": (w_ * x_ * y_ - v_ * x_ / (y_ * y_ + 1.5), True, (3.0, -2.0), (-4.0, 4.0)),
    "rational": ((x_ * x_ - 2.0 * y_) / (1.0 + x_.square() + y_.square()) + (-x_).hinge() * y_, True, (1.0, 1.0), (-3.0, 3.0)),
    "sqrt_chain": ((x_ + 5.0).sqrt() * (y_.square() + 0.25).sqrt() / (w_ + x_ * 0.125), True, (7.0, 0.0), (-2.0, 6.0)),
    "one_input_deep": ((((x_ * 0.5 + 1.0) * x_ - v_) * x_ + w_).square() / (x_.square() + 2.0), False, (0.75, 1.25), (-2.0, 2.0)),
}
SMOOTH = {  # EXP LOG SIN COS, without cancellation
    "gaussian_bump": (w_ * ((x_.square() + y_.square()) * -0.5 / v_.square()).exp(), True, (30.0, 2.0), (-3.0, 3.0)),
    "log1p_square": ((1.0 + x_.square()).log(), False, (1.0, 0.0), (-4.0, 4.0)),
    "sin_cos": (x_.sin() * y_.cos(), True, (1.0, 0.0), (-3.0, 3.0)),
    "log_barrier": (-(w_ * (v_ - x_).log()), False, (2.0, 15.0), (0.0, 10.0)),
}
FD_CASES = dict(EXACT, **SMOOTH)
# away from the kinks of the hinged programs and the zero of their square roots: the finite differences need them smooth
FD_SKIP = {"hinged_norm": lambda x, y: abs(np.hypot(x, y) - 4.0) < 0.1, "hinged_norm_inside": lambda x, y: abs(np.hypot(x, y) - 4.0) < 0.1,
           "rational": lambda x, y: abs(x) < 0.1}


def _points(name, count=20):
    _, two, _, (lo, hi) = FD_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    pts = []
    while len(pts) < count:
        x, y = rng.uniform(lo, hi, 2)
        if name in FD_SKIP and FD_SKIP[name](x, y):
            continue
        pts.append((float(x), float(y) if two else 0.0))
    return pts


def _case_line(dtype, two, w, v, block, pts):
    T = np.float32 if dtype == "f32" else np.float64
    words = ["%r" % float(b) for b in block]
    flat = []
    for x, y in pts:
        flat += [repr(float(T(x))), repr(float(T(y)))]
    return " ".join([dtype, "1" if two else "0", repr(float(w)), repr(float(v)), str(len(block))] + words + [str(len(pts))] + flat)


def _parse(out):
    """-> list of (check triple, [per point dict(jet, grad, value)])."""
    cases = []
    for line in out.splitlines():
        tok = line.split()
        if tok[0] == "check":
            cases.append((tuple(int(t) for t in tok[1:4]), []))
        else:
            vals = [float.fromhex(t) for t in tok if t not in ("jet", "grad", "value", "|")]
            cases[-1][1].append(dict(jet=vals[0:6], grad=vals[6:9], value=vals[9]))
    return cases


def _build_checker(out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off"] + list(extra) +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "host", "expr_check.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(str(tmp_path_factory.mktemp("expr") / "expr_check"))


def _run(exe, lines):
    return _parse(subprocess.run([exe], input="\n".join(lines) + "\n", text=True, capture_output=True, check=True).stdout)


# ------------------------------------------------------------------------------------------------
# the evaluator
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_arithmetic_programs_match_the_numpy_restatement_bit_for_bit(checker, dtype):
    T = np.float32 if dtype == "f32" else np.float64
    names = sorted(EXACT)
    cases = _run(checker, [_case_line(dtype, EXACT[n][1], *EXACT[n][2], abi.expr_block(EXACT[n][0].program()), _points(n))
                           for n in names])
    assert len(cases) == len(names)
    for name, (check, rows) in zip(names, cases):
        tree, two, (w, v), _ = EXACT[name]
        assert check == (0, -1, 1), name
        assert len(rows) == 20
        for (x, y), row in zip(_points(name), rows):
            want = np_jet(tree.program(), T(w), T(v), T(x), T(y), T)
            got = [T(c) for c in row["jet"]]
            assert np.array(got, T).tobytes() == np.array(want, T).tobytes(), (name, x, y, got, want)
            # the gradient-only form and the value-only form compute the same f (fx, fy) as the full jet
            assert np.array(row["grad"], T).tobytes() == np.array(want[:3], T).tobytes(), name
            assert T(row["value"]).tobytes() == T(want[0]).tobytes(), name
        assert any(r["jet"][0] != 0.0 for r in rows), name


def test_transcendental_programs_match_the_numpy_restatement(checker):
    """Each libm call is good to a couple of ulp and at most 64 ops follow: 1e-12 of the jet's largest component."""
    names = sorted(SMOOTH)
    cases = _run(checker, [_case_line("f64", SMOOTH[n][1], *SMOOTH[n][2], abi.expr_block(SMOOTH[n][0].program()), _points(n))
                           for n in names])
    for name, (check, rows) in zip(names, cases):
        tree, two, (w, v), _ = SMOOTH[name]
        assert check == (0, -1, 1), name
        for (x, y), row in zip(_points(name), rows):
            want = np.array(np_jet(tree.program(), w, v, x, y, np.float64))
            err = np.max(np.abs(np.array(row["jet"]) - want)) / np.max(np.abs(want))
            assert err <= 1e-12, (name, x, y, err)
            assert abs(row["value"] - want[0]) <= 1e-12 * np.max(np.abs(want)), name


@pytest.mark.parametrize("name", sorted(FD_CASES))
def test_derivatives_match_central_differences(checker, name):
    """The derivatives are right, not merely self-consistent: central differences of the VALUE program (h = 1e-5, fp64)
    for the gradient and of the jet's gradient for the Hessian, both good to about h^2 + eps / h = 1e-10; the bar is 1e-7
    of the largest entry, at 20 seeded points away from the programs' kinks."""
    tree, two, (w, v), _ = FD_CASES[name]
    block = abi.expr_block(tree.program())
    h = 1e-5
    pts = _points(name)
    shifted = []
    for x, y in pts:
        shifted += [(x, y), (x + h, y), (x - h, y), (x, y + h), (x, y - h)]
    (check, rows), = _run(checker, [_case_line("f64", two, w, v, block, shifted)])
    assert check == (0, -1, 1)
    for q, (x, y) in enumerate(pts):
        at, xp, xm, yp, ym = rows[5 * q:5 * q + 5]
        # the step as the program saw it (x + h is rounded)
        hx = ((x + h) - (x - h)) / 2.0
        hy = ((y + h) - (y - h)) / 2.0
        grad_fd = np.array([(xp["value"] - xm["value"]) / (2 * hx), (yp["value"] - ym["value"]) / (2 * hy) if two else 0.0])
        grad = np.array(at["jet"][1:3])
        hess = np.array(at["jet"][3:6])
        hess_fd = np.array([(xp["jet"][1] - xm["jet"][1]) / (2 * hx),
                            (yp["jet"][2] - ym["jet"][2]) / (2 * hy) if two else 0.0,
                            (yp["jet"][1] - ym["jet"][1]) / (2 * hy) if two else 0.0])
        hess_fd_t = (xp["jet"][2] - xm["jet"][2]) / (2 * hx) if two else 0.0  # d/dx of fy: the same mixed entry
        scale_g = max(np.max(np.abs(grad)), 1e-300)
        scale_h = max(np.max(np.abs(hess)), 1e-300)
        assert np.max(np.abs(grad - grad_fd)) <= 1e-7 * scale_g, (name, x, y, grad, grad_fd)
        assert np.max(np.abs(hess - hess_fd)) <= 1e-7 * scale_h, (name, x, y, hess, hess_fd)
        assert abs(hess[2] - hess_fd_t) <= 1e-7 * scale_h, (name, x, y)
        if not two:
            assert at["jet"][2] == 0.0 and at["jet"][4] == 0.0 and at["jet"][5] == 0.0


# ---- malformed programs: (block words, two inputs, ExprFault, op at fault) ----
MALFORMED = [
    ([0.0], True, 1, -1),                                   # L = 0
    ([65.0] + [float(X), 0.0] * 65, True, 1, -1),           # L = 65
    ([1.5, float(X), 0.0, float(X), 0.0], True, 1, -1),     # L not whole
    (["nan", float(X), 0.0], True, 1, -1),                  # L not a number
    ([3.0, float(X), 0.0, float(X), 0.0], True, 2, -1),     # the block ends inside the program
    ([2.0, float(X), 0.0, 99.0, 0.0], True, 3, 1),          # unknown opcode
    ([2.0, float(X), 0.0, 0.0, 0.0], True, 3, 1),           # opcode 0
    ([2.0, float(X), 0.0, 6.5, 0.0], True, 3, 1),           # opcode not whole
    ([2.0, float(X), 0.0, float(ADD), 0.0], True, 4, 1),    # binary op on one entry
    ([1.0, float(SQUARE), 0.0], True, 4, 0),                # unary op on an empty stack
    ([5.0] + [float(X), 0.0] * 5, True, 5, 4),              # a fifth entry
    ([2.0, float(X), 0.0, float(Y), 0.0], True, 6, -1),     # two entries left
    ([1.0, float(Y), 0.0], False, 7, 0),                    # PUSH_Y without a second input
]


def _malformed_lines():
    return [" ".join(["f64", "1" if two else "0", "1.0", "1.0", str(len(blk))] + [str(b) for b in blk] + ["1", "0.5", "0.25"])
            for blk, two, _, _ in MALFORMED] + ["f64 1 1.0 1.0 0 0"]  # ... and no block at all


def test_validator_rejects_malformed_programs(checker):
    cases = _run(checker, _malformed_lines())
    assert len(cases) == len(MALFORMED) + 1
    for (blk, two, fault, op), (check, rows) in zip(MALFORMED, cases):
        assert check[0] == fault and check[1] == op, (blk, check)
        assert rows == []
    assert cases[-1][0][0] == 2
    assert cases[2][0] != (0, -1, 1)


def test_stand_alone_checker_is_clean_under_the_host_sanitizers(tmp_path):
    """The same host program once with AddressSanitizer and UBSan, over every well-formed and malformed program: every
    block sits in an allocation of exactly its size."""
    exe = _build_checker(str(tmp_path / "expr_check_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    lines = [_case_line(dt, FD_CASES[n][1], *FD_CASES[n][2], abi.expr_block(FD_CASES[n][0].program()), _points(n, 4))
             for n in sorted(FD_CASES) for dt in ("f64", "f32")] + _malformed_lines()
    done = subprocess.run([exe], input="\n".join(lines) + "\n", text=True, capture_output=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr
    assert len(_parse(done.stdout)) == len(lines)


def test_depth_and_length_limits_are_the_abi_s():
    deep = x_ + (x_ + (x_ + (x_ + x_)))  # operands left to right: five entries
    depth = peak = 0
    for op, _ in deep.program():
        depth += 1 if op <= V else (-1 if op <= DIV else 0)
        peak = max(peak, depth)
    assert peak == abi.EXPR_MAX_DEPTH + 1
    assert (abi.EXPR_MAX_OPS, abi.EXPR_MAX_DEPTH) == (64, 4) and abi.COST_EXPRESSION == 24


# ------------------------------------------------------------------------------------------------
# what creation refuses
# ------------------------------------------------------------------------------------------------
def _scene_with(program, dims=(0, 1), **kw):
    """The skeleton example with one expression cost of player 0 appended -> (spec, its term index)."""
    s = examples.skeleton(T=12)
    return s, s.expression(0, program, dims, **kw)


def _refused(hip, spec, term, patch_desc=None):
    """(status, message) of ilqg_expression_check, and of the host half of ilqg_problem_create, which must agree."""
    import ctypes as C
    desc, keep = spec.build(abi.F64)
    if patch_desc is not None:
        patch_desc(desc)
    rc = hip.lib().ilqg_expression_check(C.byref(desc), term)
    msg = hip.lib().ilqg_last_error().decode() if rc else ""
    n, sid = C.c_int32(0), C.c_int32(0)
    rc2 = hip.lib().ilqg_row_program_build(C.byref(desc), None, 0, C.byref(n), C.byref(sid))
    msg2 = hip.lib().ilqg_last_error().decode() if rc2 else ""
    del keep
    assert (rc, msg) == (rc2, msg2)
    return rc, msg


OKP = [(X, 0.0), (Y, 0.0), (MUL, 0.0)]


def _raw(words, dims=(0, 1), **kw):
    """A scene whose expression term's block is the given words, whatever they are."""
    s = examples.skeleton(T=12)
    off = len(s.dense_params)
    s.dense_params += [float(w) for w in words]
    role = kw.pop("role", abi.ROLE_STATE_COST)
    t = s._term(abi.COST_EXPRESSION, role, 0, kw.pop("arg", -1), (dims[0], dims[1], -1, -1), 1.0, 0.0, 0, off)
    return s, t


def test_creation_refuses_malformed_expression_terms(hip):
    def refusal(made, patch=None):
        spec, term = made
        return _refused(hip, spec, term, patch)

    cases = [
        (_scene_with(OKP, role=abi.ROLE_STATE_CONSTRAINT), abi.ERR_UNSUPPORTED, "a constraint role is not supported"),
        (_scene_with(OKP, role=abi.ROLE_CONTROL_CONSTRAINT, control_of=0), abi.ERR_UNSUPPORTED, "a constraint role is not supported"),
        (_scene_with(OKP, role=abi.ROLE_CHILD), abi.ERR_UNSUPPORTED, "cannot be an EXTREME_VALUE child"),
        (_raw([99.0, 1.0, 0.0]), abi.ERR_INVALID, "program length L must be a whole number in 1 .. 64"),
        (_raw([0.0]), abi.ERR_INVALID, "program length L must be a whole number in 1 .. 64"),
        (_raw([3.0, X, 0.0, Y, 0.0]), abi.ERR_INVALID, "program block is out of range of ilqg_problem_desc::dense_params"),
        (_raw([2.0, X, 0.0, 42.0, 0.0]), abi.ERR_UNSUPPORTED, "op 1: unknown opcode"),
        (_raw([2.0, X, 0.0, MUL, 0.0]), abi.ERR_INVALID, "op 1: stack underflow"),
        (_raw([5.0] + [X, 0.0] * 5), abi.ERR_UNSUPPORTED, "op 4: stack overflow"),
        (_raw([2.0, X, 0.0, Y, 0.0]), abi.ERR_INVALID, "ends with 2 entries on the stack"),
        (_raw([1.0, X, 0.0], dims=(10, -1)), abi.ERR_INVALID, "idx[0] = 10 is outside its argument vector (dimension 10)"),
        (_raw([1.0, X, 0.0], dims=(-1, -1)), abi.ERR_INVALID, "idx[0] = -1 is outside"),
        (_raw([1.0, X, 0.0], dims=(3, 3)), abi.ERR_INVALID, "idx[0] and idx[1] name the same entry"),
        (_raw([1.0, X, 0.0], dims=(3, 12)), abi.ERR_INVALID, "idx[1] = 12 is neither -1 nor inside"),
        (_raw([1.0, X, 0.0], dims=(2, -1), role=abi.ROLE_CONTROL_COST, arg=0), abi.ERR_INVALID, "idx[0] = 2 is outside its argument vector (dimension 2)"),
        (_raw([1.0, Y, 0.0], dims=(3, -1)), abi.ERR_INVALID, "op 0: PUSH_Y in a program without a second input"),
    ]
    for made, status, fragment in cases:
        rc, msg = refusal(made)
        assert rc == status and fragment in msg, (fragment, rc, msg)
        assert ("expression term %d" % made[1]) in msg, msg

    def past_the_end(desc):
        desc.terms[desc.num_terms - 1].polyline = desc.num_dense_params
    rc, msg = refusal(_raw([1.0, X, 0.0]), past_the_end)
    assert rc == abi.ERR_INVALID and "program block is out of range" in msg

    def negative(desc):
        desc.terms[desc.num_terms - 1].polyline = -1
    rc, msg = refusal(_raw([1.0, X, 0.0]), negative)
    assert rc == abi.ERR_INVALID and "program block is out of range" in msg


def test_an_expression_under_an_extreme_value_parent_is_refused(hip):
    s = examples.skeleton(T=12)
    s.extreme_value(0, [lambda role: s.expression(0, OKP, (0, 1), role=abi.ROLE_STATE_COST),
                        lambda role: s.quadratic(0, 1.0, 0)], True)
    rc, msg = _refused(hip, s, len(s.terms) - 3)
    assert rc == abi.ERR_UNSUPPORTED and "cannot be an EXTREME_VALUE child" in msg


def test_well_formed_expression_terms_are_accepted_with_their_instance_parameters(hip):
    spec = examples.expression_scene(T=12)
    for name in ("p1_bump", "p2_speed_barrier", "p2_acceleration_cap"):
        hip.expression_check(spec, spec.term_index(name))
    hip.row_program_build(spec)
    hip.instance_params_check(spec, [("p1_bump", "weight"), ("p1_bump", "value"), ("p2_speed_barrier", "value")])
    import ctypes as C
    desc, keep = spec.build(abi.F64)
    rc = hip.lib().ilqg_expression_check(C.byref(desc), 0)  # a QuadraticCost
    assert rc == abi.ERR_INVALID and "is not an ILQG_COST_EXPRESSION term" in hip.lib().ilqg_last_error().decode()
    del keep


# ------------------------------------------------------------------------------------------------
# the row program
# ------------------------------------------------------------------------------------------------
RP_MAX_LSLOTS, RP_OFF_OPS, RP_OFF_SIDS, RP_OFF_COMPACT = 2, 4, 5, 13
ROP_WORDS, RO_MODE, RO_NSID, RO_KIND, RO_POLY_FIRST, RO_PATTERN = 40, 0, 2, 4, 14, 19
STACK_SLOTS = (abi.EXPR_MAX_DEPTH - 1) * 6


def _ops(words):
    n = (words[RP_OFF_SIDS] - words[RP_OFF_OPS]) // ROP_WORDS
    return [words[words[RP_OFF_OPS] + q * ROP_WORDS:words[RP_OFF_OPS] + (q + 1) * ROP_WORDS] for q in range(n)]


def test_row_program_gives_an_expression_its_pattern_entries_and_counts_its_stack(hip):
    spec = examples.expression_scene(T=12)
    words, static_id = hip.row_program_build(spec)
    assert static_id == 0, "an expression scene matches no registered structure: the row stage interprets it"
    ops = [o for o in _ops(words) if o[RO_KIND] == abi.COST_EXPRESSION]
    assert [(o[RO_MODE], o[RO_NSID], o[RO_PATTERN]) for o in ops] == [(0, 6, 2), (0, 2, 1), (0, 2, 1)]  # TERM; PAIR2, SINGLE
    # each op carries the offset of its program in the dense table: the blocks follow one another
    lengths = [1 + 2 * int(spec.dense_params[spec.terms[spec.term_index(n)]["polyline"]]) for n in ("p1_bump", "p2_speed_barrier")]
    assert [o[RO_POLY_FIRST] for o in ops] == [0, lengths[0], lengths[0] + lengths[1]]
    # the stack's lower entries are counted into the scratch behind the widest pass, and keep nothing off the compact rows
    plain = examples.expression_scene(T=12)
    plain.terms = [dict(t, kind=abi.COST_QUADRATIC, polyline=-1, idx=(t["idx"][0], 0, 0, 0)) if t["kind"] == abi.COST_EXPRESSION and
                   t["idx"][1] < 0 else (dict(t, kind=abi.COST_QUADRATIC_NORM, polyline=-1) if t["kind"] == abi.COST_EXPRESSION else t)
                   for t in plain.terms]
    plain_words, _ = hip.row_program_build(plain)
    assert words[RP_MAX_LSLOTS] == plain_words[RP_MAX_LSLOTS] + STACK_SLOTS
    assert words[words[RP_OFF_COMPACT]] == plain_words[plain_words[RP_OFF_COMPACT]] > 0


def test_row_programs_of_scenes_without_expression_terms_are_unchanged(hip):
    """Word for word what the library built before it knew the kind (tests/golden/row_programs.npz)."""
    golden = np.load(os.path.join(GOLDEN, "row_programs.npz"))
    names = [k for k in golden.files if not k.endswith("__static_id")]
    assert len(names) == 8
    for name in names:
        words, static_id = hip.row_program_build(examples.CONFIGS[name]())
        assert np.array_equal(words, golden[name]), name
        assert static_id == int(golden[name + "__static_id"]), name


# ------------------------------------------------------------------------------------------------
# the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_expression_scene_flattens_like_examples_py(tmp_path):
    entry.build_host()
    exe = str(tmp_path / "dump_expression_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + entry.host_compile_flags() +
                          ['-DEXAMPLE_HEADER="expression_scene.h"', "-DEXAMPLE_CLASS=ExpressionScene",
                           "-I" + os.path.join(ROOT, "tests", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "dump_example.cpp")] + entry.host_link_flags())
    got = abi.ProblemSpec.from_dump(subprocess.check_output([exe], text=True))
    want = examples.expression_scene()
    g, w = got.canonical(), want.canonical()
    for key in ("subsystems", "player_costs", "pairs", "T", "dt"):
        assert g[key] == w[key], key
    assert set(g["groups"]) == set(w["groups"])
    for key in w["groups"]:
        assert g["groups"][key] == w["groups"][key], key
    blocks = [t for grp in w["groups"].values() for t in grp if t[0] == abi.COST_EXPRESSION]
    assert len(blocks) == 3 and all(len(t[6]) == 1 + 2 * int(t[6][0]) for t in blocks)
    # the dense table itself: the three programs in term order, nothing else
    assert [np.float32(v) for v in got.dense_params] == [np.float32(v) for v in want.dense_params]
    np.testing.assert_allclose(np.array(got.x0, np.float32), np.array(want.x0, np.float32), rtol=1e-6, atol=1e-6)
