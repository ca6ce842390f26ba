"""Expression dynamics (ILQG_DYN_EXPRESSION, ILQG_DYN_ROW_EXPRESSION, include/ilqg.h) without a device: the header, what
creation refuses and accepts, the row program's Jacobian pass, the rules of the kind (through the stand-alone
tests/host/expr_dyn_check.cpp, over csrc/ilqg_expr.hpp) against analytic Jacobians, central differences and a numpy
integrator, and the C++ mirror (SinglePlayerExpressionSystem)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from ilqgames_amd import abi, examples
from ilqgames_amd.abi import Expr
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ilqgames_amd", "csrc")
X, Y, CONST, W, V, ADD, SUB, MUL = range(1, 9)
T12 = 12


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        entry.build()
    return h


# ------------------------------------------------------------------------------------------------
# the header
# ------------------------------------------------------------------------------------------------
def test_header_declares_the_enumerators_and_keeps_every_layout(tmp_path):
    text = open(os.path.join(ROOT, "include", "ilqg.h")).read()
    for name, value in (("ILQG_DYN_EXPRESSION", 13), ("ILQG_ROLE_DYNAMICS_ROW", 5), ("ILQG_DYN_ROW_EXPRESSION", 26)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    assert re.search(r"#define ILQG_ABI_VERSION 9\b", text) and abi.ABI_VERSION == 9
    assert (abi.DYN_EXPRESSION, abi.ROLE_DYNAMICS_ROW, abi.DYN_ROW_EXPRESSION) == (13, 5, 26)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ilqg.h"\nint main(void) { printf("%zu %zu %zu %d %d %d %d\\n", '
                   "sizeof(ilqg_subsystem), sizeof(ilqg_cost_term), sizeof(ilqg_problem_desc), ILQG_ABI_VERSION, "
                   "(int)ILQG_DYN_EXPRESSION, (int)ILQG_ROLE_DYNAMICS_ROW, (int)ILQG_DYN_ROW_EXPRESSION); return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(abi.Subsystem), C.sizeof(abi.CostTerm), C.sizeof(abi.ProblemDesc), 9, 13, 5, 26]


# ------------------------------------------------------------------------------------------------
# what creation refuses, and what it accepts
# ------------------------------------------------------------------------------------------------
def _refused(hip, spec, term=None, patch_desc=None):
    """(status, message) of the host half of ilqg_problem_create; with `term`, ilqg_expression_check must agree."""
    desc, keep = spec.build(abi.F64)
    if patch_desc is not None:
        patch_desc(desc)
    n, sid = C.c_int32(0), C.c_int32(0)
    rc = hip.lib().ilqg_row_program_build(C.byref(desc), None, 0, C.byref(n), C.byref(sid))
    msg = hip.lib().ilqg_last_error().decode() if rc else ""
    if term is not None:
        rc2 = hip.lib().ilqg_expression_check(C.byref(desc), term)
        msg2 = hip.lib().ilqg_last_error().decode() if rc2 else ""
        assert (rc, msg) == (rc2, msg2)
    del keep
    return rc, msg


def _row_term(spec, player, row):
    return next(q for q, t in enumerate(spec.terms)
                if t["kind"] == abi.DYN_ROW_EXPRESSION and t["player"] == player and t["idx"][0] == row)


def _coasting(**change):
    """coasting_car_scene with fields of player 1's heading row (row 2: X = v, Y = kappa) changed -> (spec, that term)."""
    s = examples.coasting_car_scene(T=T12)
    t = _row_term(s, 1, 2)
    s.terms[t].update(change)
    return s, t


def _coasting_block(words, **change):
    s, t = _coasting(**change)
    s.terms[t]["polyline"] = len(s.dense_params)
    s.dense_params += [float(w) for w in words]
    return s, t


def test_creation_refuses_malformed_expression_subsystems(hip):
    where = "(subsystem 1, row 2)"
    cases = [
        (_coasting(idx=(2, 5, 4, -1)), abi.ERR_INVALID, "input X = 5 is outside the subsystem's [x | u] (dimension 5)"),
        (_coasting(idx=(2, -1, 4, -1)), abi.ERR_INVALID, "input X = -1 is outside"),
        (_coasting(idx=(2, 3, 7, -1)), abi.ERR_INVALID, "input Y = 7 is neither -1 nor inside"),
        (_coasting(idx=(2, 3, 3, -1)), abi.ERR_INVALID, "inputs X and Y name the same entry"),
        (_coasting(idx=(2, 3, -1, -1)), abi.ERR_INVALID, "op 1: PUSH_Y in a program without a second input"),
        (_coasting(idx=(2, 3, 4, 0)), abi.ERR_INVALID, "idx[3] must be -1"),
        (_coasting(first_step=3), abi.ERR_UNSUPPORTED, "first_step = 3: a dynamics row cannot be gated"),
        (_coasting(constraint_slot=0), abi.ERR_INVALID, "arg and constraint_slot must be -1"),
        (_coasting_block([99.0, X, 0.0]), abi.ERR_INVALID, "program length L must be a whole number in 1 .. 64"),
        (_coasting_block([3.0, X, 0.0, Y, 0.0]), abi.ERR_INVALID, "program block is out of range of ilqg_problem_desc::dense_params"),
        (_coasting_block([2.0, X, 0.0, 42.0, 0.0]), abi.ERR_UNSUPPORTED, "op 1: unknown opcode"),
        (_coasting_block([2.0, X, 0.0, MUL, 0.0]), abi.ERR_INVALID, "op 1: stack underflow"),
        (_coasting_block([5.0] + [X, 0.0] * 5), abi.ERR_UNSUPPORTED, "op 4: stack overflow"),
        (_coasting_block([2.0, X, 0.0, Y, 0.0]), abi.ERR_INVALID, "ends with 2 entries on the stack"),
    ]
    for (spec, term), status, fragment in cases:
        rc, msg = _refused(hip, spec, term)
        assert rc == status and fragment in msg, (fragment, rc, msg)
        assert where in msg and ("dynamics-row term %d" % term) in msg, msg

    # a row defined twice; a row outside the subsystem; a missing row
    s, t = _coasting(idx=(1, 3, 4, -1))
    rc, msg = _refused(hip, s, t)
    assert rc == abi.ERR_INVALID and "(subsystem 1, row 1)" in msg and "the row is defined twice (also by term %d)" % _row_term(s, 1, 1) in msg
    s, t = _coasting(idx=(4, 3, 4, -1))
    rc, msg = _refused(hip, s, t)
    assert rc == abi.ERR_INVALID and "(subsystem 1, row 4)" in msg and "the row lies outside the subsystem's 4 states" in msg
    s = examples.coasting_car_scene(T=T12)
    del s.terms[_row_term(s, 0, 3)]
    rc, msg = _refused(hip, s)
    assert rc == abi.ERR_INVALID and "subsystem 0, row 3" in msg and "has no ILQG_DYN_ROW_EXPRESSION term" in msg

    # a row term on a subsystem of another kind; the kind and the role only occur together
    s = examples.delayed_dubins_scene(T=T12)
    t = s.dynamics_row(1, 0, Expr.x(), 3)
    rc, msg = _refused(hip, s, t)
    assert rc == abi.ERR_INVALID and "(subsystem 1, row 0)" in msg and "the subsystem is not an expression subsystem" in msg
    s, t = _coasting(role=abi.ROLE_STATE_COST)
    rc, msg = _refused(hip, s, t)
    assert rc == abi.ERR_INVALID and "only occur together" in msg

    # dimensions outside the limits
    for xdim, udim in ((9, 1), (0, 1), (4, 3), (4, 0)):
        s = abi.ProblemSpec(T12, 0.1)
        s.add_expression_player(xdim, udim, [(Expr.x(), 0, None)] * xdim)
        s.quadratic(0, 1.0, 0, 0.0, control_of=0)
        rc, msg = _refused(hip, s)
        assert rc == abi.ERR_UNSUPPORTED and "subsystem 0" in msg and "1 .. 8 states and 1 or 2 controls" in msg, (xdim, udim, msg)

    # beside a paired kind, and in a point-mass game
    for other in (abi.DYN_PLANAR_DISTURBANCE, abi.DYN_AIR_3D_PURSUER, abi.DYN_POINT_MASS_2D):
        s = abi.ProblemSpec(T12, 0.1)
        s.add_expression_player(2, 1, [(Expr.x(), 1, None), (Expr.x(), 2, None)])
        s.add_player(other)
        for i in range(2):
            s.quadratic(i, 1.0, 0, 0.0, control_of=i)
        rc, msg = _refused(hip, s)
        assert rc == abi.ERR_UNSUPPORTED and "subsystem 0: an expression subsystem (kind 13) does not occur beside" in msg, msg

    # a per-instance cost parameter on a dynamics-row term
    s = examples.coasting_car_scene(T=T12)
    for field in ("weight", "value"):
        with pytest.raises(hip.IlqgError) as e:
            hip.instance_params_check(s, [(_row_term(s, 0, 2), field)])
        assert e.value.status == abi.ERR_UNSUPPORTED and "DYN_ROW_EXPRESSION" in str(e.value) and "a dynamics row is no cost term" in str(e.value)


TWIN_SCENES = {  # scene -> the built-in kinds its twin restates
    "delayed_dubins_scene": {abi.DYN_DELAYED_DUBINS_CAR},
    "dynamics_zoo_scene": {abi.DYN_CAR_7D, abi.DYN_UNICYCLE_5D},
    "mixed_dubins_car_scene": {abi.DYN_DUBINS_CAR, abi.DYN_CAR_5D},
    "three_unicycle_scene": {abi.DYN_UNICYCLE_4D},
}


def test_well_formed_expression_subsystems_are_accepted(hip):
    covered = set()
    for name, kinds in TWIN_SCENES.items():
        spec = getattr(examples, name)(T=T12)
        twin, restated = examples.expression_dynamics_twin(spec)
        present = {s[0] for s in spec.subsystems}
        assert kinds <= present and restated == sum(1 for s in spec.subsystems if examples.expression_model_rows(s[0]))
        covered |= kinds & present
        assert twin.terms[:len(spec.terms)] == spec.terms, "term indices stay what they were"
        hip.row_program_build(twin)
        for t in range(len(spec.terms), len(twin.terms)):
            hip.expression_check(twin, t)
        rows = [i for i, s in enumerate(twin.subsystems) if s[0] == abi.DYN_EXPRESSION]
        hip.instance_subsystem_params_check(twin, rows)
    assert covered == {abi.DYN_UNICYCLE_4D, abi.DYN_DUBINS_CAR, abi.DYN_DELAYED_DUBINS_CAR, abi.DYN_UNICYCLE_5D, abi.DYN_CAR_5D,
                       abi.DYN_CAR_7D}
    s = examples.coasting_car_scene(T=T12)
    hip.row_program_build(s)
    for i in range(2):
        for r in range(4):
            hip.expression_check(s, _row_term(s, i, r))
    hip.instance_subsystem_params_check(s, [0, 1])
    hip.instance_params_check(s, [("p1_proximity", "weight"), ("p2_follow", "weight")])


# ------------------------------------------------------------------------------------------------
# the row program
# ------------------------------------------------------------------------------------------------
RP_NUM_PSLOTS, RP_MAX_LSLOTS, RP_OFF_PASS, RP_OFF_OPS, RP_OFF_SIDS, RP_OFF_PINIT, RP_OFF_REGIONS, RP_OFF_MAPS = 1, 2, 3, 4, 5, 6, 8, 9
ROP_WORDS, RO_MODE, RO_NSID, RO_KIND, ROP_JACOBIAN = 40, 0, 2, 4, 3
RPASS_WORDS, RREG_WORDS, RINIT_WORDS, RA_A, RA_B = 9, 4, 2, 0, 1
STACK_SLOTS = (abi.EXPR_MAX_DEPTH - 1) * 6


def _jacobian_maps(words, n, m):
    """-> ({(r, c): tag} of A, the same of B, the pass's slot count) of the program's pass 0; tag: "one", "dt", "-dt", a
    literal, or "computed"."""
    words = [int(w) for w in words]
    nps = words[RP_NUM_PSLOTS]
    p0 = words[words[RP_OFF_PASS]:words[RP_OFF_PASS] + RPASS_WORDS]
    reg_begin, reg_end, nl = p0[2], p0[3], p0[5]
    maps = words[words[RP_OFF_MAPS]:]

    def slot(at):
        word = maps[at // 2] & 0xffffffff
        return (word >> 16) & 0xffff if at & 1 else word & 0xffff

    def tag(s):
        if s >= nps:
            return "computed"
        code, bits = words[words[RP_OFF_PINIT] + s * RINIT_WORDS], words[words[RP_OFF_PINIT] + s * RINIT_WORDS + 1]
        kind = code & 255
        if kind == 2:
            return "dt"
        if kind == 3:
            return "-dt"
        return float(np.array([bits & 0xffffffff], np.uint32).view(np.float32)[0])

    out = {}
    for rg in range(reg_begin, reg_end):
        arr, count, offs, mo = words[words[RP_OFF_REGIONS] + rg * RREG_WORDS:words[RP_OFF_REGIONS] + (rg + 1) * RREG_WORDS]
        assert arr in (RA_A, RA_B) and offs == 0
        cols = n if arr == RA_A else m
        assert count == n * cols
        out[arr] = {(w % n, w // n): tag(slot(mo + w)) for w in range(count)}
    return out[RA_A], out[RA_B], nl


def _ri_codes_are_what_the_decoder_assumes():
    text = open(os.path.join(CSRC, "ilqg_rows.hpp")).read()
    return (re.search(r"enum\s*\{\s*RI_VALUE\s*=\s*0\s*,\s*RI_DT\s*=\s*2\s*,\s*RI_NEG_DT\s*=\s*3", text) is not None and
            re.search(r"RP_OFF_REGIONS,\s*RP_OFF_MAPS,", text) is not None)


def test_the_decoder_reads_the_row_program_s_layout():
    assert _ri_codes_are_what_the_decoder_assumes()


@pytest.mark.parametrize("scene", sorted(TWIN_SCENES))
def test_a_twin_s_jacobian_pass_has_the_built_in_s_constants_and_computed_entries(hip, scene):
    spec = getattr(examples, scene)(T=T12)
    twin, _ = examples.expression_dynamics_twin(spec)
    a0, b0, _ = _jacobian_maps(hip.row_program_build(spec)[0], spec.n, spec.m)
    a1, b1, _ = _jacobian_maps(hip.row_program_build(twin)[0], spec.n, spec.m)
    assert a0 == a1 and b0 == b1
    assert "computed" in a0.values() and "dt" in b0.values() and all(a0[(i, i)] == 1.0 for i in range(spec.n))


def test_the_coasting_car_s_jacobian_pass(hip):
    spec = examples.coasting_car_scene(T=T12)
    words, static_id = hip.row_program_build(spec)
    assert static_id == 0
    A, B, nl = _jacobian_maps(words, 8, 2)
    want_a, want_b = {}, {}
    for i in range(2):
        o = 4 * i
        for rc in ((0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (3, 3)):
            want_a[(o + rc[0], o + rc[1])] = "computed"
        want_b[(o + 2, i)] = "computed"
        for d in range(3):
            want_a[(o + d, o + d)] = 1.0
    assert {k: v for k, v in A.items() if v != 0.0} == want_a
    assert {k: v for k, v in B.items() if v != 0.0} == want_b
    assert nl == 14
    # one Jacobian op per row, with one or two slots; their jets' stack is counted into the scratch
    words = [int(w) for w in words]
    nops = (words[RP_OFF_SIDS] - words[RP_OFF_OPS]) // ROP_WORDS
    ops = [words[words[RP_OFF_OPS] + q * ROP_WORDS:words[RP_OFF_OPS] + (q + 1) * ROP_WORDS] for q in range(nops)]
    jac = [o for o in ops if o[RO_MODE] == ROP_JACOBIAN]
    assert [(o[RO_KIND], o[RO_NSID]) for o in jac] == [(abi.DYN_EXPRESSION, 2)] * 3 + [(abi.DYN_EXPRESSION, 1)] + \
        [(abi.DYN_EXPRESSION, 2)] * 3 + [(abi.DYN_EXPRESSION, 1)]
    assert words[RP_MAX_LSLOTS] >= nl + STACK_SLOTS
    # the same game on a built-in model with as few computed entries needs that much less: the stack is what is added
    plain = examples.delayed_dubins_scene(T=T12)
    _, _, nl_plain = _jacobian_maps(hip.row_program_build(plain)[0], 8, 2)
    assert nl_plain == 4


def test_row_programs_of_the_existing_scenes_are_unchanged(hip):
    golden = np.load(os.path.join(GOLDEN, "row_programs.npz"))
    names = [k for k in golden.files if not k.endswith("__static_id")]
    assert len(names) == 8
    for name in names:
        words, static_id = hip.row_program_build(examples.CONFIGS[name]())
        assert np.array_equal(words, golden[name]), name
        assert static_id == int(golden[name + "__static_id"]), name


# ------------------------------------------------------------------------------------------------
# the rules of the kind, on the host alone
# ------------------------------------------------------------------------------------------------
DT = 0.1


def _build_checker(out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off"] + list(extra) +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "host", "expr_dyn_check.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(str(tmp_path_factory.mktemp("exprdyn") / "expr_dyn_check"))


def _model_text(xdim, udim, rows, param, pts, weights=None):
    lines = ["model %d %d %r %r" % (xdim, udim, float(param), DT)]
    for r, (tree, xin, yin) in enumerate(rows):
        block = abi.expr_block(tree.program() if isinstance(tree, Expr) else tree)
        lines.append(" ".join(["row", str(xin), str(-1 if yin is None else yin), repr(1.0 if weights is None else weights[r]),
                               str(len(block))] + [repr(float(b)) for b in block]))
    lines.append("points %d" % len(pts))
    lines += [" ".join(repr(float(v)) for v in p) for p in pts]
    return "\n".join(lines) + "\n"


def _parse(out, xdim, udim):
    checks, pts = [], []
    for line in out.splitlines():
        tok = line.split()
        if tok[0] == "check":
            checks.append(tuple(int(t) for t in tok[1:5]))
            continue
        vals = [float.fromhex(t) for t in tok if t not in ("rate", "A", "B", "step", "|")]
        a0, b0, s0 = xdim, xdim + xdim * xdim, xdim + xdim * xdim + xdim * udim
        pts.append(dict(rate=np.array(vals[:a0]), A=np.array(vals[a0:b0]).reshape(xdim, xdim),
                        B=np.array(vals[b0:s0]).reshape(xdim, udim), step=np.array(vals[s0:])))
    return checks, pts


def _run(exe, text, xdim, udim):
    return _parse(subprocess.run([exe], input=text, text=True, capture_output=True, check=True).stdout, xdim, udim)


def coasting_rates(x, u, c):
    return np.array([x[3] * np.cos(x[2]), x[3] * np.sin(x[2]), x[3] * u[0], -(c * (x[3] * x[3]))])


def _analytic(kind, x, u, p):
    """(xdot, J_x, J_u) of a model, written out by hand."""
    n, m = len(x), len(u)
    Jx, Ju = np.zeros((n, n)), np.zeros((n, m))
    if kind == "coasting":
        f = coasting_rates(x, u, p)
        Jx[0, 2], Jx[0, 3] = -x[3] * np.sin(x[2]), np.cos(x[2])
        Jx[1, 2], Jx[1, 3] = x[3] * np.cos(x[2]), np.sin(x[2])
        Jx[2, 3], Ju[2, 0] = u[0], x[3]
        Jx[3, 3] = -2.0 * p * x[3]
        return f, Jx, Ju
    if kind in (abi.DYN_UNICYCLE_4D, abi.DYN_UNICYCLE_5D):
        f = [x[3] * np.cos(x[2]), x[3] * np.sin(x[2]), u[0], u[1]] + ([x[3]] if n == 5 else [])
        Jx[0, 2], Jx[0, 3], Jx[1, 2], Jx[1, 3] = -x[3] * np.sin(x[2]), np.cos(x[2]), x[3] * np.cos(x[2]), np.sin(x[2])
        Ju[2, 0] = Ju[3, 1] = 1.0
        if n == 5:
            Jx[4, 3] = 1.0
        return np.array(f), Jx, Ju
    if kind in (abi.DYN_DUBINS_CAR, abi.DYN_DELAYED_DUBINS_CAR):
        f = [p * np.cos(x[2]), p * np.sin(x[2])] + ([u[0]] if n == 3 else [x[3], u[0]])
        Jx[0, 2], Jx[1, 2] = -p * np.sin(x[2]), p * np.cos(x[2])
        if n == 3:
            Ju[2, 0] = 1.0
        else:
            Jx[2, 3], Ju[3, 0] = 1.0, 1.0
        return np.array(f), Jx, Ju
    assert kind in (abi.DYN_CAR_5D, abi.DYN_CAR_7D)
    f = [x[4] * np.cos(x[2]), x[4] * np.sin(x[2]), (x[4] / p) * np.tan(x[3]), u[0], u[1]]
    Jx[0, 2], Jx[0, 4], Jx[1, 2], Jx[1, 4] = -x[4] * np.sin(x[2]), np.cos(x[2]), x[4] * np.cos(x[2]), np.sin(x[2])
    Jx[2, 3], Jx[2, 4] = x[4] / (p * np.cos(x[3]) ** 2), np.tan(x[3]) / p
    Ju[3, 0] = Ju[4, 1] = 1.0
    if n == 7:
        f += [u[0] / (np.cos(x[3]) ** 2 * p), x[4]]
        Jx[5, 3], Ju[5, 0] = 2.0 * u[0] * np.tan(x[3]) / (np.cos(x[3]) ** 2 * p), 1.0 / (np.cos(x[3]) ** 2 * p)
        Jx[6, 4] = 1.0
    return np.array(f), Jx, Ju


COASTING_ROWS = [(Expr.y() * Expr.x().cos(), 2, 3), (Expr.y() * Expr.x().sin(), 2, 3), (Expr.x() * Expr.y(), 3, 4),
                 (-(Expr.value() * Expr.x().square()), 3, None)]
MODELS = {"coasting": (4, 1, COASTING_ROWS, float(np.float32(examples.COASTING_CAR_DRAG)))}  # param0 is a float
for _kind, _p in ((abi.DYN_UNICYCLE_4D, 0.0), (abi.DYN_DUBINS_CAR, 1.5), (abi.DYN_DELAYED_DUBINS_CAR, 2.0), (abi.DYN_UNICYCLE_5D, 0.0),
                  (abi.DYN_CAR_5D, 4.0), (abi.DYN_CAR_7D, 3.0)):
    MODELS[_kind] = examples.expression_model_rows(_kind) + (_p,)


def _model_points(key, count=12):
    xdim, udim = MODELS[key][:2]
    rng = np.random.default_rng(100 + len(str(key)) + xdim * 7 + udim)
    pts = rng.uniform(-1.0, 1.0, (count, xdim + udim))
    pts[:, 2] *= 3.0  # headings all around; steering angles stay inside (-1, 1) rad
    return pts


@pytest.mark.parametrize("key", list(MODELS), ids=[str(k) for k in MODELS])
def test_rates_and_linearisation_match_analytic_jacobians_and_central_differences(checker, key):
    """h = 1e-5 in fp64: central differences of the rates are good to about h^2 + eps / h = 1e-10; the bar is 1e-7 of the
    largest entry of J, for the analytic Jacobians too (a few roundings per entry: far inside it)."""
    xdim, udim, rows, param = MODELS[key]
    pts = _model_points(key)
    h = 1e-5
    shifted = []
    for p in pts:
        shifted.append(p)
        for e in range(xdim + udim):
            for sgn in (1.0, -1.0):
                q = p.copy()
                q[e] += sgn * h
                shifted.append(q)
    checks, out = _run(checker, _model_text(xdim, udim, rows, param, shifted), xdim, udim)
    assert checks == [(r, 0, -1, 1) for r in range(xdim)]
    stride = 1 + 2 * (xdim + udim)
    assert len(out) == stride * len(pts)
    for q, p in enumerate(pts):
        at = out[stride * q]
        f, Jx, Ju = _analytic(key, p[:xdim], p[xdim:], param)
        J = np.concatenate([Jx, Ju], axis=1)
        scale = max(np.max(np.abs(J)), 1e-300)
        assert np.max(np.abs(at["rate"] - f)) <= 1e-12 * max(np.max(np.abs(f)), 1.0)
        got = np.concatenate([(at["A"] - np.eye(xdim)) / DT, at["B"] / DT], axis=1)
        assert np.max(np.abs(got - J)) <= 1e-7 * scale, (key, q)
        fd = np.zeros_like(J)
        for e in range(xdim + udim):
            plus, minus = out[stride * q + 1 + 2 * e], out[stride * q + 2 + 2 * e]
            he = ((p[e] + h) - (p[e] - h)) / 2.0
            fd[:, e] = (plus["rate"] - minus["rate"]) / (2.0 * he)
        assert np.max(np.abs(got - fd)) <= 1e-7 * scale, (key, q)
        # a row that is one of the other entries is the constant dt itself
        for r, (tree, xin, yin) in enumerate(rows):
            if tree.program() == [(abi.EXPR_PUSH_X, 0.0)]:
                assert (at["A"][r, xin] if xin < xdim else at["B"][r, xin - xdim]) == DT


def np_rk4_step(rates, x, u, dt, T=np.float64):
    """MultiPlayerDynamicalSystem::Integrate's RK4 with two half-steps in the arithmetic of T, sub_integrate8's order."""
    x = np.array(x, T)
    h = T(dt / 2.0)
    for _ in range(2):
        k1 = h * rates(x, u)
        k2 = h * rates(x + T(0.5) * k1, u)
        k3 = h * rates(x + T(0.5) * k2, u)
        k4 = h * rates(x + k3, u)
        x = x + (k1 + T(2.0) * (k2 + k3) + k4) / T(6.0)
    return x


def test_the_step_is_the_rk4_with_two_half_steps(checker):
    xdim, udim, rows, c = MODELS["coasting"]
    pts = _model_points("coasting")
    _, out = _run(checker, _model_text(xdim, udim, rows, c, pts), xdim, udim)
    for p, at in zip(pts, out):
        want = np_rk4_step(lambda x, u: coasting_rates(x, u, c), p[:xdim], p[xdim:], DT)
        assert np.max(np.abs(at["step"] - want)) <= 1e-14 * max(np.max(np.abs(want)), 1.0)


def test_the_checker_tells_a_malformed_row(checker):
    text = _model_text(2, 1, [([(Y, 0.0)], 0, None), ([(X, 0.0)], 2, None)], 0.0, [[0.1, 0.2, 0.3]])
    checks, out = _run(checker, text, 2, 1)
    assert checks == [(0, 7, 0, 0), (1, 0, -1, 1)] and out == []


def test_stand_alone_checker_is_clean_under_the_host_sanitizers(tmp_path):
    exe = _build_checker(str(tmp_path / "expr_dyn_check_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    text = "".join(_model_text(*MODELS[k], _model_points(k, 3)) for k in MODELS)
    text += _model_text(2, 1, [([(Y, 0.0)], 0, None), ([(X, 0.0)], 2, None)], 0.0, [[0.1, 0.2, 0.3]])
    done = subprocess.run([exe], input=text, text=True, capture_output=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr
    assert done.stdout.count("rate") == 3 * len(MODELS)


# ------------------------------------------------------------------------------------------------
# the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_coasting_car_scene_flattens_like_examples_py(tmp_path):
    entry.build_host()
    exe = str(tmp_path / "dump_coasting_car_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + entry.host_compile_flags() +
                          ['-DEXAMPLE_HEADER="coasting_car_scene.h"', "-DEXAMPLE_CLASS=CoastingCarScene",
                           "-I" + os.path.join(ROOT, "tests", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "dump_example.cpp")] + entry.host_link_flags())
    got = abi.ProblemSpec.from_dump(subprocess.check_output([exe], text=True))
    want = examples.coasting_car_scene()
    g, w = got.canonical(), want.canonical()
    for key in ("subsystems", "player_costs", "pairs", "T", "dt"):
        assert g[key] == w[key], key
    assert g["subsystems"] == [(abi.DYN_EXPRESSION, 4, 1, float(np.float32(examples.COASTING_CAR_DRAG)))] * 2
    assert set(g["groups"]) == set(w["groups"]) and (0, abi.ROLE_DYNAMICS_ROW) in g["groups"]
    for key in w["groups"]:
        assert g["groups"][key] == w["groups"][key], key
    rows = [t for i in range(2) for t in w["groups"][(i, abi.ROLE_DYNAMICS_ROW)]]
    assert len(rows) == 8 and all(len(t[6]) == 1 + 2 * int(t[6][0]) for t in rows)
    # the dense table itself: the eight programs, subsystem by subsystem, nothing else
    assert [np.float32(v) for v in got.dense_params] == [np.float32(v) for v in want.dense_params]
    np.testing.assert_allclose(np.array(got.x0, np.float32), np.array(want.x0, np.float32), rtol=1e-6, atol=1e-6)
