"""Expression terms between players and as constraints, without a device (include/ilqg.h: relative inputs of the
expression kinds, ILQG_CONSTRAINT_EXPRESSION): what creation refuses, the row program the relative terms get, per-instance
columns, the C++ mirror — and the hand-written numpy restatement of examples.expression_game_scene's terms that the
device tests compare against, checked here against central differences."""
import copy
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from ilqgames_amd import abi, examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, C_, W, V, ADD, SUB, MUL, DIV = (float(v) for v in range(1, 10))


@pytest.fixture(scope="module")
def hip():
    entry.build()
    from ilqgames_amd import hip as h
    return h


# ------------------------------------------------------------------------------------------------
# the numpy restatement of expression_game_scene's terms (shared with tests/test_gpu_expression_roles.py)
# ------------------------------------------------------------------------------------------------
def gaussian(Xv, Yv, w, v):
    """w exp(-0.5 (X^2 + Y^2) / v^2) -> (f, fx, fy, fxx, fyy, fxy), derivatives by hand."""
    f = w * np.exp(-0.5 * (Xv * Xv + Yv * Yv) / (v * v))
    return f, -Xv / (v * v) * f, -Yv / (v * v) * f, (Xv * Xv / v ** 4 - 1.0 / (v * v)) * f, (Yv * Yv / v ** 4 - 1.0 / (v * v)) * f, \
        Xv * Yv / v ** 4 * f


def speed_match(Xv, Yv, w, v):
    """0.5 w (X - v)^2"""
    z = Xv * 0
    return 0.5 * w * (Xv - v) ** 2, w * (Xv - v), z, w + z, z, z


def make_disc(cx, cy):
    def disc(Xv, Yv, w, v):
        """v^2 - (x - cx)^2 - (y - cy)^2"""
        z = Xv * 0
        return v * v - (Xv - cx) ** 2 - (Yv - cy) ** 2, -2.0 * (Xv - cx), -2.0 * (Yv - cy), z - 2.0, z - 2.0, z
    return disc


def clearance(Xv, Yv, w, v):
    """v - sqrt(X^2 + Y^2)"""
    d = np.sqrt(Xv * Xv + Yv * Yv)
    return v - d, -Xv / d, -Yv / d, -Yv * Yv / d ** 3, -Xv * Xv / d ** 3, Xv * Yv / d ** 3


def upper_bound(Xv, Yv, w, v):
    """x - v"""
    z = Xv * 0
    return Xv - v, z + 1.0, z, z, z, z


def game_scene_formulas():
    """term name of examples.expression_game_scene -> its formula"""
    return {"p1_repulsion": gaussian, "p2_repulsion": gaussian, "p2_speed_match": speed_match,
            "p1_keep_out": make_disc(*examples.EXPRESSION_DISC_CENTRE), "p2_clearance": clearance,
            "p1_acceleration_max": upper_bound}


def constraint_mu(lam, g, mu, is_equality):
    """Constraint::Mu: an inactive inequality (g and |lambda| both at most 1e-4) takes no penalty"""
    return np.where((not is_equality) & (g <= 1e-4) & (np.abs(lam) <= 1e-4), 0.0, mu)


def numpy_contributions(spec, formulas, xs, us, lam=None, mu=None, NT=np.float64):
    """What the named terms of `spec` add to Q [B][T][N][n*n] (column-major), l [B][T][N][n], R / r (per control pair
    (i, j): [B][T][mj*mj] / [B][T][mj]) and the per-player total costs, and each constraint's g [B][T] (zero before its
    first step): the formula's jet at the (relative) inputs, a constraint's through Constraint::ModifyDerivatives with
    lam [B][slots][T] and mu [B], scattered with the signs of the differences."""
    B, n, T, N = xs.shape[0], spec.n, spec.T, len(spec.subsystems)
    xs, us = xs.astype(NT), us.astype(NT)
    dQ, dl = np.zeros((B, T, N, n * n)), np.zeros((B, T, N, n))
    dR, dr, gs = {}, {}, {}
    dc = np.zeros((B, N))
    for name, fn in formulas.items():
        t = spec.terms[spec.term_index(name)]
        i, idx, k0 = t["player"], t["idx"], t.get("first_step", 0)
        on_state = t["role"] in (abi.ROLE_STATE_COST, abi.ROLE_STATE_CONSTRAINT)
        is_constraint = t["kind"] == abi.CONSTRAINT_EXPRESSION
        vec = xs if on_state else us[:, :, sum(spec.udims[:t["arg"]]):sum(spec.udims[:t["arg"] + 1])]
        Xv = vec[:, :, idx[0]] - (vec[:, :, idx[2]] if idx[2] >= 0 else NT(0))
        Yv = (vec[:, :, idx[1]] - (vec[:, :, idx[3]] if idx[3] >= 0 else NT(0))) if idx[1] >= 0 else Xv * 0
        with np.errstate(all="ignore"):
            f, fx, fy, fxx, fyy, fxy = [np.asarray(a, NT) for a in fn(Xv, Yv, NT(np.float32(t["weight"])), NT(np.float32(t["value"])))]
        live = (np.arange(T) >= k0)[None, :]
        if is_constraint:
            L = np.zeros((B, T)) if lam is None else lam[:, t["constraint_slot"], :].astype(NT)
            M = np.zeros((B, 1)) if mu is None else np.asarray(mu, NT)[:, None]
            me = constraint_mu(L, f, M, bool(t["flags"] & abi.FLAG_EQUALITY))
            gx, gy = L * fx + me * f * fx, L * fy + me * f * fy
            hxx, hyy = L * fxx + me * (fx * fx + f * fxx), L * fyy + me * (fy * fy + f * fyy)
            hxy = L * fxy + me * (fx * fy + f * fxy)
            gs[name] = np.where(live, f, 0.0)
        else:
            gx, gy, hxx, hyy, hxy = fx, fy, fxx, fyy, fxy
            dc[:, i] += np.sum(np.where(live, f, 0.0), axis=1)
        # the entries the term names: (index, sign, which input)
        ent = [(idx[0], 1.0, 0)] + ([(idx[2], -1.0, 0)] if idx[2] >= 0 else []) + \
              ([(idx[1], 1.0, 1)] if idx[1] >= 0 else []) + ([(idx[3], -1.0, 1)] if idx[3] >= 0 else [])
        grad, hess = (gx, gy), ((hxx, hxy), (hxy, hyy))
        dim = n if on_state else spec.udims[t["arg"]]
        Gl, Hl = np.zeros((B, T, dim)), np.zeros((B, T, dim * dim))
        for a, sa, ta in ent:
            Gl[:, :, a] += np.where(live, sa * grad[ta], 0.0)
            for b_, sb, tb in ent:
                Hl[:, :, a + dim * b_] += np.where(live, sa * sb * hess[ta][tb], 0.0)
        if on_state:
            dl[:, :, i] += Gl
            dQ[:, :, i] += Hl
        else:
            key = (i, t["arg"])
            dr[key] = dr.get(key, 0) + Gl
            dR[key] = dR.get(key, 0) + Hl
    return dQ, dl, dR, dr, dc, gs


def without_expressions(spec):
    s = copy.deepcopy(spec)
    s.terms = [t for t in s.terms if t["kind"] not in (abi.COST_EXPRESSION, abi.CONSTRAINT_EXPRESSION)]
    s.term_names = {}
    s.dense_params = []
    s._num_constraints = 0
    return s


def test_hand_derivatives_match_central_differences():
    """Every formula of the restatement: gradient and Hessian by hand against central differences of the value and of
    the gradient, 1e-6 relative in fp64."""
    rng = np.random.default_rng(7)
    h = 1e-5
    for name, fn in game_scene_formulas().items():
        for _ in range(5):
            x, y = rng.uniform(1.0, 4.0) * rng.choice([-1, 1]), rng.uniform(1.0, 4.0) * rng.choice([-1, 1])
            w, v = 3.0, 2.5
            at = lambda a, b: [float(q) for q in fn(np.float64(a), np.float64(b), w, v)]  # noqa: E731
            f, fx, fy, fxx, fyy, fxy = at(x, y)
            num = dict(fx=(at(x + h, y)[0] - at(x - h, y)[0]) / (2 * h), fy=(at(x, y + h)[0] - at(x, y - h)[0]) / (2 * h),
                       fxx=(at(x + h, y)[1] - at(x - h, y)[1]) / (2 * h), fyy=(at(x, y + h)[2] - at(x, y - h)[2]) / (2 * h),
                       fxy=(at(x, y + h)[1] - at(x, y - h)[1]) / (2 * h))
            scale = max(abs(f), abs(fx), abs(fy), abs(fxx), abs(fyy), abs(fxy), 1.0)
            for key, got in zip(("fx", "fy", "fxx", "fyy", "fxy"), (fx, fy, fxx, fyy, fxy)):
                assert abs(got - num[key]) < 1e-6 * scale, (name, key, got, num[key])


def test_the_formulas_are_the_programs_of_the_scene():
    """... and they are what the scene's programs compute: np_jet of each program at relative inputs, fp64, 1e-12."""
    from test_expression_cost import np_jet
    spec = examples.expression_game_scene(T=12)
    rng = np.random.default_rng(8)
    for name, fn in game_scene_formulas().items():
        t = spec.terms[spec.term_index(name)]
        L = int(spec.dense_params[t["polyline"]])
        blk = spec.dense_params[t["polyline"] + 1:t["polyline"] + 1 + 2 * L]
        program = [(int(blk[2 * e]), blk[2 * e + 1]) for e in range(L)]
        x, y = rng.uniform(1.0, 4.0), rng.uniform(-4.0, -1.0)
        w, v = np.float64(np.float32(t["weight"])), np.float64(np.float32(t["value"]))
        got = [float(c) for c in np_jet(program, w, v, np.float64(x), np.float64(y), np.float64)]
        want = [float(c) for c in fn(np.float64(x), np.float64(y), w, v)]
        if t["idx"][1] < 0:  # a one-input program knows no y
            want[2] = want[4] = want[5] = 0.0
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, err_msg=name)


# ------------------------------------------------------------------------------------------------
# what creation refuses
# ------------------------------------------------------------------------------------------------
def _refused(hip, spec, term):
    """(status, message) of ilqg_expression_check, and of the host half of ilqg_problem_create, which must agree."""
    import ctypes as C
    desc, keep = spec.build(abi.F64)
    rc = hip.lib().ilqg_expression_check(C.byref(desc), term)
    msg = hip.lib().ilqg_last_error().decode() if rc else ""
    n, sid = C.c_int32(0), C.c_int32(0)
    rc2 = hip.lib().ilqg_row_program_build(C.byref(desc), None, 0, C.byref(n), C.byref(sid))
    msg2 = hip.lib().ilqg_last_error().decode() if rc2 else ""
    del keep
    assert (rc, msg) == (rc2, msg2)
    return rc, msg


def _raw(words, idx, kind=abi.COST_EXPRESSION, role=abi.ROLE_STATE_COST, arg=-1, constraint=None):
    """The skeleton example with one expression term of player 0 appended, its block the given words and its idx as given."""
    s = examples.skeleton(T=12)
    off = len(s.dense_params)
    s.dense_params += [float(w) for w in words]
    if constraint is None:
        constraint = kind == abi.CONSTRAINT_EXPRESSION
    return s, s._term(kind, role, 0, arg, tuple(idx), 1.0, 0.0, 0, off, constraint=constraint)


ONE = [1.0, X, 0.0]
TWO = [3.0, X, 0.0, Y, 0.0, MUL, 0.0]
K25 = dict(kind=abi.CONSTRAINT_EXPRESSION, role=abi.ROLE_STATE_CONSTRAINT)


def test_creation_refuses_malformed_relative_inputs(hip):
    cases = [
        (_raw(TWO, (0, 1, -1, 6)), "idx[3] = 6 without idx[2]"),
        (_raw(ONE, (0, -1, 5, 6)), "idx[3] = 6 on a one-input term"),
        (_raw(TWO, (0, 1, 5, -1)), "idx[3] = -1 on a two-input term"),
        (_raw(TWO, (0, 1, 10, 6)), "idx[2] = 10 is neither -1 nor inside its argument vector (dimension 10)"),
        (_raw(TWO, (0, 1, -2, 6)), "idx[2] = -2 is neither -1 nor inside"),
        (_raw(TWO, (0, 1, 5, 11)), "idx[3] = 11 is neither -1 nor inside"),
        (_raw(TWO, (0, 1, 0, 6)), "idx[0] and idx[2] name the same entry"),
        (_raw(TWO, (0, 1, 5, 1)), "idx[1] and idx[3] name the same entry"),
        (_raw(TWO, (0, 1, 1, 6)), "idx[1] and idx[2] name the same entry"),
        (_raw(TWO, (0, 1, 5, 5)), "idx[2] and idx[3] name the same entry"),
        (_raw(ONE, (0, -1, 2, -1), role=abi.ROLE_CONTROL_COST, arg=0), "idx[2] = 2 is neither -1 nor inside its argument vector (dimension 2)"),
        (_raw(TWO, (0, 1, 0, 6), **K25), "idx[0] and idx[2] name the same entry"),
        (_raw(ONE, (0, -1, 2, -1), kind=abi.CONSTRAINT_EXPRESSION, role=abi.ROLE_CONTROL_CONSTRAINT, arg=0), "idx[2] = 2 is neither"),
    ]
    for (spec, term), fragment in cases:
        rc, msg = _refused(hip, spec, term)
        assert rc == abi.ERR_INVALID and fragment in msg, (fragment, rc, msg)
        assert ("expression term %d: " % term) in msg, msg


def test_creation_refuses_misplaced_and_malformed_expression_constraints(hip):
    cases = [
        (_raw(TWO, (0, 1, -1, -1), kind=abi.CONSTRAINT_EXPRESSION, role=abi.ROLE_STATE_COST), abi.ERR_INVALID, "role must be a state or control constraint"),
        (_raw(ONE, (0, -1, -1, -1), kind=abi.CONSTRAINT_EXPRESSION, role=abi.ROLE_CONTROL_COST, arg=0), abi.ERR_INVALID, "role must be a state or control constraint"),
        (_raw(TWO, (0, 1, -1, -1), kind=abi.CONSTRAINT_EXPRESSION, role=abi.ROLE_CHILD), abi.ERR_INVALID, "cannot be an EXTREME_VALUE child"),
        (_raw(TWO, (0, 1, -1, -1), constraint=False, **K25), abi.ERR_INVALID, "constraint_slot = -1"),
        # one case of each class of malformed program
        (_raw([99.0, X, 0.0], (0, 1, -1, -1), **K25), abi.ERR_INVALID, "program length L must be a whole number in 1 .. 64"),
        (_raw([3.0, X, 0.0, Y, 0.0], (0, 1, -1, -1), **K25), abi.ERR_INVALID, "program block is out of range of ilqg_problem_desc::dense_params"),
        (_raw([2.0, X, 0.0, 42.0, 0.0], (0, 1, -1, -1), **K25), abi.ERR_UNSUPPORTED, "op 1: unknown opcode"),
        (_raw([2.0, X, 0.0, MUL, 0.0], (0, 1, -1, -1), **K25), abi.ERR_INVALID, "op 1: stack underflow"),
        (_raw([5.0] + [X, 0.0] * 5, (0, 1, -1, -1), **K25), abi.ERR_UNSUPPORTED, "op 4: stack overflow"),
        (_raw([2.0, X, 0.0, Y, 0.0], (0, 1, -1, -1), **K25), abi.ERR_INVALID, "ends with 2 entries on the stack"),
        (_raw([1.0, Y, 0.0], (3, -1, 4, -1), **K25), abi.ERR_INVALID, "op 0: PUSH_Y in a program without a second input"),
    ]
    for (spec, term), status, fragment in cases:
        rc, msg = _refused(hip, spec, term)
        assert rc == status and fragment in msg, (fragment, rc, msg)
        assert ("expression term %d: " % term) in msg, msg
    # a multiplier slot is one term's
    spec, term = _raw(TWO, (0, 1, 5, 6), **K25)
    spec.proximity_constraint(1, (5, 6), (0, 1), 3.0, False)
    spec.terms[-1]["constraint_slot"] = spec.terms[term]["constraint_slot"]
    rc, msg = _refused(hip, spec, term)
    assert rc == abi.ERR_INVALID and "constraint_slot = 0 is also term %d's" % (len(spec.terms) - 1) in msg, msg


def test_an_expression_constraint_under_an_extreme_value_parent_is_refused(hip):
    s = examples.skeleton(T=12)
    off = len(s.dense_params)
    s.dense_params += TWO
    s.extreme_value(0, [lambda role: s._term(abi.CONSTRAINT_EXPRESSION, abi.ROLE_STATE_CONSTRAINT, 0, -1, (0, 1, -1, -1), 1.0, 0.0, 0, off,
                                             constraint=True),
                        lambda role: s.quadratic(0, 1.0, 0)], True)
    rc, msg = _refused(hip, s, len(s.terms) - 3)
    assert rc == abi.ERR_INVALID and "cannot be an EXTREME_VALUE child" in msg, msg


def test_the_game_scene_is_accepted_with_its_instance_parameters(hip):
    spec = examples.expression_game_scene(T=12)
    assert abi.CONSTRAINT_EXPRESSION == 25 and spec.num_constraints == 3
    for name in game_scene_formulas():
        hip.expression_check(spec, spec.term_index(name))
    hip.row_program_build(spec)
    # weight and value columns on both kinds: what the programs push
    hip.instance_params_check(spec, [("p1_repulsion", "weight"), ("p1_repulsion", "value"), ("p2_speed_match", "value"),
                                     ("p2_clearance", "value"), ("p2_clearance", "weight"), ("p1_acceleration_max", "value")])
    # an equality flag is the expression constraint's too (and still no other built-in kind's)
    eq = copy.deepcopy(spec)
    eq.terms[eq.term_index("p2_clearance")]["flags"] = abi.FLAG_EQUALITY
    hip.row_program_build(eq)
    import ctypes as C
    desc, keep = spec.build(abi.F64)
    rc = hip.lib().ilqg_expression_check(C.byref(desc), 0)  # a QuadraticCost: the message is the one kind 24 came with
    assert rc == abi.ERR_INVALID and "is not an ILQG_COST_EXPRESSION term" in hip.lib().ilqg_last_error().decode()
    del keep


# ------------------------------------------------------------------------------------------------
# the row program
# ------------------------------------------------------------------------------------------------
RP_MAX_LSLOTS, RP_OFF_OPS, RP_OFF_SIDS, RP_OFF_COMPACT = 2, 4, 5, 13
ROP_WORDS, RO_MODE, RO_SID, RO_NSID, RO_KIND, RO_ROLE, RO_POLY_FIRST, RO_SLOT, RO_K_START, RO_PATTERN = 40, 0, 1, 2, 4, 5, 14, 15, 18, 19
PAT_SINGLE, PAT_PAIR2, PAT_PAIR4 = 1, 2, 3
STACK_SLOTS = (abi.EXPR_MAX_DEPTH - 1) * 6


def _ops(words):
    n = (words[RP_OFF_SIDS] - words[RP_OFF_OPS]) // ROP_WORDS
    return [words[words[RP_OFF_OPS] + q * ROP_WORDS:words[RP_OFF_OPS] + (q + 1) * ROP_WORDS] for q in range(n)]


def _sids(words, op):
    b = words[RP_OFF_SIDS] + op[RO_SID]
    return [int(v) for v in words[b:b + op[RO_NSID]]]


def _built_in_stand_in(spec):
    """The scene with every expression term replaced, in place, by a built-in kind of the same pattern over the same
    indices: PROXIMITY / CONSTRAINT_PROXIMITY (PAIR4), QUADRATIC_NORM over (idx0, idx2) or
    CONSTRAINT_POLYLINE2_SIGNED_DISTANCE / QUADRATIC_NORM (PAIR2), QUADRATIC / CONSTRAINT_SINGLE_DIMENSION (SINGLE)."""
    s = copy.deepcopy(spec)
    for t in s.terms:
        if t["kind"] not in (abi.COST_EXPRESSION, abi.CONSTRAINT_EXPRESSION):
            continue
        cons = t["kind"] == abi.CONSTRAINT_EXPRESSION
        i0, i1, i2, i3 = t["idx"]
        if i2 >= 0 and i1 >= 0:
            t.update(kind=abi.CONSTRAINT_PROXIMITY if cons else abi.COST_PROXIMITY, polyline=-1, value=1.0)
        elif i2 >= 0:
            assert not cons
            t.update(kind=abi.COST_QUADRATIC_NORM, idx=(i0, i2, 0, 0), polyline=-1)
        elif i1 >= 0:
            t.update(kind=abi.CONSTRAINT_POLYLINE2_SIGNED_DISTANCE if cons else abi.COST_QUADRATIC_NORM, polyline=0 if cons else -1)
        else:
            t.update(kind=abi.CONSTRAINT_SINGLE_DIMENSION if cons else abi.COST_QUADRATIC, idx=(i0, 0, 0, 0), polyline=-1)
    return s


def test_row_program_gives_relative_terms_the_entries_of_the_built_in_kinds(hip):
    spec = examples.expression_game_scene(T=12)
    words, static_id = hip.row_program_build(spec)
    assert static_id == 0
    plain_words, _ = hip.row_program_build(_built_in_stand_in(spec))
    ops, plain_ops = _ops(words), _ops(plain_words)
    mine = [(q, o) for q, o in enumerate(ops) if o[RO_KIND] in (abi.COST_EXPRESSION, abi.CONSTRAINT_EXPRESSION)]
    # p1: repulsion, keep-out, acceleration bound; p2: repulsion, speed match, clearance — in pass order
    assert [(o[RO_KIND], o[RO_PATTERN], o[RO_NSID]) for _, o in mine] == [
        (24, PAT_PAIR4, 20), (25, PAT_PAIR2, 6), (25, PAT_SINGLE, 2), (24, PAT_PAIR4, 20), (24, PAT_PAIR2, 6), (25, PAT_PAIR4, 20)]
    # the closest-point op of the stand-in's polyline constraint is the one op the stand-in has more
    plain_terms = [o for o in plain_ops if o[RO_MODE] == 0]
    mine_terms = [o for o in ops if o[RO_MODE] == 0]
    assert len(plain_terms) == len(mine_terms)
    seen = set()
    for a, b in zip(mine_terms, plain_terms):
        assert (a[RO_PATTERN], a[RO_NSID], a[RO_ROLE], a[RO_SLOT], a[RO_K_START]) == (b[RO_PATTERN], b[RO_NSID], b[RO_ROLE], b[RO_SLOT], b[RO_K_START])
        # the same slots in the same order: PAT_PAIR4's twenty of a ProximityCost on those indices, PAT_PAIR2's six
        assert _sids(words, a) == _sids(plain_words, b)
        if a[RO_KIND] in (24, 25):
            seen.add((a[RO_KIND], a[RO_PATTERN]))
            assert b[RO_KIND] not in (24, 25)
    assert seen == {(24, PAT_PAIR4), (24, PAT_PAIR2), (25, PAT_PAIR4), (25, PAT_PAIR2), (25, PAT_SINGLE)}
    # the gate of the keep-out disc travels in its op
    assert [o[RO_K_START] for _, o in mine] == [0, spec.terms[spec.term_index("p1_keep_out")]["first_step"], 0, 0, 0, 0]
    assert spec.terms[spec.term_index("p1_keep_out")]["first_step"] == 3
    # each op carries the offset of its program in the dense table
    by_term = sorted(o[RO_POLY_FIRST] for _, o in mine)
    offs, off = [], 0
    for t in spec.terms:
        if t["kind"] in (24, 25):
            offs.append(off)
            off += 1 + 2 * int(spec.dense_params[t["polyline"]])
    assert by_term == offs and off == len(spec.dense_params)
    # the stack is counted into the scratch behind the widest pass (max_lslots; the widest gradient-only pass's, max_gslots,
    # is not part of the program's words: the probing solves of the device tests run in it), and keeps the scene on the
    # compact rows
    assert words[RP_MAX_LSLOTS] == plain_words[RP_MAX_LSLOTS] + STACK_SLOTS
    assert words[words[RP_OFF_COMPACT]] == plain_words[plain_words[RP_OFF_COMPACT]] > 0


def test_twins_of_the_built_in_scenes_keep_their_entries(hip):
    """examples.expression_game_twin: a twin's ops name the slots of the original's, term for term."""
    for make, replaced in ((lambda: examples.skeleton(T=12), 8), (lambda: examples.three_player_intersection(T=12), 15),
                           (lambda: examples.mixed_dubins_car_scene(T=12, constrained=True), 12)):
        spec = make()
        twin, count = examples.expression_game_twin(spec)
        assert count == replaced
        w0, _ = hip.row_program_build(spec)
        w1, sid = hip.row_program_build(twin)
        assert sid == 0
        t0, t1 = [o for o in _ops(w0) if o[RO_MODE] == 0], [o for o in _ops(w1) if o[RO_MODE] == 0]
        assert len(t0) == len(t1)
        for a, b in zip(t0, t1):
            assert a[RO_PATTERN] == b[RO_PATTERN] and _sids(w0, a) == _sids(w1, b)
        assert w1[words_compact(w1)] == w0[words_compact(w0)]


def words_compact(w):
    return w[RP_OFF_COMPACT]


# ------------------------------------------------------------------------------------------------
# the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_expression_game_scene_flattens_like_examples_py(tmp_path):
    entry.build_host()
    exe = str(tmp_path / "dump_expression_game_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + entry.host_compile_flags() +
                          ['-DEXAMPLE_HEADER="expression_game_scene.h"', "-DEXAMPLE_CLASS=ExpressionGameScene",
                           "-I" + os.path.join(ROOT, "tests", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "dump_example.cpp")] + entry.host_link_flags())
    text = subprocess.check_output([exe], text=True)
    got = abi.ProblemSpec.from_dump(text)
    want = examples.expression_game_scene()
    g, w = got.canonical(), want.canonical()
    for key in ("subsystems", "player_costs", "pairs", "T", "dt"):
        assert g[key] == w[key], key
    assert set(g["groups"]) == set(w["groups"])
    for key in w["groups"]:
        assert g["groups"][key] == w["groups"][key], key
    # from_dump keeps idx[2..3] and kind 25
    rel = sorted(tuple(t["idx"]) for t in got.terms if t["kind"] == abi.COST_EXPRESSION)
    assert rel == [(0, 1, 5, 6), (5, 6, 0, 1), (9, -1, 4, -1)]
    cons = sorted((tuple(t["idx"]), t["role"], t["first_step"]) for t in got.terms if t["kind"] == abi.CONSTRAINT_EXPRESSION)
    assert cons == [((0, 1, -1, -1), abi.ROLE_STATE_CONSTRAINT, 3), ((1, -1, -1, -1), abi.ROLE_CONTROL_CONSTRAINT, 0),
                    ((5, 6, 0, 1), abi.ROLE_STATE_CONSTRAINT, 0)]
    assert got.num_constraints == 3
    assert [np.float32(v) for v in got.dense_params] == [np.float32(v) for v in want.dense_params]
    np.testing.assert_allclose(np.array(got.x0, np.float32), np.array(want.x0, np.float32), rtol=1e-6, atol=1e-6)
