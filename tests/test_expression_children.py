"""Expression terms as children of an ExtremeValueCost (include/ilqg.h, kind 24 "As a child") without a device: what
creation accepts and refuses, what the row program gives a child's two ops, the scratch it counts for the children's
stack, the row programs of the scenes without such children, the C++ mirror, and the numpy restatement the GPU tests
compare against (tests/shaped_children.py) checked against the programs themselves."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from ilqgames_amd import abi, examples
from helpers import GOLDEN
import shaped_children as sc
from test_expression_cost import np_jet, _ops, _refused, OKP, RP_MAX_LSLOTS, RO_MODE, RO_NSID, RO_KIND, RO_POLY_FIRST, RO_PATTERN, STACK_SLOTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 12
RP_NUM_PASSES, RP_OFF_PASS, RPASS_WORDS, RO_AUX, RO_ROLE, RO_PLAYER, RO_FLAGS, RO_IDX0 = 0, 3, 9, 3, 5, 6, 7, 8
ROP_EXT_EVAL, ROP_EXT_APPLY = 1, 2
PAT_SINGLE, PAT_PAIR2, PAT_PAIR4 = 1, 2, 3
REACHABILITY = ("three_player_collision_avoidance_reachability", "three_player_intersection_reachability")


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        entry.build()
    return h


def _expression_children(spec):
    return [q for _, kids in sc.parents_of(spec) for q in kids if spec.terms[q]["kind"] == abi.COST_EXPRESSION]


def _pattern(term):
    """include/ilqg.h's table."""
    _, i1, i2, _ = term["idx"]
    return (PAT_PAIR4 if i1 >= 0 else PAT_PAIR2) if i2 >= 0 else (PAT_PAIR2 if i1 >= 0 else PAT_SINGLE)


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,count", list(zip(REACHABILITY, (6, 2))))
def test_restated_children_of_the_reachability_scenes_are_accepted(hip, scene, count):
    spec = getattr(examples, scene)(T=T)
    twin, replaced = examples.reachability_twin(spec)
    kids = _expression_children(twin)
    assert len(kids) == count and replaced >= count
    for q in kids:
        assert twin.terms[q]["role"] == abi.ROLE_CHILD and spec.terms[q]["kind"] == abi.COST_SIGNED_DISTANCE
        assert twin.terms[q]["idx"] == spec.terms[q]["idx"] and twin.terms[q]["value"] == spec.terms[q]["value"]
        hip.expression_check(twin, q)
    words, static_id = hip.row_program_build(twin)
    assert static_id == 0, "expression children match no registered structure: the row stage interprets them"
    # the twins existing callers get are what they were: no child is touched without the argument
    plain, _ = examples.expression_game_twin(spec)
    assert [t["kind"] for t in plain.terms if t["role"] == abi.ROLE_CHILD] == [abi.COST_SIGNED_DISTANCE] * count


def test_the_seven_children_of_the_shaped_scene_are_accepted_with_their_instance_parameters(hip):
    spec = examples.shaped_reachability_scene(T=T)
    assert (spec.n, spec.udims) == (10, [2, 2]) and [pc[2] for pc in spec.player_costs] == [abi.MIN, abi.MAX]
    kids = _expression_children(spec)
    assert kids == [spec.term_index(n) for n in examples.SHAPED_CHILDREN] and len(kids) == 7
    for q in kids:
        assert spec.terms[q]["role"] == abi.ROLE_CHILD and spec.terms[q]["arg"] == -1
        hip.expression_check(spec, q)
    assert [_pattern(spec.terms[q]) for q in kids] == [PAT_SINGLE] * 4 + [PAT_PAIR4, PAT_PAIR2, PAT_SINGLE]
    assert hip.row_program_build(spec)[1] == 0
    # the time leaf sits in the moving disc's program, and only there
    uses_time = [any(int(spec.dense_params[spec.terms[q]["polyline"] + 1 + 2 * e]) == abi.EXPR_PUSH_TIME
                     for e in range(int(spec.dense_params[spec.terms[q]["polyline"]]))) for q in kids]
    assert uses_time == [n == "p2_moving_disc" for n in examples.SHAPED_CHILDREN]
    # a child's weight and value columns: what its program pushes, per instance
    hip.instance_params_check(spec, [(n, "value") for n in examples.SHAPED_CHILDREN] + [("p2_ellipse", "weight"), ("p1_box_left", "weight")])


def test_creation_refuses_malformed_children_and_names_the_term(hip):
    # role CHILD, but no parent lists the term
    s = examples.skeleton(T=T)
    orphan = s.expression(0, OKP, (0, 1), role=abi.ROLE_CHILD)
    rc, msg = _refused(hip, s, orphan)
    assert rc == abi.ERR_UNSUPPORTED and "cannot be an EXTREME_VALUE child" in msg and "no ILQG_COST_EXTREME_VALUE term lists" in msg, msg
    assert ("expression term %d: " % orphan) in msg
    # inside a parent's range, but with a top-level role
    s = examples.skeleton(T=T)
    s.extreme_value(0, [lambda role: s.expression(0, OKP, (0, 1), role=abi.ROLE_STATE_COST), lambda role: s.quadratic(0, 1.0, 0)], True)
    term = len(s.terms) - 3
    rc, msg = _refused(hip, s, term)
    assert rc == abi.ERR_UNSUPPORTED and "a term with a top-level role cannot be an EXTREME_VALUE child" in msg, msg
    assert "give it ILQG_ROLE_CHILD" in msg and ("expression term %d: " % term) in msg and ("term %d lists it" % (len(s.terms) - 1)) in msg
    # ... the same with a control-cost role
    s = examples.skeleton(T=T)
    s.extreme_value(0, [lambda role: s.expression(0, [(abi.EXPR_PUSH_X, 0.0)], (0,), role=abi.ROLE_CONTROL_COST, control_of=0)], True)
    rc, msg = _refused(hip, s, len(s.terms) - 2)
    assert rc == abi.ERR_UNSUPPORTED and "a term with a top-level role cannot be an EXTREME_VALUE child" in msg, msg
    # listed by two parents
    s = examples.skeleton(T=T)
    s.extreme_value(0, [lambda role: s.expression(0, OKP, (0, 1), role=role), lambda role: s.quadratic(0, 1.0, 0)], False)
    shared = len(s.terms) - 3
    s._term(abi.COST_EXTREME_VALUE, abi.ROLE_STATE_COST, 1, -1, (0,), 1.0, 0.0, 0, -1, shared, 2)
    rc, msg = _refused(hip, s, shared)
    assert rc == abi.ERR_INVALID and "cannot be an EXTREME_VALUE child of more than one parent" in msg, msg
    assert ("expression term %d: " % shared) in msg and "2 ILQG_COST_EXTREME_VALUE terms list it" in msg
    # a malformed program is refused in a child as anywhere else, the child named
    s = examples.skeleton(T=T)
    s.extreme_value(0, [lambda role: s.expression(0, [(abi.EXPR_PUSH_X, 0.0), (abi.EXPR_MUL, 0.0)], (0,), role=role)], False)
    rc, msg = _refused(hip, s, len(s.terms) - 2)
    assert rc == abi.ERR_INVALID and "op 1: stack underflow" in msg and ("expression term %d: " % (len(s.terms) - 2)) in msg, msg
    # ... and so are a child's indices: its argument vector is the state
    s = examples.skeleton(T=T)
    s.extreme_value(0, [lambda role: s.expression(0, [(abi.EXPR_PUSH_X, 0.0)], (10,), role=role)], False)
    rc, msg = _refused(hip, s, len(s.terms) - 2)
    assert rc == abi.ERR_INVALID and "idx[0] = 10 is outside its argument vector (dimension 10)" in msg, msg


def test_constraint_and_nested_children_stay_refused(hip):
    ONE = [1.0, abi.EXPR_PUSH_X, 0.0]
    # an expression CONSTRAINT with role CHILD under a parent: ILQG_ERR_INVALID as before
    s = examples.skeleton(T=T)
    off = len(s.dense_params)
    s.dense_params += ONE
    s.extreme_value(0, [lambda role: s._term(abi.CONSTRAINT_EXPRESSION, role, 0, -1, (0, -1, -1, -1), 1.0, 0.0, 0, off, constraint=True)], True)
    rc, msg = _refused(hip, s, len(s.terms) - 2)
    assert rc == abi.ERR_INVALID and "an expression constraint cannot be an EXTREME_VALUE child" in msg, msg
    # an expression under an ExtremeValueCost that is itself a child of another: the outer range holds it too, and a term
    # is one parent's
    s = examples.skeleton(T=T)
    s.extreme_value(0, [lambda role: (s.extreme_value(0, [lambda r: s.expression(0, OKP, (0, 1), role=r)], False),
                                      s.terms[-1].update(role=role))], True)
    grandchild = len(s.terms) - 3
    rc, msg = _refused(hip, s, grandchild)
    assert rc == abi.ERR_INVALID and "child of more than one parent" in msg and ("expression term %d: " % grandchild) in msg, msg


# ------------------------------------------------------------------------------------------------
# the row program
# ------------------------------------------------------------------------------------------------
def _program_offsets(spec):
    """Offset of each expression term's program in the dense table the library builds: the blocks follow one another in
    term order (build_expression_blocks; these scenes hold no affine constraint and no expression model)."""
    off, out = 0, {}
    for q, t in enumerate(spec.terms):
        if t["kind"] in (abi.COST_EXPRESSION, abi.CONSTRAINT_EXPRESSION):
            out[q] = off
            off += 1 + 2 * int(spec.dense_params[t["polyline"]])
    return out


def _specs_with_children():
    out = [("shaped", examples.shaped_reachability_scene(T=T))]
    for scene in REACHABILITY:
        out.append((scene, examples.reachability_twin(getattr(examples, scene)(T=T))[0]))
    return out


@pytest.mark.parametrize("name,spec", _specs_with_children(), ids=[n for n, _ in _specs_with_children()])
def test_each_expression_child_has_an_eval_and_an_apply_op_with_its_pattern_and_program(hip, name, spec):
    words, _ = hip.row_program_build(spec)
    ops = _ops(words)
    offsets = _program_offsets(spec)
    fbits = lambda v: int(np.array([v], np.float32).view(np.int32)[0])
    for parent, kids in sc.parents_of(spec):
        pt = spec.terms[parent]
        for aux, q in enumerate(kids):
            t = spec.terms[q]
            if t["kind"] != abi.COST_EXPRESSION:
                continue
            mine = [o for o in ops if o[RO_KIND] == abi.COST_EXPRESSION and o[RO_POLY_FIRST] == offsets[q] and
                    o[RO_PLAYER] == pt["player"] and o[RO_MODE] in (ROP_EXT_EVAL, ROP_EXT_APPLY)]
            assert sorted(o[RO_MODE] for o in mine) == [ROP_EXT_EVAL, ROP_EXT_APPLY], (name, q)
            for o in mine:
                assert o[RO_AUX] == aux and o[RO_PATTERN] == _pattern(t), (name, q)
                assert tuple(o[RO_IDX0:RO_IDX0 + 4]) == tuple(t["idx"])
                assert o[RO_ROLE] == pt["role"] and (o[RO_FLAGS] & abi.FLAG_IS_MIN) == (pt["flags"] & abi.FLAG_IS_MIN)
                assert (o[12], o[13]) == (fbits(t["weight"]), fbits(t["value"]))  # RO_WEIGHT, RO_VALUE
            ev, ap = sorted(mine, key=lambda o: o[RO_MODE])
            assert ev[RO_NSID] == 0 and ap[RO_NSID] == {PAT_SINGLE: 2, PAT_PAIR2: 6, PAT_PAIR4: 20}[_pattern(t)]
    # no expression op carries a pattern other than its own table's
    assert all(o[RO_PATTERN] in (PAT_SINGLE, PAT_PAIR2, PAT_PAIR4) for o in ops if o[RO_KIND] == abi.COST_EXPRESSION)
    assert len({o[RO_POLY_FIRST] for o in ops if o[RO_KIND] in (abi.COST_EXPRESSION, abi.CONSTRAINT_EXPRESSION)}) == len(offsets)


def _plain(spec):
    """`spec` with every expression child replaced by a built-in kind of the same scatter pattern (QuadraticCost,
    QuadraticNormCost, SignedDistanceCost): the same slots, no stack."""
    import copy
    s = copy.deepcopy(spec)
    for q in _expression_children(s):
        t = s.terms[q]
        kind = {PAT_SINGLE: abi.COST_QUADRATIC, PAT_PAIR2: abi.COST_QUADRATIC_NORM, PAT_PAIR4: abi.COST_SIGNED_DISTANCE}[_pattern(t)]
        t.update(kind=kind, polyline=-1, idx=tuple(e if e >= 0 else 0 for e in t["idx"]))
    assert not any(t["kind"] == abi.COST_EXPRESSION for t in s.terms)
    s.dense_params = [v for v in s.dense_params] if any(t["kind"] == abi.CONSTRAINT_EXPRESSION for t in s.terms) else []
    return s


def _passes(words):
    return [words[words[RP_OFF_PASS] + q * RPASS_WORDS:words[RP_OFF_PASS] + (q + 1) * RPASS_WORDS] for q in range(words[RP_NUM_PASSES])]


def test_row_program_counts_the_childrens_stack_in_both_scratch_widths(hip):
    """The full pass keeps every slot of a pass live, the gradient-only one its gradient slots; the jet stack of a child
    lies behind either, kExprStackScalars wide, and must fit the LDS scratch the chunk width is chosen for."""
    spec = examples.shaped_reachability_scene(T=T)
    words, _ = hip.row_program_build(spec)
    plain_words, _ = hip.row_program_build(_plain(spec))
    live = max(p[5] for p in _passes(words))  # li_count of the widest pass
    assert [p[5] for p in _passes(words)] == [p[5] for p in _passes(plain_words)], "the stack has no slot ids"
    assert words[RP_MAX_LSLOTS] >= live + STACK_SLOTS
    assert words[RP_MAX_LSLOTS] == plain_words[RP_MAX_LSLOTS] + STACK_SLOTS
    # the gradient-only width is not in the program's words: the probing row kernel's LDS is sized from it
    kw = dict(batch=64, num_cus=256, probe=True, split_trial=True)
    a, b = hip.schedule_build(spec, abi.F64, **kw), hip.schedule_build(_plain(spec), abi.F64, **kw)
    assert a["prog_kind"] != b["prog_kind"] and a["static_id"] == 0
    if a["rows_cw"] == b["rows_cw"]:
        assert a["lds_prows"] - b["lds_prows"] >= STACK_SLOTS * a["rows_cw"] * 8, (a["lds_prows"], b["lds_prows"])
        assert a["lds_rows"] - b["lds_rows"] >= STACK_SLOTS * a["rows_cw"] * 8, (a["lds_rows"], b["lds_rows"])
    else:  # a narrower chunk was chosen so that the wider scratch fits
        assert a["rows_cw"] < b["rows_cw"]


def test_row_programs_of_the_reachability_scenes_without_expression_children_are_unchanged(hip):
    """Word for word what the library built before an expression could be a child
    (tests/golden/reachability_row_programs.npz, T = 12)."""
    golden = np.load(os.path.join(GOLDEN, "reachability_row_programs.npz"))
    for scene in REACHABILITY:
        words, static_id = hip.row_program_build(getattr(examples, scene)(T=T))
        assert np.array_equal(words, golden[scene]), scene
        assert static_id == int(golden[scene + "__static_id"]), scene
    assert int(golden[REACHABILITY[0] + "__static_id"]) != 0


# ------------------------------------------------------------------------------------------------
# the numpy restatement the GPU tests compare against, checked against the programs
# ------------------------------------------------------------------------------------------------
def test_analytic_child_jets_match_the_programs():
    """shaped_children.shaped_child_jet (formulas) against np_jet (the op table applied to the scene's own programs) in
    float64 at seeded points: 1e-12 of the jet's largest component."""
    spec = examples.shaped_reachability_scene(T=T)
    rng = np.random.default_rng(7)
    for name in examples.SHAPED_CHILDREN:
        t = spec.terms[spec.term_index(name)]
        L = int(spec.dense_params[t["polyline"]])
        blk = spec.dense_params[t["polyline"] + 1:t["polyline"] + 1 + 2 * L]
        program = [(int(blk[2 * e]), blk[2 * e + 1]) for e in range(L)]
        for _ in range(10):
            X, Y, tm = rng.uniform(-6, 6), rng.uniform(-6, 6), float(rng.integers(0, T)) * 0.125  # (exact as a float immediate)
            want = _np_jet_with_time(program, np.float64(np.float32(t["weight"])), np.float64(np.float32(t["value"])), X, Y, tm)
            got = [float(c) for c in sc.shaped_child_jet(name, np.float64(np.float32(t["value"])), np.float64(X), np.float64(Y), np.float64(tm))]
            if t["idx"][1] < 0:
                got = [got[0], got[1], 0.0, got[3], 0.0, 0.0]
            assert np.max(np.abs(np.array(got) - np.array(want))) <= 1e-12 * np.max(np.abs(want)), (name, X, Y, tm, got, want)


def _np_jet_with_time(program, w, v, x, y, t):
    """np_jet knows the ops before PUSH_TIME: the time is a constant of the step, so it goes in as one."""
    return [float(c) for c in np_jet([(abi.EXPR_PUSH_CONST, t) if op == abi.EXPR_PUSH_TIME else (op, imm) for op, imm in program],
                                     w, v, x, y, np.float64)]


# ------------------------------------------------------------------------------------------------
# the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_shaped_reachability_scene_flattens_like_examples_py(tmp_path):
    entry.build_host()
    exe = str(tmp_path / "dump_shaped_reachability_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + entry.host_compile_flags() +
                          ['-DEXAMPLE_HEADER="shaped_reachability_scene.h"', "-DEXAMPLE_CLASS=ShapedReachabilityScene",
                           "-I" + os.path.join(ROOT, "tests", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "dump_example.cpp")] + entry.host_link_flags())
    got = abi.ProblemSpec.from_dump(subprocess.check_output([exe], text=True))
    want = examples.shaped_reachability_scene()
    g, w = got.canonical(), want.canonical()
    for key in ("subsystems", "player_costs", "pairs", "T", "dt"):
        assert g[key] == w[key], key
    assert set(g["groups"]) == set(w["groups"])
    for key in w["groups"]:
        assert g["groups"][key] == w["groups"][key], key
    # the children ride in their parents' keys: seven programs, each parent's in child order
    parents = [t for grp in w["groups"].values() for t in grp if t[0] == abi.COST_EXTREME_VALUE]
    assert sorted(len(p[7]) for p in parents) == [3, 4] and all(k[0] == abi.COST_EXPRESSION for p in parents for k in p[7])
    # the descriptor's words themselves: every child with role CHILD inside its parent's range, and the dense table
    kids = [(t["kind"], t["role"], t["player"], tuple(t["idx"]), np.float32(t["value"])) for t in got.terms if t["role"] == abi.ROLE_CHILD]
    assert kids == [(t["kind"], t["role"], t["player"], tuple(t["idx"]), np.float32(t["value"])) for t in want.terms if t["role"] == abi.ROLE_CHILD]
    assert [np.float32(v) for v in got.dense_params] == [np.float32(v) for v in want.dense_params]
    np.testing.assert_allclose(np.array(got.x0, np.float32), np.array(want.x0, np.float32), rtol=1e-6, atol=1e-6)
    # the mirror's description builds: the checks and the row program are the library's
    from ilqgames_amd import hip
    got.T = T
    for q in _expression_children(got):
        hip.expression_check(got, q)
    hip.row_program_build(got)


def test_the_demo_dumps_the_same_description(tmp_path):
    entry.build_host()
    exe = os.path.join(ROOT, "tests", "host", "_bin", "shaped_reachability_demo")
    got = abi.ProblemSpec.from_dump(subprocess.check_output([exe, "dump"], text=True))
    want = examples.shaped_reachability_scene()
    assert got.canonical()["groups"] == want.canonical()["groups"]
    for field in ("convergence_tolerance", "max_solver_iters", "initial_alpha_scaling", "max_backtracking_steps", "expected_decrease_fraction"):
        assert getattr(got.params, field) == pytest.approx(getattr(want.params, field)), field
