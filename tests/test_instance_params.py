"""Per-instance cost parameters, the checks that need no GPU: the C header against the ctypes mirror, what
ilqg_instance_params_check accepts and refuses (host only: the library is loaded without a device, as
scripts/gen_static_rowprogs.py does for ilqg_row_program_build), the term names of the scene builders, and the C++
mirror's resolution of (Cost*, field) to term indices."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ilqgames_amd import abi, examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return h


def test_instance_param_layout_and_abi_version_match_the_c_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "ilqg.h"
int main(void) {
  printf("%zu %zu %zu %d %d %d\n", sizeof(ilqg_instance_param), offsetof(ilqg_instance_param, term),
         offsetof(ilqg_instance_param, field), (int)ILQG_ABI_VERSION, (int)ILQG_PARAM_WEIGHT, (int)ILQG_PARAM_VALUE);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(abi.InstanceParam), abi.InstanceParam.term.offset, abi.InstanceParam.field.offset,
                   abi.ABI_VERSION, abi.PARAM_WEIGHT, abi.PARAM_VALUE]
    assert abi.ABI_VERSION == 9
    assert abi.PARAM_FIELDS == {"weight": abi.PARAM_WEIGHT, "value": abi.PARAM_VALUE}


def test_library_reports_the_abi_version_of_the_mirror(hip):
    assert hip.lib().ilqg_abi_version() == abi.ABI_VERSION


def test_term_names_point_at_the_named_terms():
    s = examples.modified_three_player_intersection()
    assert s.term_index("p1_nominal_speed") == 11  # quadratic(0, 10.0, P1V, 8.0)
    t = s.terms[11]
    assert (t["kind"], t["player"], t["idx"][0], t["weight"], t["value"]) == (abi.COST_QUADRATIC, 0, 4, 10.0, 8.0)
    assert s.terms[s.term_index("p2_proximity_p1")]["kind"] == abi.COST_PROXIMITY
    assert s.terms[s.term_index("p3_lane")]["kind"] == abi.COST_QUADRATIC_POLYLINE2
    r = examples.three_player_collision_avoidance_reachability()
    t = r.terms[r.term_index("p2_u1_max")]
    assert (t["kind"], t["player"], t["value"]) == (abi.CONSTRAINT_SINGLE_DIMENSION, 1, 0.1) and t["constraint_slot"] >= 0
    assert r.terms[r.term_index("p1_distance_child1")]["role"] == abi.ROLE_CHILD
    with pytest.raises(KeyError):
        s.term_index("no such term")
    # names are no part of the descriptor
    named, _k1 = s.build(abi.F64)
    plain = examples.modified_three_player_intersection()
    plain.term_names = {}
    other, _k2 = plain.build(abi.F64)
    assert named.num_terms == other.num_terms == 30
    assert C.string_at(named.terms, C.sizeof(abi.CostTerm) * 30) == C.string_at(other.terms, C.sizeof(abi.CostTerm) * 30)


ACCEPTED = [
    (examples.modified_three_player_intersection,
     [("p1_nominal_speed", "value"), ("p1_nominal_speed", "weight"), ("p2_lane", "weight"), ("p1_proximity_p2", "weight"),
      ("p1_proximity_p2", "value"), (1, "value"), (18, "weight")]),  # 1: a lane boundary's threshold, 18: a control cost
    (examples.three_player_collision_avoidance_reachability,
     [("p1_u0_max", "value"), ("p3_u1_min", "value"), ("p2_distance_child0", "value"), (0, "weight")]),
    (examples.three_player_intersection_reachability,
     [("p1_distance_p2", "value"), ("p1_distance_p3", "value"), ("p3_proximity_p1", "weight"), ("p2_lane", "weight")]),
    (lambda: examples.mixed_dubins_car_scene(constrained=True),
     [("p1_goal_x", "value"), ("p2_clearance_p1", "value"), ("p2_speed_max", "value"), ("p1_turn_rate_max", "value")]),
]


@pytest.mark.parametrize("make,params", ACCEPTED)
def test_check_accepts(hip, make, params):
    hip.instance_params_check(make(), params)
    hip.instance_params_check(make(), [])


def _refused(hip, spec, params, term, *words):
    with pytest.raises(hip.IlqgError) as e:
        hip.instance_params_check(spec, params)
    assert e.value.status == abi.ERR_UNSUPPORTED, str(e.value)
    msg = str(e.value)
    assert "term %d" % term in msg, msg
    for w in words:
        assert w in msg, msg


def test_check_refuses_with_a_message_naming_the_term(hip):
    s = examples.modified_three_player_intersection()
    _refused(hip, s, [(30, "weight")], 30, "out of range")
    _refused(hip, s, [(-1, "value")], -1, "out of range")
    _refused(hip, s, [("p1_nominal_speed", "value"), ("p2_lane", "weight"), ("p1_nominal_speed", "value")], 11, "twice")
    _refused(hip, s, [("p1_lane", "value")], 0, "QUADRATIC_POLYLINE2")
    _refused(hip, s, [(11, 2)], 11, "ilqg_param_field")
    r = examples.three_player_collision_avoidance_reachability()
    ext = r.terms[r.term_index("p1_distance_child1") + 1]
    assert ext["kind"] == abi.COST_EXTREME_VALUE
    _refused(hip, r, [(r.term_index("p1_distance_child1") + 1, "weight")], r.term_index("p1_distance_child1") + 1, "EXTREME_VALUE")
    _refused(hip, r, [(r.term_index("p1_distance_child1") + 1, "value")], r.term_index("p1_distance_child1") + 1, "EXTREME_VALUE")
    _refused(hip, r, [("p1_distance_child0", "weight")], r.term_index("p1_distance_child0"), "SIGNED_DISTANCE", "weight")
    _refused(hip, r, [("p1_u0_max", "weight")], r.term_index("p1_u0_max"), "CONSTRAINT_SINGLE_DIMENSION", "weight")
    m = examples.mixed_dubins_car_scene(constrained=True)
    _refused(hip, m, [("p2_clearance_p1", "weight")], m.term_index("p2_clearance_p1"), "CONSTRAINT_PROXIMITY")
    z = examples.cost_zoo_scene()
    kinds = [t["kind"] for t in z.terms]
    for kind, field, word in ((abi.COST_NOMINAL_PATH_LENGTH, "value", "tabulated"), (abi.COST_ROUTE_PROGRESS, "value", "tabulated"),
                              (abi.COST_POLYLINE2_SIGNED_DISTANCE, "weight", "weight"),
                              (abi.CONSTRAINT_POLYLINE2_SIGNED_DISTANCE, "weight", "weight"),
                              (abi.COST_CURVATURE, "value", "CURVATURE")):
        if kind in kinds:
            _refused(hip, z, [(kinds.index(kind), field)], kinds.index(kind), word)
    if abi.COST_NOMINAL_PATH_LENGTH in kinds:
        hip.instance_params_check(z, [(kinds.index(abi.COST_NOMINAL_PATH_LENGTH), "weight")])
    a = examples.affine_constraint_scene()
    kinds = [t["kind"] for t in a.terms]
    for kind in (abi.CONSTRAINT_AFFINE_SCALAR, abi.CONSTRAINT_AFFINE_VECTOR):
        for field in ("weight", "value"):
            _refused(hip, a, [(kinds.index(kind), field)], kinds.index(kind), "dense")


def test_cpp_mirror_resolves_objects_to_the_terms_the_builder_names():
    """tests/host/instance_params_demo.cpp builds the headline scene with the mirrored classes and declares three of its
    cost objects: the flattener resolves each to the term that examples.py names (the flattener orders terms player by
    player, so the INDEX differs from the Python builder's; the term is the same one)."""
    import __graft_entry__
    exe = os.path.join(ROOT, "tests", "host", "_bin", "instance_params_demo")
    if not os.path.exists(exe):
        __graft_entry__.build_host()
    lines = subprocess.check_output([exe, "resolve"], text=True, timeout=120).splitlines()
    got = [tuple(int(v) for v in ln.split()) for ln in lines[:3]]
    assert lines[3].split() == ["stray", "0"]
    dump = abi.ProblemSpec.from_dump("\n".join(lines[4:]))
    s = examples.modified_three_player_intersection()
    assert dump.canonical() == s.canonical()
    for (term, field), (name, want_field) in zip(got, (("p1_nominal_speed", abi.PARAM_VALUE), ("p2_lane", abi.PARAM_WEIGHT),
                                                       ("p1_proximity_p2", abi.PARAM_WEIGHT))):
        assert field == want_field
        a, b = dump.terms[term], s.terms[s.term_index(name)]
        for k in ("kind", "role", "player", "idx", "flags"):
            assert a[k] == b[k], (name, k)
        assert np.float32(a["weight"]) == np.float32(b["weight"]) and np.float32(a["value"]) == np.float32(b["value"])
        # and it is the only such term: the index is not ambiguous
        same = [q for q, t in enumerate(dump.terms) if all(t[k] == a[k] for k in ("kind", "player", "idx", "value"))]
        assert same == [term]
