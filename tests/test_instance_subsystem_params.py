"""Per-instance subsystem parameters, the checks that need no GPU: the two prototypes of the C header, what
ilqg_instance_subsystem_params_check accepts and refuses (host only: the library is loaded without a device, as
tests/test_instance_params.py does), and the C++ mirror's resolution of AddSubsystem(object) / AddSubsystem(row) to rows
of the descriptor."""
import os
import subprocess
import tempfile

import pytest

from ilqgames_amd import abi, examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KIND_NAMES = {abi.DYN_UNICYCLE_4D: "UNICYCLE_4D", abi.DYN_UNICYCLE_4D_DISTURBED: "UNICYCLE_4D_DISTURBED",
              abi.DYN_PLANAR_DISTURBANCE: "PLANAR_DISTURBANCE", abi.DYN_POINT_MASS_2D: "POINT_MASS_2D",
              abi.DYN_UNICYCLE_5D: "UNICYCLE_5D"}


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return h


def test_c_header_declares_both_calls_and_keeps_abi_version_9():
    """The snippet takes the address of both functions with their exact prototypes: a missing or differently typed
    declaration does not compile (-Werror)."""
    src = r'''
#include <stdio.h>
#include "ilqg.h"
typedef ilqg_status (*declare_fn)(ilqg_problem*, int32_t, const int32_t*);
typedef ilqg_status (*check_fn)(const ilqg_problem_desc*, int32_t, const int32_t*);
int main(void) {
  declare_fn d = &ilqg_problem_declare_instance_subsystem_params;
  check_fn c = &ilqg_instance_subsystem_params_check;
  (void)d;
  (void)c;
  printf("%d %d\n", (int)ILQG_ABI_VERSION, (int)ILQG_MAX_INSTANCE_PARAMS);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        obj = os.path.join(td, "t.o")
        subprocess.check_call(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", c, "-o", obj])
        pre = subprocess.check_output(["gcc", "-E", "-dM", "-I", os.path.join(ROOT, "include"), "-include", "ilqg.h",
                                       "-x", "c", os.devnull], text=True)
    defs = dict(ln.split()[1:3] for ln in pre.splitlines() if ln.startswith("#define ILQG_") and len(ln.split()) >= 3)
    assert int(defs["ILQG_ABI_VERSION"]) == abi.ABI_VERSION == 9
    assert int(defs["ILQG_MAX_INSTANCE_PARAMS"]) == 256


def test_library_exports_both_calls(hip):
    assert "ilqg_problem_declare_instance_subsystem_params" in hip.EXPORTS
    assert "ilqg_instance_subsystem_params_check" in hip.EXPORTS
    for name in hip.EXPORTS:
        assert hasattr(hip.lib(), name), name
    assert hip.lib().ilqg_abi_version() == 9


ACCEPTED = [
    (examples.modified_three_player_intersection, [0, 1], (abi.DYN_CAR_5D, abi.DYN_CAR_5D)),
    (examples.mixed_dubins_car_scene, [0, 1], None),
    (examples.dynamics_zoo_scene, [0], (abi.DYN_CAR_7D,)),
    (examples.delayed_dubins_scene, [0, 1], None),
    (examples.air_3d, [0, 1], (abi.DYN_AIR_3D_EVADER, abi.DYN_AIR_3D_PURSUER)),
]


@pytest.mark.parametrize("make,rows,kinds", ACCEPTED)
def test_check_accepts(hip, make, rows, kinds):
    spec = make()
    if kinds is not None:
        assert tuple(spec.subsystems[r][0] for r in rows) == kinds
    hip.instance_subsystem_params_check(spec, rows)
    hip.instance_subsystem_params_check(spec, list(reversed(rows)))  # columns are in the caller's order
    for r in rows:
        hip.instance_subsystem_params_check(spec, [r])
    hip.instance_subsystem_params_check(spec, [])


def test_accepted_scenes_cover_every_kind_that_reads_param0():
    kinds = set()
    for make, rows, _ in ACCEPTED:
        spec = make()
        kinds |= {spec.subsystems[r][0] for r in rows}
    assert kinds >= {abi.DYN_CAR_5D, abi.DYN_CAR_7D, abi.DYN_DUBINS_CAR, abi.DYN_DELAYED_DUBINS_CAR,
                     abi.DYN_AIR_3D_EVADER, abi.DYN_AIR_3D_PURSUER}
    assert examples.roundabout_merging().subsystems[0][0] == abi.DYN_CAR_6D


def test_check_accepts_car_6d(hip):
    hip.instance_subsystem_params_check(examples.roundabout_merging(), [0, 1, 2, 3])


def _refused(hip, spec, rows, row, *words):
    with pytest.raises(hip.IlqgError) as e:
        hip.instance_subsystem_params_check(spec, rows)
    assert e.value.status == abi.ERR_UNSUPPORTED, str(e.value)
    msg = str(e.value)
    assert "subsystem %d" % row in msg, msg
    for w in words:
        assert w in msg, msg


def _refused_kind(hip, spec, row):
    kind = spec.subsystems[row][0]
    assert kind in KIND_NAMES, (row, kind)
    _refused(hip, spec, [row], row, KIND_NAMES[kind])


def test_check_refuses_with_a_message_naming_the_subsystem_and_its_kind(hip):
    s = examples.modified_three_player_intersection()
    assert s.subsystems[2][0] == abi.DYN_UNICYCLE_4D
    _refused_kind(hip, s, 2)
    _refused(hip, s, [0, 2], 2, "UNICYCLE_4D")  # one refused row refuses the declaration
    z = examples.dynamics_zoo_scene()
    assert z.subsystems[1][0] == abi.DYN_UNICYCLE_5D
    _refused_kind(hip, z, 1)
    a = examples.modified_air_3d()
    assert a.subsystems[0][0] == abi.DYN_POINT_MASS_2D
    _refused_kind(hip, a, 0)
    u = examples.two_player_unicycle_4d_scene()
    assert [sub[0] for sub in u.subsystems] == [abi.DYN_UNICYCLE_4D_DISTURBED, abi.DYN_PLANAR_DISTURBANCE]
    _refused_kind(hip, u, 0)
    _refused_kind(hip, u, 1)
    # rows out of range, the same row twice
    _refused(hip, s, [-1], -1, "out of range")
    _refused(hip, s, [len(s.subsystems)], len(s.subsystems), "out of range")
    _refused(hip, s, [0, 1, 0], 0, "twice")


def test_check_refuses_more_columns_than_the_table_may_hold(hip):
    """Every row over the eight a problem can have is a duplicate or out of range, and a count over
    ILQG_MAX_INSTANCE_PARAMS is refused before any row is looked at; the sum with the declared cost columns is the
    handle's to check, and a handle needs a device
    (tests/test_gpu_instance_subsystem_params.py::test_cost_and_subsystem_columns_together_may_not_exceed_the_maximum)."""
    s = examples.modified_three_player_intersection()
    with pytest.raises(hip.IlqgError) as e:
        hip.instance_subsystem_params_check(s, [0] * 257)
    assert e.value.status == abi.ERR_INVALID and "ILQG_MAX_INSTANCE_PARAMS" in str(e.value)
    _refused(hip, s, [0, 1] * 128, 0, "twice")


def test_cost_field_2_stays_refused(hip):
    """Subsystem parameters have a call of their own: no third ilqg_param_field."""
    with pytest.raises(hip.IlqgError) as e:
        hip.instance_params_check(examples.modified_three_player_intersection(), [(11, 2)])
    assert e.value.status == abi.ERR_UNSUPPORTED and "ilqg_param_field" in str(e.value)


def _demo():
    import __graft_entry__
    exe = os.path.join(ROOT, "tests", "host", "_bin", "instance_subsystem_params_demo")
    if not os.path.exists(exe):
        __graft_entry__.build_host()
    return exe


def test_cpp_mirror_resolves_subsystem_objects_to_rows():
    """tests/host/instance_subsystem_params_demo.cpp resolve: the headline scene built with the mirrored classes,
    AddSubsystem(object) of its two cars -> rows 0 and 1 (and the cost column beside them -> its term), a car of another
    system -> false with a reason, AddSubsystem(3) -> false, the pedestrian's row -> refused by the library, subsystems
    named to a caller that takes none -> false; the description it flattens is the builder's."""
    lines = subprocess.check_output([_demo(), "resolve"], text=True, timeout=120).splitlines()
    assert lines[0].split()[0] == "term" and int(lines[0].split()[2]) == abi.PARAM_VALUE
    assert lines[1:3] == ["row 0", "row 1"]
    foreign = lines[3].split(None, 2)
    assert foreign[:2] == ["foreign", "0"] and "no subsystem of the problem" in foreign[2]
    row3 = lines[4].split(None, 2)
    assert row3[:2] == ["row3", "0"] and "row 3" in row3[2]
    walker = lines[5].split(None, 2)
    assert walker[0] == "walker" and int(walker[1]) == abi.ERR_UNSUPPORTED
    assert "subsystem 2" in walker[2] and "UNICYCLE_4D" in walker[2]
    norows = lines[6].split(None, 2)
    assert norows[:2] == ["norows", "0"] and "subsystems" in norows[2]
    dump = abi.ProblemSpec.from_dump("\n".join(lines[7:]))
    s = examples.modified_three_player_intersection()
    assert dump.canonical() == s.canonical()
    t = dump.terms[int(lines[0].split()[1])]
    b = s.terms[s.term_index("p1_nominal_speed")]
    assert all(t[k] == b[k] for k in ("kind", "role", "player", "idx", "flags"))


def test_existing_demo_resolve_output_keeps_its_form():
    """tests/host/instance_params_demo.cpp is untouched: three (term, field) lines, the stray line, the dump."""
    exe = os.path.join(ROOT, "tests", "host", "_bin", "instance_params_demo")
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build_host()
    lines = subprocess.check_output([exe, "resolve"], text=True, timeout=120).splitlines()
    assert [len(ln.split()) for ln in lines[:3]] == [2, 2, 2]
    assert lines[3] == "stray 0"
    assert abi.ProblemSpec.from_dump("\n".join(lines[4:])).canonical() == examples.modified_three_player_intersection().canonical()
