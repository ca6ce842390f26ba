"""Per-instance solver parameters, the checks that need no GPU: the C header's ilqg_solver_field against the ctypes
mirror, what ilqg_instance_solver_params_check accepts and refuses (host only: the library is loaded without a device),
and the C++ mirror's hand-out of InstanceParams::AddSolverParam."""
import os
import subprocess
import tempfile

import pytest

from ilqgames_amd import abi, examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARABLE = ["convergence_tolerance", "max_solver_iters", "initial_alpha_scaling", "geometric_alpha_scaling",
              "max_backtracking_steps", "expected_decrease_fraction", "unconstrained_solver_max_iters",
              "geometric_mu_scaling", "geometric_mu_downscaling", "geometric_lambda_downscaling",
              "constraint_error_tolerance"]


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return h


def test_solver_field_enum_matches_the_c_header_and_the_struct_order():
    names = [n.upper() for n in abi.SOLVER_FIELD_NAMES]
    src = '#include <stdio.h>\n#include "ilqg.h"\nint main(void) {\n  printf("' + "%d " * (len(names) + 2) + '\\n", ' + \
        ", ".join("(int)ILQG_SOLVER_" + n for n in names) + ", (int)ILQG_NUM_SOLVER_FIELDS, (int)ILQG_MAX_INSTANCE_PARAMS);\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got == list(range(13)) + [13, abi.MAX_INSTANCE_PARAMS]
    # a field's number is its member's place in ilqg_solver_params
    assert [f[0] for f in abi.SolverParams._fields_] == list(abi.SOLVER_FIELD_NAMES)
    assert set(abi.SOLVER_FIELDS) - set(DECLARABLE) == {"linesearch", "open_loop"}
    ints = {f[0] for f in abi.SolverParams._fields_ if f[1] is not abi.C.c_float}
    assert ints - {"linesearch", "open_loop"} == set(abi.SOLVER_INT_FIELDS)


def test_check_accepts_every_declarable_field(hip):
    spec = examples.modified_three_player_intersection()
    hip.instance_solver_params_check(spec, DECLARABLE)
    hip.instance_solver_params_check(spec, [abi.SOLVER_FIELDS[n] for n in reversed(DECLARABLE)])
    for name in DECLARABLE:
        hip.instance_solver_params_check(spec, [name])
    hip.instance_solver_params_check(spec, [])


def _refused(hip, fields, status, text, count=None):
    with pytest.raises(hip.IlqgError) as e:
        hip.instance_solver_params_check(examples.modified_three_player_intersection(), fields, count=count)
    assert e.value.status == status, str(e.value)
    assert str(e.value) == "ilqg status %d: %s" % (status, text)


def test_check_refuses_with_literal_messages(hip):
    kernels = "it selects kernels and the host's schedule and cannot vary per instance"
    _refused(hip, ["initial_alpha_scaling", "linesearch"], abi.ERR_UNSUPPORTED,
             "instance parameter 1 (solver field linesearch): " + kernels)
    _refused(hip, ["open_loop"], abi.ERR_UNSUPPORTED, "instance parameter 0 (solver field open_loop): " + kernels)
    for bad in (13, -1, 1000):
        _refused(hip, ["max_solver_iters", bad], abi.ERR_UNSUPPORTED,
                 "instance parameter 1 (solver field %d): not an ilqg_solver_field" % bad)
    _refused(hip, ["initial_alpha_scaling", "max_solver_iters", "initial_alpha_scaling"], abi.ERR_UNSUPPORTED,
             "instance parameter 2 (solver field initial_alpha_scaling): declared twice (also parameter 0)")
    count_text = "instance solver parameters: count must be 0 .. ILQG_MAX_INSTANCE_PARAMS"
    _refused(hip, ["initial_alpha_scaling"], abi.ERR_INVALID, count_text, count=-1)
    # A total over the maximum.  This host-only check sees no handle and so no cost or subsystem columns: the one total
    # it can refuse is a solver count above what the table may hold, whatever the fields name, and that is its count
    # message.  The three-group refusal, with the three counts in its text, is the handle's:
    # tests/test_gpu_instance_solver_params.py::test_declaration_and_binding_refusals.
    _refused(hip, ["initial_alpha_scaling"] * (abi.MAX_INSTANCE_PARAMS + 1), abi.ERR_INVALID, count_text)


def test_cpp_mirror_hands_out_the_field_list_the_python_harness_declares(hip):
    """tests/host/instance_solver_params_demo.cpp resolve: ResolveInstanceParams returns the fields AddSolverParam named,
    in order, as the numbers the Python harness passes for the same names; open_loop resolves and is refused by the
    library by name; fields named to a caller that takes none are an error, not dropped."""
    import __graft_entry__
    exe = os.path.join(ROOT, "tests", "host", "_bin", "instance_solver_params_demo")
    if not os.path.exists(exe):
        __graft_entry__.build_host()
    lines = subprocess.check_output([exe, "resolve"], text=True, timeout=120).splitlines()
    names = ["initial_alpha_scaling", "expected_decrease_fraction", "max_backtracking_steps", "max_solver_iters"]
    arr, count = hip._instance_solver_fields(names)
    assert [ln.split() for ln in lines[:4]] == [["field", str(arr[c])] for c in range(count)]
    assert lines[4] == "open_loop %d instance parameter 0 (solver field open_loop): it selects kernels and the host's " \
                       "schedule and cannot vary per instance" % abi.ERR_UNSUPPORTED
    assert lines[5] == "nofields 0 instance parameters name solver fields, the caller takes none"
    dump = abi.ProblemSpec.from_dump("\n".join(lines[6:]))
    assert dump.canonical() == examples.modified_three_player_intersection().canonical()
