"""The solve schedule on the host alone: every case of tests/golden/schedule_cases.json — what solves on an MI355X chose,
recorded by tests/golden/make_schedule_cases.py from the library before the schedule moved into csrc/ilqg_schedule.hpp —
replayed through ilqg_schedule_build with the recorded CU count, field by field; and the recorded probing rounds through
the per-round functions, in a stand-alone program built with plain g++ (once more with sanitizers)."""
import json
import os
import subprocess

import pytest

import schedule_cases as sc
from ilqgames_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "schedule_cases.json")))
C = GOLDEN["num_cus"]
K_BOUND, PROG_IDS = 1000, {0: 0, 1: -1, 2: -2}  # kBoundProg, kExprProg, kExprDynProg (csrc/ilqg_solve.hpp)

# recorded field -> the same fact from ilqg_schedule_info, where it is not the member of that name
DERIVED = {
    # (the fused kernel's structure as the solve ran it: none under a split pass)
    "static_prog": lambda s: 0 if s["split"] else s["static_prog"],
    "trial_prog": lambda s: (s["static_prog"] or PROG_IDS[s["prog_kind"]]) + K_BOUND * s["bound"],
    "rows_prog": lambda s: s["static_id"] + K_BOUND * s["bound"] if s["static_id"] else PROG_IDS[s["prog_kind"]],
    "prows_prog": lambda s: s["static_id"] + K_BOUND * s["bound"] if s["static_id"] else PROG_IDS[s["prog_kind"]],
    "decide_solver": lambda s: s["decide_solver"] if s["lists"] else -1,  # (-1: the solve binds no split kernels)
    "roll_xdyn": lambda s: int(s["prog_kind"] == 2) if s["lists"] else -1,
    "lds_proll_fat": lambda s: s["lds_proll"],
    "has_proll_single": lambda s: s["proll_single"],
    "has_proll_lanes": lambda s: s["proll_lanes"],
}

CASES = sc.decode_cases(GOLDEN)
GROUPS = sorted({c[:3] for c in CASES}, key=str)


def replay(scene, dtype, T, batch, oname, active, num_cus=C):
    opts = sc.OPTION_SETS[oname]
    spec = sc.make_spec(scene, T, bool(opts.get("open_loop")))
    kw = sc.solve_kwargs(opts)
    if active < 0:
        kw["fixed_iters"] = 1
    return hip.schedule_build(spec, dtype, batch, num_cus, active=None if active < 0 else active,
                              tables_bound=opts.get("bind") == "tables", solver_bound=opts.get("bind") == "solver", **kw)


def test_golden_holds_every_case():
    """The file is the generator's full product: every scene, horizon, precision, batch and option set (decode_cases
    fails on a file that holds fewer or more), every specialised solve with its finer record."""
    assert GOLDEN["scenes"] == list(sc.SCENES) and GOLDEN["option_sets"] == list(sc.OPTION_SETS)
    assert len(CASES) == sum(len(keys) for _, keys in sc.case_blocks(sc.SCENES, sc.OPTION_SETS, C))
    fields = {f for g in sc.FIELD_GROUPS.values() for f in g}
    assert all(set(rec) == ({"word"} if rec["word"] & 32 else fields) for *_, rec in CASES)  # (32: ILQG_SCHEDULE_GENERIC)


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "%s-%s-T%d" % (g[0], ("f32", "f64")[g[1]], g[2]))
def test_replay(group):
    wrong, count = [], 0
    for scene, dtype, T, batch, oname, active, rec in CASES:
        if (scene, dtype, T) != group:
            continue
        count += 1
        got = replay(scene, dtype, T, batch, oname, active)
        for f, want in rec.items():
            have = DERIVED[f](got) if f in DERIVED and len(rec) > 1 else got[f]
            if have != want:
                wrong.append((oname, batch, f, want, have))
        if got["packed"] != int(got["sweep_kind"] == 3):
            wrong.append((oname, batch, "packed", got["sweep_kind"], got["packed"]))
    assert count > 0 and not wrong, "%d of %d cases differ, the first: %s" % (len({w[:2] for w in wrong}), count, wrong[:8])


# ---- the per-round functions, stand-alone ----
def _build_checker(out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + list(extra) +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ilqgames_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "schedule_check.cpp"), "-o", out])
    return out


def _round_requests():
    """(request lines, expected reply lines) of every recorded probing round and probing launch."""
    info = replay("n15", 1, 8, 4, "default", -1)
    limits = (info["probe_max"], info["probe_budget"])
    req, want = [], []
    for row in GOLDEN["rounds"]["rows"]:
        r = dict(zip(GOLDEN["rounds"]["fields"], row))
        # the deep-search state the round began in: what it ended in, unless this is the round whose rule sets it
        rule = r["deep_rule"] and r["tail_rounds"] == 3 and 2 * r["instances"] >= r["tail_first"]
        deep_in = 0 if rule else r["deep_out"]
        req.append("R %d %d %d %d %d %d %d %d %d %d %d %d" % (limits + (
            r["deep_rule"], r["pairs"], r["lane_width"], r["pool_entries"], r["instances"], r["probe_first"], r["probe_lanes"],
            r["tail_rounds"], r["tail_first"], deep_in)))
        want.append("R %d %d" % (r["probe_k"], r["deep_out"]))
    for row in GOLDEN["forms"]["rows"]:
        r = dict(zip(GOLDEN["forms"]["fields"], row))
        req.append("F %d %d %d %d %d %d %d %d %d" % (r["num_cus"], r["pairs"], r["lane_width"], r["lanes_auto"], r["has_lanes"],
                                                     r["has_single"], r["probe_lanes"], r["instances"], r["probe_k"]))
        want.append("F %d" % r["form"])
    return req, want


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_round_functions(tmp_path, flags):
    exe = _build_checker(str(tmp_path / "schedule_check"), flags)
    req, want = _round_requests()
    assert len(GOLDEN["rounds"]["rows"]) > 100 and len(GOLDEN["forms"]["rows"]) > 100
    out = subprocess.run([exe], input="\n".join(req) + "\n", text=True, capture_output=True, check=True).stdout.splitlines()
    wrong = [(q, w, o) for q, w, o in zip(req, want, out) if w != o]
    assert len(out) == len(want) and not wrong, wrong[:8]


def test_generic_problem_reports_generic_bits():
    got = replay("generic", 1, 8, 4, "default", -1)
    assert got["word"] & 32 and got["rows_cw"] == 0 and got["lds_trial"] == 0


def test_refusals():
    spec = sc.make_spec("n4", 8)
    with pytest.raises(hip.IlqgError):
        hip.schedule_build(spec, 1, 0, C)
    with pytest.raises(hip.IlqgError):
        hip.schedule_build(spec, 1, 4, 0)
