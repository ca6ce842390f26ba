"""Per-instance solver parameters on the device (ilqg_problem_declare_instance_solver_params): a line search, a
stopping rule and an augmented-Lagrangian schedule for each game of a batch.

As for the other per-instance columns (shared check: tests/instance_harness.py) the checks are EXACT: an instance of a
heterogeneous batch must return the bits of the same instance solved in a problem created with its vector written into
ilqg_problem_desc::params — the values are floats on both paths and enter the arithmetic at the same place — over every
instance and every output array.  The integer members are swept BELOW the descriptor's values, which are their ceilings;
what happens at and above the ceiling is test_ceiling_of_the_integer_members."""
import copy
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ilqgames_amd import abi, examples
from instance_harness import KEYS, check_baked_equals_bound, headline as _headline, same_bits as _same_bits, to_numpy as _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED_ERROR = "instance parameters cannot be declared while values are bound: unbind first"


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


LINE_SEARCH = ["initial_alpha_scaling", "geometric_alpha_scaling", "expected_decrease_fraction", "max_backtracking_steps",
               "convergence_tolerance", "max_solver_iters"]
AL_FIELDS = ["geometric_mu_scaling", "geometric_mu_downscaling", "geometric_lambda_downscaling",
             "constraint_error_tolerance", "unconstrained_solver_max_iters"]
ALL_FIELDS = [n for n in abi.SOLVER_FIELD_NAMES if n not in ("linesearch", "open_loop")]

# The headline scene (descriptor: 0.1, 0.5, 0.001, 100 back-tracking steps, tolerance 1, 25 iterations) under four
# vectors of LINE_SEARCH, chosen on the CPU with the oracle's SolveILQ at examples.jittered_x0(spec, 12, seed=6), fp64 and
# fp32 (instance b takes vector b % 4; the merit function starts near 6e5 and falls by thousands per iteration):
#   0  a full first step under a 0.3 Armijo fraction: every one of instances 0, 4, 8 rejects 14 .. 51 steps in one of its
#      searches, accepts the next and goes on to end with status 1 (the accepted steps are tiny, so a rounding can turn one
#      of the three into a failed search on the device: one is enough)                     -> BACK-TRACKED AND WENT ON
#   1  the bench's pair 0.1 / 0.001 with tolerance 2e4: instances 1, 5, 9 converge after 25, 13 and 15 iterations, no
#      step rejected                                                                     -> CONVERGED, NO REJECTED STEP
#   2  the example's own pair 1.0 / 0.9 with THREE back-tracking steps: instances 2, 6, 10 fail their second to fifth
#      search, status 0                                                            -> GAVE UP AT ITS OWN DEPTH, 3 < 100
#   3  the bench's pair with FOUR iterations: instances 3, 7, 11 stop after four, not converged, status 1
#                                                                                  -> STOPPED AT ITS OWN CAP, 4 < 25
CLASS_VECTORS = np.array([[1.0, 0.5, 0.3, 100, 1.0, 25],
                          [0.1, 0.5, 0.001, 100, 2e4, 25],
                          [1.0, 0.5, 0.9, 3, 1.0, 25],
                          [0.1, 0.5, 0.001, 100, 1.0, 4]], dtype=np.float32)


def _own(spec, fields):
    return np.array([getattr(spec.params, f) for f in fields], dtype=np.float32)


def _baked(spec, fields, row, cost=(), subs=()):
    """The spec with one vector written in: [cost | subsystem | solver] columns, an integer member truncated."""
    s = copy.deepcopy(spec)
    row = list(row)
    for (name, field) in cost:
        s.terms[s.term_index(name)][field] = float(np.float32(row.pop(0)))
    for r in subs:
        kind, xd, ud, _ = s.subsystems[r]
        s.subsystems[r] = (kind, xd, ud, float(np.float32(row.pop(0))))
    for f, v in zip(fields, row):
        setattr(s.params, f, int(v) if f in abi.SOLVER_INT_FIELDS else float(np.float32(v)))
    return s


def _bound(hip, spec, dtype, fields, table, cost=(), subs=(), order="csv"):
    """The problem with the table bound; `order`: in which the cost, subsystem and solVer declarations are made."""
    prob = hip.Problem(spec, dtype)
    for what in order:
        if what == "c" and cost:
            prob.declare_instance_params(list(cost))
        elif what == "s" and subs:
            prob.declare_instance_subsystem_params(list(subs))
        elif what == "v":
            prob.declare_instance_solver_params(fields)
    prob.bind_instance_values(table)
    return prob


def _check(hip, spec, dtype, fields, vectors, **kw):
    vectors = np.asarray(vectors, dtype=np.float32)
    return check_baked_equals_bound(hip, spec, dtype, lambda table: _bound(hip, spec, dtype, fields, table),
                                    lambda row: _baked(spec, fields, row), vectors, **kw)


def _line_search_vectors(spec):
    """Four vectors of LINE_SEARCH about a scene's own parameters, the integer members at or below them."""
    a0, g, fr, bt, tol, it = (float(v) for v in _own(spec, LINE_SEARCH))
    return np.array([[a0, g, fr, bt, tol, it],
                     [0.5 * a0, 0.7, min(0.9, 10.0 * fr), min(bt, 5), 4.0 * tol, it],
                     [min(1.0, 2.0 * a0), 0.5, fr, bt, tol, max(2, int(it) // 2)],
                     [a0, 0.25, 0.5, 3, tol, it]], dtype=np.float32)


# ---- 1. bound equals baked, bit for bit ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("split_trial", [True, False])
@pytest.mark.parametrize("fixed_iters", [0, 6])
def test_headline_line_search_vectors_bound_equal_baked(hip, dtype, split_trial, fixed_iters):
    """deterministic: the partner solves its three instances alone.  split_trial off: the fused trial kernel's decision
    section; on: the decision kernel.  fixed_iters: the tolerance and the cap are not read, the line search is."""
    _check(hip, _headline(), dtype, LINE_SEARCH, CLASS_VECTORS, deterministic=True, split_trial=split_trial,
           fixed_iters=fixed_iters)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("probe_lanes", [None, True, False])
def test_handoff_and_probing_bound_equal_baked(hip, dtype, probe_lanes):
    """Hand-off and probing at AUTO (None: every option the library's choice), then the split passes with the probing
    rollouts a lane per candidate and two candidates per wavefront.  Vector 0's searches reject dozens of steps and vector
    2's end at a depth of three: the probing kernels read each instance's own depth and scaling."""
    kw = {} if probe_lanes is None else dict(split_trial=True, probe_lanes=probe_lanes)
    prob, out, x0, which = _check(hip, _headline(), dtype, LINE_SEARCH, CLASS_VECTORS, whole_batch_partner=True, **kw)
    o = prob.solve(x0, **kw)
    assert int(_np(prob.solve_state(o)["backtracks"]).sum()) > 0, "the line searches should back-track: nothing was probed"


# ---- 2. the batch is not vacuous ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_the_batch_holds_every_class_of_line_search_outcome(hip, dtype):
    """CLASS_VECTORS above says which vector gives which class and how they were chosen (the oracle alone produces all
    four at this x0).  Vector 0: back-tracked and went on; 1: converged with no rejected step; 2: gave up at its OWN
    max_backtracking_steps (3, the descriptor's is 100); 3: stopped at its OWN max_solver_iters (4, the descriptor's 25)."""
    spec = _headline()
    B = 12
    x0 = examples.jittered_x0(spec, B, seed=6)
    which = np.arange(B) % 4
    prob = _bound(hip, spec, dtype, LINE_SEARCH, CLASS_VECTORS[which])
    o = prob.solve(x0)
    status, iters, conv = (_np(o[k]) for k in ("status", "iters", "converged"))
    rejected = _np(prob.solve_state(o)["backtracks"])
    print("status", status, "iters", iters, "converged", conv, "rejected", rejected)
    went_on = (which == 0) & (rejected > 0) & (status == 1)
    clean = (which == 1) & (conv == 1) & (rejected == 0) & (status == 1)
    own_depth, depth = int(CLASS_VECTORS[2, 3]), spec.params.max_backtracking_steps
    gave_up = (which == 2) & (status == 0) & (rejected >= own_depth) & (rejected < depth)
    own_cap, cap = int(CLASS_VECTORS[3, 5]), spec.params.max_solver_iters
    capped = (which == 3) & (iters == own_cap) & (conv == 0) & (status == 1)
    assert own_depth < depth and own_cap < cap
    for name, members in (("back-tracked and went on", went_on), ("converged, no rejected step", clean),
                          ("gave up at its own depth", gave_up), ("stopped at its own cap", capped)):
        assert members.any(), name
    # nothing but vector 3 stops at four iterations with status 1, nothing under the descriptor's depth fails after < 100
    assert not ((which != 3) & (iters == own_cap) & (status == 1) & (conv == 0)).any()


# ---- 3. augmented Lagrangian ----
def _avoidance():
    spec = examples.three_player_collision_avoidance_reachability()
    spec.params.max_solver_iters = 12
    spec.params.unconstrained_solver_max_iters = 4
    return spec


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_augmented_lagrangian_schedule_bound_equals_baked(hip, dtype):
    """The exit path's reads: the three geometric_* members, the constraint error tolerance and the inner solves' cap.
    Outer-iteration counts, from `iters` (in this mode the log entries of all inner solves, at most 1 + cap each): the
    constraint error starts at +inf as the reference's does, so the first inner solve is always followed by a multiplier
    update and a second one; under vector 1's tolerance (1e6) the error is below it from then on and the outer loop ends
    — at most TWO inner solves, 2 (1 + 4) entries — while an instance with more entries than that ran at least three."""
    spec = _avoidance()
    mu_s, mu_d, lam_d, cet, cap = (float(v) for v in _own(spec, AL_FIELDS))
    vectors = np.array([[mu_s, mu_d, lam_d, cet, cap],
                        [mu_s, mu_d, lam_d, 1e6, cap],
                        [mu_s, mu_d, lam_d, cet, 1],
                        [2.0 * mu_s, 0.5 * mu_d, 0.5 * lam_d, 0.1 * cet, 3]], dtype=np.float32)
    prob, out, x0, which = _check(hip, spec, dtype, AL_FIELDS, vectors, B=8, deterministic=True, augmented_lagrangian=True)
    two_inner_solves = 2 * (1 + int(cap))
    print("iters", out["iters"], "status", out["status"])
    assert two_inner_solves < spec.params.max_solver_iters
    assert (out["iters"][which == 1] <= two_inner_solves).all()
    assert (out["iters"][which != 1] > two_inner_solves).any()


# ---- 4. the run-time-dimensioned kernels ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("padded_sweep", [True, False])
def test_run_time_dimensioned_kernels_bound_equal_baked(hip, dtype, padded_sweep):
    """The mixed Dubins + Car5D scene: the generic trial and decision kernels, and the first step from the padded
    specialised sweep's kernel or from the run-time-dimensioned sweep's."""
    spec = examples.mixed_dubins_car_scene()
    spec.params.max_solver_iters = 12
    _check(hip, spec, dtype, LINE_SEARCH, _line_search_vectors(spec), B=8, deterministic=True, padded_sweep=padded_sweep)


# ---- 5. the single-wave sweep ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_single_wave_sweep_bound_equals_baked(hip, dtype):
    """Requested at the small batch (the library picks it from five instances per CU); the partner is a whole batch of
    the same size, the same schedule."""
    prob, _, _, _ = _check(hip, _headline(), dtype, LINE_SEARCH, CLASS_VECTORS, whole_batch_partner=True,
                           single_wave_sweep=True, split_trial=True)
    assert prob.last_schedule() & abi.SCHEDULE_SINGLE_WAVE_SWEEP, "the single-wave sweep did not run: nothing was checked"


# ---- 6. the ceiling of the integer members ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_ceiling_of_the_integer_members(hip, dtype):
    """A float at or above the descriptor's value, +inf or NaN in an integer column gives the descriptor's value: the
    unbound problem's bits.  Below it the instance's own value holds: 3 stops at three iterations, a negative value, -inf
    and 0 at none."""
    spec = _headline()
    fields = ["max_solver_iters", "max_backtracking_steps"]
    cap, depth = spec.params.max_solver_iters, spec.params.max_backtracking_steps
    rows = np.array([[1e9, 1e9], [np.inf, np.inf], [np.nan, np.nan], [cap, depth], [cap + 0.5, depth + 1], [3e9, 5e9],
                     [3, depth], [3.9, np.nan], [-5, depth], [-np.inf, depth], [0, depth], [-0.0, 1e9]], dtype=np.float32)
    B = len(rows)
    at_ceiling, three, none = np.arange(0, 6), np.arange(6, 8), np.arange(8, 12)
    x0 = examples.jittered_x0(spec, B, seed=6)
    plain = hip.Problem(spec, dtype).solve(x0, deterministic=True)
    bound = _bound(hip, spec, dtype, fields, rows).solve(x0, deterministic=True)
    for k in KEYS:
        assert _same_bits(_np(bound[k])[at_ceiling], _np(plain[k])[at_ceiling]), k
    iters = _np(bound["iters"])
    assert (_np(plain["iters"]) > 3).all()
    assert (iters[three] == 3).all() and (_np(bound["status"])[three] == 1).all(), iters
    assert (iters[none] == 0).all(), iters
    # ... and they are the three iterations of a problem created with max_solver_iters = 3
    s3 = copy.deepcopy(spec)
    s3.params.max_solver_iters = 3
    ref = hip.Problem(s3, dtype).solve(x0, deterministic=True)
    for k in KEYS:
        assert _same_bits(_np(bound[k])[three], _np(ref[k])[three]), k


# ---- 7. rewriting the table between a solve and solve_again, under a mask ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_solve_again_with_rewritten_table_and_mask(hip, dtype):
    import torch
    spec = _headline()
    spec.params.max_solver_iters = 8
    B, BV = 8, 4
    vals = CLASS_VECTORS.copy()
    vals[:, 5] = [8, 8, 8, 4]
    vals2 = vals[[1, 3, 0, 2]].copy()
    which = np.arange(B) % BV
    x0 = examples.jittered_x0(spec, B, seed=33)
    x0b = examples.jittered_x0(spec, B, seed=34)
    active = np.array([1, 0, 1, 1, 0, 1, 1, 0], dtype=np.int32)
    act_d = torch.as_tensor(active, device="cuda")
    prob = hip.Problem(spec, dtype)
    prob.single_wave_sweep = False  # pinned: the slices below must run the batch's schedule
    prob.declare_instance_solver_params(LINE_SEARCH)
    table = prob.bind_instance_values(torch.as_tensor(vals[which], device="cuda").contiguous())
    bufs = prob.solve(x0)
    first = {k: _np(bufs[k]).copy() for k in KEYS}
    table.copy_(torch.as_tensor(vals2[which], device="cuda"))  # rewritten in place, on the device
    prob.solve_again(x0b, bufs, active=act_d)
    out = {k: _np(bufs[k]) for k in KEYS}
    for b in np.nonzero(active == 0)[0]:
        for k in KEYS:
            assert _same_bits(out[k][b], first[k][b]), ("masked instance touched", b, k)
    followed = False
    for v in range(BV):
        sel = np.nonzero(which == v)[0]
        p1 = hip.Problem(_baked(spec, LINE_SEARCH, vals[v]), dtype)
        p1.single_wave_sweep = False
        rb = p1.solve(x0[sel])
        for k in KEYS:
            assert _same_bits(first[k][sel], _np(rb[k])), (k, v)
        # what the first vector would have done in the second call, to see that the second was followed
        stay = {k: val.clone() for k, val in rb.items() if hasattr(val, "clone")}
        act_sel = act_d[torch.as_tensor(sel, device="cuda")].contiguous()
        p1.solve_again(x0b[sel], stay, active=act_sel)
        # the same solver state carried into a problem with the second vector: its workspace layout is the same
        p2 = hip.Problem(_baked(spec, LINE_SEARCH, vals2[v]), dtype)
        p2.single_wave_sweep = False
        p2.solve_again(x0b[sel], rb, active=act_sel)
        for k in KEYS:
            for j, b in enumerate(sel):
                if active[b]:
                    assert _same_bits(out[k][b], _np(rb[k])[j]), (k, b)
                    followed = followed or not _same_bits(out[k][b], _np(stay[k])[j])
    assert followed, "the second call should differ from what the first table gives"


# ---- 8. identity table ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("scene", ["headline", "avoidance", "mixed"])
def test_identity_table_changes_nothing(hip, dtype, scene):
    """Every declarable member, each column the descriptor's own value."""
    spec, kw = {"headline": (_headline(), {}), "avoidance": (_avoidance(), dict(augmented_lagrangian=True)),
                "mixed": (examples.mixed_dubins_car_scene(), {})}[scene]
    spec.params.max_solver_iters = min(spec.params.max_solver_iters, 12)
    B = 10
    x0 = examples.jittered_x0(spec, B, seed=9)
    prob = hip.Problem(spec, dtype)
    plain = {k: _np(v) for k, v in prob.solve(x0, **kw).items() if k in KEYS}
    assert int(plain["iters"].min()) > 0
    prob.declare_instance_solver_params(ALL_FIELDS)
    prob.bind_instance_values(np.tile(_own(spec, ALL_FIELDS), (B, 1)))
    bound = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(bound[k]), plain[k]), k
    prob.bind_instance_values(None)
    again = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(again[k]), plain[k]), k


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("split_trial", [True, False])
def test_one_handle_unbound_bound_unbound_follows_the_table_of_each_call(hip, dtype, split_trial):
    """The decision kernel has a twin for problems with no solver column bound, picked at every solve: on ONE handle an
    unbound solve, a solve under a table that is NOT the identity (every second instance capped at three iterations, the
    others at the descriptor's own values), and an unbound solve again.  The middle call follows its table — the capped
    instances return the bits of a problem created with the cap, the others the unbound bits — and the calls around it
    do not."""
    spec = _headline()
    spec.params.max_solver_iters = 10
    fields = ["initial_alpha_scaling", "max_solver_iters"]
    B = 8
    x0 = examples.jittered_x0(spec, B, seed=9)
    kw = dict(deterministic=True, split_trial=split_trial)
    table = np.tile(_own(spec, fields), (B, 1))
    capped = np.arange(B) % 2 == 1
    table[capped, 1] = 3
    prob = hip.Problem(spec, dtype)
    plain = {k: _np(v) for k, v in prob.solve(x0, **kw).items() if k in KEYS}
    assert int(plain["iters"].min()) > 3
    prob.declare_instance_solver_params(fields)
    prob.bind_instance_values(table)
    bound = {k: _np(v) for k, v in prob.solve(x0, **kw).items() if k in KEYS}
    assert (bound["iters"][capped] == 3).all(), bound["iters"]
    ref = hip.Problem(_baked(spec, fields, table[1]), dtype).solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(bound[k][capped], _np(ref[k])[capped]), k
        assert _same_bits(bound[k][~capped], plain[k][~capped]), k
    prob.bind_instance_values(None)
    again = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(again[k]), plain[k]), k


# ---- 9. all three column groups in one table ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("order", ["".join(p) for p in itertools.permutations("csv")])
def test_cost_subsystem_and_solver_columns_together(hip, dtype, order):
    """One cost column, one subsystem column and two solver columns, declared in every order: the table is
    [cost | subsystem | solver] all the same."""
    spec = _headline()
    spec.params.max_solver_iters = 10
    cost, subs, fields = [("p1_nominal_speed", "value")], [0], ["initial_alpha_scaling", "max_solver_iters"]
    vectors = np.array([[9.0, 3.0, 0.2, 10], [7.0, 4.5, 0.05, 6]], dtype=np.float32)
    check_baked_equals_bound(hip, spec, dtype, lambda table: _bound(hip, spec, dtype, fields, table, cost, subs, order),
                             lambda row: _baked(spec, fields, row, cost, subs), vectors, B=8, deterministic=True)


# ---- 10. the other entry points ignore solver columns; the handle's refusals ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_other_entry_points_ignore_solver_columns(hip, dtype):
    spec = examples.three_player_intersection_reachability(T=20)
    spec.params.max_solver_iters = 6
    B = 4
    x0 = examples.jittered_x0(spec, B, seed=42)
    plain = hip.Problem(spec, dtype)
    sol = plain.solve(x0, deterministic=True)
    args = [sol[k] for k in ("xs", "us", "P", "alpha")]
    table = np.tile(np.array([0.5, 0.3, 0.7, 2, 50.0, 1], dtype=np.float32), (B, 1)) * np.arange(1, B + 1, dtype=np.float32)[:, None]
    bound = _bound(hip, spec, dtype, LINE_SEARCH, table)

    def calls(p):
        out = [_np(a) for a in p.quadraticize(sol["xs"], sol["us"])]
        out += [_np(a) for a in p.total_costs(sol["xs"], sol["us"])]
        out += [_np(p.strategy_costs(x0, *args)), _np(p.strategy_costs(x0, *args, euler=False))]
        out += [_np(a) for a in p.check_local_nash(x0, *args, max_perturbation=0.1)]
        out += [_np(p.check_sufficient_nash(sol["xs"], sol["us"]))]
        return out
    for q, (a, b) in enumerate(zip(calls(bound), calls(plain))):
        assert _same_bits(a, b), q
    assert not _same_bits(_np(bound.solve(x0, deterministic=True)["xs"]), _np(sol["xs"])), "the solves read the columns"


def test_declaration_and_binding_refusals(hip):
    import torch
    MAX = abi.MAX_INSTANCE_PARAMS
    spec = _headline()
    extra = [spec.quadratic(0, 1.0, d % 5, 0.0) for d in range(MAX // 2)]
    cost = [(t, f) for t in extra for f in ("weight", "value")]
    prob = hip.Problem(spec, abi.F64)
    B = 4

    def refused(call, status, text):
        with pytest.raises(hip.IlqgError) as e:
            call()
        assert e.value.status == status and str(e.value) == "ilqg status %d: %s" % (status, text), str(e.value)

    # bind without a declaration
    table = torch.zeros((B, 2), dtype=torch.float32, device="cuda")
    refused(lambda: hip._check(hip.lib().ilqg_problem_bind_instance_values(prob.h, B, hip._ptr(table))), abi.ERR_INVALID,
            "no instance parameters are declared (ilqg_problem_declare_instance_params)")
    with pytest.raises(ValueError):
        prob.bind_instance_values(table)
    # refused fields are errors on the handle too, and leave nothing declared
    refused(lambda: prob.declare_instance_solver_params(["initial_alpha_scaling", "open_loop"]), abi.ERR_UNSUPPORTED,
            "instance parameter 1 (solver field open_loop): it selects kernels and the host's schedule and cannot vary per instance")
    assert prob.instance_solver_fields == []
    # the total over the maximum, whichever declaration comes last; a refused call leaves the earlier ones standing
    prob.declare_instance_params(cost[:MAX - 4])
    prob.declare_instance_subsystem_params([0, 1])
    prob.declare_instance_solver_params(["initial_alpha_scaling", "max_solver_iters"])  # 252 + 2 + 2: full
    over = "instance parameters: %d cost columns + %d subsystem columns + %d solver columns exceed ILQG_MAX_INSTANCE_PARAMS"
    refused(lambda: prob.declare_instance_solver_params(LINE_SEARCH[:3]), abi.ERR_INVALID, over % (MAX - 4, 2, 3))
    refused(lambda: prob.declare_instance_params(cost[:MAX - 3]), abi.ERR_INVALID, over % (MAX - 3, 2, 2))
    prob.declare_instance_subsystem_params([])
    refused(lambda: prob.declare_instance_subsystem_params([0, 1, 0]), abi.ERR_UNSUPPORTED,
            "instance parameter 2 (subsystem 0): declared twice (also parameter 0)")
    refused(lambda: prob.declare_instance_solver_params(LINE_SEARCH[:5]), abi.ERR_INVALID, over % (MAX - 4, 0, 5))
    assert prob.instance_solver_fields == [abi.SOLVER_FIELDS["initial_alpha_scaling"], abi.SOLVER_FIELDS["max_solver_iters"]]
    prob.bind_instance_values(np.ones((2, MAX - 2), dtype=np.float32))
    # declare while bound, each of the three calls
    for declare in (lambda: prob.declare_instance_solver_params([]), lambda: prob.declare_instance_solver_params(LINE_SEARCH),
                    lambda: prob.declare_instance_params([]), lambda: prob.declare_instance_subsystem_params([0])):
        refused(declare, abi.ERR_INVALID, DECLARED_ERROR)
    prob.bind_instance_values(None)
    prob.declare_instance_params([])
    # solver columns alone: a cost-evaluating call on another batch is still refused, what evaluates no cost is not
    x0 = examples.jittered_x0(spec, B, seed=1)
    prob.bind_instance_values(np.tile(_own(spec, ["initial_alpha_scaling", "max_solver_iters"]), (B, 1)))
    bufs = prob.solve(x0, fixed_iters=1)
    a3 = [bufs[k][:3].contiguous() for k in ("xs", "us", "P", "alpha")]
    x3 = torch.as_tensor(x0[:3], device="cuda").contiguous()
    for call in (lambda: prob.solve(x3, fixed_iters=1), lambda: prob.total_costs(a3[0], a3[1])):
        refused(call, abi.ERR_INVALID, "per-instance parameter values are bound for a batch of 4, this call has 3 instances")
    prob.rollout(x3, *a3)
    prob.linearize(a3[0], a3[1])
    prob.bind_instance_values(None)
    prob.declare_instance_solver_params([])
    refused(lambda: hip._check(hip.lib().ilqg_problem_bind_instance_values(prob.h, B, hip._ptr(table))), abi.ERR_INVALID,
            "no instance parameters are declared (ilqg_problem_declare_instance_params)")


# ---- 11. the C++ mirror ----
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_host_mirror_solve_batch_with_solver_params(hip, dtype):
    """tests/host/instance_solver_params_demo.cpp solve: GameSolver::SolveBatch(x0s, instance_params) on the headline
    scene built with the mirrored classes, four AddSolverParam columns per instance.  The harness solves the same inputs
    on the descriptor the C++ flattener produced, as one bound batch.  The mirror's containers are float: the harness's
    outputs are rounded to float before the exact comparison."""
    exe = os.path.join(ROOT, "tests", "host", "_bin", "instance_solver_params_demo")
    assert os.path.exists(exe), "build() compiles tests/host/instance_solver_params_demo.cpp"
    B = 6
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.bin")
        subprocess.run([exe, "solve", "f64" if dtype == abi.F64 else "f32", str(B), out], check=True, timeout=300)
        raw = np.fromfile(out, dtype=np.float64)
    resolved = subprocess.check_output([exe, "resolve"], text=True, timeout=120).splitlines()
    fields = [int(ln.split()[1]) for ln in resolved[:4]]
    spec = abi.ProblemSpec.from_dump("\n".join(resolved[6:]))
    assert spec.canonical() == _headline().canonical()
    n, m, T = spec.n, spec.m, spec.T
    at = 0

    def take(k, shape):
        nonlocal at
        a = raw[at:at + k].reshape(shape)
        at += k
        return a
    x0 = take(B * n, (B, n))
    vals = take(B * len(fields), (B, len(fields))).astype(np.float32)
    xs = take(B * T * n, (B, T, n)).astype(np.float32)
    us = take(B * T * m, (B, T, m)).astype(np.float32)
    assert at == raw.size
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_solver_params(fields)
    prob.bind_instance_values(vals)
    sol = prob.solve(x0)
    assert int(_np(sol["iters"]).min()) > 0
    assert _same_bits(_np(sol["xs"]).astype(np.float32), xs)
    assert _same_bits(_np(sol["us"]).astype(np.float32), us)
    plain = hip.Problem(spec, dtype).solve(x0)
    assert not _same_bits(_np(plain["xs"]).astype(np.float32), xs), "the table must have acted"
