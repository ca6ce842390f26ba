"""Per-instance time nominals on the device (ilqg_problem_bind_instance_time_nominals,
ilqg_instance_time_nominals_build, ilqg_problem_time_nominal_terms).

Every check is EXACT: an instance of a heterogeneous batch must return the bits of the same instance solved in a problem
created with its (nominal speed, initial route position) written into the descriptor — the device builder tabulates with
the function the host builder calls — so nothing here has a tolerance.  T = 20, B = 12 over 4 reference vectors, both
precisions; every comparison runs over every instance and every output array."""
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ilqgames_amd import abi, examples
from test_instance_time_nominals import (MIXED_VECTORS, TWO_CAR_VECTORS, ZOO_VECTORS, mixed_route_scene, time_terms,
                                         two_car_scene, with_references, zoo20)
from instance_harness import KEYS, check_baked_equals_bound, same_bits as _same_bits, to_numpy as _np

pytestmark = pytest.mark.gpu

DTYPES = [abi.F64, abi.F32]


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


def reach_scene():
    """two_player_reachability (a max-over-time and a min-over-time player; its line searches back-track) at T = 20 with
    a way-point for player 1 moving along a bent line and a nominal on its x position."""
    s = examples.two_player_reachability(T=20)
    s.params.max_solver_iters = 8
    line = s.add_polyline([(0.0, -10.0), (4.0, -7.0), (4.0, 6.0)])
    s.route_progress(0, 0.05, 5.0, line, (0, 1), 0.0)
    s.nominal_path_length(1, 0.02, 0, 1.0)
    return s


# the line: 5 m, then 13 m
REACH_VECTORS = np.array([[[5.0, 0.0], [1.0, 0.0]], [[4.0, 3.5], [2.0, 0.0]], [[6.0, 10.0], [-1.0, 0.0]],
                          [[2.0, 17.0], [0.5, 0.0]]], dtype=np.float32)

SCENES = {"two_car": (two_car_scene, TWO_CAR_VECTORS), "zoo": (zoo20, ZOO_VECTORS),
          "mixed": (mixed_route_scene, MIXED_VECTORS), "reach": (reach_scene, REACH_VECTORS)}


def _bound_problem(hip, spec, dtype, speed_pos):
    """A problem with the table the device builder makes of speed_pos [B][tables][2] bound."""
    prob = hip.Problem(spec, dtype)
    prob.bind_instance_time_nominals(prob.build_instance_time_nominals(speed_pos))
    return prob


# ---- 1. the device builder against the host builder ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_device_builder_equals_host_tables(hip, scene, dtype):
    """Block b of ilqg_instance_time_nominals_build is the table of the descriptor with vector b, byte for byte (vectors
    that pass the lane's corners and run off its end: tests/test_instance_time_nominals.py); the term lookup names the
    time-dependent terms in descriptor order."""
    make, vecs = SCENES[scene]
    spec = make()
    prob = hip.Problem(spec, dtype)
    assert prob.time_nominal_terms() == time_terms(spec)
    which = np.arange(12) % 4
    table = _np(prob.build_instance_time_nominals(vecs[which]))
    assert table.shape == (12, len(time_terms(spec)), spec.T, 2) and table.dtype == np.float64
    for b in range(12):
        want = hip.time_nominal_table(with_references(spec, vecs[which[b]]), dtype)
        assert _same_bits(table[b], want), (b, np.nonzero(table[b] != want))
    assert not _same_bits(table[0], table[1])


# ---- 2. bound equals baked, bit for bit ----
def _check_baked_equals_bound(hip, spec, vecs, dtype, **kw):
    return check_baked_equals_bound(hip, spec, dtype, lambda speed_pos: _bound_problem(hip, spec, dtype, speed_pos),
                                    lambda vec: with_references(spec, vec), vecs, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split_trial", [True, False])
@pytest.mark.parametrize("fixed_iters", [0, 6])
def test_two_car_scene_bound_equals_baked(hip, dtype, split_trial, fixed_iters):
    """(10, 2, 2), the interpreter's rows: the fused trial kernel's bound twin and the split rows kernel."""
    spec = two_car_scene()
    assert hip.Problem(spec, dtype).row_program()[1] == 0, "a scene with a time-dependent term runs the interpreter"
    _check_baked_equals_bound(hip, spec, TWO_CAR_VECTORS, dtype, deterministic=True, split_trial=split_trial,
                              fixed_iters=fixed_iters)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split_trial", [True, False])
def test_dynamics_zoo_scene_bound_equals_baked(hip, dtype, split_trial):
    """(17, 3, 2) at T = 20: three tables, the routes passing lane 2's corners and running off both lanes' ends."""
    _check_baked_equals_bound(hip, zoo20(), ZOO_VECTORS, dtype, deterministic=True, split_trial=split_trial)


@pytest.mark.parametrize("dtype", DTYPES)
def test_augmented_lagrangian_bound_equals_baked(hip, dtype):
    """The constrained two-car scene: the multiplier update and the constraint error of the exit kernel run beside the
    time-dependent costs of the same LDS tables."""
    spec = two_car_scene(constrained=True)
    _check_baked_equals_bound(hip, spec, TWO_CAR_VECTORS, dtype, deterministic=True, augmented_lagrangian=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("probe_lanes", [True, False])
def test_probing_passes_bound_equal_baked(hip, dtype, probe_lanes):
    """Free-running with the speculative line search in both forms of its rollouts, on a scene whose line searches
    back-track; the probing rows find the instance's block through the list slot's instance id."""
    spec = reach_scene()
    prob, _, x0, _ = _check_baked_equals_bound(hip, spec, REACH_VECTORS, dtype, whole_batch_partner=True, split_trial=True,
                                               probe=True, probe_lanes=probe_lanes)
    o = prob.solve(x0, split_trial=True, probe=True, probe_lanes=probe_lanes)
    backtracks = int(_np(prob.solve_state(o)["backtracks"]).sum())
    print("back-tracking steps of the last iteration:", backtracks)
    assert backtracks > 0, "the line searches should back-track: nothing was probed"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("padded_sweep", [True, False])
def test_run_time_dimensioned_kernels_bound_equal_baked(hip, dtype, padded_sweep):
    _check_baked_equals_bound(hip, mixed_route_scene(), MIXED_VECTORS, dtype, deterministic=True, padded_sweep=padded_sweep)


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_batch_schedule_bound_equals_baked(hip, dtype):
    """Without `deterministic`, at six instances per CU with the single-wave sweep pinned: the partner is a homogeneous
    batch of the same size."""
    _, cus = hip.device_info()
    prob, _, _, _ = _check_baked_equals_bound(hip, two_car_scene(), TWO_CAR_VECTORS[:2], dtype, B=6 * cus,
                                              whole_batch_partner=True, fixed_iters=4, single_wave_sweep=True)
    print("schedule of the bound solve: %#x" % prob.last_schedule())


# ---- 3. a table whose every block is the baked one ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scene", ["two_car", "two_car_al", "zoo", "mixed"])
def test_identity_table_changes_nothing(hip, dtype, scene):
    spec, kw = {"two_car": (two_car_scene(), {}), "two_car_al": (two_car_scene(constrained=True), dict(augmented_lagrangian=True)),
                "zoo": (zoo20(), {}), "mixed": (mixed_route_scene(), {})}[scene]
    B = 12
    x0 = examples.jittered_x0(spec, B, seed=9)
    prob = hip.Problem(spec, dtype)
    plain = {k: _np(v) for k, v in prob.solve(x0, **kw).items() if k in KEYS}
    baked = hip.time_nominal_table(spec, dtype)
    prob.bind_instance_time_nominals(np.tile(baked, (B, 1, 1, 1)))
    bound = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(bound[k]), plain[k]), k
    prob.bind_instance_time_nominals(None)
    again = prob.solve(x0, **kw)
    for k in KEYS:
        assert _same_bits(_np(again[k]), plain[k]), k
    assert int(plain["iters"].min()) > 0


# ---- 4. arbitrary per-step references: the rows of a quadraticisation are independent ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scene", ["two_car", "zoo", "mixed"])
def test_scrambled_per_step_references_quadraticize_row_by_row(hip, scene, dtype):
    """Row k of instance b's block is row k of the baked table of vector v(b, k), a seeded scramble over the 4 vectors in
    time.  With t_extreme NULL, ilqg_quadraticize_batch on fixed xs, us returns, for each (b, k), the bits of row k from
    the problem baked with vector v(b, k) on the same xs, us — no oracle needed."""
    make, vecs = SCENES[scene]
    spec = make()
    B, T = 12, spec.T
    rng = np.random.default_rng(17)
    v = rng.integers(0, 4, size=(B, T))
    assert all(len(set(v[b])) > 1 for b in range(B))
    baked = np.stack([hip.time_nominal_table(with_references(spec, vec), dtype) for vec in vecs])  # [4][tables][T][2]
    table = np.empty((B,) + baked.shape[1:], dtype=np.float64)
    for b in range(B):
        table[b] = baked[v[b], :, np.arange(T), :].transpose(1, 0, 2)
    x0 = examples.jittered_x0(spec, B, seed=3)
    base = hip.Problem(spec, dtype)
    sol = base.solve(x0, fixed_iters=2)  # some trajectory off the nominal
    xs, us = sol["xs"], sol["us"]
    prob = hip.Problem(spec, dtype)
    prob.bind_instance_time_nominals(table)
    got = [_np(a) for a in prob.quadraticize(xs, us)]
    per_vector = []
    for vec in vecs:
        per_vector.append([_np(a) for a in hip.Problem(with_references(spec, vec), dtype).quadraticize(xs, us)])
    differ = False
    for name, a, refs in zip("QlRr", got, zip(*per_vector)):
        assert a.shape[:2] == (B, T), name
        for b in range(B):
            for k in range(T):
                assert _same_bits(a[b, k], refs[v[b, k]][b, k]), (name, b, k)
        differ = differ or any(not _same_bits(refs[0], r) for r in refs[1:])
    assert differ, "the vectors should change the quadraticisation"


# ---- 5. the other entry points ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_solve_again_after_rewriting_the_bound_table_under_a_mask(hip, dtype):
    """The table is read at every call: rewritten in place on the device, without another bind, the next solve_again
    tracks the new references — what a receding-horizon caller does between replans."""
    import torch
    spec = two_car_scene()
    spec.params.max_solver_iters = 8
    B, BV = 8, 4
    vecs, vecs2 = TWO_CAR_VECTORS, TWO_CAR_VECTORS[[2, 3, 0, 1]]
    which = np.arange(B) % BV
    x0 = examples.jittered_x0(spec, B, seed=33)
    x0b = examples.jittered_x0(spec, B, seed=34)
    active = np.array([1, 0, 1, 1, 0, 1, 1, 0], dtype=np.int32)
    act_d = torch.as_tensor(active, device="cuda")
    prob = hip.Problem(spec, dtype)
    prob.single_wave_sweep = False  # pinned: the slices below must run the batch's schedule
    table = prob.bind_instance_time_nominals(prob.build_instance_time_nominals(vecs[which]))
    bufs = prob.solve(x0)
    first = {k: _np(bufs[k]).copy() for k in KEYS}
    prob.build_instance_time_nominals(vecs2[which], out=table)  # rewritten on the device, in stream order; still bound
    prob.solve_again(x0b, bufs, active=act_d)
    out = {k: _np(bufs[k]) for k in KEYS}
    for b in np.nonzero(active == 0)[0]:
        for k in KEYS:
            assert _same_bits(out[k][b], first[k][b]), ("masked instance touched", b, k)
    changed = False
    for v in range(BV):
        sel = np.nonzero(which == v)[0]
        p1 = hip.Problem(with_references(spec, vecs[v]), dtype)
        p1.single_wave_sweep = False
        rb = p1.solve(x0[sel])
        for k in KEYS:
            assert _same_bits(first[k][sel], _np(rb[k])), (k, v)
        # the same solver state carried into a problem with the second vector: its workspace layout is the same
        p2 = hip.Problem(with_references(spec, vecs2[v]), dtype)
        p2.single_wave_sweep = False
        p2.solve_again(x0b[sel], rb, active=act_d[torch.as_tensor(sel, device="cuda")].contiguous())
        for k in KEYS:
            for j, b in enumerate(sel):
                if active[b]:
                    assert _same_bits(out[k][b], _np(rb[k])[j]), (k, b)
                    changed = changed or (k == "xs" and not _same_bits(out[k][b], first[k][b]))
    assert changed


@pytest.mark.parametrize("dtype", DTYPES)
def test_strategy_costs_and_nash_checks_bound_equal_baked(hip, dtype):
    """reach_scene has a max-over-time player: the sufficient check's handle copy starts each chunk at its own block."""
    spec = reach_scene()
    spec.params.max_solver_iters = 6
    B = 4
    x0 = examples.jittered_x0(spec, B, seed=42)
    prob = _bound_problem(hip, spec, dtype, REACH_VECTORS)
    sol = prob.solve(x0, deterministic=True)
    args = [sol[k] for k in ("xs", "us", "P", "alpha")]
    costs = _np(prob.strategy_costs(x0, *args))
    ok, margin = (_np(a) for a in prob.check_local_nash(x0, *args, max_perturbation=0.1))
    psd = _np(prob.check_sufficient_nash(sol["xs"], sol["us"]))
    totals = _np(prob.total_costs(sol["xs"], sol["us"])[0])
    for b in range(B):
        ref = hip.Problem(with_references(spec, REACH_VECTORS[b]), dtype)
        a1 = [v[b:b + 1].contiguous() for v in args]
        assert _same_bits(costs[b:b + 1], _np(ref.strategy_costs(x0[b:b + 1], *a1))), b
        ok1, margin1 = (_np(a) for a in ref.check_local_nash(x0[b:b + 1], *a1, max_perturbation=0.1))
        assert _same_bits(ok[b:b + 1], ok1) and _same_bits(margin[b:b + 1], margin1), b
        assert _same_bits(psd[b:b + 1], _np(ref.check_sufficient_nash(a1[0], a1[1]))), b
        assert _same_bits(totals[b:b + 1], _np(ref.total_costs(a1[0], a1[1])[0])), b
    plain = _np(hip.Problem(spec, dtype).strategy_costs(x0, *args))
    assert not _same_bits(plain, costs), "the references should change the strategy costs"


VALUE_DECL = [(2, "value"), (6, "value")]  # two_car_scene: the two players' nominal speeds (QUADRATIC on V)
VALUE_ROWS = np.array([[4.5, 5.5], [6.0, 3.5], [5.25, 4.75]], dtype=np.float32)  # three vectors against four references
OTHER_LANES = np.array([[(-20.0, -3.0), (20.0, -3.0)], [(-20.0, -2.0), (20.0, -4.5)]], dtype=np.float32)  # two against four


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", list(itertools.permutations("vrt")), ids=lambda o: "".join(o))
def test_values_routes_and_time_nominals_bound_together_in_every_order(hip, dtype, order):
    """Twelve instances, twelve combinations of (value vector, layout of the lane no route-progress term uses, reference
    vector).  The partner of reference v is a problem created with it that binds the value rows and routes of v's
    instances."""
    spec = two_car_scene()
    assert spec.terms[2]["kind"] == spec.terms[6]["kind"] == abi.COST_QUADRATIC
    B, kw = 12, dict(deterministic=True, fixed_iters=6)
    which = np.arange(B) % 4
    values = VALUE_ROWS[np.arange(B) % 3]
    lanes = OTHER_LANES[(np.arange(B) // 6) % 2]
    assert len({(b % 4, b % 3, (b // 6) % 2) for b in range(B)}) == B
    x0 = examples.jittered_x0(spec, B, seed=6)
    prob = hip.Problem(spec, dtype)
    prob.declare_instance_params(VALUE_DECL)
    prob.declare_instance_routes([1])
    table = prob.build_instance_time_nominals(TWO_CAR_VECTORS[which])
    binds = {"v": lambda: prob.bind_instance_values(values), "r": lambda: prob.bind_instance_routes(lanes),
             "t": lambda: prob.bind_instance_time_nominals(table)}
    for name in order:
        binds[name]()
    out = {k: _np(v) for k, v in prob.solve(x0, **kw).items() if k in KEYS}
    for v in range(4):
        sel = np.nonzero(which == v)[0]
        ref_prob = hip.Problem(with_references(spec, TWO_CAR_VECTORS[v]), dtype)
        ref_prob.declare_instance_params(VALUE_DECL)
        ref_prob.declare_instance_routes([1])
        ref_prob.bind_instance_values(values[sel])
        ref_prob.bind_instance_routes(lanes[sel])
        ref = ref_prob.solve(x0[sel], **kw)
        for k in KEYS:
            assert _same_bits(out[k][sel], _np(ref[k])), (k, v)
    # unbinding the other two leaves this one bound
    prob.bind_instance_values(None)
    prob.bind_instance_routes(None)
    alone = _np(prob.solve(x0, **kw)["xs"])
    ref = _bound_problem(hip, spec, dtype, TWO_CAR_VECTORS[which]).solve(x0, **kw)
    assert _same_bits(alone, _np(ref["xs"])) and not _same_bits(alone, out["xs"])


# ---- 6. the handle's refusals, each before any kernel is launched ----
def test_binding_errors(hip):
    import torch
    B = 4
    # no time-dependent term
    plain_spec = examples.modified_three_player_intersection()
    plain = hip.Problem(plain_spec, abi.F64)
    assert plain.time_nominal_terms() == []
    some = torch.zeros((B, 1, plain_spec.T, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(hip.IlqgError) as e:
        plain.bind_instance_time_nominals(some)
    assert e.value.status == abi.ERR_INVALID and "no time-dependent term" in str(e.value)
    with pytest.raises(hip.IlqgError) as e:
        hip._check(hip.lib().ilqg_instance_time_nominals_build(plain.h, B, hip._ptr(some), hip._ptr(some), None))
    assert e.value.status == abi.ERR_INVALID and "no time-dependent term" in str(e.value)
    plain.bind_instance_time_nominals(None)  # unbinding nothing is fine

    spec = two_car_scene()
    prob = hip.Problem(spec, abi.F64)
    x0 = examples.jittered_x0(spec, B, seed=1)
    table = prob.build_instance_time_nominals(TWO_CAR_VECTORS)
    for batch in (0, -3):
        with pytest.raises(hip.IlqgError) as e:
            hip._check(hip.lib().ilqg_problem_bind_instance_time_nominals(prob.h, batch, hip._ptr(table)))
        assert e.value.status == abi.ERR_INVALID and "batch" in str(e.value)
        with pytest.raises(hip.IlqgError) as e:
            hip._check(hip.lib().ilqg_instance_time_nominals_build(prob.h, batch, hip._ptr(table), hip._ptr(table), None))
        assert e.value.status == abi.ERR_INVALID and "batch" in str(e.value)
    count = hip.C.c_int32(0)
    arr = (hip.C.c_int32 * 2)()
    with pytest.raises(hip.IlqgError) as e:
        hip._check(hip.lib().ilqg_problem_time_nominal_terms(prob.h, arr, 2, hip.C.byref(count)))
    assert e.value.status == abi.ERR_INVALID and "too small" in str(e.value) and count.value == 3
    prob.bind_instance_time_nominals(table)
    # batch mismatch: every cost-evaluating entry point
    x3 = x0[:3]
    bufs = prob.solve(x0, fixed_iters=1)
    a3 = [bufs[k][:3].contiguous() for k in ("xs", "us", "P", "alpha")]
    calls = [lambda: prob.solve(x3, fixed_iters=1), lambda: prob.solve(x3, fixed_iters=1, augmented_lagrangian=True),
             lambda: prob.quadraticize(a3[0], a3[1]), lambda: prob.total_costs(a3[0], a3[1]),
             lambda: prob.strategy_costs(x3, *a3), lambda: prob.check_local_nash(x3, *a3, max_perturbation=0.1),
             lambda: prob.check_sufficient_nash(a3[0], a3[1]), lambda: prob.solve_again(x3, prob.alloc_solve_buffers(3))]
    for q, call in enumerate(calls):
        with pytest.raises(hip.IlqgError) as e:
            call()
        assert e.value.status == abi.ERR_INVALID and "time nominals are bound for a batch of 4" in str(e.value), q
    prob.linearize(a3[0], a3[1])  # evaluates no cost: ignores the binding
    prob.rollout(x3, *a3)
    # the other bindings with another batch, and the other way round
    prob.declare_instance_params([(2, "value")])
    prob.declare_instance_routes([1])
    with pytest.raises(hip.IlqgError) as e:
        prob.bind_instance_values(np.full((3, 1), 5.0, dtype=np.float32))
    assert e.value.status == abi.ERR_INVALID and "time nominals are bound for a batch of 4" in str(e.value)
    with pytest.raises(hip.IlqgError) as e:
        prob.bind_instance_routes(OTHER_LANES[[0, 1, 0]])
    assert e.value.status == abi.ERR_INVALID and "time nominals are bound for a batch of 4" in str(e.value)
    prob.bind_instance_time_nominals(None)
    prob.bind_instance_values(np.full((3, 1), 5.0, dtype=np.float32))
    with pytest.raises(hip.IlqgError) as e:
        prob.bind_instance_time_nominals(table)
    assert e.value.status == abi.ERR_INVALID and "values are bound for a batch of 3" in str(e.value)
    prob.bind_instance_values(None)
    prob.bind_instance_routes(OTHER_LANES[[0, 1, 0]])
    with pytest.raises(hip.IlqgError) as e:
        prob.bind_instance_time_nominals(table)
    assert e.value.status == abi.ERR_INVALID and "routes are bound for a batch of 3" in str(e.value)
    prob.bind_instance_routes(None)
    prob.solve(x3, fixed_iters=1)  # nothing bound: any batch


def test_the_two_older_refusals_are_unchanged_on_the_handle(hip):
    """A pin of old behaviour on a handle whose time-dependent terms the new lookup names: those terms still take no
    per-instance `value` column, and their polyline no per-instance route."""
    spec = two_car_scene()
    prob = hip.Problem(spec, abi.F64)
    assert prob.time_nominal_terms() == time_terms(spec)
    for ti in time_terms(spec):
        with pytest.raises(hip.IlqgError) as e:
            prob.declare_instance_params([(ti, "value")])
        assert e.value.status == abi.ERR_UNSUPPORTED and "term %d" % ti in str(e.value) and "tabulated" in str(e.value)
    with pytest.raises(hip.IlqgError) as e:
        prob.declare_instance_routes([1, 0])
    msg = str(e.value)
    assert e.value.status == abi.ERR_UNSUPPORTED and "polyline 0" in msg and "ROUTE_PROGRESS" in msg
    assert "tabulates its per-step nominals" in msg
    prob.declare_instance_routes([1])


# ---- 7. the C++ mirror ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_mirror_solve_batch_with_instance_time_nominals(hip, dtype):
    """tests/host/instance_time_nominals_demo.cpp: GameSolver::SolveBatch(x0s, instance_params) with AddReference and
    FillInstanceTimeNominals on a two-car scene built with the mirrored classes, its inputs and outputs written as raw
    arrays.  The table the C++ helper tabulated on the host must be, bit for bit, the device builder's for the same
    (speed, position) pairs (the unnamed cost keeping its own); the Python harness then solves the same inputs on the
    descriptor the C++ flattener produced.  The mirror's containers are float, as the reference's: the harness's outputs
    are rounded to float before the exact comparison."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "host", "_bin", "instance_time_nominals_demo")
    assert os.path.exists(exe), "build() compiles tests/host/instance_time_nominals_demo.cpp"
    B = 6
    name = "f64" if dtype == abi.F64 else "f32"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.bin")
        subprocess.run([exe, "solve", name, str(B), out], check=True, timeout=300)
        raw = np.fromfile(out, dtype=np.float64)
    lines = subprocess.check_output([exe, "resolve", name], text=True, timeout=120).splitlines()
    tables = int(lines[0].split()[1])
    named = [int(v) for v in lines[1].split()[1:]]
    spec = abi.ProblemSpec.from_dump("\n".join(lines[lines.index("dump") + 1:]))
    assert tables == len(time_terms(spec)) == 3 and named == [2, 0]
    n, m, T = spec.n, spec.m, spec.T
    at = 0

    def take(k, shape):
        nonlocal at
        a = raw[at:at + k].reshape(shape)
        at += k
        return a
    x0 = take(B * n, (B, n))
    speed_pos = take(B * len(named) * 2, (B, len(named), 2)).astype(np.float32)
    table = take(B * tables * T * 2, (B, tables, T, 2))
    xs = take(B * T * n, (B, T, n))
    us = take(B * T * m, (B, T, m))
    assert at == raw.size
    full = np.tile(np.array([[spec.terms[ti]["value"], spec.terms[ti]["value2"]] for ti in time_terms(spec)],
                            dtype=np.float32), (B, 1, 1))
    full[:, named] = speed_pos
    prob = hip.Problem(spec, dtype)
    assert _same_bits(_np(prob.build_instance_time_nominals(full)), table)
    prob.bind_instance_time_nominals(table)
    sol = prob.solve(x0)
    assert int(_np(sol["iters"]).min()) > 0
    assert _same_bits(_np(sol["xs"]).astype(np.float32), xs.astype(np.float32))
    assert _same_bits(_np(sol["us"]).astype(np.float32), us.astype(np.float32))
    plain = hip.Problem(spec, dtype).solve(x0)
    assert not _same_bits(_np(plain["xs"]).astype(np.float32), xs.astype(np.float32)), "the references must have acted"
