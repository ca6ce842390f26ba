"""The cases of tests/golden/schedule_cases.json: which scenes, batches and option sets the solve schedule is recorded
for (tests/golden/make_schedule_cases.py, on the GPU) and replayed on (tests/test_schedule.py through the host-only
ilqg_schedule_build, tests/test_gpu_schedule.py against a real solve)."""
import numpy as np

from ilqgames_amd import abi, examples

# name -> (constructor taking T, the shape it lands on or None for the run-time-dimensioned kernels)
SCENES = {
    "n14": (lambda T: examples.modified_three_player_intersection(T=T), (14, 3, 2)),
    "n16": (lambda T: examples.three_player_intersection(T=T), (16, 3, 2)),
    "n15": (lambda T: examples.three_player_collision_avoidance_reachability(T=T), (15, 3, 2)),
    "n24": (lambda T: examples.roundabout_merging(T=T, open_loop=False), (24, 4, 2)),
    "n4": (lambda T: examples.two_player_unicycle_4d_scene(T=T), (4, 2, 2)),
    # (2, 2, 1) holds no problem a solve can run (no model has one state): the smallest (n, 2, 1) scene instead
    "n3": (lambda T: examples.air_3d(T=T), (3, 2, 1)),
    "expression_cost": (lambda T: examples.expression_scene(T=T), (10, 2, 2)),
    "expression_dynamics": (lambda T: examples.coasting_car_scene(T=T), (8, 2, 1)),
    "generic": (lambda T: examples.mixed_dubins_car_scene(T=T), None),
}

CHOICE_FIELDS = ("split_trial", "handoff", "probe", "counted", "compact_rows", "round_bursts", "generic_kernels",
                 "single_wave_sweep", "adjoint_expected_decrease", "static_rows", "padded_sweep", "probe_lanes",
                 "sweep_forms")

# name -> what the case sets: keyword arguments of hip.Problem.solve, and beside them
#   open_loop: the spec's solver parameter; bind: "tables" (a per-instance cost column) or "solver" (a solver column);
#   masked: a free-running solve of a batch of 8 C with this many instances active (an int, or "5C")
OPTION_SETS = {"default": {}, "deterministic": {"deterministic": True}}
for _f in CHOICE_FIELDS:
    OPTION_SETS[_f + "_on"] = {_f: True}
    OPTION_SETS[_f + "_off"] = {_f: False}
OPTION_SETS.update({
    "augmented_lagrangian": {"augmented_lagrangian": True},
    "open_loop": {"open_loop": True},
    "masked_3": {"masked": 3},
    "masked_5C": {"masked": "5C"},
    "tables_bound": {"bind": "tables"},
    "solver_bound": {"bind": "solver"},
})


def batches(C):
    return [1, C, C + 1, 2 * C, 2 * C + 1, 4 * C, 4 * C + 1, 5 * C - 1, 5 * C, 1279, 1280, 8 * C - 1, 8 * C]


def horizons(scene):
    return (8, 100) if scene == "n14" else (8,)


def make_spec(scene, T, open_loop=False):
    spec = SCENES[scene][0](T)
    if open_loop:
        spec.params.open_loop = 1
    return spec


def solve_kwargs(opts):
    """The hip.Problem.solve keywords of an option set (without the meta keys)."""
    return {k: v for k, v in opts.items() if k not in ("open_loop", "bind", "masked")}


def case_batch(opts, batch, C):
    """(batch, active instances or -1) of a case: a masked case runs 8 C instances whatever the listed batch."""
    if "masked" not in opts:
        return batch, -1
    return 8 * C, (5 * C if opts["masked"] == "5C" else int(opts["masked"]))


def tables_term(spec):
    """The first state or control cost of the spec: the term whose weight the tables_bound cases declare per instance."""
    for q, t in enumerate(spec.terms):
        if t["role"] in (abi.ROLE_STATE_COST, abi.ROLE_CONTROL_COST) and t["kind"] == abi.COST_QUADRATIC:
            return q
    raise AssertionError("no quadratic cost to bind")


def solve_case(prob, spec, opts, batch, C, bufs_cache):
    """Runs the case's solve on `prob` (created from `spec`, with the case's open_loop); -> last_schedule()."""
    import torch
    B, active = case_batch(opts, batch, C)
    x0 = np.tile(np.asarray(spec.x0, dtype=np.float64), (B, 1))
    if B not in bufs_cache:
        bufs_cache[B] = prob.alloc_solve_buffers(B)
    bufs = bufs_cache[B]
    for k in ("xs", "us", "P", "alpha"):
        bufs[k].zero_()
    kw = dict(solve_kwargs(opts))
    if active >= 0:
        mask = torch.zeros(B, dtype=torch.int32, device="cuda")
        mask[:active] = 1
        kw["active"] = mask
    else:
        kw["fixed_iters"] = 1
    bind = opts.get("bind")
    if bind == "tables":
        q = tables_term(spec)
        prob.declare_instance_params([(q, "weight")])
        prob.bind_instance_values(np.full((B, 1), spec.terms[q]["weight"], dtype=np.float32))
    elif bind == "solver":
        prob.declare_instance_solver_params(["initial_alpha_scaling"])
        prob.bind_instance_values(np.full((B, 1), spec.params.initial_alpha_scaling, dtype=np.float32))
    try:
        prob.solve(x0, bufs, **kw)
        torch.cuda.synchronize()
        return prob.last_schedule()
    finally:
        if bind:
            prob.bind_instance_values(None)
            prob.declare_instance_params([])
            prob.declare_instance_solver_params([])


# ---- the file's layout ----
# The cases stand in one fixed order (case_blocks): a block per (scene, horizon, precision, option set), in it a case per
# batch.  A case's record is cut into groups of fields that change together; per group the file holds the distinct
# value tuples ("values"; null: a solve on the run-time-dimensioned kernels, which has the word alone), the distinct
# blocks as tuples of value ids ("blocks") and the run lengths of the block ids over the blocks in order ("runs").
FIELD_GROUPS = {
    "word": ["word"],
    "batch": ["sched_batch", "num_cus", "prio_div", "nt_exit"],
    "rounds": ["split", "counted", "handoff", "lists", "bursts", "probe", "timed", "read_restarts", "cap", "has_proll_single",
               "has_proll_lanes", "decide_solver", "roll_xdyn"],
    "rows": ["rows_cw", "row_chunks", "lds_part", "compact", "static_id", "static_prog", "static_in_regs", "trial_prog",
             "rows_prog", "prows_prog"],
    "sweep": ["defer_forward", "single_wave", "adjoint", "b_const", "sweep_kind", "sweep_forms", "sweep_threads"],
    "shape": ["lane_width", "pairs", "lanes_auto", "deep_tails"],
    "lds": ["lds_trial", "lds_roll", "lds_rows", "lds_decide", "lds_proll", "lds_proll_fat", "lds_proll_single",
            "lds_proll_lanes", "lds_prows", "lds_sweep", "lds_exit"],
}


def case_blocks(scenes, option_sets, C):
    """[((scene, T, dtype, option set), [(batch, active), ...]), ...] in the file's order."""
    out = []
    for scene in scenes:
        for T in horizons(scene):
            for dtype in (abi.F32, abi.F64):
                for oname in option_sets:
                    keys = []
                    for batch in batches(C):
                        key = case_batch(OPTION_SETS[oname], batch, C)
                        if key not in keys:  # (a masked case has one batch of its own)
                            keys.append(key)
                    out.append(((scene, T, dtype, oname), keys))
    return out


def encode_records(blocks, records):
    """records: per case, in the order of `blocks`, a dict of every recorded field (the word alone: no finer record)."""
    at, groups = 0, {}
    for name, fields in FIELD_GROUPS.items():
        groups[name] = {"fields": fields, "values": [], "blocks": [], "runs": []}
    for _, keys in blocks:
        block = records[at:at + len(keys)]
        at += len(keys)
        for name, g in groups.items():
            ids = []
            for rec in block:
                v = [rec[f] for f in g["fields"]] if g["fields"][0] in rec else None
                if v not in g["values"]:
                    g["values"].append(v)
                ids.append(g["values"].index(v))
            if ids not in g["blocks"]:
                g["blocks"].append(ids)
            b = g["blocks"].index(ids)
            if g["runs"] and g["runs"][-1][0] == b:
                g["runs"][-1][1] += 1
            else:
                g["runs"].append([b, 1])
    assert at == len(records)
    return groups


def decode_cases(golden):
    """[(scene, dtype, T, batch, option set, active, record), ...]: every case of the file with its recorded fields."""
    blocks = case_blocks(golden["scenes"], golden["option_sets"], golden["num_cus"])
    per_block = [[{} for _ in keys] for _, keys in blocks]
    for g in golden["groups"].values():
        ids = [b for b, count in g["runs"] for _ in range(count)]
        assert len(ids) == len(blocks)
        for recs, b in zip(per_block, ids):
            assert len(g["blocks"][b]) == len(recs)
            for rec, v in zip(recs, g["blocks"][b]):
                if g["values"][v] is not None:
                    rec.update(zip(g["fields"], g["values"][v]))
    return [(scene, dtype, T, batch, oname, active, rec)
            for ((scene, T, dtype, oname), keys), recs in zip(blocks, per_block) for (batch, active), rec in zip(keys, recs)]
