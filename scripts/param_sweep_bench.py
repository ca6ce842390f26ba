#!/usr/bin/env python
"""What per-instance cost parameters cost and what they buy: the headline scene (n = 14 intersection, T = 100) at
B = 1024, fp64, 20 fixed iterations from a zero warm start, bench.py's line-search parameters.

  (a) unbound                 the problem as bench.py solves it
  (b) bound, identity         a table bound whose every row holds the baked values: the price of the overlay's reads
  (c) bound, spread           a seeded spread of nominal speeds, lane weights and proximity weights, one vector per instance
  (d) one problem per vector  what a user had before: V problems created with V of those vectors, each solving its
                              B / V instances, one after another (V small so that this stays short; with one vector
                              per instance it would be B solves of one instance each)

A fixed-iteration solve still back-tracks: the games of the spread are harder than the baked one (the scene bakes proximity
weight 0), and an iteration that rejects step sizes costs more passes.  So the line also carries, as the yardstick for (c),
`baked_spread_vector_its`: ONE problem created with the first vector of the spread solving all B instances unbound, and
the mean number of rejected step sizes per instance in the last iteration of (a), (c) and that run.

--subsystems: the same four legs for per-instance SUBSYSTEM parameters — the two cars' inter-axle distances (baked: 4.0 m):
unbound; bound with every row the baked 4.0; bound with one wheelbase pair per instance drawn from [2.5, 5.0]; one problem
per pair (V pairs, V solves of B / V instances).

--routes: the same four legs for per-instance ROUTES — the three bend points of player 2's turn lane displaced by up to
1 m over V distinct layouts (instance b plays layout b % V): unbound; bound with every row the baked lane; bound with the V
layouts; the same V layouts as V problems solved one after another, B / V instances each.

--references: the same four legs for per-instance TIME NOMINALS — the scene gains a way-point for each car (a
RouteProgressCost on its lane, weight 5; a scene with a time-dependent term runs the interpreted row stage, so leg (a) is
this scene unbound, not bench.py's), and V reference vectors draw the cars' nominal speeds from [3, 8] m/s and their
initial route positions from +-5 m about the baked ones (instance b tracks vector b % V): unbound; bound with every block
the baked table; bound with the V references (tabulated on the device by ilqg_instance_time_nominals_build); the same V
references as V problems solved one after another, B / V instances each.

--solver-params: the same four legs for per-instance SOLVER parameters, on FREE-RUNNING solves (the stopping rule and the
line search are what varies, so nothing is fixed: --iters is not used and iterations/s counts the iterations the
instances report) of the scene created with the example's OWN line-search parameters (initial_alpha_scaling 1.0,
expected_decrease_fraction 0.9 — the descriptor's integer members are the sweep's ceilings): unbound; bound with every
row the baked values; bound with V = 16 line-search vectors, initial step {1, 0.5, 0.25, 0.1} x Armijo fraction
{0.9, 0.1, 0.01, 0.001} (instance b takes vector b % V); the same V vectors as V problems solved one after another,
B / V instances each.  Before the JSON line it prints, per vector, the share of its instances that succeeded and their
mean iterations and rejected steps — the table a user runs the feature for.

Prints one JSON line: iterations/s of each.
python scripts/param_sweep_bench.py [--batch 1024] [--repeats 5] [--vectors 16]
                                    [--subsystems | --routes | --references | --solver-params]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

DECLARED = [("p1_nominal_speed", "value", 6.0, 10.0), ("p2_nominal_speed", "value", 4.0, 8.0),
            ("p3_nominal_speed", "value", 1.0, 2.0), ("p1_lane", "weight", 15.0, 35.0), ("p2_lane", "weight", 15.0, 35.0),
            ("p3_lane", "weight", 15.0, 35.0), ("p1_proximity_p2", "weight", 0.0, 30.0), ("p2_proximity_p1", "weight", 0.0, 30.0),
            ("p3_proximity_p1", "weight", 0.0, 30.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--vectors", type=int, default=16)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--subsystems", action="store_true", help="the wheelbases of the two cars instead of cost parameters")
    ap.add_argument("--routes", action="store_true", help="the bend of player 2's turn lane instead of cost parameters")
    ap.add_argument("--references", action="store_true", help="a way-point per car, its speed and start per instance")
    ap.add_argument("--solver-params", action="store_true", help="a line search per instance, free-running solves")
    args = ap.parse_args()
    import torch
    from ilqgames_amd import abi, examples, hip
    dtype = abi.F64 if args.dtype == "f64" else abi.F32
    B, K, V = args.batch, args.iters, args.vectors
    assert B % V == 0
    spec = examples.modified_three_player_intersection()
    spec.params.initial_alpha_scaling = 0.1
    spec.params.expected_decrease_fraction = 0.001
    x0 = hip._dev(examples.jittered_x0(spec, B, seed=0), dtype)
    params = [(d[0], d[1]) for d in DECLARED]
    rng = np.random.default_rng(0)
    lo, hi = np.array([d[2] for d in DECLARED]), np.array([d[3] for d in DECLARED])
    spread = (lo + (hi - lo) * rng.random((B, len(DECLARED)))).astype(np.float32)
    identity = np.tile(np.array([spec.terms[spec.term_index(n)][f] for n, f in params], dtype=np.float32), (B, 1))

    def timed(solves):
        """Median over the repeats of the device time of `solves` = [(problem, x0 slice, buffers)], run back to back."""
        times = []
        for rep in range(args.repeats + 1):  # the first pass is the warm-up
            for _, _, bufs in solves:
                for k in ("xs", "us", "P", "alpha"):
                    bufs[k].zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for prob, x, bufs in solves:
                prob.solve(x, bufs, fixed_iters=K)
            e1.record()
            torch.cuda.synchronize()
            if rep > 0:
                times.append(e0.elapsed_time(e1) * 1e-3)
        return float(np.median(times))

    if args.solver_params:
        spec = examples.modified_three_player_intersection()  # its own 1.0 / 0.9: the descriptor is the ceiling
        fields = ["initial_alpha_scaling", "geometric_alpha_scaling", "expected_decrease_fraction", "max_backtracking_steps"]
        own = np.array([getattr(spec.params, f) for f in fields], dtype=np.float32)
        grid = [(a0, fr) for a0 in (1.0, 0.5, 0.25, 0.1) for fr in (0.9, 0.1, 0.01, 0.001)]
        assert V == len(grid), "--solver-params sweeps %d vectors" % len(grid)
        vectors = np.array([[a0, own[1], fr, own[3]] for a0, fr in grid], dtype=np.float32)
        which = np.arange(B) % V

        def timed_free(solves):
            """-> (median device time of the free-running `solves`, the iterations their instances reported)."""
            times = []
            for rep in range(args.repeats + 1):  # the first pass is the warm-up
                for _, _, bufs in solves:
                    for k in ("xs", "us", "P", "alpha"):
                        bufs[k].zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for prob, x, bufs in solves:
                    prob.solve(x, bufs)
                e1.record()
                torch.cuda.synchronize()
                if rep > 0:
                    times.append(e0.elapsed_time(e1) * 1e-3)
            return float(np.median(times)), sum(int(bufs["iters"].sum().item()) for _, _, bufs in solves)

        def its(solves):
            t, iters = timed_free(solves)
            return iters / t

        prob = hip.Problem(spec, dtype)
        bufs = prob.alloc_solve_buffers(B)
        out = dict(batch=B, dtype=args.dtype, fields=fields, vectors=V)
        out["unbound_its"] = its([(prob, x0, bufs)])
        prob.declare_instance_solver_params(fields)
        prob.bind_instance_values(np.tile(own, (B, 1)))
        out["bound_identity_its"] = its([(prob, x0, bufs)])
        prob.bind_instance_values(vectors[which])
        out["bound_vectors_its"] = its([(prob, x0, bufs)])
        status, iters = bufs["status"].cpu().numpy(), bufs["iters"].cpu().numpy()
        rejected = prob.solve_state(bufs)["backtracks"].cpu().numpy()
        print("vector  alpha0  fraction  success  mean_iters  mean_rejected")
        table = []
        for v, (a0, fr) in enumerate(grid):
            sel = which == v
            row = (float(status[sel].mean()), float(iters[sel].mean()), float(rejected[sel].mean()))
            table.append([a0, fr] + [round(r, 3) for r in row])
            print("%6d  %6.2f  %8.3f  %6.1f%%  %10.2f  %13.2f" % (v, a0, fr, 100.0 * row[0], row[1], row[2]))
        out["per_vector"] = table
        prob.bind_instance_values(None)
        solves = []
        for v in range(V):
            s = copy.deepcopy(spec)
            for f, val in zip(fields, vectors[v]):
                setattr(s.params, f, int(val) if f in abi.SOLVER_INT_FIELDS else float(val))
            p = hip.Problem(s, dtype)
            sel = torch.as_tensor(np.nonzero(which == v)[0], device="cuda")
            solves.append((p, x0[sel].contiguous(), p.alloc_solve_buffers(len(sel))))
        out["per_vector_problems_its"] = its(solves)
        print(json.dumps(out))
        return

    if args.references:
        baked = []  # (speed, pos0) of the two way-points: the cars start 970 m and 955 m along their lanes
        for player, lane, xy, speed, pos0 in ((0, 0, (0, 1), 8.0, 970.0), (1, 1, (5, 6), 6.0, 955.0)):
            spec.route_progress(player, 5.0, speed, lane, xy, pos0)
            baked.append((speed, pos0))
        terms = [ti for ti, t in enumerate(spec.terms) if t["kind"] == abi.COST_ROUTE_PROGRESS]
        refs = np.tile(np.array(baked, dtype=np.float32), (V, 1, 1))
        refs[:, :, 0] = (3.0 + 5.0 * rng.random((V, len(terms)))).astype(np.float32)
        refs[:, :, 1] += (10.0 * rng.random((V, len(terms))) - 5.0).astype(np.float32)
        assert len({r.tobytes() for r in refs}) == V
        which = np.arange(B) % V
        prob = hip.Problem(spec, dtype)
        assert prob.time_nominal_terms() == terms
        bufs = prob.alloc_solve_buffers(B)
        out = dict(batch=B, iters=K, dtype=args.dtype, tables=len(terms), references=V)
        out["unbound_its"] = B * K / timed([(prob, x0, bufs)])
        prob.bind_instance_time_nominals(np.tile(hip.time_nominal_table(spec, dtype), (B, 1, 1, 1)))
        out["bound_identity_its"] = B * K / timed([(prob, x0, bufs)])
        prob.bind_instance_time_nominals(prob.build_instance_time_nominals(refs[which]))
        out["bound_references_its"] = B * K / timed([(prob, x0, bufs)])
        out["bound_references_backtracks"] = float(prob.solve_state(bufs)["backtracks"].float().mean().item())
        prob.bind_instance_time_nominals(None)
        solves = []
        for v in range(V):
            s = copy.deepcopy(spec)
            for ti, (speed, pos0) in zip(terms, refs[v]):
                s.terms[ti]["value"], s.terms[ti]["value2"] = float(speed), float(pos0)
            p = hip.Problem(s, dtype)
            sel = torch.as_tensor(np.nonzero(which == v)[0], device="cuda")
            solves.append((p, x0[sel].contiguous(), p.alloc_solve_buffers(len(sel))))
        out["per_reference_problems_its"] = B * K / timed(solves)
        print(json.dumps(out))
        return

    if args.routes:
        lane, bend = 1, [2, 3, 4]  # examples.py: lane2 and its three bend points
        baked = np.array(spec.polylines[lane], dtype=np.float32)
        layouts = np.tile(baked, (V, 1, 1))
        layouts[:, bend] += (2.0 * rng.random((V, len(bend), 2)) - 1.0).astype(np.float32)
        assert len({l.tobytes() for l in layouts}) == V
        which = np.arange(B) % V
        prob = hip.Problem(spec, dtype)
        bufs = prob.alloc_solve_buffers(B)
        out = dict(batch=B, iters=K, dtype=args.dtype, routes=[lane], layouts=V)
        out["unbound_its"] = B * K / timed([(prob, x0, bufs)])
        prob.declare_instance_routes([lane])
        prob.bind_instance_routes(np.tile(baked, (B, 1, 1)))
        out["bound_identity_its"] = B * K / timed([(prob, x0, bufs)])
        prob.bind_instance_routes(layouts[which])
        out["bound_layouts_its"] = B * K / timed([(prob, x0, bufs)])
        out["bound_layouts_backtracks"] = float(prob.solve_state(bufs)["backtracks"].float().mean().item())
        prob.bind_instance_routes(None)
        solves = []
        for v in range(V):
            s = copy.deepcopy(spec)
            s.polylines[lane] = [(float(x), float(y)) for x, y in layouts[v]]
            p = hip.Problem(s, dtype)
            sel = torch.as_tensor(np.nonzero(which == v)[0], device="cuda")
            solves.append((p, x0[sel].contiguous(), p.alloc_solve_buffers(len(sel))))
        out["per_layout_problems_its"] = B * K / timed(solves)
        print(json.dumps(out))
        return

    if args.subsystems:
        rows = [0, 1]
        wheelbases = (2.5 + 2.5 * rng.random((B, len(rows)))).astype(np.float32)
        prob = hip.Problem(spec, dtype)
        bufs = prob.alloc_solve_buffers(B)
        out = dict(batch=B, iters=K, dtype=args.dtype, subsystems=rows, vectors=V)
        out["unbound_its"] = B * K / timed([(prob, x0, bufs)])
        prob.declare_instance_subsystem_params(rows)
        prob.bind_instance_values(np.tile(np.array([spec.subsystems[r][3] for r in rows], dtype=np.float32), (B, 1)))
        out["bound_identity_its"] = B * K / timed([(prob, x0, bufs)])
        prob.bind_instance_values(wheelbases)
        out["bound_spread_its"] = B * K / timed([(prob, x0, bufs)])
        out["bound_spread_backtracks"] = float(prob.solve_state(bufs)["backtracks"].float().mean().item())
        prob.bind_instance_values(None)
        per = B // V
        solves = []
        for v in range(V):
            s = copy.deepcopy(spec)
            for r, val in zip(rows, wheelbases[v]):
                kind, xd, ud, _ = s.subsystems[r]
                s.subsystems[r] = (kind, xd, ud, float(val))
            p = hip.Problem(s, dtype)
            solves.append((p, x0[v * per:(v + 1) * per].contiguous(), p.alloc_solve_buffers(per)))
        out["per_vector_problems_its"] = B * K / timed(solves)
        print(json.dumps(out))
        return

    prob = hip.Problem(spec, dtype)
    bufs = prob.alloc_solve_buffers(B)
    out = dict(batch=B, iters=K, dtype=args.dtype, declared=len(DECLARED), vectors=V)
    out["unbound_its"] = B * K / timed([(prob, x0, bufs)])
    out["unbound_backtracks"] = float(prob.solve_state(bufs)["backtracks"].float().mean().item())
    prob.declare_instance_params(params)
    prob.bind_instance_values(identity)
    out["bound_identity_its"] = B * K / timed([(prob, x0, bufs)])
    prob.bind_instance_values(spread)
    out["bound_spread_its"] = B * K / timed([(prob, x0, bufs)])
    out["bound_spread_backtracks"] = float(prob.solve_state(bufs)["backtracks"].float().mean().item())
    prob.bind_instance_values(None)
    # the alternative: V problems, B / V instances each, one after another
    per = B // V
    solves = []
    for v in range(V):
        s = copy.deepcopy(spec)
        for (name, field), val in zip(params, spread[v]):
            s.terms[s.term_index(name)][field] = float(val)
        p = hip.Problem(s, dtype)
        solves.append((p, x0[v * per:(v + 1) * per].contiguous(), p.alloc_solve_buffers(per)))
    out["per_vector_problems_its"] = B * K / timed(solves)
    one = solves[0][0]
    one_bufs = one.alloc_solve_buffers(B)
    out["baked_spread_vector_its"] = B * K / timed([(one, x0, one_bufs)])
    out["baked_spread_vector_backtracks"] = float(one.solve_state(one_bufs)["backtracks"].float().mean().item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
