#!/usr/bin/env python
"""What expression children of an ExtremeValueCost cost against the built-in children they restate: BASELINE.json
configuration 5's scene, examples.three_player_collision_avoidance_reachability (n = 15, T = 100, three players with
max-over-time costs, the specialised (15, 3, 2) kernels with the registered static row program), against its
examples.reachability_twin — the six SignedDistanceCost children as expression children and the twelve control box
constraints as expression constraints, the interpreted row stage — at B = 2048, fp64, a fixed number of iterations from a
zero warm start, the library's AUTO schedule.  The two solves alternate in one process.  Prints one JSON line: iterations
per second of both (median of --repeats timed solves, with the smallest and largest: the run-to-run spread) and their ratio.

--children-only: the twin keeps the built-in control constraints (only the children are restated), which isolates what
the children themselves cost.

  python scripts/expression_children_bench.py [--children-only] [--batch 2048] [--iters 20] [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--children-only", action="store_true", help="restate the children only, keep the built-in constraints")
    args = ap.parse_args()
    import torch
    from ilqgames_amd import abi, examples, hip
    spec = examples.three_player_collision_avoidance_reachability()
    twin, replaced = examples.reachability_twin(spec)
    if args.children_only:
        for q, t in enumerate(spec.terms):
            if t["role"] != abi.ROLE_CHILD:
                replaced -= twin.terms[q]["kind"] != t["kind"]
                twin.terms[q] = dict(t)
    x0 = examples.jittered_x0(spec, args.batch, seed=1)
    probs = [hip.Problem(spec, abi.F64), hip.Problem(twin, abi.F64)]
    bufs = [p.alloc_solve_buffers(args.batch) for p in probs]
    times = [[], []]
    for rep in range(args.repeats + 1):  # the first pair warms up
        for q, prob in enumerate(probs):
            for k in ("xs", "us", "P", "alpha"):
                bufs[q][k].zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            prob.solve(x0, bufs[q], fixed_iters=args.iters)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[q].append(e0.elapsed_time(e1) * 1e-3)
    work = args.batch * args.iters
    rate = lambda ts: dict(median=round(work / float(np.median(ts))), slowest=round(work / max(ts)), fastest=round(work / min(ts)))
    out = dict(scene="three_player_collision_avoidance_reachability", batch=args.batch, iters=args.iters, dtype="f64",
               terms_replaced=int(replaced), terms=len(spec.terms), built_in_its=rate(times[0]), expression_its=rate(times[1]),
               ratio=round(float(np.median(times[0]) / np.median(times[1])), 4), schedule=[p.last_schedule() for p in probs])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
