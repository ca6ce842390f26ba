#!/usr/bin/env python
"""What an expression cost costs against the built-in kind it restates: examples.cost_zoo_scene (n = 10, T = 100, the
specialised (10, 2, 2) kernels, interpreted row stage) and its twin (examples.expression_twin: ten of its terms — the
single-dimension QuadraticCosts, the CurvatureCosts, the SemiquadraticNormCosts on a state pair — as expression costs) at
B = 1024, 20 fixed iterations from a zero warm start, the library's AUTO schedule, both precisions.  Prints one JSON line:
iterations per second of both and their ratio (median of --repeats timed solves, alternating).

--relative: examples.skeleton against its examples.expression_game_twin (its proximity costs over relative inputs, beside
the restatements above), the same fixed-iteration solve.  --constraints: examples.three_player_intersection (n = 16, the
(16, 3, 2) kernels) against its twin with six expression proximity constraints, an augmented-Lagrangian solve (the
iterations are each instance's own: the rate is their sum over the time).

  python scripts/expression_cost_bench.py [--relative | --constraints] [--batch 1024] [--iters 20] [--repeats 5]
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--relative", action="store_true", help="skeleton against its twin with expression proximity costs")
    ap.add_argument("--constraints", action="store_true",
                    help="three_player_intersection against its twin with six expression proximity constraints, AL solve")
    args = ap.parse_args()
    import torch
    from ilqgames_amd import abi, examples, hip
    al = args.constraints
    if args.constraints:
        scene, spec = "three_player_intersection", examples.three_player_intersection()
        twin, replaced = examples.expression_game_twin(spec)
    elif args.relative:
        scene, spec = "skeleton", examples.skeleton()
        twin, replaced = examples.expression_game_twin(spec)
    else:
        scene, spec = "cost_zoo_scene", examples.cost_zoo_scene()
        twin, replaced = examples.expression_twin(spec)
    x0 = examples.jittered_x0(spec, args.batch, seed=1)
    out = dict(scene=scene, batch=args.batch, iters=None if al else args.iters, terms_replaced=replaced, terms=len(spec.terms))
    for dtype, name in ((abi.F64, "f64"), (abi.F32, "f32")):
        probs = [hip.Problem(spec, dtype), hip.Problem(twin, dtype)]
        bufs = [p.alloc_solve_buffers(args.batch) for p in probs]
        times, done = [[], []], [0, 0]
        for rep in range(args.repeats + 1):  # the first pair warms up
            for q, prob in enumerate(probs):
                for k in ("xs", "us", "P", "alpha"):
                    bufs[q][k].zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                if al:
                    prob.solve(x0, bufs[q], augmented_lagrangian=True)
                else:
                    prob.solve(x0, bufs[q], fixed_iters=args.iters)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[q].append(e0.elapsed_time(e1) * 1e-3)
                done[q] = int(bufs[q]["iters"].sum().item()) if al else args.batch * args.iters
        its = [done[q] / float(np.median(times[q])) for q in range(2)]
        out[name] = dict(built_in_its=round(its[0]), expression_its=round(its[1]), ratio=round(its[1] / its[0], 4),
                         schedule=[p.last_schedule() for p in probs])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
