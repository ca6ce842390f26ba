#!/usr/bin/env python
"""What an expression cost costs against the built-in kind it restates: examples.cost_zoo_scene (n = 10, T = 100, the
specialised (10, 2, 2) kernels, interpreted row stage) and its twin (examples.expression_twin: ten of its terms — the
single-dimension QuadraticCosts, the CurvatureCosts, the SemiquadraticNormCosts on a state pair — as expression costs) at
B = 1024, 20 fixed iterations from a zero warm start, the library's AUTO schedule, both precisions.  Prints one JSON line:
iterations per second of both and their ratio (median of --repeats timed solves, alternating).

  python scripts/expression_cost_bench.py [--batch 1024] [--iters 20] [--repeats 5]
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
    args = ap.parse_args()
    import torch
    from ilqgames_amd import abi, examples, hip
    spec = examples.cost_zoo_scene()
    twin, replaced = examples.expression_twin(spec)
    x0 = examples.jittered_x0(spec, args.batch, seed=1)
    out = dict(scene="cost_zoo_scene", batch=args.batch, iters=args.iters, terms_replaced=replaced, terms=len(spec.terms))
    for dtype, name in ((abi.F64, "f64"), (abi.F32, "f32")):
        probs = [hip.Problem(spec, dtype), hip.Problem(twin, dtype)]
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
        its = [args.batch * args.iters / float(np.median(t)) for t in times]
        out[name] = dict(built_in_its=round(its[0]), expression_its=round(its[1]), ratio=round(its[1] / its[0], 4),
                         schedule=[p.last_schedule() for p in probs])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
