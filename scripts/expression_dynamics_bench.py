#!/usr/bin/env python
"""What expression dynamics cost against the built-in kinds they restate: examples.delayed_dubins_scene (n = 8, the
specialised (8, 2, 1) kernels) and examples.dynamics_zoo_scene (n = 17, (17, 3, 2): one Car7D, two Unicycle5D), each
against its examples.expression_dynamics_twin (every subsystem an ILQG_DYN_EXPRESSION subsystem), T = 100, fixed
iterations from a zero warm start, the library's AUTO schedule, both precisions.  delayed_dubins_scene: B = 1024, 20
iterations.  dynamics_zoo_scene: B = 256, 5 iterations — from a zero warm start its line searches reject about ten steps
an iteration and instance (the built-in kinds' too: the count is printed), every one a rollout, so the sizes of the first
scene take the twin minutes a solve.  Prints one JSON line per scene: iterations per second of both and their ratio — the
median of --repeats timed solves, the two problems alternating, with the spread (slowest, fastest) of each — and, on
stderr, each warm-up solve's time and rejected steps.

  python scripts/expression_dynamics_bench.py [--scene NAME] [--batch B] [--iters K] [--repeats 7]
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
    ap.add_argument("--batch", type=int, default=None, help="default: 1024 (delayed_dubins_scene), 256 (dynamics_zoo_scene)")
    ap.add_argument("--iters", type=int, default=None, help="default: 20 (delayed_dubins_scene), 5 (dynamics_zoo_scene)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scene", choices=["delayed_dubins_scene", "dynamics_zoo_scene"], default=None)
    args = ap.parse_args()
    import torch
    from ilqgames_amd import abi, examples, hip
    sizes = {"delayed_dubins_scene": (1024, 20), "dynamics_zoo_scene": (256, 5)}
    for scene in ([args.scene] if args.scene else list(sizes)):
        batch = args.batch if args.batch is not None else sizes[scene][0]
        iters = args.iters if args.iters is not None else sizes[scene][1]
        spec = getattr(examples, scene)()
        twin, restated = examples.expression_dynamics_twin(spec)
        x0 = examples.jittered_x0(spec, batch, seed=1)
        out = dict(scene=scene, batch=batch, iters=iters, subsystems_restated=restated)
        for dtype, name in ((abi.F64, "f64"), (abi.F32, "f32")):
            probs = [hip.Problem(spec, dtype), hip.Problem(twin, dtype)]
            bufs = [p.alloc_solve_buffers(batch) for p in probs]
            times, backtracks = [[], []], [0, 0]
            for rep in range(args.repeats + 1):  # the first pair warms up
                for q, prob in enumerate(probs):
                    for k in ("xs", "us", "P", "alpha"):
                        bufs[q][k].zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    prob.solve(x0, bufs[q], fixed_iters=iters)
                    e1.record()
                    torch.cuda.synchronize()
                    secs = e0.elapsed_time(e1) * 1e-3
                    if rep:
                        times[q].append(secs)
                    else:  # progress, and what the line searches of the warm-up solve rejected (stderr: the line stays JSON)
                        rejected = int(prob.solve_state(bufs[q])["backtracks"].sum().item())
                        sys.stderr.write("%s %s %s: warm-up solve %.3f s, %d rejected steps\n" %
                                         (scene, name, "twin" if q else "built-in", secs, rejected))
                        sys.stderr.flush()
                        backtracks[q] = rejected
            done = batch * iters
            its = [done / float(np.median(t)) for t in times]
            spread = [[round(done / max(t)), round(done / min(t))] for t in times]
            out[name] = dict(built_in_its=round(its[0]), expression_its=round(its[1]), ratio=round(its[1] / its[0], 4),
                             built_in_spread=spread[0], expression_spread=spread[1], rejected_steps=backtracks,
                             schedule=[p.last_schedule() for p in probs])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
