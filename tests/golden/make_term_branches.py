"""Writes tests/golden/term_branches.json: for every one-term case of tests/term_cases.py and both shapes, how many of
its 402 points take each branch the kind has, and on how many points the fp32 and the fp64 oracle take different
branches (tests/test_gpu_term_branches.py leaves those out in fp32); and the same census along the operating points of
the one-iteration solves that wrap the cases.  Everything is a function of the oracle and of
the committed draw alone, so it is computed here on the CPU and committed; the CPU test recomputes it, the GPU test
fails if it compares fewer points.  Run from the repo root:  python tests/golden/make_term_branches.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle  # noqa: E402
import term_cases as tc  # noqa: E402


def census():
    """{"points": the one-term cases at their 402 points, "games": the same cases along the coasting lines of the
    forced-step solves (which draw of x0 was taken, the branches met, at how many steps two lanes differ in branch)}"""
    out = {"points": {}, "games": {}}
    for shape in tc.SHAPES:
        for name in tc.case_names(shape):
            out["points"]["%s:%s" % (name, shape)] = tc.case_census(name, shape)[0]
        for name in tc.game_names(shape):
            out["games"]["%s:%s" % (name, shape)] = tc.game_census(name, shape)
    return out


if __name__ == "__main__":
    pyoracle.build(force=False)
    result = census()
    for key, c in result["points"].items():
        print(key, c["points"] - c["differ"], "/", c["points"])
    for key, c in result["games"].items():
        print("game", key, "draw", c["draw"], "steps at which lanes differ", c["lanes_differ"])
    json.dump(result, open(os.path.join(ROOT, "tests", "golden", "term_branches.json"), "w"), indent=1)
