"""Writes tests/golden/lq_time_games.json: per game of tests/lq_time_games.py and per output, how far the numpy reference
is from itself in the next wider scalar type — gap64 = |float64 - longdouble|, gap32 = |float32 - float64|, the largest
relative distance over the 3 instances and the 4 forced iterations, as tests/golden/make_lq_games.py records them for
tests/lq_games.py.  The device's bars are 100 x these (tests/test_gpu_expression_time.py); tests/test_lq_time_games.py
recomputes them and holds the file to them within a factor of 2.  CPU only.  Run from the repo root:
python tests/golden/make_lq_time_games.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lq_time_games  # noqa: E402

out = {}
for name in lq_time_games.GAMES:
    out[name] = lq_time_games.gaps(name)
    print(name, " ".join("%s %.1e/%.1e" % (q, out[name]["gap64"][q], out[name]["gap32"][q]) for q in lq_time_games.OUTPUTS))
json.dump(out, open(os.path.join(ROOT, "tests", "golden", "lq_time_games.json"), "w"), indent=1)
