"""Writes tests/golden/schedule_cases.json: the schedule a solve chose (ilqg_problem_last_schedule) for every case of
tests/schedule_cases.py, on the device it is run on, with that device's CU count.  Needs a GPU; run from the repo root:
    python tests/golden/make_schedule_cases.py
The finer fields (chunk widths, LDS bytes, which instantiation each launch was bound to, the per-round probing choices)
are no part of the API: they are read from the file ILQG_SCHED_DUMP names, where the library under record was built with
a print of its schedule locals into that file ("S key=value ..." per solve, "R ..." / "F ..." per probing round); without
the variable only the schedule words are recorded.  The file's layout (tests/schedule_cases.py: encode_records) keeps it
small: the cases stand in one fixed order, and what repeats from case to case is stored once."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import schedule_cases as sc  # noqa: E402
from ilqgames_amd import abi, hip  # noqa: E402

DUMP = os.environ.get("ILQG_SCHED_DUMP")


def dump_lines():
    """The lines the library printed since the last call."""
    if not DUMP or not os.path.exists(DUMP):
        return []
    lines = open(DUMP).read().splitlines()
    open(DUMP, "w").close()
    return lines


def parse(line):
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split()[1:])}


class Table:
    """Distinct rows of integers under one list of field names; add() -> the row's index."""

    def __init__(self):
        self.fields, self.rows, self.index = None, [], {}

    def add(self, rec):
        if self.fields is None:
            self.fields = list(rec)
        row = tuple(rec[f] for f in self.fields)
        if row not in self.index:
            self.index[row] = len(self.rows)
            self.rows.append(list(row))
        return self.index[row]

    def json(self):
        return {"fields": self.fields or [], "rows": self.rows}


def main():
    name, C = hip.device_info()
    scenes, optsets = list(sc.SCENES), list(sc.OPTION_SETS)
    rounds, forms = Table(), Table()
    blocks, records = sc.case_blocks(scenes, optsets, C), []
    dump_lines()
    probs = {}
    for (scene, T, dtype, oname), keys in blocks:
        opts = sc.OPTION_SETS[oname]
        pkey = (scene, T, dtype, bool(opts.get("open_loop")))
        if pkey not in probs:
            spec = sc.make_spec(scene, T, pkey[3])
            probs = {k: v for k, v in probs.items() if k[:3] == pkey[:3]}  # (a scene's problems go when the next one's come)
            probs[pkey] = (hip.Problem(spec, dtype), spec, {})
        prob, spec, bufs = probs[pkey]
        for batch, _ in keys:
            word = sc.solve_case(prob, spec, opts, batch, C, bufs)  # (a refused solve ends the recording)
            s = [parse(l) for l in dump_lines() if l.startswith("S ")]
            assert len(s) <= 1 and all(r["word"] == word for r in s)
            records.append(s[0] if s else {"word": word})
        print(scene, T, dtype, oname, len(records), flush=True)
    # the per-round choices: free-running solves that back-track (the n = 15 and n = 16 scenes at their own horizon)
    for scene in ("n15", "n16"):
        spec = sc.make_spec(scene, 100)
        for dtype in (abi.F32, abi.F64):
            prob = hip.Problem(spec, dtype)
            for B in (64, 1024):
                for al in ((False, True) if scene == "n16" else (False,)):
                    prob.solve(sc.examples.jittered_x0(spec, B, seed=1), augmented_lagrangian=al)
                    for l in dump_lines():
                        if l.startswith("R "):
                            rounds.add(parse(l))
                        elif l.startswith("F "):
                            forms.add(parse(l))
            print(scene, dtype, len(rounds.rows), len(forms.rows), flush=True)
    out = {"device": name, "num_cus": C, "scenes": scenes, "option_sets": optsets,
           "groups": sc.encode_records(blocks, records), "rounds": rounds.json(), "forms": forms.json()}
    path = os.path.join(ROOT, os.environ.get("ILQG_SCHED_OUT", os.path.join("tests", "golden", "schedule_cases.json")))
    write_json(path, out)
    print("wrote", path, len(records), "cases")


def write_json(path, out):
    """One line per table row, so that a change of the record shows as the rows it changes."""
    def rows(v, depth):
        if depth == 0 or not isinstance(v, (list, dict)):
            return json.dumps(v, separators=(",", ":"))
        if isinstance(v, dict):
            return "{\n" + ",\n".join("%s:%s" % (json.dumps(k), rows(x, depth - 1)) for k, x in v.items()) + "\n}"
        return "[\n" + ",\n".join(rows(x, depth - 1) for x in v) + "\n]"
    with open(path, "w") as f:
        f.write(rows(out, 3) + "\n")


if __name__ == "__main__":
    main()
