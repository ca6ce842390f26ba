"""The branch census of the one-term cases (tests/term_cases.py): what tests/test_gpu_term_branches.py compares the
device on, established on the CPU from the oracle alone."""
import json
import os

import numpy as np
import pytest

from ilqgames_amd import abi
import term_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "term_branches.json")
MIN_POINTS = 12
# the branches the stage test of test_gpu_parity.py never or hardly reaches, by name: a census that merely lost one of
# them would otherwise still pass the "every branch it lists" condition
REQUIRED = [
    "cost_orientation.wrapped", "cost_orientation.negative_remainder", "cost_orientation.plain",
    "cost_semiquadratic.oriented.active", "cost_semiquadratic.unoriented.active", "cost_semiquadratic.oriented.on_threshold",
    "cost_semiquadratic.control.oriented.active", "cost_semiquadratic.control.unoriented.active",
    "cost_semiquadratic_norm.oriented.active", "cost_semiquadratic_norm.unoriented.active",
    "cost_semiquadratic_norm.control.oriented.active", "cost_semiquadratic_norm.control.unoriented.active",
    "cost_semiquadratic_norm.control.oriented.inactive",
    "constraint_polyline2_signed_distance.oriented.right_vertex", "constraint_polyline2_signed_distance.oriented.left_vertex",
    "constraint_polyline2_signed_distance.unoriented.right_vertex",
    "constraint_polyline2_signed_distance.unoriented.left_vertex",
    "constraint_polyline2_signed_distance.unoriented.right_interior", "constraint_polyline2_signed_distance.oriented.mu0",
    "cost_polyline2_signed_distance.oriented.left", "cost_polyline2_signed_distance.unoriented.left",
    "cost_polyline2_signed_distance.oriented.vertex", "cost_polyline2_signed_distance.unoriented.vertex",
    "cost_quadratic_polyline2.end_point", "cost_quadratic_polyline2.vertex", "cost_quadratic_polyline2.interior",
    "cost_semiquadratic_polyline2.oriented.active_vertex", "cost_semiquadratic_polyline2.oriented.active_interior",
    "cost_semiquadratic_polyline2.oriented.end_point", "cost_semiquadratic_polyline2.oriented.on_threshold",
    "cost_semiquadratic_polyline2.unoriented.active_interior", "cost_semiquadratic_polyline2.unoriented.on_threshold",
    "cost_proximity.active", "cost_proximity.inactive", "cost_proximity.on_threshold",
    "cost_signed_distance.oriented.all", "cost_signed_distance.unoriented.all",
    "cost_extreme_value.max.child0", "cost_extreme_value.max.child1", "cost_extreme_value.min.child0",
    "cost_extreme_value.min.child1",
    "cost_locally_convex_proximity.x_active", "cost_locally_convex_proximity.y_active", "cost_locally_convex_proximity.tie",
    "cost_locally_convex_proximity.outside", "cost_locally_convex_proximity.on_threshold",
    "cost_weighted_convex_proximity.x_active", "cost_weighted_convex_proximity.y_active",
    "cost_weighted_convex_proximity.tie", "cost_weighted_convex_proximity.difference_positive",
    "cost_weighted_convex_proximity.difference_not_positive", "cost_weighted_convex_proximity.on_threshold",
    "constraint_proximity.oriented.mu0", "constraint_proximity.unoriented.mu0", "constraint_proximity.oriented.mu",
    "constraint_proximity.unoriented.mu", "constraint_proximity.oriented.lambda_on_threshold",
    "constraint_single_dimension.oriented.mu0", "constraint_single_dimension.unoriented.mu0",
    "constraint_single_dimension.oriented.lambda_on_threshold", "constraint_single_dimension.oriented.g_on_threshold",
    "constraint_single_dimension.oriented.g_just_below_threshold", "constraint_single_dimension.oriented.g_just_above_threshold",
    "constraint_single_dimension.unoriented.g_just_below_threshold",
    "constraint_proximity.oriented.g_just_below_threshold", "constraint_proximity.oriented.g_just_above_threshold",
    "constraint_proximity.unoriented.g_just_below_threshold", "constraint_proximity.unoriented.g_just_above_threshold",
    "constraint_polyline2_signed_distance.oriented.g_just_below_threshold",
    "constraint_polyline2_signed_distance.oriented.g_just_above_threshold",
    "constraint_polyline2_signed_distance.unoriented.g_just_below_threshold",
    "constraint_polyline2_signed_distance.unoriented.g_just_above_threshold",
    "constraint_polyline2_signed_distance.oriented.lambda_on_threshold",
    "final_time.before", "final_time.after",
]
INACTIVE = (".inactive", ".outside", ".before")
ACTIVE = (".active", ".x_active", ".y_active", ".active_vertex", ".active_interior")


@pytest.fixture(scope="module")
def census(oracle):
    return {"%s:%s" % (name, shape): tc.case_census(name, shape)[0]
            for shape in tc.SHAPES for name in tc.case_names(shape)}


@pytest.fixture(scope="module")
def games(oracle):
    return {"%s:%s" % (name, shape): tc.game_census(name, shape)
            for shape in tc.SHAPES for name in tc.game_names(shape)}


def test_census_equals_the_committed_file(census, games):
    """Regenerating tests/golden/term_branches.json (make_term_branches.py) reproduces it."""
    assert json.load(open(GOLDEN)) == {"points": census, "games": games}


@pytest.mark.parametrize("shape", tc.SHAPES)
def test_every_branch_of_every_kind_has_points(census, shape):
    """Per kind (summed over the cases of the kind, points both precisions classify alike only): every branch has at
    least 12 points, and the branches the issue names are among them."""
    total = {}
    for key, c in census.items():
        if key.endswith(":" + shape):
            for f, cnt in c["flags"].items():
                total[f] = total.get(f, 0) + cnt
    missing = [f for f in REQUIRED if f not in total]
    assert not missing, missing
    thin = {f: cnt for f, cnt in total.items() if cnt < MIN_POINTS}
    assert not thin, thin


def test_precisions_take_the_same_branch(census):
    """At most 2 % of a case's points are classified differently by the fp32 and the fp64 oracle."""
    for key, c in census.items():
        assert c["differ"] <= 0.02 * c["points"], (key, c["differ"])


@pytest.mark.parametrize("shape", tc.SHAPES)
def test_flags_agree_with_the_oracle_rows(oracle, shape):
    """The classification is tied to the oracle's own output: where every term of the case is on an inactive branch
    the oracle's rows are bit for bit the base problem's (the control costs alone), and where a term is on an active
    branch they are not."""
    for name in tc.case_names(shape):
        p = tc.case_points(name, shape)
        classes = tc.case_classes(name, shape, abi.F64)
        rows = [oracle.OracleProblem(s).quadraticize(abi.F64, p["xs"], p["us"], p["lam"], p["mu"], p["te"])
                for s in (p["spec"], tc.make_spec(None, shape))]
        same = np.ones((tc.B, tc.T), bool)
        for a, b in zip(*rows):
            same &= (a.reshape(tc.B, tc.T, -1) == b.reshape(tc.B, tc.T, -1)).all(axis=2)
        for b in range(tc.B):
            for k in range(tc.T):
                flags = [f for f in classes[b, k] if not f.endswith((".on_threshold", ".tie"))]
                if flags and all(f.endswith(INACTIVE) for f in flags):
                    assert same[b, k], (name, b, k, flags)
                elif any(f.endswith(ACTIVE) for f in flags):
                    assert not same[b, k], (name, b, k, flags)


def _by_kind(cases, shape):
    total = {}
    for key, c in cases.items():
        if key.endswith(":" + shape):
            for f, cnt in c["flags"].items():
                total[f] = total.get(f, 0) + cnt
    return total


@pytest.mark.parametrize("shape", tc.SHAPES)
def test_games_reach_every_branch_along_their_coasting_lines(census, games, shape):
    """The operating points of the one-iteration solves (functions of x0 alone) meet the same condition: per kind every
    branch that is not a single point of measure zero (a threshold hit exactly, a tie) has at least 12 points, and
    wherever a case has more than one branch, lanes of one wavefront sit in different branches at some step.  That
    the oracle resolves every instance of every game in both precisions is what term_cases.game_inputs selects by."""
    reachable = {f for key, c in census.items() if key.endswith(":" + shape) and key.split(":")[0] in tc.game_names(shape)
                 for f in c["flags"] if not f.endswith(tc.BOUNDARY_FLAGS)}
    total = _by_kind(games, shape)
    thin = {f: total.get(f, 0) for f in reachable | set(total) if total.get(f, 0) < MIN_POINTS}
    assert not thin, thin
    for key, c in games.items():
        if key.endswith(":" + shape) and len(c["flags"]) > 1:
            assert c["lanes_differ"] > 0, key
