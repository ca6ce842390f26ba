"""What the feedback sweep may assume about B (ilqg_sweep_b_structure_build, host only): the library calls a problem's B
"constant" when its solves read compact rows, no entry of B is computed and every row and column of B holds at most
one entry — B is then dt times a signed selection matrix, the same at every step and in every instance, and the
player-parallel sweep takes its entries from registers (ilqg_solve_options::sweep_forms).  The list is checked against
the B the oracle's Linearize returns: where the library says constant, B is exactly the listed entries and nothing else,
at any state."""
import os

import numpy as np
import pytest

from ilqgames_amd import abi, examples


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return h


def _listed_b(spec, entries):
    """The (n, m) matrix the entry list stands for."""
    B = np.zeros((spec.n, spec.m))
    for row, col, kind, bits in entries:
        assert 0 <= row < spec.n and 0 <= col < spec.m
        assert B[row, col] == 0.0, "an entry listed twice"
        B[row, col] = {abi.B_ENTRY_DT: spec.dt, abi.B_ENTRY_NEG_DT: -spec.dt}.get(
            int(kind), float(np.array([bits], np.int32).view(np.float32)[0]))
    return B


@pytest.mark.parametrize("scene", sorted(examples.CONFIGS))
def test_listed_entries_are_the_oracles_b(hip, oracle, scene):
    spec = examples.CONFIGS[scene]()
    constant, entries = hip.sweep_b_structure(spec)
    listed = _listed_b(spec, entries)
    rng = np.random.default_rng(3)
    xs = rng.normal(0.0, 2.0, (2, spec.T, spec.n))  # two random states per step (two instances)
    us = rng.normal(0.0, 1.0, (2, spec.T, spec.m))
    _, Bm = oracle.OracleProblem(spec).linearize(abi.F64, xs, us)
    Bo = Bm.reshape(2, spec.T, spec.m, spec.n).transpose(0, 1, 3, 2)  # column-major words -> [row][column]
    at = listed != 0.0
    assert np.array_equal(Bo[..., at], np.broadcast_to(listed[at], Bo[..., at].shape))  # wherever an entry is listed
    if constant:
        assert np.array_equal(Bo, np.broadcast_to(listed, Bo.shape))  # ... and nothing else, at any state
        assert np.all((listed != 0.0).sum(axis=0) <= 1) and np.all((listed != 0.0).sum(axis=1) <= 1)
    assert hip.sweep_b_structure(spec, abi.F32)[0] == constant


REGISTERED = ["modified_three_player_intersection",             # the headline, (14, 3, 2)
              "three_player_intersection",                       # (16, 3, 2)
              "three_player_collision_avoidance_reachability",  # config 5's scene, (15, 3, 2)
              "roundabout_merging"]                              # (24, 4, 2)


@pytest.mark.parametrize("scene", REGISTERED)
def test_registered_scenes_have_a_constant_b(hip, scene):
    spec = examples.CONFIGS[scene]()
    _, static_id = hip.row_program_build(spec)
    assert static_id > 0, "a registered structure"
    constant, entries = hip.sweep_b_structure(spec)
    assert constant
    assert len(entries) == spec.m and sorted(entries[:, 1]) == list(range(spec.m))  # one entry per control
    assert set(entries[:, 2]) == {abi.B_ENTRY_DT}


def test_headline_entries_are_the_six_the_sweep_expects(hip):
    _, entries = hip.sweep_b_structure(examples.modified_three_player_intersection())
    assert sorted((int(r), int(c)) for r, c, _, _ in entries) == [(3, 0), (4, 1), (8, 2), (9, 3), (12, 4), (13, 5)]


def _two_car7d():
    s = abi.ProblemSpec()
    for i in range(2):
        s.add_player(abi.DYN_CAR_7D, 4.0)
    for i in range(2):
        s.quadratic(i, 1.0, 0, 0.0, control_of=i)
        s.quadratic(i, 1.0, 1, 0.0, control_of=i)
    return s


@pytest.mark.parametrize("make", [examples.dynamics_zoo_scene, _two_car7d, examples.air_3d],
                         ids=["car7d_zoo", "two_car7d", "air_3d"])
def test_a_computed_entry_of_b_is_not_constant(hip, make):
    """Car7D: B(kappa, omega) is computed and shares column omega with the constant B(phi, omega); Air3D: the evader's
    turn rate enters (rx, ry) through computed entries."""
    constant, _ = hip.sweep_b_structure(make())
    assert not constant
