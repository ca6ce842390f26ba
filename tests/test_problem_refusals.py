"""What problem creation refuses before it builds a device table, through the host-only entry point
(ilqg_row_program_build: the same validation and table building as ilqg_problem_create, no device needed): the status and
a fragment of the message of each refusal, in the order creation checks them."""
import ctypes as C
import os

import pytest

from ilqgames_amd import abi, examples


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return h


def _build(hip, spec, patch_desc=None, dtype=abi.F64):
    """(status, message) of ilqg_row_program_build on the spec's descriptor, after `patch_desc(desc)`."""
    desc, keep = spec.build(dtype)
    if patch_desc is not None:
        patch_desc(desc)
    n, sid = C.c_int32(0), C.c_int32(0)
    rc = hip.lib().ilqg_row_program_build(C.byref(desc), None, 0, C.byref(n), C.byref(sid))
    del keep
    return rc, (hip.lib().ilqg_last_error().decode() if rc else "")


def _two_cars():
    return examples.skeleton()


def _players(*kinds):
    s = abi.ProblemSpec()
    for i, kind in enumerate(kinds):
        s.add_player(kind, 1.0)
    for i, kind in enumerate(kinds):
        s.quadratic(i, 1.0, 0, 0.0, control_of=i)
    return s


def _set(field, value):
    def patch(desc):
        setattr(desc, field, value)
    return patch


def _subsystem(i, **fields):
    def patch(desc):
        for k, v in fields.items():
            setattr(desc.subsystems[i], k, v)
    return patch


def _with_term(spec, index, **fields):
    spec.terms[index].update(fields)
    return spec


def _first(spec, kind):
    return [t["kind"] for t in spec.terms].index(kind)


def _no_control_hessian():
    s = _two_cars()
    s.terms = [t for t in s.terms if not (t["role"] == abi.ROLE_CONTROL_COST and t["player"] == 1)]
    return s


def _wcp_speed_index(value):
    s = examples.weighted_proximity_scene()
    return _with_term(s, _first(s, abi.COST_WEIGHTED_CONVEX_PROXIMITY), idx_extra=(value, 0))


def _equality_on_single_dimension():
    s = examples.mixed_dubins_car_scene(constrained=True)
    return _with_term(s, _first(s, abi.CONSTRAINT_SINGLE_DIMENSION), flags=abi.FLAG_EQUALITY)


def _affine(**fields):
    s = examples.affine_constraint_scene()
    return _with_term(s, _first(s, abi.CONSTRAINT_AFFINE_VECTOR), **fields)


def _time_dependent(kind, **fields):
    s = examples.dynamics_zoo_scene()
    return _with_term(s, _first(s, kind), **fields)


def _route_without_segment():
    s = examples.dynamics_zoo_scene()
    t = s.terms[_first(s, abi.COST_ROUTE_PROGRESS)]
    t["polyline"] = s.add_polyline([(0.0, 0.0)])
    return s


def _empty_extreme_value():
    s = examples.three_player_collision_avoidance_reachability()
    return _with_term(s, _first(s, abi.COST_EXTREME_VALUE), child_count=0)


def _quadratic_outside_the_state():
    s = _two_cars()
    s.quadratic(0, 1.0, s.n, 0.0)
    return s


# (name, spec maker, descriptor patch or None, status, fragment of the message)
REFUSALS = [
    ("no players", _two_cars, _set("num_players", 0), abi.ERR_INVALID, "bad player count"),
    ("too many players", _two_cars, _set("num_players", abi.MAX_PLAYERS + 1), abi.ERR_INVALID, "bad player count"),
    ("horizon of one step", _two_cars, _set("T", 1), abi.ERR_INVALID, "bad horizon"),
    ("horizon beyond the tables", _two_cars, _set("T", 257), abi.ERR_INVALID, "bad horizon"),
    ("unknown subsystem kind", _two_cars, _subsystem(1, kind=99), abi.ERR_UNSUPPORTED, "unknown subsystem kind / dimension"),
    ("kind zero", _two_cars, _subsystem(0, kind=0), abi.ERR_UNSUPPORTED, "unknown subsystem kind / dimension"),
    ("wrong state dimension", _two_cars, _subsystem(0, xdim=4), abi.ERR_UNSUPPORTED, "unknown subsystem kind / dimension"),
    ("wrong control dimension", _two_cars, _subsystem(1, udim=1), abi.ERR_UNSUPPORTED, "unknown subsystem kind / dimension"),
    ("a disturbance without its unicycle", lambda: _players(abi.DYN_UNICYCLE_4D, abi.DYN_PLANAR_DISTURBANCE), None,
     abi.ERR_UNSUPPORTED, "shared-state kinds only occur as the pairs"),
    ("the Air3D pair the wrong way round", lambda: _players(abi.DYN_AIR_3D_PURSUER, abi.DYN_AIR_3D_EVADER), None,
     abi.ERR_UNSUPPORTED, "shared-state kinds only occur as the pairs"),
    ("a third player beside a pair", lambda: _players(abi.DYN_AIR_3D_EVADER, abi.DYN_AIR_3D_PURSUER, abi.DYN_UNICYCLE_4D),
     None, abi.ERR_UNSUPPORTED, "shared-state kinds only occur as the pairs"),
    ("a point mass among cars", lambda: _players(abi.DYN_CAR_5D, abi.DYN_POINT_MASS_2D), None,
     abi.ERR_UNSUPPORTED, "point masses (kind 9) only occur in games made of point masses"),
    ("a car among point masses", lambda: _players(abi.DYN_POINT_MASS_2D, abi.DYN_CAR_5D), None,
     abi.ERR_UNSUPPORTED, "point masses (kind 9) only occur in games made of point masses"),
    ("35 states", lambda: _players(*[abi.DYN_CAR_7D] * 5), None, abi.ERR_UNSUPPORTED, "more than ILQG_MAX_XDIM states"),
    ("a player without a control Hessian", _no_control_hessian, None, abi.ERR_INVALID,
     "player 1 is missing a control Hessian"),
    ("a speed index beyond the state", lambda: _wcp_speed_index(10), None, abi.ERR_INVALID,
     "WeightedConvexProximityCost must be a top-level state cost with speed indices"),
    ("a negative speed index", lambda: _wcp_speed_index(-1), None, abi.ERR_INVALID,
     "WeightedConvexProximityCost must be a top-level state cost with speed indices"),
    ("an equality that is not affine", _equality_on_single_dimension, None, abi.ERR_INVALID,
     "ILQG_FLAG_EQUALITY is only defined for the affine constraints"),
    ("an affine constraint without coefficients", lambda: _affine(polyline=-1), None, abi.ERR_INVALID,
     "a coefficient block inside ilqg_problem_desc::dense_params"),
    ("a coefficient block past the end", lambda: _affine(polyline=10 ** 6), None, abi.ERR_INVALID,
     "a coefficient block inside ilqg_problem_desc::dense_params"),
    ("no dense_params at all", examples.affine_constraint_scene, _set("dense_params", None), abi.ERR_INVALID,
     "a coefficient block inside ilqg_problem_desc::dense_params"),
    ("an affine constraint without a multiplier slot", lambda: _affine(constraint_slot=-1), None, abi.ERR_INVALID,
     "an affine constraint must be a state / control constraint with a multiplier slot"),
    ("a path-length cost as a child", lambda: _time_dependent(abi.COST_NOMINAL_PATH_LENGTH, role=abi.ROLE_CHILD), None,
     abi.ERR_INVALID, "a time-dependent cost must be a top-level state cost"),
    ("a route cost without a polyline", lambda: _time_dependent(abi.COST_ROUTE_PROGRESS, polyline=-1), None,
     abi.ERR_INVALID, "a time-dependent cost must be a top-level state cost"),
    ("a route without a segment", _route_without_segment, None, abi.ERR_INVALID,
     "RouteProgressCost: the route needs a segment"),
    ("a route position that goes negative", lambda: _time_dependent(abi.COST_ROUTE_PROGRESS, value2=-1.0), None,
     abi.ERR_INVALID, "a route position that stays non-negative"),
    ("an ExtremeValueCost without children", _empty_extreme_value, None, abi.ERR_UNSUPPORTED,
     "row program: bad ExtremeValueCost"),
    ("a quadratic cost outside the state", _quadratic_outside_the_state, None, abi.ERR_UNSUPPORTED,
     "row program: a term's indices are out of range or not distinct"),
]


@pytest.mark.parametrize("name,make,patch,status,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("dtype", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_creation_refuses(hip, dtype, name, make, patch, status, fragment):
    rc, msg = _build(hip, make(), patch, dtype)
    assert rc == status, (rc, msg)
    assert fragment in msg, msg


def test_the_first_failing_check_is_the_one_reported(hip):
    """A description that trips several checks reports the earliest: the player count before the horizon, a subsystem
    before a term, a term before the row program."""
    def both(desc):
        desc.num_players, desc.T = 0, 1
    assert "bad player count" in _build(hip, _two_cars(), both)[1]
    s = _wcp_speed_index(10)
    assert "unknown subsystem kind" in _build(hip, s, _subsystem(0, kind=99))[1]
    assert "bad horizon" in _build(hip, s, lambda d: (_subsystem(0, kind=99)(d), _set("T", 1)(d)))[1]
    s = _no_control_hessian()
    s.quadratic(0, 1.0, s.n, 0.0)
    assert "missing a control Hessian" in _build(hip, s)[1]
    s = _equality_on_single_dimension()
    s.quadratic(0, 1.0, s.n, 0.0)
    assert "ILQG_FLAG_EQUALITY" in _build(hip, s)[1]


def test_null_arguments_and_the_untouched_scenes(hip):
    n = C.c_int32(0)
    desc, keep = _two_cars().build(abi.F64)
    assert hip.lib().ilqg_row_program_build(C.byref(desc), None, 0, None, None) == abi.ERR_INVALID
    assert hip.lib().ilqg_row_program_build(None, None, 0, C.byref(n), None) == abi.ERR_INVALID
    assert "null argument" in hip.lib().ilqg_last_error().decode()
    # a refusal leaves nothing behind: the scenes the cases above were cut from still build, again and again
    for make in (_two_cars, examples.weighted_proximity_scene, examples.affine_constraint_scene, examples.dynamics_zoo_scene,
                 examples.three_player_collision_avoidance_reachability,
                 lambda: examples.mixed_dubins_car_scene(constrained=True)):
        for _ in range(3):
            rc, msg = _build(hip, make())
            assert rc == abi.OK, msg
    words = (C.c_int32 * 4)()
    assert hip.lib().ilqg_row_program_build(C.byref(desc), words, 4, C.byref(n), None) == abi.ERR_INVALID
    assert "buffer too small" in hip.lib().ilqg_last_error().decode() and n.value > 4
    del keep
