"""One-term problems for every built-in cost and constraint kind, the points they are checked at, and the branch each
point takes.

Every case is built in two shapes: two Car5D players (n = 10, a specialised instantiation) and Car5D + Unicycle4D
(n = 9, the run-time-dimensioned kernels; the second player's position stays at indices (5, 6)).  T = 67 and B = 6: one
full wavefront of rows plus a tail is the smallest horizon at which a row chunk is both full and partial, and every
(instance, step) is a point of its own.

Points, all rounded to fp32 first so that both precisions see the same input:
  instances 0 .. 4   random, uniform in [-3, 3]^n with controls in [-1, 1] (positions of the kinds with rare branches
                     are placed so that the branch occurs, see _place), re-drawn where the branch changes within a
                     relative 1e-3 of the point or the point is within 1e-3 of a singularity;
  instance 5         for the kinds that have them, boundary points: dyadic coordinates exactly on a threshold (the
                     arithmetic is exact, the comparison operator alone decides), and for every constraint the
                     multipliers 0, float32(1e-4) and its two neighbours.

`classify` restates only the DECISIONS of oracle/ilqg_oracle.hpp (EvaluateTerm / QuadraticizeTerm / ConstraintMu), in
the precision asked for; the polyline search itself is the oracle's (polyline_closest_point).  tests/test_term_branches.py
ties it back to the oracle: wherever a flag says "inactive" or "before", the oracle's rows are the base problem's,
and wherever one says "active" they are not.  The other flags — left / right, vertex / interior, end point, wrapped,
which child, mu0 / mu, the on-threshold markers — rest on this restatement alone: they only COUNT points for the
census (a wrong flag miscounts, it cannot make a device comparison pass), and a new kind needs its lines here."""
import functools
import zlib

import numpy as np

from ilqgames_amd import abi
from ilqgames_amd.abi import DYN_CAR_5D, DYN_UNICYCLE_4D, ProblemSpec
from test_oracle_models import COST_BUILDERS, LANE, _cost_spec

T, B = 67, 6
SHAPES = ("car_car", "car_unicycle")
SHORT = [(-2.0, -2.0), (0.5, 1.0), (2.0, 2.0)]   # both end points inside the box: the end point rule is reachable
AXIS = [(-2.0, -1.0), (2.0, -1.0), (2.0, 2.0)]   # axis-aligned and dyadic: every quantity of the search is exact
# two turns of more than 90 degrees: in the outer wedge of such a vertex the sign of the distance is decided by the side
# of the shortcut segment across the vertex, and the line through the vertex along the previous shortcut cuts the wedge
# in two — the one place where taking the wrong one of a segment's two shortcuts shows
HAIRPIN = [(-2.5, -2.0), (-0.5, -1.0), (1.5, 1.5), (-1.0, 2.5), (-2.5, 0.5)]
SMALL32 = np.float32(1e-4)                        # constants::kSmallNumber as the float the code compares with
KIND_NAMES = {getattr(abi, k): k.lower() for k in dir(abi) if k.startswith(("COST_", "CONSTRAINT_"))}
POLYLINE_KINDS = (abi.COST_QUADRATIC_POLYLINE2, abi.COST_SEMIQUADRATIC_POLYLINE2, abi.COST_POLYLINE2_SIGNED_DISTANCE,
                  abi.CONSTRAINT_POLYLINE2_SIGNED_DISTANCE)
PAIR_KINDS = (abi.COST_PROXIMITY, abi.COST_SIGNED_DISTANCE, abi.CONSTRAINT_PROXIMITY, abi.COST_RELATIVE_DISTANCE,
              abi.COST_LOCALLY_CONVEX_PROXIMITY, abi.COST_WEIGHTED_CONVEX_PROXIMITY)
CONVEX_KINDS = (abi.COST_LOCALLY_CONVEX_PROXIMITY, abi.COST_WEIGHTED_CONVEX_PROXIMITY)


GAME_FINAL_TIME = {"final_time_mid_chunk": 1.05, "final_time_last_step": 2.25}   # first active steps 11 and 23 = T - 1


def _final_time(threshold, s):
    return s.final_time(threshold, s.proximity(0, 4.0, (0, 1), (5, 6), 3.0))


def _shared_search(s):
    # two terms on one polyline and position pair (one closest-point search serves both) next to one on another polyline
    lane = s.add_polyline(LANE)
    s.quadratic_polyline2(0, 1.0, lane, (0, 1))
    s.semiquadratic_polyline2(0, 2.0, lane, (0, 1), 0.5, True)
    s.polyline2_signed_distance(0, s.add_polyline(SHORT), (0, 1), 0.5, True)


def _extreme_min(s):
    s.extreme_value(0, [lambda role: s.signed_distance(0, (0, 1), (5, 6), 2.0, True, role=role),
                        lambda role: s.signed_distance(0, (2, 3), (7, 8), 1.0, True, role=role)], is_min=True)


EXTRA_BUILDERS = {
    "signed_distance_flipped": lambda s: s.signed_distance(0, (0, 1), (5, 6), 2.0, False),
    "proximity_constraint_within": lambda s: s.proximity_constraint(0, (0, 1), (5, 6), 3.0, True),
    "single_dimension_constraint_above": lambda s: s.single_dimension_constraint(0, 4, 0.25, False),
    # threshold 0: g is the coordinate itself, so g == float32(1e-4) exactly is a point
    "single_dimension_constraint_zero": lambda s: s.single_dimension_constraint(0, 4, 0.0, True),
    # (the threshold of 10 m above keeps g negative everywhere in the box: this one has both signs)
    "polyline2_signed_distance_constraint_left": lambda s: s.polyline2_signed_distance_constraint(
        0, s.add_polyline(LANE), (0, 1), 0.5, True),
    "polyline2_signed_distance_hairpin": lambda s: s.polyline2_signed_distance(0, s.add_polyline(HAIRPIN), (0, 1), 0.25, True),
    "polyline2_signed_distance_constraint_hairpin": lambda s: s.polyline2_signed_distance_constraint(
        0, s.add_polyline(HAIRPIN), (0, 1), 0.5, True),
    # on the axis-aligned polyline the distance is a coordinate difference: g can be put next to float32(1e-4)
    "polyline2_signed_distance_constraint_axis": lambda s: s.polyline2_signed_distance_constraint(
        0, s.add_polyline(AXIS), (0, 1), 0.5, True),
    "polyline2_signed_distance_constraint_axis_right": lambda s: s.polyline2_signed_distance_constraint(
        0, s.add_polyline(AXIS), (0, 1), -0.5, False),
    "polyline2_signed_distance_constraint_short_right": lambda s: s.polyline2_signed_distance_constraint(
        0, s.add_polyline(SHORT), (0, 1), -0.5, False),
    "semiquadratic_control_right": lambda s: s.semiquadratic(0, 5.0, 1, 0.1, True, control_of=0),
    "semiquadratic_control_left": lambda s: s.semiquadratic(0, 5.0, 0, -0.25, False, control_of=0),
    "semiquadratic_norm_control_r": lambda s: s.semiquadratic_norm(0, 1.0, (0, 1), 0.5, True, control_of=0),
    "semiquadratic_norm_control_l": lambda s: s.semiquadratic_norm(0, 2.0, (0, 1), 0.75, False, control_of=0),
    "extreme_value_min": _extreme_min,
    "orientation_negative_nominal": lambda s: s.orientation(0, 2.0, 2, -np.pi / 2),
    "quadratic_polyline2_short": lambda s: s.quadratic_polyline2(0, 1.0, s.add_polyline(SHORT), (0, 1)),
    "quadratic_polyline2_axis": lambda s: s.quadratic_polyline2(0, 1.0, s.add_polyline(AXIS), (0, 1)),
    "semiquadratic_polyline2_short": lambda s: s.semiquadratic_polyline2(0, 1.0, s.add_polyline(SHORT), (0, 1), 0.5, True),
    "semiquadratic_polyline2_axis_r": lambda s: s.semiquadratic_polyline2(0, 1.0, s.add_polyline(AXIS), (0, 1), 0.5, True),
    "semiquadratic_polyline2_axis_l": lambda s: s.semiquadratic_polyline2(0, 1.0, s.add_polyline(AXIS), (0, 1), -0.5,
                                                                           False),
    "final_time_step0": functools.partial(_final_time, 0.0),
    "final_time_mid_chunk": functools.partial(_final_time, 3.65),   # first active step 37, inside the first row chunk
    "final_time_last_step": functools.partial(_final_time, 6.55),   # first active step 66 = T - 1
    "shared_polyline_search": _shared_search,
}
DENSE = ("affine_scalar_constraint", "affine_vector_constraint", "affine_scalar_constraint_equality")


def _weighted(shape):
    v2 = 9 if shape == "car_car" else 8   # the second player's speed
    return lambda s: s.weighted_convex_proximity(0, 2.0, (0, 1), (5, 6), 4, v2, 3.0)


def case_names(shape):
    names = [k for k in COST_BUILDERS if shape == "car_car" or k not in DENSE]   # the dense kinds: test_gpu_affine.py
    return names + list(EXTRA_BUILDERS) + ["weighted_convex_proximity"]


def builder(name, shape, game=False):
    if name == "weighted_convex_proximity":
        return _weighted(shape)
    if game and name in GAME_FINAL_TIME:   # the same three places of the gate in the games' shorter horizon
        return functools.partial(_final_time, GAME_FINAL_TIME[name])
    return COST_BUILDERS.get(name) or EXTRA_BUILDERS[name]


def make_spec(name, shape, horizon=T):
    """The one-term problem: unit quadratic control costs (the base problem) plus the case's term(s) on player 0."""
    build = builder(name, shape) if name is not None else (lambda s: None)
    if shape == "car_car":
        s = _cost_spec(build)
    else:
        s = ProblemSpec(T=horizon)
        s.add_player(DYN_CAR_5D, 4.0, state_reg=0.0, control_reg=0.0)
        s.add_player(DYN_UNICYCLE_4D)
        s.quadratic(0, 1.0, 0, 0.0, control_of=0)
        s.quadratic(1, 1.0, 0, 0.0, control_of=1)
        build(s)
        s.x0 = np.zeros(s.n)
    s.T = horizon
    return s


def case_terms(spec):
    """Indices of the terms the case added: player 0's, after the two control costs that come first; children excluded."""
    return [ti for ti in range(2, len(spec.terms))
            if spec.terms[ti]["role"] != abi.ROLE_CHILD and spec.terms[ti]["player"] == 0]


# ---------------------------------------------------------------------------------------------------------------------
# the branch a point takes
# ---------------------------------------------------------------------------------------------------------------------
def _sgn(F, x):
    return F(int(F(0) < x) - int(x < F(0)))


def _mu_flags(F, g, lam):
    small = F(SMALL32)
    lam = F(lam)
    out = ["mu0" if (g <= small and abs(lam) <= small) else "mu"]
    if g == small:
        out.append("g_on_threshold")
    elif F(0) < g < small:
        out.append("g_just_below_threshold")
    elif small < g <= F(4) * small:
        out.append("g_just_above_threshold")
    if np.float32(lam) == SMALL32:
        out.append("lambda_on_threshold")
    return out


def _leaf_flags(pyoracle, spec, t, F, dtype, v, lam):
    kind = t["kind"]
    val = F(np.float32(t["value"]))
    oriented = bool(t["flags"] & abi.FLAG_ORIENTED)
    i = t["idx"]
    if kind == abi.COST_SEMIQUADRATIC:
        d = v[i[0]] - val
        if d == 0:
            return ["on_threshold"]   # the value is 0, the Hessian already carries the weight (semiquadratic_cost.cpp:63-85)
        return ["active" if (d > 0) == oriented else "inactive"]
    if kind == abi.COST_SEMIQUADRATIC_NORM:
        norm = np.hypot(v[i[0]], v[i[1]])
        if norm == val:
            return ["on_threshold"]
        return ["active" if (norm > val) == oriented else "inactive"]
    if kind == abi.COST_ORIENTATION:
        a = float(v[i[0]] - val) + np.pi
        return ["negative_remainder" if a < 0 else "wrapped" if a >= 2 * np.pi else "plain"]
    if kind in PAIR_KINDS:
        dx, dy = v[i[0]] - v[i[2]], v[i[1]] - v[i[3]]
        if kind == abi.COST_PROXIMITY:
            dsq, vsq = dx * dx + dy * dy, val * val
            return ["on_threshold", "inactive"] if dsq == vsq else ["inactive" if dsq > vsq else "active"]
        if kind in CONVEX_KINDS:
            vsq = val * val
            if dx * dx >= vsq or dy * dy >= vsq:
                return ["outside"] + (["on_threshold"] if dx * dx == vsq or dy * dy == vsq else [])
            ax, ay = val - abs(dx), val - abs(dy)
            sx, sy = ax * ax, ay * ay
            d = dx if sx < sy else dy
            return ["x_active" if sx < sy else "y_active", "difference_positive" if d > 0 else "difference_not_positive"] + \
                (["tie"] if sx == sy else [])
        if kind == abi.CONSTRAINT_PROXIMITY:
            g = np.hypot(dx, dy) - val
            return _mu_flags(F, g if oriented else -g, lam)
        return ["all"]
    if kind == abi.CONSTRAINT_SINGLE_DIMENSION:
        return _mu_flags(F, v[i[0]] - val if oriented else val - v[i[0]], lam)
    if kind in POLYLINE_KINDS:
        r = pyoracle.polyline_closest_point(spec.polylines[t["polyline"]], (float(v[i[0]]), float(v[i[1]])), dtype)
        ssd = F(r["ssd"])
        where = "vertex" if r["is_vertex"] else "interior"
        if kind == abi.COST_QUADRATIC_POLYLINE2:
            return ["end_point"] if r["is_endpoint"] else [where]
        if kind == abi.COST_SEMIQUADRATIC_POLYLINE2:
            sst = _sgn(F, val) * val * val
            if not ((ssd > sst and oriented) or (ssd < sst and not oriented)):
                return ["inactive"] + (["on_threshold"] if ssd == sst else [])
            return ["end_point"] if r["is_endpoint"] else ["active_" + where]
        side = "right" if ssd > 0 else "left"
        if kind == abi.COST_POLYLINE2_SIGNED_DISTANCE:
            return [side, where]
        sd = _sgn(F, ssd) * np.sqrt(abs(ssd))
        return [side, where, side + "_" + where] + _mu_flags(F, sd - val if oriented else val - sd, lam)
    if kind in (abi.CONSTRAINT_AFFINE_SCALAR, abi.CONSTRAINT_AFFINE_VECTOR):
        return ["all"]   # drawn with multipliers above the threshold: the gate is test_gpu_affine.py's
    return ["all"]


def _signed_distance_value(F, t, v):
    i = t["idx"]
    cost = F(np.float32(t["value"])) - np.hypot(v[i[0]] - v[i[2]], v[i[1]] - v[i[3]])
    return cost if t["flags"] & abi.FLAG_ORIENTED else -cost


def lambda_slot_step(spec, k):
    """RelativeTimeTracker::TimeIndex truncates (k * dt) / dt in double: the multiplier slot step k reads."""
    return int((k * spec.dt) / spec.dt)


def _argument(spec, t, x, u):
    """The vector the term is a function of: the state, or the control of player `arg`."""
    if t["role"] not in (abi.ROLE_CONTROL_COST, abi.ROLE_CONTROL_CONSTRAINT):
        return x
    off = sum(spec.udims[:t["arg"]])
    return u[off:off + spec.udims[t["arg"]]]


def classify(pyoracle, spec, dtype, x, u, lam, k):
    """Flags "<kind>[.control][.oriented|.unoriented].<branch>" of the point (x, u, lam[slot]) at step k."""
    F = np.float32 if dtype == abi.F32 else np.float64
    x, u = np.asarray(x, F), np.asarray(u, F)
    out = []
    for ti in case_terms(spec):
        t = spec.terms[ti]
        control = t["role"] in (abi.ROLE_CONTROL_COST, abi.ROLE_CONTROL_CONSTRAINT)
        v = _argument(spec, t, x, u)
        prefix = KIND_NAMES[t["kind"]] + (".control" if control else "")
        if t["first_step"] > 0:
            out.append("final_time." + ("before" if k < t["first_step"] else "after"))
            if k < t["first_step"]:
                continue
        if t["kind"] == abi.COST_EXTREME_VALUE:
            is_min = bool(t["flags"] & abi.FLAG_IS_MIN)
            kids = [spec.terms[q] for q in range(t["child_begin"], t["child_begin"] + t["child_count"])]
            values = [_signed_distance_value(F, c, v) for c in kids]
            best = int(np.argmin(values) if is_min else np.argmax(values))
            out.append("%s.%s.child%d" % (prefix, "min" if is_min else "max", best))
            continue
        has_orientation = t["kind"] in (abi.COST_SEMIQUADRATIC, abi.COST_SEMIQUADRATIC_NORM, abi.COST_SIGNED_DISTANCE,
                                        abi.COST_SEMIQUADRATIC_POLYLINE2, abi.COST_POLYLINE2_SIGNED_DISTANCE,
                                        abi.CONSTRAINT_PROXIMITY, abi.CONSTRAINT_SINGLE_DIMENSION,
                                        abi.CONSTRAINT_POLYLINE2_SIGNED_DISTANCE)
        if has_orientation:
            prefix += ".oriented" if t["flags"] & abi.FLAG_ORIENTED else ".unoriented"
        slot = t["constraint_slot"]
        lam_k = lam[slot, lambda_slot_step(spec, k)] if slot >= 0 else 0.0
        out += [prefix + "." + f for f in _leaf_flags(pyoracle, spec, t, F, dtype, v, lam_k)]
    return tuple(out)


def _regular(pyoracle, spec, x, u):
    """Not within 1e-3 (relative to the box) of a singularity: distance 0, a norm of 0, v = 0 in CurvatureCost."""
    near = 3e-3
    for ti in range(2, len(spec.terms)):
        t = spec.terms[ti]
        if t["player"] != 0:
            continue
        v = _argument(spec, t, x, u)
        i = t["idx"]
        if t["kind"] in PAIR_KINDS and np.hypot(v[i[0]] - v[i[2]], v[i[1]] - v[i[3]]) < near:
            return False
        if t["kind"] in (abi.COST_QUADRATIC_NORM, abi.COST_SEMIQUADRATIC_NORM) and np.hypot(v[i[0]], v[i[1]]) < near:
            return False
        if t["kind"] == abi.COST_CURVATURE and abs(v[i[1]]) < near:
            return False
        if t["kind"] in POLYLINE_KINDS:
            r = pyoracle.polyline_closest_point(spec.polylines[t["polyline"]], (float(v[i[0]]), float(v[i[1]])), abi.F64)
            if abs(r["ssd"]) < near * near:
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the points
# ---------------------------------------------------------------------------------------------------------------------
def _place(spec, rng, x):
    """Moves a random point to where the case's rare branches are: around the vertices of its polylines (the vertex
    wedges of a gently bending lane are narrow) and inside / around the square of the convex proximities."""
    for ti in range(2, len(spec.terms)):
        t = spec.terms[ti]
        i = t["idx"]
        if t["kind"] in POLYLINE_KINDS and rng.random() < 0.5:
            pts = spec.polylines[t["polyline"]]
            inside = [p for p in pts if abs(p[0]) <= 3 and abs(p[1]) <= 3]
            vx, vy = inside[rng.integers(len(inside))]
            a, r = rng.uniform(0, 2 * np.pi), rng.uniform(0.1, 1.5)
            x[i[0]], x[i[1]] = vx + r * np.cos(a), vy + r * np.sin(a)
        if t["kind"] in CONVEX_KINDS:
            x[i[2]], x[i[3]] = x[i[0]] - rng.uniform(-3.5, 3.5), x[i[1]] - rng.uniform(-3.5, 3.5)
    return x


def _dyadic(rng, lo, hi, size):
    return rng.integers(int(lo * 8), int(hi * 8) + 1, size=size) / 8.0


def _boundary(spec, rng):
    """-> list of (x, u) exactly on / next to the thresholds of the case's last term; empty where the kind has none.
    The coordinates are dyadic (or a float32 neighbour of a threshold), so every operation up to the comparison is
    exact and what follows is at most single correctly rounded operations both sides perform alike: these points are
    judged without a conditioning allowance (`exact`).  That holds for SingleDimensionConstraint (g = x - value is one
    exact subtraction) and for ProximityConstraint too (the points have dy = 0, so hypot is |dx| and g one exact
    subtraction).  Only the polyline constraint's points keep the allowance: there g passes through
    sgn(ssd) sqrt(|ssd|) of a squared cross product, which is rounded twice before the subtraction cancels."""
    t = spec.terms[-1]
    kind, i, val = t["kind"], t["idx"], np.float32(t["value"])
    control = t["role"] == abi.ROLE_CONTROL_COST
    pts = []

    def base():
        return _dyadic(rng, -3, 3, spec.n), _dyadic(rng, -1, 1, spec.m)

    def put(setter):
        x, u = base()
        setter(u if control else x)
        pts.append((x, u))
    if kind == abi.COST_SEMIQUADRATIC:
        for v in (val, np.nextafter(val, np.float32(9)), np.nextafter(val, np.float32(-9))) * 8:
            put(lambda a, v=v: a.__setitem__(i[0], v))
    elif kind == abi.COST_PROXIMITY or kind in CONVEX_KINDS:
        thr = float(val)
        convex = kind in CONVEX_KINDS
        offsets = [(thr, 0.0), (0.0, thr), (-thr, 0.0), (0.0, -thr), (thr - 0.125, 0.0), (thr + 0.125, 0.0),
                   (0.0, -thr + 0.125), (0.0, -thr - 0.125)]
        if convex:   # on one axis' threshold with the other inside; ties of the two axes, every sign pattern
            offsets += [(thr, 1.5), (-thr, -0.75), (2.25, thr), (-1.125, -thr), (1.5, 1.5), (-1.5, 1.5), (1.5, -1.5),
                        (-1.5, -1.5), (2.5, 2.5), (-0.25, 0.25), (0.75, -0.75), (-2.0, -2.0)]
        for dx, dy in offsets * 3:
            def setter(a, dx=dx, dy=dy):
                a[i[2]], a[i[3]] = _dyadic(rng, -1, 1, 2) * 0.5
                a[i[0]], a[i[1]] = a[i[2]] + dx, a[i[3]] + dy
            put(setter)
    elif kind in (abi.CONSTRAINT_SINGLE_DIMENSION, abi.CONSTRAINT_PROXIMITY):
        # g on both sides of float32(1e-4), and well inside; with the four edge multipliers these cycle through all pairs
        sign = 1.0 if t["flags"] & abi.FLAG_ORIENTED else -1.0
        on = [SMALL32, np.nextafter(SMALL32, np.float32(0)), np.nextafter(SMALL32, np.float32(1))]
        for g in ([float(v) for v in on] * 3 + [-0.5] if val == 0 else (0.5e-4, 2e-4, -0.5)):
            if kind == abi.CONSTRAINT_SINGLE_DIMENSION:
                put(lambda a, g=g: a.__setitem__(i[0], np.float32(float(val) + sign * g)))
            else:
                def setter(a, g=g):
                    a[i[2]], a[i[3]] = _dyadic(rng, -1, 1, 2) * 0.5
                    a[i[0]], a[i[1]] = np.float32(a[i[2]] + float(val) + sign * g), a[i[3]]
                put(setter)
    elif kind == abi.CONSTRAINT_POLYLINE2_SIGNED_DISTANCE and spec.polylines[t["polyline"]] == AXIS:
        # g = +-(sd - threshold) with sd = +-(distance to the first segment y = -1, or to the last one x = 2):
        # g just below and just above float32(1e-4), and well inside, to the side where |threshold| is a distance
        side = 1.0 if t["flags"] & abi.FLAG_ORIENTED else -1.0   # +1: right of the polyline (below y = -1, beyond x = 2)
        for g in (0.5e-4, 2e-4, -0.25):
            d = np.float32(abs(float(val)) + g)
            x, u = base()
            x[i[0]], x[i[1]] = _dyadic(rng, -1, 1, 1)[0], np.float32(-1.0 - side * d)
            pts.append((x, u))
            x, u = base()
            x[i[0]], x[i[1]] = np.float32(2.0 + side * d), _dyadic(rng, 0, 1, 1)[0]
            pts.append((x, u))
    elif kind in (abi.COST_QUADRATIC_POLYLINE2, abi.COST_SEMIQUADRATIC_POLYLINE2) and \
            spec.polylines[t["polyline"]] == AXIS:
        # the 1e-4 end point rule: the closest point lies `along` from the first / last vertex on its segment.
        # 2^-7 and 2^-6 are on its two sides with exact squares; float32(0.01) and its neighbours straddle it.
        c = np.float32(0.01)
        alongs = [2.0 ** -7, 2.0 ** -6, float(c), float(np.nextafter(c, np.float32(0))), float(np.nextafter(c, np.float32(1)))]
        right = kind == abi.COST_QUADRATIC_POLYLINE2 or bool(t["flags"] & abi.FLAG_ORIENTED)
        off = 1.0 if right else -1.0   # to the right of the first segment is below it, of the last segment beyond x = 2
        for a_ in alongs * 2:
            x, u = base()
            x[i[0]], x[i[1]] = np.float32(-2.0 + a_), -1.0 - off
            pts.append((x, u))
            x, u = base()
            x[i[0]], x[i[1]] = 2.0 + off, np.float32(2.0 - a_)
            pts.append((x, u))
        if kind == abi.COST_SEMIQUADRATIC_POLYLINE2:   # ssd == sst, and a dyadic step to either side
            thr = abs(float(val))
            for d in (thr, thr + 0.125, thr - 0.125) * 6:
                x, u = base()
                x[i[0]], x[i[1]] = _dyadic(rng, -1, 1, 1)[0], -1.0 - off * d
                pts.append((x, u))
                x, u = base()
                x[i[0]], x[i[1]] = 2.0 + off * d, _dyadic(rng, 0, 1, 1)[0]
                pts.append((x, u))
    return pts


@functools.lru_cache(maxsize=None)
def case_points(name, shape):
    """-> dict(spec, xs [B][T][n], us [B][T][m], lam [B][nc][T] or None, mu [B] or None, te [B][N], exact [B][T] bool)
    in float64 holding float32 values.  Deterministic: a function of (name, shape) alone."""
    from oracle import pyoracle
    spec = make_spec(name, shape)
    n, m, nc = spec.n, spec.m, spec.num_constraints
    seed = zlib.crc32((name + ":" + shape).encode())
    rng = np.random.default_rng(seed)
    xs, us = np.zeros((B, T, n)), np.zeros((B, T, m))
    lam = np.zeros((B, nc, T)) if nc else None
    if nc:
        gate = name not in DENSE
        positive = rng.uniform(0.05, 2.0, (B, nc, T))
        lam[:] = np.where(rng.random((B, nc, T)) < (0.5 if gate else 0.0), 0.0, positive).astype(np.float32)
        edge = [0.0, float(SMALL32), float(np.nextafter(SMALL32, np.float32(0))), float(np.nextafter(SMALL32, np.float32(1)))]
        if gate:
            lam[B - 1] = np.resize(np.array(edge), T)[None, :]
    boundary = _boundary(spec, rng)
    exact = np.zeros((B, T), bool)

    def stable(x, u, b, k):
        if not _regular(pyoracle, spec, x, u):
            return False
        want = classify(pyoracle, spec, abi.F64, x, u, lam[b] if nc else None, k)
        if classify(pyoracle, spec, abi.F32, x, u, lam[b] if nc else None, k) != want:
            return False
        for _ in range(4):   # 1e-3 of the box's half-width, every coordinate, random signs
            xn = (x + 3e-3 * rng.choice((-1.0, 1.0), n)).astype(np.float32)
            un = (u + 1e-3 * rng.choice((-1.0, 1.0), m)).astype(np.float32)
            if classify(pyoracle, spec, abi.F64, xn, un, lam[b] if nc else None, k) != want:
                return False
        return True
    for b in range(B):
        for k in range(T):
            if b == B - 1 and boundary:
                x, u = boundary[k % len(boundary)]
                xs[b, k], us[b, k] = np.float32(x), np.float32(u)
                exact[b, k] = spec.terms[-1]["kind"] != abi.CONSTRAINT_POLYLINE2_SIGNED_DISTANCE
                continue
            for _ in range(200):
                x = _place(spec, rng, rng.uniform(-3, 3, n)).astype(np.float32)
                u = rng.uniform(-1, 1, m).astype(np.float32)
                if stable(x, u, b, k):
                    break
            else:
                raise AssertionError("no regular point for %s" % name)
            xs[b, k], us[b, k] = x, u
    mu = np.array([10.0, 11.0, 12.5, 5.0, 10.0, 10.0]) if nc else None
    te = rng.integers(0, T, size=(B, len(spec.subsystems))).astype(np.int32)
    return dict(spec=spec, xs=xs, us=us, lam=lam, mu=mu, te=te, exact=exact)


def case_classes(name, shape, dtype):
    """[B][T] object array of the flag tuples of every point in the oracle's `dtype` arithmetic."""
    from oracle import pyoracle
    p = case_points(name, shape)
    out = np.empty((B, T), object)
    for b in range(B):
        for k in range(T):
            out[b, k] = classify(pyoracle, p["spec"], dtype, p["xs"][b, k], p["us"][b, k],
                                 None if p["lam"] is None else p["lam"][b], k)
    return out


@functools.lru_cache(maxsize=None)
def case_census(name, shape):
    """-> dict(points, differ, flags {flag: count over the points both precisions classify alike}), agree [B][T]."""
    c64, c32 = case_classes(name, shape, abi.F64), case_classes(name, shape, abi.F32)
    agree = np.array([[c64[b, k] == c32[b, k] for k in range(T)] for b in range(B)])
    flags = {}
    for b in range(B):
        for k in range(T):
            if agree[b, k]:
                for f in c64[b, k]:
                    flags[f] = flags.get(f, 0) + 1
    return dict(points=B * T, differ=int((~agree).sum()), flags=dict(sorted(flags.items()))), agree


# ---------------------------------------------------------------------------------------------------------------------
# the same cases inside a solve: one forced-step iteration from the zero warm start
# ---------------------------------------------------------------------------------------------------------------------
GAME_T, GAME_B = 24, 8
# not wrapped in a game: the dense kinds (test_gpu_affine.py), and the control-vector cases — the controls of the zero
# warm start are zero, so their rows see one branch only (and SemiquadraticNormCost is singular at u = 0)
GAME_SKIP = DENSE + ("semiquadratic_control_right", "semiquadratic_control_left", "semiquadratic_norm_control_r",
                     "semiquadratic_norm_control_l")
BOUNDARY_FLAGS = (".on_threshold", ".tie", ".lambda_on_threshold", ".g_on_threshold", ".g_just_below_threshold",
                  ".g_just_above_threshold")


def game_names(shape):
    return [k for k in case_names(shape) if k not in GAME_SKIP]


def game_spec(name, shape):
    """The case's term on player 0 inside a well-posed game: a unit quadratic cost on every control of both players and
    a weight-0.1 quadratic on every state of player 2."""
    s = ProblemSpec(T=GAME_T)
    s.add_player(DYN_CAR_5D, 4.0)
    s.add_player(DYN_CAR_5D if shape == "car_car" else DYN_UNICYCLE_4D, 4.0)
    s.quadratic(0, 1.0, -1, 0.0, control_of=0)
    s.quadratic(1, 1.0, -1, 0.0, control_of=1)
    builder(name, shape, game=True)(s)
    for d in range(5, s.n):
        s.quadratic(1, 0.1, d, 0.0)
    s.x0 = np.zeros(s.n)
    return s


def _game_draw(spec, shape, rng):
    x0 = np.zeros((GAME_B, spec.n))
    for off, car in ((0, True), (5, shape == "car_car")):
        x0[:, off:off + 2] = rng.uniform(-3, 3, (GAME_B, 2))
        x0[:, off + 2] = rng.uniform(-np.pi, np.pi, GAME_B)
        if car:
            x0[:, off + 3] = rng.uniform(-0.3, 0.3, GAME_B)
        speed = rng.uniform(-1.5, 6.0, GAME_B)   # a few reversing: the speed constraints then see both signs of g
        x0[:, off + (4 if car else 3)] = np.where(np.abs(speed) < 0.3, 2.0, speed)
    x0 = x0.astype(np.float32).astype(np.float64)
    steps = rng.choice([0.5, 0.25, 0.125], size=(GAME_B, 1))
    return dict(spec=spec, x0=x0, steps=steps, x0_nudged=x0 + 1e-12 * rng.standard_normal(x0.shape))


def _game_coasting(pyoracle, g):
    spec = g["spec"]
    z = lambda *shape_: np.zeros(shape_)  # noqa: E731
    return pyoracle.OracleProblem(spec).rollout(abi.F64, g["x0"], z(GAME_B, GAME_T, spec.n), z(GAME_B, GAME_T, spec.m),
                                                z(GAME_B, GAME_T, spec.m * spec.n), z(GAME_B, GAME_T, spec.m))


def _game_classes(pyoracle, g):
    xs, us = _game_coasting(pyoracle, g)
    lam = np.zeros((max(g["spec"].num_constraints, 1), GAME_T))
    return [[classify(pyoracle, g["spec"], abi.F64, xs[b, k], us[b, k], lam, k) for b in range(GAME_B)]
            for k in range(GAME_T)]


def game_mask(pyoracle, g, dtype):
    """conditioning() of test_gpu_forced.py after the one iteration: which instances the oracle itself resolves."""
    from test_gpu_forced import conditioning
    op = pyoracle.OracleProblem(g["spec"])
    ref = op.solve(dtype, g["x0"], fixed_iters=1, forced_steps=g["steps"], merit_log_len=1)
    return conditioning(op, g["x0"], g["x0_nudged"], g["steps"], 1, dtype, ref, GAME_B)[0], ref


def game_draw(name, shape, draw):
    """Draw number `draw` of the game's seeded sequence, as game_inputs returns it: no selection, no oracle run."""
    g = _game_draw(game_spec(name, shape), shape,
                   np.random.default_rng([zlib.crc32(("game:" + name + ":" + shape).encode()), draw]))
    g["draw"] = draw
    return g


@functools.lru_cache(maxsize=None)
def game_inputs(name, shape):
    """-> dict(spec, x0 [B][n], steps [B][1], x0_nudged, draw): position in [-3, 3]^2, any heading, speed up to 6 m/s, a
    little steering — the operating point of the first iteration is the coasting line from x0, which crosses the
    thresholds of the case at a step that differs from instance to instance.  Out of a seeded sequence of draws the
    one is taken on which the rarest branch of the case has the most points (12 are enough) among those on which the
    oracle resolves every instance in both precisions (the conditioning mask is full), every instance ends with
    status 1, and — where the case has more than one branch — two lanes differ in branch at some step."""
    from oracle import pyoracle
    spec = game_spec(name, shape)
    wanted = [f for f in case_census(name, shape)[0]["flags"] if not f.endswith(BOUNDARY_FLAGS)]
    if name in GAME_FINAL_TIME:
        wanted += ["final_time.after"]
    candidates = []

    def resolved(g):
        return all(game_mask(pyoracle, g, d)[0].all() and np.all(game_mask(pyoracle, g, d)[1]["status"] == 1)
                   for d in (abi.F64, abi.F32))
    for draw in range(24):   # the draws in which every branch of the case has the most points come first
        rng = np.random.default_rng([zlib.crc32(("game:" + name + ":" + shape).encode()), draw])
        g = _game_draw(spec, shape, rng)
        classes = _game_classes(pyoracle, g)
        if len(wanted) > 1 and not any(len(set(row)) > 1 for row in classes):
            continue
        count = {f: 0 for f in wanted}
        for row in classes:
            for c in row:
                for f in c:
                    count[f] = count.get(f, 0) + 1
        fewest = min(12, min(count.values()))
        if fewest == 12 and resolved(g):
            g["draw"] = draw
            return g
        if fewest < 12:
            candidates.append((-fewest, draw, g))
    for _, draw, g in sorted(candidates, key=lambda c: c[:2]):
        if resolved(g):
            g["draw"] = draw
            return g
    raise AssertionError("no well-conditioned draw for the game of %s %s" % (name, shape))


@functools.lru_cache(maxsize=None)
def game_census(name, shape):
    """Branches along the coasting lines (the fp64 oracle's rollout of the zero strategy), multipliers 0:
    -> dict(points, flags {flag: count}, lanes_differ: steps at which two instances sit in different branches)."""
    from oracle import pyoracle
    g = game_inputs(name, shape)
    flags, differ = {}, 0
    for classes in _game_classes(pyoracle, g):
        differ += len(set(classes)) > 1
        for c in classes:
            for f in c:
                flags[f] = flags.get(f, 0) + 1
    return dict(points=GAME_B * GAME_T, draw=g["draw"], flags=dict(sorted(flags.items())), lanes_differ=differ)
