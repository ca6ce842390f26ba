"""Per-instance time nominals, the checks that need no GPU: the prototypes of the C header and their agreement with
hip.EXPORTS, the host-only table (ilqg_time_nominal_table_build) against a numpy restatement in the same arithmetic
(exact), the one tabulating function the host builder and the device kernel share, called from a sanitised stand-alone
program, and the refusals that need no device.  Also the scenes and reference vectors the GPU tests
(tests/test_gpu_instance_time_nominals.py) share."""
import copy
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from ilqgames_amd import abi, examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_KINDS = (abi.COST_NOMINAL_PATH_LENGTH, abi.COST_ROUTE_PROGRESS)
CALLS = ("ilqg_problem_bind_instance_time_nominals", "ilqg_instance_time_nominals_build",
         "ilqg_problem_time_nominal_terms", "ilqg_time_nominal_table_build")


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return h


# ---- scenes and reference vectors (shared with the GPU tests) ----
def time_terms(spec):
    """Indices of the spec's time-dependent terms: table q belongs to the q-th of them."""
    return [ti for ti, t in enumerate(spec.terms) if t["kind"] in TIME_KINDS]


def with_references(spec, vec):
    """The spec with row q of vec = (nominal speed, initial route position) written into its q-th time-dependent term."""
    s = copy.deepcopy(spec)
    terms = time_terms(s)
    assert len(terms) == len(vec)
    for ti, (speed, pos0) in zip(terms, vec):
        s.terms[ti]["value"] = float(np.float32(speed))
        if s.terms[ti]["kind"] == abi.COST_ROUTE_PROGRESS:
            s.terms[ti]["value2"] = float(np.float32(pos0))
    return s


def zoo20():
    """dynamics_zoo_scene at T = 20: (17, 3, 2), tables = [path length of player 2 | route on lane 1 | route on lane 2]."""
    s = examples.dynamics_zoo_scene(T=20)
    s.params.max_solver_iters = 12
    return s


# lane 1 is one segment of 2000 m; lane 2 has corners at route positions 995 and 995 + sqrt(50) and ends at ~1997.07
ZOO_VECTORS = np.array([
    [[5.0, 0.0], [6.0, 970.0], [4.0, 968.0]],       # the scene's own
    [[3.5, 0.0], [4.5, 972.5], [5.0, 994.25]],      # lane 2's first corner is passed at step 2, the second at step 17
    [[6.5, 0.0], [7.0, 1999.0], [3.0, 1996.5]],     # both routes run off their polyline's end
    [[4.25, 0.0], [5.5, 965.0], [6.0, 960.75]],
], dtype=np.float32)


def two_car_scene(T=20, dt=0.1, constrained=False):
    """Two Car5D (n = 10, N = 2, m_i = 2) on a lane with a corner: a route-progress term per player and a nominal path
    length on player 2's x position — the smallest specialised scene with all three kinds of table."""
    prm = abi.SolverParams.default()
    prm.max_backtracking_steps = 100
    prm.initial_alpha_scaling = 0.1
    prm.convergence_tolerance = 0.01
    prm.expected_decrease_fraction = 0.001
    prm.max_solver_iters = 12
    prm.unconstrained_solver_max_iters = 4
    s = abi.ProblemSpec(T, dt, prm)
    for _ in range(2):
        s.add_player(abi.DYN_CAR_5D, 4.0)
    X, Y, H, PHI, V = [0, 5], [1, 6], [2, 7], [3, 8], [4, 9]
    lane = s.add_polyline([(-20.0, 0.0), (0.0, 0.0), (6.0, 2.5), (14.0, 2.5)])
    other = s.add_polyline([(-20.0, -3.0), (20.0, -3.0)])
    for i in range(2):
        s.quadratic(i, 25.0, 0, 0.0, control_of=i)
        s.quadratic(i, 15.0, 1, 0.0, control_of=i)
        s.quadratic(i, 4.0, V[i], 5.0)
        s.semiquadratic(i, 50.0, PHI[i], 0.4, True)
    s.route_progress(0, 3.0, 5.0, lane, (X[0], Y[0]), 10.0)
    s.nominal_path_length(1, 1.5, X[1], 4.0)        # on a position dimension: x tracks 4 m/s * t
    s.route_progress(1, 2.0, 4.0, lane, (X[1], Y[1]), 2.0)
    s.quadratic_polyline2(1, 5.0, other, (X[1], Y[1]))
    s.proximity(0, 50.0, (X[0], Y[0]), (X[1], Y[1]), 3.0)
    s.proximity(1, 50.0, (X[1], Y[1]), (X[0], Y[0]), 3.0)
    if constrained:
        s.single_dimension_constraint(0, V[0], 5.5, True)
        s.proximity_constraint(1, (X[1], Y[1]), (X[0], Y[0]), 2.0, False)
    s.x0 = [-10.0, 0.3, 0.0, 0.0, 4.0, -18.0, -0.4, 0.0, 0.0, 3.0]
    s.position_dims, s.heading_dims, s.speed_dims = list(zip(X, Y)), H, V
    return s


# the lane: 20 m, then sqrt(42.25) = 6.5 m, then 8 m: corners at route positions 20 and 26.5, the end at 34.5
TWO_CAR_VECTORS = np.array([
    [[5.0, 10.0], [4.0, 0.0], [4.0, 2.0]],          # the scene's own
    [[6.0, 17.5], [2.5, 0.0], [7.0, 14.25]],        # both routes pass the first corner, player 1's the second too
    [[3.0, 31.0], [6.0, 0.0], [5.5, 26.0]],         # player 1's runs off the end at step 12; player 2's passes corner 2
    [[-2.0, 12.0], [-1.5, 0.0], [0.0, 5.0]],        # backwards, and a way-point that stands still
], dtype=np.float32)


def mixed_route_scene(T=20):
    """mixed_dubins_car_scene (control dimensions (1, 2): the run-time-dimensioned kernels) with a route-progress term
    on the car's lane."""
    s = examples.mixed_dubins_car_scene(T=T)
    s.params.max_solver_iters = 12
    s.route_progress(1, 3.0, 5.0, 0, (3, 4), 40.0)
    return s


# the lane: 50 m, sqrt(416) ~ 20.396 m, 60 m
MIXED_VECTORS = np.array([[[5.0, 40.0]], [[6.0, 48.5]], [[4.0, 128.0]], [[3.0, 69.5]]], dtype=np.float32)


# ---- numpy restatement of build_time_nominals: float64 products, cumulative sums and the point in S ----
def numpy_time_nominal_table(spec, S):
    out = np.zeros((len(time_terms(spec)), spec.T, 2), dtype=np.float64)
    dt = np.float64(spec.dt)
    for q, ti in enumerate(time_terms(spec)):
        t = spec.terms[ti]
        speed = np.float64(np.float32(t["value"]))
        if t["kind"] == abi.COST_NOMINAL_PATH_LENGTH:
            for k in range(spec.T):
                out[q, k, 0] = (np.float64(k) * dt) * speed
            continue
        pts = np.asarray(spec.polylines[t["polyline"]], dtype=np.float32).astype(S)
        a, b = pts[:-1], pts[1:]
        dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
        length = np.sqrt(dx * dx + dy * dy)
        assert length.dtype == S
        ux, uy = (b[:, 0] - a[:, 0]) / length, (b[:, 1] - a[:, 1]) / length
        cumulative = [S(0)]
        for seg_len in length:
            cumulative.append(S(cumulative[-1] + seg_len))
        cumulative = np.array(cumulative, dtype=S)
        pos0 = np.float64(np.float32(t["value2"]))
        for k in range(spec.T):
            pos = S(pos0 + (np.float64(k) * dt - 0.0) * speed)
            upper = int(np.searchsorted(cumulative, pos, side="right"))  # std::upper_bound
            if upper == len(cumulative):
                upper -= 1
            idx = upper - 1
            remaining = S(pos - cumulative[idx])
            out[q, k, 0] = np.float64(S(a[idx, 0] + S(remaining * ux[idx])))
            out[q, k, 1] = np.float64(S(a[idx, 1] + S(remaining * uy[idx])))
    return out


def _scalar(dtype):
    return np.float32 if dtype == abi.F32 else np.float64


TABLE_CASES = [("zoo", lambda: examples.dynamics_zoo_scene(), None), ("zoo20", zoo20, ZOO_VECTORS),
               ("two_car", two_car_scene, TWO_CAR_VECTORS[:3]), ("mixed", mixed_route_scene, MIXED_VECTORS)]


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("name,make,vectors", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_host_only_table_equals_numpy_restatement(hip, name, make, vectors, dtype):
    """dynamics_zoo_scene as it is (T = 100: lane 2's corner at route position 995 is passed) and routes whose position
    passes corners and runs off the polyline's end: every double of the table, ==."""
    spec = make()
    specs = [spec] if vectors is None else [with_references(spec, v) for v in vectors]
    corner = off_end = False
    for s in specs:
        got = hip.time_nominal_table(s, dtype)
        want = numpy_time_nominal_table(s, _scalar(dtype))
        assert got.shape == want.shape == (len(time_terms(s)), s.T, 2)
        assert got.dtype == np.float64 and np.array_equal(got, want), np.nonzero(got != want)
        for t in (s.terms[ti] for ti in time_terms(s)):
            if t["kind"] != abi.COST_ROUTE_PROGRESS:
                continue
            pts = np.asarray(s.polylines[t["polyline"]], dtype=np.float64)
            cum = np.concatenate([[0.0], np.cumsum(np.hypot(*(pts[1:] - pts[:-1]).T))])
            first, last = t["value2"], t["value2"] + (s.T - 1) * s.dt * t["value"]
            corner = corner or any(first < c < last for c in cum[1:-1])
            off_end = off_end or last > cum[-1]
    assert corner, "a route position should pass a corner"
    if vectors is not None:
        assert off_end, "a route position should run off the polyline's end"
    if dtype == abi.F32 and name == "zoo":  # the two precisions tabulate different doubles for the bent lane
        assert not np.array_equal(hip.time_nominal_table(spec, abi.F32)[2], hip.time_nominal_table(spec, abi.F64)[2])


TABULATE_PROGRAM = r'''
// Reads [T, tables | dt | per table: route, nseg, speed, pos0, nseg * 21 floats, nseg * 21 doubles | tables * T * 2 doubles
// tabulated in float geometry | the same in double geometry] and rebuilds both tables with the function the library's
// host builder and its device kernel share; prints the number of differing bytes of each.  Then the rule for positions
// Polyline2::PointAt CHECK-fails on: a negative and a NaN route position stay on segment 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "ilqg_time_nominal.hpp"
#include "ilqg_segment.hpp"

struct Table {
  int route, nseg;
  float speed, pos0;
  std::vector<float> sf;
  std::vector<double> sd;
};

template <class S>
static long long differing(const std::vector<Table>& tabs, int T, double dt, const std::vector<double>& want) {
  std::vector<double> got;
  for (const Table& t : tabs)
    for (int k = 0; k < T; k++) {
      double pair[2];
      const S* segs = nullptr;
      if (sizeof(S) == sizeof(float)) segs = reinterpret_cast<const S*>(t.sf.data());
      else segs = reinterpret_cast<const S*>(t.sd.data());
      ilqg::time_nominal<S>(t.route != 0, t.speed, t.pos0, k, dt, segs, t.nseg, pair);
      got.push_back(pair[0]);
      got.push_back(pair[1]);
    }
  if (got.size() != want.size()) return -1;
  long long bad = 0;
  const unsigned char* a = reinterpret_cast<const unsigned char*>(got.data());
  const unsigned char* b = reinterpret_cast<const unsigned char*>(want.data());
  for (size_t i = 0; i < got.size() * sizeof(double); i++) bad += a[i] != b[i];
  return bad;
}

template <class S>
static void off_polyline() {
  // a polyline with a corner, (0, 0) -> (3, 4) -> (3, 10), built by the segment function itself
  const float pts[6] = {0.f, 0.f, 3.f, 4.f, 3.f, 10.f};
  S segs[2 * ilqg::kTimeNominalSegStride];
  for (int c = 0; c < 2; c++) ilqg::segment_and_shortcuts(pts, 2, c, segs + c * ilqg::kTimeNominalSegStride);
  double x = 0, y = 0, pair[2];
  ilqg::polyline_point_at<S>(segs, 2, S(-2.5), &x, &y);  // backwards along segment 0: (-1.5, -2)
  std::printf("%.17g %.17g\n", x, y);
  ilqg::time_nominal<S>(true, -10.f, 1.f, 3, 0.25, segs, 2, pair);  // position 1 - 7.5 = -6.5: (-3.9, -5.2)
  std::printf("%.17g %.17g\n", pair[0], pair[1]);
  ilqg::polyline_point_at<S>(segs, 2, std::numeric_limits<S>::quiet_NaN(), &x, &y);
  std::printf("%d %d\n", int(std::isnan(x)), int(std::isnan(y)));
  ilqg::time_nominal<S>(true, std::numeric_limits<float>::quiet_NaN(), 1.f, 2, 0.25, segs, 2, pair);
  std::printf("%d %d\n", int(std::isnan(pair[0])), int(std::isnan(pair[1])));
  ilqg::polyline_point_at<S>(segs, 2, S(13), &x, &y);  // past the end, along the last segment: (3, 12)
  std::printf("%.17g %.17g\n", x, y);
  ilqg::polyline_point_at<S>(segs, 1, S(7), &x, &y);  // one segment: past its end along itself, (4.2, 5.6)
  std::printf("%.17g %.17g\n", x, y);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; };
  int T = 0, ntab = 0;
  double dt = 0;
  if (!rd(&T, sizeof(int)) || !rd(&ntab, sizeof(int)) || !rd(&dt, sizeof(double))) return 3;
  std::vector<Table> tabs(ntab);
  for (Table& t : tabs) {
    if (!rd(&t.route, sizeof(int)) || !rd(&t.nseg, sizeof(int)) || !rd(&t.speed, sizeof(float)) || !rd(&t.pos0, sizeof(float)))
      return 3;
    t.sf.resize(size_t(t.nseg) * ilqg::kTimeNominalSegStride);
    t.sd.resize(t.sf.size());
    if (!rd(t.sf.data(), sizeof(float) * t.sf.size()) || !rd(t.sd.data(), sizeof(double) * t.sd.size())) return 3;
  }
  std::vector<double> wf(size_t(ntab) * T * 2), wd(wf.size());
  if (!rd(wf.data(), sizeof(double) * wf.size()) || !rd(wd.data(), sizeof(double) * wd.size())) return 3;
  std::fclose(f);
  std::printf("%lld %lld %d\n", differing<float>(tabs, T, dt, wf), differing<double>(tabs, T, dt, wd), int(wf.size()));
  off_polyline<float>();
  off_polyline<double>();
  return 0;
}
'''


def test_shared_tabulating_function_rebuilds_the_tables_bytewise_under_sanitizers(hip):
    """A stand-alone program with its own main, compiled with -fsanitize=address,undefined against
    ilqgames_amd/csrc/ilqg_time_nominal.hpp and ilqg_segment.hpp alone, rebuilds the tables of every case above; the
    tables it is compared with are build_time_nominals' (ilqg_time_nominal_table_build, called here from the unsanitised
    library).  It then takes positions off the polyline: negative and NaN stay on segment 0 (no index leaves the
    table under the sanitizers), past the end runs along the last segment.  Nothing sanitised is loaded into Python."""
    specs = [examples.dynamics_zoo_scene()]
    for _, make, vectors in TABLE_CASES[1:]:
        specs += [with_references(make(), v) for v in vectors]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "tabulate.cpp")
        open(src, "w").write(TABULATE_PROGRAM)
        exe = os.path.join(td, "tabulate")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-ffp-contract=off", "-I", os.path.join(ROOT, "ilqgames_amd", "csrc"), src, "-o", exe])
        total = 0
        for k, spec in enumerate(specs):
            sf, sd = hip.segment_table(spec, abi.F32), hip.segment_table(spec, abi.F64)
            wf, wd = hip.time_nominal_table(spec, abi.F32), hip.time_nominal_table(spec, abi.F64)
            first = np.concatenate([[0], np.cumsum([len(p) - 1 for p in spec.polylines])])
            path = os.path.join(td, "case%d.bin" % k)
            with open(path, "wb") as f:
                f.write(np.array([spec.T, len(time_terms(spec))], dtype=np.int32).tobytes())
                f.write(np.float64(spec.dt).tobytes())
                for ti in time_terms(spec):
                    t = spec.terms[ti]
                    route = t["kind"] == abi.COST_ROUTE_PROGRESS
                    lo, hi = (first[t["polyline"]], first[t["polyline"] + 1]) if route else (0, 0)
                    f.write(np.array([int(route), hi - lo], dtype=np.int32).tobytes())
                    f.write(np.array([t["value"], t["value2"]], dtype=np.float32).tobytes())
                    f.write(sf[lo:hi].tobytes() + sd[lo:hi].tobytes())
                f.write(wf.tobytes() + wd.tobytes())
            out = subprocess.run([exe, path], check=True, text=True, capture_output=True, timeout=60)
            assert out.stderr == "", out.stderr
            lines = out.stdout.splitlines()
            bad_f, bad_d, count = (int(v) for v in lines[0].split())
            assert (bad_f, bad_d, count) == (0, 0, wf.size), (k, lines[0])
            total += count
        assert total > 0
    # the positions off the polyline (the same in every run): float, then double
    assert len(lines) == 13
    for S, block in ((np.float32, lines[1:7]), (np.float64, lines[7:13])):
        vals = [[float(v) for v in line.split()] for line in block]
        ux, uy = S(S(3) / S(5)), S(S(4) / S(5))
        assert vals[0] == [float(S(S(0) + S(S(-2.5) * ux))), float(S(S(0) + S(S(-2.5) * uy)))]
        assert vals[1] == [float(S(S(0) + S(S(-6.5) * ux))), float(S(S(0) + S(S(-6.5) * uy)))]
        assert vals[2] == [1, 1] and vals[3] == [1, 1]
        assert vals[4] == [3.0, 12.0]
        assert vals[5] == [float(S(S(0) + S(S(7) * ux))), float(S(S(0) + S(S(7) * uy)))]
    assert abs(vals[0][0] + 1.5) < 1e-12 and abs(vals[1][1] + 5.2) < 1e-12


# ---- the header, the exports ----
def test_c_header_declares_the_calls_and_keeps_abi_version_9():
    """The snippet takes the address of every function with its exact prototype: a missing or differently typed
    declaration does not compile (-Werror)."""
    src = r'''
#include <stdio.h>
#include "ilqg.h"
typedef ilqg_status (*bind_fn)(ilqg_problem*, int32_t, const double*);
typedef ilqg_status (*build_fn)(const ilqg_problem*, int32_t, const float*, double*, void*);
typedef ilqg_status (*terms_fn)(const ilqg_problem*, int32_t*, int32_t, int32_t*);
typedef ilqg_status (*table_fn)(const ilqg_problem_desc*, int32_t, double*, int32_t, int32_t*);
int main(void) {
  bind_fn b = &ilqg_problem_bind_instance_time_nominals;
  build_fn d = &ilqg_instance_time_nominals_build;
  terms_fn t = &ilqg_problem_time_nominal_terms;
  table_fn h = &ilqg_time_nominal_table_build;
  (void)b; (void)d; (void)t; (void)h;
  printf("%d\n", (int)ILQG_ABI_VERSION);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", c, "-o", c + ".o"])
    assert abi.ABI_VERSION == 9


def test_library_exports_the_calls_and_exports_agree_with_the_header(hip):
    for name in CALLS:
        assert name in hip.EXPORTS and hasattr(hip.lib(), name), name
    assert hip.lib().ilqg_abi_version() == 9
    header = open(os.path.join(ROOT, "include", "ilqg.h")).read()
    declared = set(re.findall(r"\b(ilqg_[a-z_0-9]+)\s*\(", header))
    assert set(CALLS) <= declared
    assert declared == set(hip.EXPORTS), declared ^ set(hip.EXPORTS)
    assert len(hip.EXPORTS) == len(set(hip.EXPORTS))


# ---- refusals that need no device ----
def _table_build(hip, spec, dtype, out, capacity):
    desc, keep = spec.build(abi.F64)
    count = hip.C.c_int32(-1)
    rc = hip.lib().ilqg_time_nominal_table_build(hip.C.byref(desc), dtype, out, capacity, hip.C.byref(count))
    del keep
    return rc, count.value


def test_host_only_builder_refusals_and_empty_table(hip):
    lib = hip.lib()
    spec = zoo20()
    count = hip.C.c_int32(0)
    assert lib.ilqg_time_nominal_table_build(None, abi.F64, None, 0, hip.C.byref(count)) == abi.ERR_INVALID
    desc, keep = spec.build(abi.F64)
    assert lib.ilqg_time_nominal_table_build(hip.C.byref(desc), abi.F64, None, 0, None) == abi.ERR_INVALID
    del keep
    rc, _ = _table_build(hip, spec, 7, None, 0)
    assert rc == abi.ERR_INVALID and "dtype" in lib.ilqg_last_error().decode()
    rc, n = _table_build(hip, spec, abi.F32, None, 0)
    assert (rc, n) == (0, 3 * 20 * 2)
    buf = np.zeros(n, dtype=np.float64)
    rc, _ = _table_build(hip, spec, abi.F32, buf.ctypes.data_as(hip.C.c_void_p), n - 1)
    assert rc == abi.ERR_INVALID and "too small" in lib.ilqg_last_error().decode() and not buf.any()
    # a scene without a time-dependent term has an empty table
    plain = examples.modified_three_player_intersection()
    assert not time_terms(plain)
    assert _table_build(hip, plain, abi.F64, None, 0) == (0, 0)
    assert hip.time_nominal_table(plain, abi.F64).shape == (0, plain.T, 2)
    # the descriptor path keeps its ILQG_ERR_INVALID for a route position that turns negative (the device builder does not)
    backwards = with_references(two_car_scene(), TWO_CAR_VECTORS[3])
    backwards.terms[time_terms(backwards)[0]]["value"] = -20.0
    with pytest.raises(hip.IlqgError) as e:
        hip.time_nominal_table(backwards, abi.F64)
    assert e.value.status == abi.ERR_INVALID and "non-negative" in str(e.value)


def test_calls_on_a_null_handle_return_what_the_neighbouring_calls_return(hip):
    """No handle exists without a device; on a null handle the new calls answer as ilqg_problem_bind_instance_values
    does."""
    lib = hip.lib()
    count = hip.C.c_int32(0)
    neighbour = lib.ilqg_problem_bind_instance_values(None, 1, None)
    assert lib.ilqg_problem_bind_instance_time_nominals(None, 1, None) == neighbour == abi.ERR_INVALID
    assert lib.ilqg_instance_time_nominals_build(None, 1, None, None, None) == abi.ERR_INVALID
    assert lib.ilqg_problem_time_nominal_terms(None, None, 0, hip.C.byref(count)) == abi.ERR_INVALID


def test_the_two_older_refusals_are_unchanged(hip):
    """A per-instance `value` column of the two time-dependent kinds, and a per-instance route for the polyline of a
    ROUTE_PROGRESS term, are refused with the messages they had — a pin of old behaviour; what these terms take instead
    is a block of the new table, which ilqg_time_nominal_table_build returns one table per such term for."""
    for make in (zoo20, two_car_scene, mixed_route_scene):
        spec = make()
        assert hip.time_nominal_table(spec, abi.F32).shape == (len(time_terms(spec)), spec.T, 2)
        for ti in time_terms(spec):
            with pytest.raises(hip.IlqgError) as e:
                hip.instance_params_check(spec, [(ti, "value")])
            assert e.value.status == abi.ERR_UNSUPPORTED and "term %d" % ti in str(e.value) and "tabulated" in str(e.value)
            hip.instance_params_check(spec, [(ti, "weight")])
            if spec.terms[ti]["kind"] == abi.COST_ROUTE_PROGRESS:
                q = spec.terms[ti]["polyline"]
                with pytest.raises(hip.IlqgError) as e:
                    hip.instance_routes_check(spec, [q])
                msg = str(e.value)
                assert e.value.status == abi.ERR_UNSUPPORTED and "polyline %d" % q in msg and "ROUTE_PROGRESS" in msg
                assert "tabulates its per-step nominals" in msg
    hip.instance_routes_check(two_car_scene(), [1])  # a polyline no route-progress term uses may still vary


# ---- the C++ mirror, host only ----
def demo_exe():
    import __graft_entry__
    exe = os.path.join(ROOT, "tests", "host", "_bin", "instance_time_nominals_demo")
    if not os.path.exists(exe):
        __graft_entry__.build_host()
    return exe


def test_cpp_mirror_resolves_references_by_address_to_tables_and_tabulates_as_the_library(hip):
    """tests/host/instance_time_nominals_demo.cpp resolve: AddReference(route of player 2), AddReference(route of player
    1) -> tables 2 and 0 of 3; a cost that is not time-dependent and a cost of no problem -> false with a reason; a row
    whose route position turns negative -> false with the library's message; the description it flattens has the three
    time-dependent terms in table order."""
    lines = subprocess.check_output([demo_exe(), "resolve"], text=True, timeout=120).splitlines()
    assert lines[0] == "tables 3" and lines[1] == "references 2 0"
    for line in lines[2:4]:
        refused = line.split(None, 2)
        assert refused[:2] == ["refused", "0"] and "no NominalPathLengthCost or RouteProgressCost" in refused[2]
    negative = lines[4].split(None, 2)
    assert negative[:2] == ["negative", "0"] and "instance 0" in negative[2] and "non-negative" in negative[2]
    assert lines[5] == "dump"
    spec = abi.ProblemSpec.from_dump("\n".join(lines[6:]))
    kinds = [spec.terms[ti]["kind"] for ti in time_terms(spec)]
    assert kinds == [abi.COST_ROUTE_PROGRESS, abi.COST_NOMINAL_PATH_LENGTH, abi.COST_ROUTE_PROGRESS]
    assert hip.time_nominal_table(spec, abi.F64).shape == (3, spec.T, 2)
