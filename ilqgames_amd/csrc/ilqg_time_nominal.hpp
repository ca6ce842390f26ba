// ilqg_time_nominal.hpp — one per-step nominal of a time-dependent cost (DevProblem::time_nominal_f / _d), in the one
// form the host builder (build_time_nominals, ilqg_problem.hpp) and the device builder of a per-instance table
// (time_nominals_kernel, ilqg_instances.hpp) both call.  NominalPathLengthCost (src/nominal_path_length_cost.cpp:53): the
// double product t_k * speed.  RouteProgressCost (src/route_progress_cost.cpp:57-59): Polyline2::PointAt
// (src/polyline2.cpp:68-103) at a route position that is a scalar of the geometry made from a double expression.  Plain
// C++ apart from the two function attributes: a host-only program includes it (and ilqg_segment.hpp) as it is.
#pragma once

#include "ilqg_segment.hpp"  // kSegmentScalars: a segment's layout in the table

namespace ilqg {

constexpr int kTimeNominalSegStride = 3 * kSegmentScalars;  // a segment and its two shortcuts (kSegStride)

// Polyline2::PointAt on `nseg` consecutive segments of a segment table of precision S (`segs`: the polyline's first).
// The cumulative lengths are summed in S in segment order; the segment is the last one whose cumulative start is not
// greater than route_pos — what std::upper_bound over the cumulative lengths, stepped back once, picks, with a position
// past the end on the last segment (upper == end).  PointAt CHECKs route_pos >= 0; here a negative or NaN position
// compares false everywhere and so stays on segment 0, extrapolating backwards along it.
template <class S>
ILQG_SEGMENT_FN void polyline_point_at(const S* segs, int nseg, S route_pos, double* px, double* py) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int idx = 0;
  S start = S(0), cumulative = S(0);
  for (int c = 1; c < nseg; c++) {
    cumulative = cumulative + segs[(c - 1) * kTimeNominalSegStride + 4];
    if (cumulative <= route_pos) {
      idx = c;
      start = cumulative;
    }
  }
  const S remaining = route_pos - start;
  const S* sg = segs + idx * kTimeNominalSegStride;
  *px = double(S(sg[0] + remaining * sg[5]));
  *py = double(S(sg[1] + remaining * sg[6]));
}

// The nominal pair of step k: t = RelativeTime(k) = double(k) * dt (relative_time_tracker.h:63-65), initial time 0.
//   route false   (t * speed, 0)                                       `pos0`, `segs`, `nseg` are not read
//   route true    PointAt(S(pos0 + (t - 0) * speed)) on the polyline's segments
// No contraction: every product and sum rounds on its own, on the host and on the device alike.
template <class S>
ILQG_SEGMENT_FN void time_nominal(bool route, float speed, float pos0, int k, double dt, const S* segs, int nseg,
                                  double* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double tk = double(k) * dt;
  out[0] = tk * double(speed);
  out[1] = 0.0;
  if (route) {
    const double pos = double(pos0) + (tk - 0.0) * double(speed);
    polyline_point_at(segs, nseg, S(pos), &out[0], &out[1]);
  }
}

}  // namespace ilqg
