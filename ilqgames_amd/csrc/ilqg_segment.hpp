// ilqg_segment.hpp — one LineSegment2 (include/ilqgames/geometry/line_segment2.h:55-62) of the segment table
// (DevProblem::segs_f / segs_d), in the one form the host builder (build_segments, ilqg_problem.hpp) and the device
// builder of a per-instance route table (route_segments_kernel, ilqg_instances.hpp) both call.  Plain C++ apart from the two
// function attributes: a host-only program includes it as it is.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ILQG_SEGMENT_FN __host__ __device__ inline
#else
#define ILQG_SEGMENT_FN inline
#endif

namespace ilqg {

ILQG_SEGMENT_FN float segment_sqrt(float v) { return __builtin_sqrtf(v); }
ILQG_SEGMENT_FN double segment_sqrt(double v) { return __builtin_sqrt(v); }

constexpr int kSegmentScalars = 7;  // of one LineSegment2: [p1x p1y p2x p2y len ux uy]

// The segment a -> b from the points' floats, in S's arithmetic.  No contraction: every product and sum rounds on its
// own, on the host and on the device alike (a fused dx * dx + dy * dy would differ in the last bit of the length).
template <class S>
ILQG_SEGMENT_FN void line_segment2(const float* a, const float* b, S* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const S ax = a[0], ay = a[1], bx = b[0], by = b[1];
  const S dx = ax - bx, dy = ay - by;
  const S len = segment_sqrt(dx * dx + dy * dy);
  out[0] = ax; out[1] = ay; out[2] = bx; out[3] = by;
  out[4] = len; out[5] = (bx - ax) / len; out[6] = (by - ay) / len;
}

// Segment c of a polyline of nseg segments (points `pts`, nseg + 1 of them) with its two shortcuts (src/polyline2.cpp:
// 126-133): [segment | prev.p1 -> p2 | p1 -> next.p2], 3 * kSegmentScalars scalars
template <class S>
ILQG_SEGMENT_FN void segment_and_shortcuts(const float* pts, int nseg, int c, S* out) {
  const int pm = c > 0 ? c - 1 : c, pn = c + 2 <= nseg ? c + 2 : c + 1;
  line_segment2(pts + 2 * c, pts + 2 * (c + 1), out);
  line_segment2(pts + 2 * pm, pts + 2 * (c + 1), out + kSegmentScalars);
  line_segment2(pts + 2 * c, pts + 2 * pn, out + 2 * kSegmentScalars);
}

}  // namespace ilqg
