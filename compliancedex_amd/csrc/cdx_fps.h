// Farthest-point sampling rule, shared by the sampling kernels (cdx_fps.hip) and the host build (host_ref.cpp:
// cdxh_fps, the CPU yardstick of those kernels).  The reference down-samples its sensed clouds with open3d's
// farthest_point_down_sample (optimize_pregrasp.py:904, get_observable_pcd.py:40) before GPIS.fit.
//
// Cloud X [P, 3], 1 ≤ K ≤ P < 2³¹, 0 ≤ start < P.  All arithmetic is float64 (a float32 cloud is widened on load).
//   dist[j] = +inf for a row whose three coordinates are finite, −1 for any other row (and that never changes).
//   Round i = 0 … K−1:  sel[i] = s (s = start in round 0);  radius[i] = dist[s] before this round's update;
//     for every row j:  q = (dx·dx + dy·dy) + dz·dz, d* = X[j,*] − X[s,*], every product and sum rounded on its own
//     (both builds compile this header without FMA contraction);  dist[j] = q if q < dist[j] — a NaN q (non-finite
//     centre) and a row at −1 change nothing;
//     the next s is the SMALLEST index among the rows with the largest dist.
// Consequences: the first k entries of a K-sample are the k-sample; radius[1:] is non-increasing; once every finite
// row is chosen dist is 0 on all of them and the rule repeats the lowest finite index; a non-finite row is chosen
// only as `start` (or when no row is finite: then every round takes row 0 after `start`).
#pragma once
#include "cdx_hd.h"

namespace cdx {

// dist of a row before the first round.
CDX_HD double fps_init_dist(double x, double y, double z) {
  return (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z)) ? (double)INFINITY : -1.0;
}

// Squared distance of row (x, y, z) to the centre (cx, cy, cz), in the rule's order of operations.
CDX_HD double fps_sqdist(double x, double y, double z, double cx, double cy, double cz) {
  const double dx = x - cx, dy = y - cy, dz = z - cz;
  return (dx * dx + dy * dy) + dz * dz;
}

// The running minimum.
CDX_HD double fps_update(double dist, double q) { return q < dist ? q : dist; }

// Order of the arg-max: candidate (d, i) beats the holder (bd, bi) on a larger dist, or the same dist at a smaller
// index.  dist is never NaN.
CDX_HD bool fps_beats(double d, int64_t i, double bd, int64_t bi) { return d > bd || (d == bd && i < bi); }

}  // namespace cdx
