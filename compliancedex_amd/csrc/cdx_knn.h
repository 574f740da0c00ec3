// k-nearest-neighbour search and cloud normals: the rule shared by the kernels (cdx_knn.hip) and the host build
// (host_ref.cpp: cdxh_knn, cdxh_cloud_normals, cdxh_sym3_eig and the grid functions, the CPU yardsticks of those
// kernels).  The reference's completion merge estimates and orients normals of a sensed cloud with open3d
// (concatenate_pcd.py:35-36); open3d's remove_statistical_outlier and compute_point_cloud_distance are the same query
// with a few operations per row after it.  Parity with open3d's own covariance (raw moments) and its closed-form
// eigen-solver is unpinned and not attempted (open3d is not a dependency).
//
// Neighbours.  Cloud X [P, 3], queries Q [M, 3] (Q null: Q = X, and a point is then its own first neighbour, as in
//   open3d), float32 or float64 widened on load, 1 ≤ K ≤ CDX_KNN_MAX_K.
//   d2 = cdx::fps_sqdist(x, q) = (dx·dx + dy·dy) + dz·dz, every product and sum rounded on its own.
//   Row m of the result: the K smallest (d2, index) pairs in ascending order (knn_before), ties on d2 to the smaller
//   cloud index.  A cloud row with a non-finite coordinate is never a neighbour.  Pairs with d2 > max_d2 are left out
//   (+inf: none are; a pair whose d2 overflows to +inf is still a pair).  count[m] = pairs found; slots past it hold
//   index −1 and d2 = +inf.  A query with a non-finite coordinate gets count 0.  K > P: the lists are short.
//
// The grid (mode 2).  Over the bounding box [lo, hi] of the finite rows, n0 = knn_grid_n0(P) cells along the longest
//   axis: inv = n0 / max extent (0 when the extent is 0 or the quotient is not finite), n[a] = knn_cell(hi[a]) + 1.
//   knn_cell(x) = floor((x − lo[a]) · inv) clamped to 0 … n[a]−1, for rows and for queries alike (a query outside the
//   box lands in a border cell).  Beside the rows in cell order the grid keeps, per axis a and slab c (the rows whose
//   cell index along a is c), below[a][c] = the largest coordinate a of the rows in slabs ≤ c (−inf if none) and
//   above[a][c] = the smallest of the rows in slabs ≥ c (+inf if none): true extrema of the rows the rounded
//   assignment put there.  A query in cell cq visits the cells at Chebyshev distance r = 0, 1, … from cq.  Every row
//   in a cell at distance > r differs from cq by more than r on some axis a, so it lies in a slab ≥ cq[a]+r+1 or
//   ≤ cq[a]−r−1 there and its |x[a] − q[a]|, as rounded, is at least g = min over the six of
//   max(0, above[a][cq[a]+r+1] − q[a]) and max(0, q[a] − below[a][cq[a]−r−1]): rounding is monotone, so a row
//   beyond the extremum has a rounded difference no smaller.  Its d2 ≥ g·g (knn_ring_bound) for the same reason: the
//   rounded square is monotone and the rounded sum of non-negative terms is no smaller than either.  The walk stops
//   once knn_ring_bound(r) is STRICTLY greater than the K-th pair's d2 (an equal d2 at a smaller index would still
//   enter) or than max_d2 (no row out there is within the radius, however short the list), once no row is left out
//   there, or once r reaches the largest n[a] (every cell was visited).  The bound uses no property of knn_cell.
//
// Normals.  A row is computed from its c = count neighbours in list order: mean m by sequential float64 sums divided
//   by c; the six entries of C = (1/c) Σ (x − m)(x − m)ᵀ summed in the same order (each product rounded, then added);
//   sym3_eig(C); the normal is the eigenvector of the smallest eigenvalue.  Sign with an eye point: flipped when
//   (nx·ex + ny·ey) + nz·ez < 0, e = eye − p (open3d's orient_normals_towards_camera_location).  Without: the
//   component of largest magnitude is made positive, the lowest axis on a tie.  c < 3 or a C with a non-finite entry:
//   normal (0, 0, 1) (then signed like any other) and NaN eigenvalues, open3d's fallback.  A non-finite point: NaN
//   normal and eigenvalues.
//
// sym3_eig: cyclic Jacobi on the symmetric 3×3 A = (a00 a01 a02; a11 a12; a22), V = I.
//   At most CDX_KNN_SWEEPS = 10 sweeps.  Before each sweep: off = (a01² + a02²) + a12²; stop when off == 0 (or is NaN).
//   A sweep visits (p, q) = (0, 1), (0, 2), (1, 2), r the third index.  With g = |apq|: if g == 0 nothing; if
//   |app| + g == |app| and |aqq| + g == |aqq| (g below the last place of both) apq = 0 and nothing else; otherwise
//     θ = (aqq − app) / (2·apq);  t = sign(θ) / (|θ| + sqrt(θ·θ + 1)) (sign(0) = +1);  c = 1 / sqrt(t·t + 1);  s = t·c
//     app −= t·apq;  aqq += t·apq;  apq = 0;  (arp, arq) = (c·arp − s·arq, s·arp + c·arq)
//     V's columns p and q likewise: (vkp, vkq) = (c·vkp − s·vkq, s·vkp + c·vkq), k = 0, 1, 2.
//   Then the three (eigenvalue, column) pairs are ordered ascending by three compare-exchanges (0,1), (1,2), (0,1)
//   that swap on a strictly greater left value.  Every rotation is an orthogonal similarity to a few units in the
//   last place of ‖A‖_F, so 10 sweeps × 3 rotations leave a backward error well inside 256 · 2⁻⁵² · ‖A‖_F.
#pragma once
#include "cdx_fps.h"
#include "cdx_hd.h"

#define CDX_KNN_SWEEPS 10
#define CDX_KNN_MAX_DIM 256  // cells along one axis at most

namespace cdx {

CDX_HD bool knn_finite3(double x, double y, double z) {
  return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// Order of the lists: (d, i) comes before (bd, bi).  d is never NaN for a finite row and a finite query; a NaN d is
// before nothing.
CDX_HD bool knn_before(double d, int64_t i, double bd, int64_t bi) { return d < bd || (d == bd && i < bi); }

// Cells along the longest axis for a cloud of P rows: the smallest n with n³ ≥ 2·P, at most CDX_KNN_MAX_DIM.
CDX_HD int knn_grid_n0(int64_t P) {
  int n = 1;
  while (n < CDX_KNN_MAX_DIM && (int64_t)n * n * n < 2 * P) ++n;
  return n;
}

// What the query walk reads of a prepared grid.
struct KnnGrid {
  double lo[3];
  double inv;
  int32_t n[3];
  int32_t pad;
};

// Cells per unit length from the box's largest extent.
CDX_HD double knn_grid_inv(double ext, int n0) {
  const double inv = (double)n0 / ext;
  return (ext > 0.0 && __builtin_isfinite(inv)) ? inv : 0.0;
}

// Cell index along one axis, before the clamp to the axis' cell count: 0 … CDX_KNN_MAX_DIM−1.
CDX_HD int knn_cell_raw(double x, double lo, double inv) {
  const double t = floor((x - lo) * inv);
  return t > 0.0 ? (t < (double)(CDX_KNN_MAX_DIM - 1) ? (int)t : CDX_KNN_MAX_DIM - 1) : 0;  // NaN → 0
}

CDX_HD int knn_cell(double x, double lo, double inv, int n) {
  const int c = knn_cell_raw(x, lo, inv);
  return c < n ? c : n - 1;
}

// One side of one axis of the ring bound: e is above[a][cq+r+1] (far = e − q) or below[a][cq−r−1] (far = q − e).
CDX_HD double knn_gap(double far) { return far > 0.0 ? far : 0.0; }  // a NaN (inf − inf) counts as 0

// Lower bound on d2 of every row outside the rings 0 … r around cell cq.  below / above: [3][CDX_KNN_MAX_DIM].
// *none: no row lies out there at all (every extremum is infinite), so the walk may stop whatever the list holds.
CDX_HD double knn_ring_bound(const KnnGrid& g, const double* below, const double* above, const double* q,
                             const int* cq, int r, bool* none) {
  double m = (double)INFINITY;
  bool any = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int up = cq[a] + r + 1, dn = cq[a] - r - 1;
    if (up < g.n[a]) {
      const double e = above[a * CDX_KNN_MAX_DIM + up];
      const double v = knn_gap(e - q[a]);
      any = any || e < (double)INFINITY;
      m = v < m ? v : m;
    }
    if (dn >= 0) {
      const double e = below[a * CDX_KNN_MAX_DIM + dn];
      const double v = knn_gap(q[a] - e);
      any = any || e > -(double)INFINITY;
      m = v < m ? v : m;
    }
  }
  *none = !any;
  return m * m;
}

// ---- normals ------------------------------------------------------------------------------------------------------

// One Jacobi rotation on (app, aqq, apq) with the third row's (arp, arq) and V's columns p, q.
CDX_HD void sym3_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                        double& v1p, double& v1q, double& v2p, double& v2q) {
  const double g = fabs(apq);
  if (g == 0.0) return;
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
    apq = 0.0;
    return;
  }
  const double theta = (aqq - app) / (2.0 * apq);
  const double den = fabs(theta) + sqrt(theta * theta + 1.0);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / den;
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  double x = arp, y = arq;
  arp = c * x - s * y;
  arq = s * x + c * y;
  x = v0p, y = v0q;
  v0p = c * x - s * y;
  v0q = s * x + c * y;
  x = v1p, y = v1q;
  v1p = c * x - s * y;
  v1q = s * x + c * y;
  x = v2p, y = v2q;
  v2p = c * x - s * y;
  v2q = s * x + c * y;
}

CDX_HD void sym3_order(double& wa, double& wb, double& a0, double& a1, double& a2, double& b0, double& b1,
                       double& b2) {
  if (wa > wb) {
    double t = wa; wa = wb; wb = t;
    t = a0; a0 = b0; b0 = t;
    t = a1; a1 = b1; b1 = t;
    t = a2; a2 = b2; b2 = t;
  }
}

// Eigen-decomposition of the symmetric (a00 a01 a02; a11 a12; a22): w[3] ascending, V[9] row-major with the unit
// eigenvector of w[j] in column j.
CDX_HD void sym3_eig(double a00, double a01, double a02, double a11, double a12, double a22, double* w, double* V) {
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < CDX_KNN_SWEEPS; ++sweep) {
    const double off = (a01 * a01 + a02 * a02) + a12 * a12;
    if (!(off != 0.0) || off != off) break;
    sym3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
    sym3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
    sym3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
  }
  sym3_order(a00, a11, v00, v10, v20, v01, v11, v21);
  sym3_order(a11, a22, v01, v11, v21, v02, v12, v22);
  sym3_order(a00, a11, v00, v10, v20, v01, v11, v21);
  w[0] = a00; w[1] = a11; w[2] = a22;
  V[0] = v00; V[1] = v01; V[2] = v02;
  V[3] = v10; V[4] = v11; V[5] = v12;
  V[6] = v20; V[7] = v21; V[8] = v22;
}

// Running sums of the normal of one row: the neighbours are fed twice in list order, first to the mean, then to the
// covariance.
struct KnnMoments {
  double sx, sy, sz;
  double mx, my, mz;
  double c00, c01, c02, c11, c12, c22;
};

CDX_HD void knn_moments_init(KnnMoments& k) {
  k.sx = k.sy = k.sz = 0.0;
  k.c00 = k.c01 = k.c02 = k.c11 = k.c12 = k.c22 = 0.0;
  k.mx = k.my = k.mz = 0.0;
}
CDX_HD void knn_moments_sum(KnnMoments& k, double x, double y, double z) {
  k.sx += x;
  k.sy += y;
  k.sz += z;
}
CDX_HD void knn_moments_mean(KnnMoments& k, int c) {
  k.mx = k.sx / (double)c;
  k.my = k.sy / (double)c;
  k.mz = k.sz / (double)c;
}
CDX_HD void knn_moments_cov(KnnMoments& k, double x, double y, double z) {
  const double dx = x - k.mx, dy = y - k.my, dz = z - k.mz;
  k.c00 += dx * dx;
  k.c01 += dx * dy;
  k.c02 += dx * dz;
  k.c11 += dy * dy;
  k.c12 += dy * dz;
  k.c22 += dz * dz;
}

// From the sums to the normal n[3] and the eigenvalues w[3] of the row at p.  has_eye: orient towards eye.
// cov[6], if given, receives the covariance entries (00, 01, 02, 11, 12, 22).
CDX_HD void knn_normal_finish(KnnMoments& k, int c, const double* p, bool has_eye, const double* eye, double* n,
                              double* w, double* cov) {
  const double nan = __builtin_nan("");
  const double fc = (double)(c > 0 ? c : 1);
  const double c00 = k.c00 / fc, c01 = k.c01 / fc, c02 = k.c02 / fc, c11 = k.c11 / fc, c12 = k.c12 / fc,
               c22 = k.c22 / fc;
  if (cov) {
    cov[0] = c00; cov[1] = c01; cov[2] = c02; cov[3] = c11; cov[4] = c12; cov[5] = c22;
  }
  if (!knn_finite3(p[0], p[1], p[2])) {
    n[0] = n[1] = n[2] = nan;
    w[0] = w[1] = w[2] = nan;
    return;
  }
  if (c < 3 || !knn_finite3(c00, c01, c02) || !knn_finite3(c11, c12, c22)) {
    n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
    w[0] = w[1] = w[2] = nan;
  } else {
    double V[9];
    sym3_eig(c00, c01, c02, c11, c12, c22, w, V);
    n[0] = V[0]; n[1] = V[3]; n[2] = V[6];
  }
  bool flip;
  if (has_eye) {
    const double ex = eye[0] - p[0], ey = eye[1] - p[1], ez = eye[2] - p[2];
    flip = (n[0] * ex + n[1] * ey) + n[2] * ez < 0.0;
  } else {
    const double ax = fabs(n[0]), ay = fabs(n[1]), az = fabs(n[2]);
    const double lead = (ax >= ay && ax >= az) ? n[0] : (ay >= az ? n[1] : n[2]);
    flip = lead < 0.0;
  }
  if (flip) {
    n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2];
  }
}

}  // namespace cdx
