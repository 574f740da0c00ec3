// Ray casting and depth unprojection rules, shared by the ray kernels (cdx_ray.hip) and the host build (host_ref.cpp:
// cdxh_ray_cast, cdxh_depth_unproject — the CPU yardsticks of those kernels).  The reference makes its partial clouds
// with a PyBullet depth camera and open3d's create_from_depth_image (get_observable_pcd.py:26-40) and filters
// completed points with open3d's RaycastingScene.cast_rays (concatenate_pcd.py:41-49); parity with open3d, Embree and
// PyBullet is unpinned (none of them is a dependency): this header is the statement both builds are held to.
//
// Ray–face test (Möller–Trumbore).  Face vertices v0, v1, v2 are float32 values widened to float64; o, d, tmin, tmax
// are float64; d is not normalised, so t is in units of |d|.  Every product, sum and quotient is rounded on its own
// (both builds compile this header without FMA contraction), sums of three associate to the left:
//   e1 = v1 − v0, e2 = v2 − v0, p = d × e2, det = e1·p, T = o − v0, q = T × e1
//   u = (T·p)/det, v = (d·q)/det, t = (e2·q)/det
//   a × b = (a.y·b.z − a.z·b.y, a.z·b.x − a.x·b.z, a.x·b.y − a.y·b.x),  a·b = (a.x·b.x + a.y·b.y) + a.z·b.z
// Hit iff det is finite, det·det > 2⁻⁴⁰·((e1·e1)·(e2·e2))·(d·d)  (|det| > 2⁻²⁰·|e1||e2||d|: a face seen at less than
// about 1e-6 rad off its plane, or whose edges e1, e2 are that close to parallel, is not hit; det = 0 never is),
// u ≥ 0, v ≥ 0, u + v ≤ 1 and tmin ≤ t ≤ tmax.  The determinant threshold is part of the rule: it bounds the relative
// rounding error of u, v and t, which is what lets the hierarchy walk skip nodes with a proof.
//
// First hit: the smallest t; equal t goes to the smallest ORIGINAL face index.  A miss gives t = +inf, face = −1,
// u = v = 0.  A ray with a non-finite component of o or d, or with d = 0, is a miss.
//
// Pixel rays (render): pixel (i, j) — row i, column j — of a pinhole camera (fx, fy, cx, cy) has the camera-frame
// direction ((j − cx)/fx, (i − cy)/fy, 1): x right, y down, z forward.  With the float64 camera-to-world matrix M
// (row-major 4×4) the world ray is d[k] = (M[k][0]·dx + M[k][1]·dy) + M[k][2], o[k] = M[k][3].  The z component is 1, so
// t is the z-depth.
//
// Depth unprojection (what open3d's create_from_depth_image does, as far as it can be stated without open3d): depth is
// uint16, float32 or float64 [H, W]; Z = float for uint16 and float32 depth, double for float64.
//   z = (Z)depth / (Z)depth_scale; the pixel is dropped if depth == 0 or z ≥ (Z)depth_trunc, or — with a z mask, z_max
//   not NaN — unless (double)z < z_max.  Otherwise, in float64: x = ((j − cx)·z)/fx, y = ((i − cy)·z)/fy, and with a
//   transform M: out[k] = ((M[k][0]·x + M[k][1]·y) + M[k][2]·z) + M[k][3].
// Pixels come in row-major order over i = 0, stride, 2·stride, … < H (outer) and j likewise < W (inner).
#pragma once
#include "cdx_hd.h"

namespace cdx {

constexpr double RAY_DET_TAU2 = 0x1p-40;  // square of the relative determinant threshold 2⁻²⁰
constexpr int32_t RAY_NO_FACE = 0x7fffffff;  // the holder's index before any hit (loses every tie)

struct RayHit { double t, u, v; int32_t face; };

CDX_HD RayHit ray_miss() {
  RayHit h;
  h.t = (double)INFINITY; h.u = 0.0; h.v = 0.0; h.face = RAY_NO_FACE;
  return h;
}

// A ray the rule casts at all: finite o and d, d ≠ 0.
CDX_HD bool ray_valid(const double* o, const double* d) {
  const bool fin = __builtin_isfinite(o[0]) && __builtin_isfinite(o[1]) && __builtin_isfinite(o[2]) &&
                   __builtin_isfinite(d[0]) && __builtin_isfinite(d[1]) && __builtin_isfinite(d[2]);
  return fin && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
}

CDX_HD double ray_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
CDX_HD void ray_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The ray–face test on the face's nine float32 coordinates (v0 xyz, v1 xyz, v2 xyz).
CDX_HD bool ray_face(const double* o, const double* d, const float* f, double tmin, double tmax, double& t, double& u,
                     double& v) {
  const double v0[3] = {(double)f[0], (double)f[1], (double)f[2]};
  const double e1[3] = {(double)f[3] - v0[0], (double)f[4] - v0[1], (double)f[5] - v0[2]};
  const double e2[3] = {(double)f[6] - v0[0], (double)f[7] - v0[1], (double)f[8] - v0[2]};
  double p[3], q[3];
  ray_cross(d, e2, p);
  const double det = ray_dot(e1, p);
  const double lim = ((ray_dot(e1, e1) * ray_dot(e2, e2)) * ray_dot(d, d)) * RAY_DET_TAU2;
  const bool ok = __builtin_isfinite(det) && det * det > lim;
  const double T[3] = {o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]};
  u = ray_dot(T, p) / det;
  ray_cross(T, e1, q);
  v = ray_dot(d, q) / det;
  t = ray_dot(e2, q) / det;
  return ok && u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t >= tmin && t <= tmax;
}

// Order of the first hit: candidate (t, face) beats the holder on a smaller t, or the same t at a smaller index.
CDX_HD bool ray_beats(double t, int32_t face, double bt, int32_t bface) { return t < bt || (t == bt && face < bface); }

// One face against one ray, folded into the ray's holder.
CDX_HD void ray_update(const double* o, const double* d, const float* f, int32_t face, double tmin, double tmax,
                       RayHit& best) {
  double t, u, v;
  if (ray_face(o, d, f, tmin, tmax, t, u, v) && ray_beats(t, face, best.t, best.face)) {
    best.t = t; best.u = u; best.v = v; best.face = face;
  }
}

// The outputs of a holder: a miss is (+inf, −1, 0, 0).
CDX_HD void ray_result(const RayHit& best, double& t, int32_t& face, double& u, double& v) {
  const bool hit = best.face != RAY_NO_FACE;
  t = hit ? best.t : (double)INFINITY;
  face = hit ? best.face : -1;
  u = hit ? best.u : 0.0;
  v = hit ? best.v : 0.0;
}

// Node skip of the hierarchy walk.  Rays inside the walk's domain (others never skip a node): |o| ≤ 1e6 per
// component, 2⁻⁶⁴ ≤ max |d| ≤ 2⁶⁴ — no product of the face test or of the ball test overflows, and none that matters
// underflows.
constexpr double RAY_O_LIM = 1e6, RAY_D_MIN = 0x1p-64, RAY_D_MAX = 0x1p64;
constexpr double RAY_KAPPA = 1e-6;  // additive margin per unit of |o − c|₁ + R (60× the error bound)

CDX_HD bool ray_in_domain(const double* o, const double* d) {
  const double dm = fmax(fmax(fabs(d[0]), fabs(d[1])), fabs(d[2]));
  return fabs(o[0]) <= RAY_O_LIM && fabs(o[1]) <= RAY_O_LIM && fabs(o[2]) <= RAY_O_LIM && dm >= RAY_D_MIN &&
         dm <= RAY_D_MAX;
}

// True only if no point o + s·d, s0 ≤ s ≤ s1, lies within R + κ·(|o − c|₁ + R) of c: the closest such point is
// evaluated at the clamped minimiser s* = −(L·d)/(d·d), L = o − c.  Any NaN gives false (the node is kept).
CDX_HD bool ray_ball_miss(const double* o, const double* d, double s0, double s1, float cx, float cy, float cz, float R) {
  const double L[3] = {o[0] - (double)cx, o[1] - (double)cy, o[2] - (double)cz};
  const double a = ray_dot(d, d), b = ray_dot(L, d);
  double s = -b / a;
  s = fmin(fmax(s, s0), s1);
  const double q[3] = {L[0] + s * d[0], L[1] + s * d[1], L[2] + s * d[2]};
  const double g = ray_dot(q, q);
  const double l1 = (fabs(L[0]) + fabs(L[1])) + fabs(L[2]);
  const double th = (double)R + RAY_KAPPA * (l1 + (double)R);
  return g > th * th;
}

// World ray of pixel (i, j): intr = (fx, fy, cx, cy), M = camera-to-world, row-major 4×4.
CDX_HD void pixel_ray(int i, int j, const double* intr, const double* M, double* o, double* d) {
  const double dx = ((double)j - intr[2]) / intr[0], dy = ((double)i - intr[3]) / intr[1];
  for (int k = 0; k < 3; ++k) {
    d[k] = (M[4 * k] * dx + M[4 * k + 1] * dy) + M[4 * k + 2];
    o[k] = M[4 * k + 3];
  }
}

// Unprojection of one pixel of raw depth `raw` (already converted to Z): false if the pixel is dropped, else the
// point (transformed by M if given).
template <typename Z>
CDX_HD bool depth_point(Z raw, int i, int j, const double* intr, double depth_scale, double depth_trunc, double z_max,
                        const double* M, double* out) {
  const Z z = raw / (Z)depth_scale;
  if (raw == (Z)0 || z >= (Z)depth_trunc) return false;
  const double zz = (double)z;
  if (z_max == z_max && !(zz < z_max)) return false;
  const double x = (((double)j - intr[2]) * zz) / intr[0];
  const double y = (((double)i - intr[3]) * zz) / intr[1];
  if (M) {
    for (int k = 0; k < 3; ++k) out[k] = ((M[4 * k] * x + M[4 * k + 1] * y) + M[4 * k + 2] * zz) + M[4 * k + 3];
  } else {
    out[0] = x; out[1] = y; out[2] = zz;
  }
  return true;
}

}  // namespace cdx
