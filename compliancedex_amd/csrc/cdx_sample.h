// Area-weighted surface sampling rule, shared by the sampling kernels (cdx_sample.hip) and the host build
// (host_ref.cpp: cdxh_sample_prepare / cdxh_sample_draw, the CPU yardstick of those kernels).  The reference opens
// every run on a mesh object with open3d's sample_points_poisson_disk (optimize_pregrasp.py:887, gpis.py:199-263).
// Both builds compile this header without FMA contraction.
//
// Faces [F, 3, 3] float32 or float64, widened to float64 on load; 1 ≤ F ≤ INT32_MAX/9.
//   Area    e1 = v1 − v0, e2 = v2 − v0, c = e1 × e2 (every product and difference rounded on its own),
//           n2 = (cx·cx + cy·cy) + cz·cz, area = 0.5·sqrt(n2).  A face with a non-finite coordinate, or a non-finite or
//           zero n2, has area 0.
//   Weight  A = the largest area;  w_f = (uint64) floor(area_f / A · 2³²), so 0 ≤ w_f ≤ 2³²;  C_f = Σ_{g ≤ f} w_g in
//           uint64 (F·2³² < 2⁶⁴: no overflow);  T = C_{F−1}.  Integers, so every order of summation gives the same
//           bits: the kernels scan in parallel, the host in a plain loop.  A face below 2⁻³² of the largest area has
//           weight 0 and is NEVER drawn.  A == 0 (no usable face): every weight is 0, T = 0, and the table's `info`
//           word is 1; every sample drawn from such a table has face −1 and NaN outputs.
//   Sample  i = first + row (uint64), seed uint64:
//           (r0, r1, r2, r3) = Philox4x32-10(counter = (i lo, i hi, 0, 0), key = (seed lo, seed hi));
//           t = mulhi64((r1 << 32) | r0, T);  face = the smallest f with C_f > t;
//           u = (r2 + 0.5)·2⁻³², v = (r3 + 0.5)·2⁻³²;  if u + v > 1 then u = 1 − u and v = 1 − v;
//           p = (v0 + u·e1) + v·e2 per component;  normal = c / sqrt(n2).
// A sample depends only on (seed, i): the first k of a K-sample are the k-sample, and `first` shards one stream.
#pragma once
#include "cdx_hd.h"

namespace cdx {

// Philox4x32-10 (Salmon et al., SC'11) with the standard multipliers and Weyl key increments.
CDX_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* r) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

CDX_HD uint64_t sample_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// A face in the rule's terms.
struct SampleFace {
  double v0[3], e1[3], e2[3], c[3], n2;
  bool finite;  // all nine coordinates
};

template <typename T>
CDX_HD SampleFace sample_face(const T* f) {  // f: the face's 9 values
  SampleFace s;
  s.finite = true;
  for (int k = 0; k < 9; ++k) s.finite = s.finite && __builtin_isfinite((double)f[k]);
  for (int k = 0; k < 3; ++k) {
    s.v0[k] = (double)f[k];
    s.e1[k] = (double)f[3 + k] - s.v0[k];
    s.e2[k] = (double)f[6 + k] - s.v0[k];
  }
  s.c[0] = s.e1[1] * s.e2[2] - s.e1[2] * s.e2[1];
  s.c[1] = s.e1[2] * s.e2[0] - s.e1[0] * s.e2[2];
  s.c[2] = s.e1[0] * s.e2[1] - s.e1[1] * s.e2[0];
  s.n2 = (s.c[0] * s.c[0] + s.c[1] * s.c[1]) + s.c[2] * s.c[2];
  return s;
}

CDX_HD double sample_area(const SampleFace& s) {
  return (s.finite && __builtin_isfinite(s.n2) && s.n2 != 0.0) ? 0.5 * sqrt(s.n2) : 0.0;
}

// A: the largest area of the mesh.
CDX_HD uint64_t sample_weight(double area, double A) {
  return A > 0.0 ? (uint64_t)floor(area / A * 4294967296.0) : (uint64_t)0;
}

// t below T = the table's total, and the barycentric pair, of sample i.
CDX_HD void sample_uniforms(uint64_t seed, uint64_t i, uint64_t T, uint64_t& t, double& u, double& v) {
  uint32_t r[4];
  philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  t = sample_mulhi64(((uint64_t)r[1] << 32) | r[0], T);
  u = ((double)r[2] + 0.5) * 0x1p-32;
  v = ((double)r[3] + 0.5) * 0x1p-32;
  if (u + v > 1.0) {
    u = 1.0 - u;
    v = 1.0 - v;
  }
}

// The smallest index in [lo, hi) whose entry exceeds t; hi when there is none.
CDX_HD int64_t sample_upper(const uint64_t* C, int64_t lo, int64_t hi, uint64_t t) {
  int64_t n = hi - lo;
  while (n > 0) {
    const int64_t half = n >> 1;
    if (C[lo + half] > t) {
      n = half;
    } else {
      lo += half + 1;
      n -= half + 1;
    }
  }
  return lo;
}

CDX_HD void sample_point(const SampleFace& s, double u, double v, double* p) {
  for (int k = 0; k < 3; ++k) p[k] = (s.v0[k] + u * s.e1[k]) + v * s.e2[k];
}

// Unit normal of a face that has area (a square root and three divisions: the draw skips it when nobody asks).
CDX_HD void sample_normal(const SampleFace& s, double* normal) {
  const double len = sqrt(s.n2);
  for (int k = 0; k < 3; ++k) normal[k] = s.c[k] / len;
}

}  // namespace cdx
