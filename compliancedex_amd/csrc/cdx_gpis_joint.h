// The GPIS posterior of (f, ∂f/∂x, ∂f/∂y, ∂f/∂z) at one query: the rule shared by the kernel (cdx_gpis_joint.hip)
// and the host build (host_ref.cpp: cdxh_gpis_joint).
//   Σ(x) = P0 − WᵀW,   W = L⁻¹·[k, ∂ₓk, ∂ᵧk, ∂_z k]  (N × 4),   E11 = L·Lᵀ,
//   P0 = diag(k0, κ, κ, κ): the prior of the value and of the gradient (cross terms zero).
// Per (query x, inducing point x_j), d = x − x_j: b₀ = k, b_{1..3} = kd·d from gpis_k — the kd of the mean's
// gradient.  The output is the upper triangle of Σ, row-major: ff, fx, fy, fz, xx, xy, xz, yy, yz, zz — signed:
// far from the data the TPS and joint forms are indefinite and nothing here hides it.
#pragma once
#include "cdx_gpis.h"

namespace cdx {

constexpr int JOINT_OUT = 10;    // entries of the upper triangle
constexpr int JOINT_BLOCK = 128; // columns of L⁻ᵀ one unit of work covers (8 MFMA column tiles)
constexpr int JOINT_SPLITS = 4;  // at most this many partial sums per query

// Column blocks of a state and the number of partial sums its queries are cut into: split s takes the blocks
// s, s + S, s + 2S, …  in this order.  Both depend on N alone, so a query's sums are formed in one order whatever
// the batch it arrives in.
CDX_HD int joint_blocks(int N) { return (N + JOINT_BLOCK - 1) / JOINT_BLOCK; }
CDX_HD int joint_splits(int N) {
  const int nb = joint_blocks(N);
  return nb < JOINT_SPLITS ? nb : JOINT_SPLITS;
}

// Component c (0: k, 1..3: ∂k/∂x_c) of the query's covariance with the inducing point at distance d.  A query with a
// non-finite coordinate gets NaN in all four components (0·d is NaN exactly when d is ±inf or NaN), whatever the
// kernel's own limit at infinity is; a finite query however far is evaluated as it stands.
template <int KT, bool GENSQRT = false>
CDX_HD double gpis_joint_entry(double d0, double d1, double d2, int c, double R, double inv_s2) {
  const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
  double k, kd;
  gpis_k<KT, GENSQRT>(r2, R, inv_s2, k, kd);
  const double dc = c == 1 ? d0 : (c == 2 ? d1 : d2);
  const double poison = 0.0 * d0 + 0.0 * d1 + 0.0 * d2;
  return (c == 0 ? k : kd * dc) + poison;
}

// g[10] += the upper triangle of w·wᵀ for one whitened column w = (W_n0, W_n1, W_n2, W_n3).
CDX_HD void gpis_joint_gram(const double* w, double* g) {
  int e = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b, ++e) g[e] = fma(w[a], w[b], g[e]);
}

// Prior entry e of the upper triangle.
template <int KT>
CDX_HD double gpis_joint_prior(int e, double R, double inv_s2) {
  if (e == 0) return gpis_k0<KT>(R);
  return (e == 4 || e == 7 || e == 9) ? gpis_kappa<KT>(R, inv_s2) : 0.0;
}

}  // namespace cdx
