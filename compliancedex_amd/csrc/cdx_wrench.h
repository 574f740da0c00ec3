// Batched minimum-wrench contact forces: the rule shared by the kernel (cdx_wrench.hip) and the host build
// (host_ref.cpp: cdxh_min_wrench, the CPU yardstick of that kernel).  The reference asks the same question of cvxpy /
// cvxpylayers / SCS (math_utils.py:6-57: solve_minimum_wrench, minimum_wrench_reward, compute_margin); parity with
// that solver is unpinned and not attempted: wherever zero wrench is reachable the reference's optimum is a ≥ 6-dimensional
// family of forces and SCS returns whichever member it lands on, so its forces, margins and targets are solver-defined.
//
// Problem.  Per candidate row, independent of every other row.  Inputs: tips p_i and normals n_i (i < T ≤ 8), used as
//   n̂_i = n_i / sqrt((nx² + ny²) + nz²); per call mu > 0, f_min ≥ 0, reg > 0.  r_i = p_i − mean_i(p_i),
//   c = 1/sqrt(1 + mu²).
//       minimise over F ∈ R^{T×3}:   ½‖Σ F_i‖ + ½‖Σ r_i × F_i‖ + (reg/2)·Σ‖F_i‖²
//       subject to, for every i:     n̂_i·F_i ≤ −c‖F_i‖   and   n̂_i·F_i ≤ −f_min
//   reg = 0 is the reference's problem (math_utils.py:23-27); reg > 0 picks the least-effort member of its optimal
//   family, which makes the solution unique.  Every candidate is its own problem: the reference's function is only
//   well-formed for one candidate (with E > 1 it constrains all 4E forces, puts F[0..3] alone in the objective and
//   centres on the mean of all 4E tips), and E = 1 here is that formulation.
//
// Feasible set.  With F_i = −(a·n̂_i + t), t ⟂ n̂_i, the constraints are a ≥ f_min and ‖t‖ ≤ mu·a: a truncated cone
//   C_i.  mw_project is its Euclidean projection: (a, t) onto the cone ‖t‖ ≤ mu·a — inside: kept; mu‖t‖ ≤ −a: the
//   apex; else a′ = (mu‖t‖ + a)/(1 + mu²), t′ = t·mu·a′/‖t‖ — and, if a′ < f_min, a = f_min with the ORIGINAL t clipped
//   to the radius mu·f_min.
//
// Certificate.  With G = [I … I; skew(r_1) … skew(r_T)] and g_i = (Gᵀy)_i = y_f + y_τ × r_i, for any y = (y_f, y_τ)
//   with ‖y_f‖ ≤ ½ and ‖y_τ‖ ≤ ½
//       D(y) = Σ_i [ (reg/2)‖x_i‖² + g_i·x_i ],   x_i = P_{C_i}(−g_i/reg)
//   is a lower bound of the optimum (the two norms written as maxima over the balls, min and max exchanged), and the
//   objective P(F) of a feasible F an upper bound.  The objective is reg-strongly convex, so a pair with gap
//   P − D satisfies ‖F − F*‖ ≤ sqrt(2·gap/reg).
//
// Iteration: ADMM on f(x) + g(Kx), K = [G_f; G_τ/ℓ; I], ℓ = sqrt(Σ‖r_i‖²/T) (1 if that is 0), f(x) = (reg/2)‖x‖²,
//   g(z) = ½‖z_f‖ + (ℓ/2)‖z_τ‖ + ι_C(z_x), scaled multiplier u, penalty ρ, κ = reg + ρ.  A_i = [I; skew(r_i)/ℓ] (6 × 3).
//   Start: z_x,i = P_{C_i}(0) = −f_min·n̂_i, z_f = z_τ = 0, u = 0; iters = 0; best gap = +inf.
//   S = (κ/ρ)·I₆ + Σ_i A_i·A_iᵀ = L·Lᵀ, factorised once (Woodbury: (κI + ρ·Σ A_iᵀA_i)⁻¹ = (I − Aᵀ·S⁻¹·A)/κ).
//   check(y):  F = z_x (feasible: it is a projection), gap = P(F) − D(y).  If gap < best gap: forces ← F, dual ← y,
//     best gap ← gap, best P ← P.  If best gap ≤ tol·max(1, |best P|): status 0, stop.
//   check(0).  Then, while iters < max_iters:  iters += 1;
//     b_i = ρ·((d_f + d_τ × r_i) + (z_x,i − u_x,i)),  d_f = z_f − u_f,  d_τ = (z_τ − u_τ)/ℓ
//     h = (Σ b_i, (Σ r_i × b_i)/ℓ);  w = S⁻¹·h (two substitutions);  x_i = (b_i − (w_f + (w_τ/ℓ) × r_i))/κ
//     v_f = Σ x_i + u_f,  z_f = shrink(v_f, ½/ρ),  u_f = v_f − z_f;   v_τ = (Σ r_i × x_i)/ℓ + u_τ,
//     z_τ = shrink(v_τ, (ℓ/2)/ρ),  u_τ = v_τ − z_τ;   shrink(v, t) = 0 if ‖v‖ ≤ t, else v·(1 − t/‖v‖)
//     v_i = x_i + u_x,i,  z_x,i = P_{C_i}(v_i),  u_x,i = v_i − z_x,i
//     if iters is a multiple of check_every or iters == max_iters:  check(y) with y_f = ρ·u_f, y_τ = ρ·u_τ/ℓ, each
//     scaled back onto its ball if its norm exceeds ½.
//   Leaving the loop without a certificate is status 1: the returned pair is the best one checked (the start at the
//   latest), finite and feasible.  Sums over the tips run i = 0 … T−1 left to right; a norm is sqrt((x² + y²) + z²).
//
// Outputs.  forces [T][3] and dual [6] as above; wrench = ‖ΣF‖ + ‖Σ r×F‖ (no ½ factors, no reg term:
//   math_utils.py:33-35); margin_i = (−F_i/‖F_i‖)·n̂_i − c (compute_margin), 0 for a zero force (the cone's apex, only
//   reachable with f_min = 0); gap = P − D of the returned pair; iters; status.  grad [T][3] (optional) is the partial
//   derivative of wrench with respect to the tips with F held constant, ∂‖τ‖/∂p_j = F_j × τ̂ − (1/T)·Σ_i F_i × τ̂
//   (τ = Σ r×F; 0 where ‖τ‖ is exactly 0; the net force does not depend on p) — exactly what the reference's autograd
//   delivers, whose skew matrices and normals are detached so that only torch.cross(r, solution) carries a gradient.
//   The implicit sensitivity dF*/d(p, n) is out of scope.
//   A row with a non-finite tip or normal, or a normal whose squared length is 0 or not finite, has status 2: every
//   float output NaN, iters 0.  The rule is stated for inputs whose squares and sums stay finite in float64.
//
// Storage.  Every per-row array (WrMem) is addressed as base[i·s]: s = 1 on the host, and on the device the arrays of
// the lanes of a workgroup are interleaved in LDS (s = lanes, base shifted by the lane), as in cdx_ik.h: 15T + 33
// doubles a row, no array indexed at run time lives in registers.
#pragma once
#include "cdx_hd.h"

#if defined(__HIPCC__)
#define CDX_WR_UNROLL _Pragma("unroll")
#else
#define CDX_WR_UNROLL
#endif

namespace cdx {

// Per-row storage of the solve, element i at base[i·s].
struct WrMem {
  double *n, *r, *x, *z, *u;  // 3T each: n̂, r, b (then x), z_x, u_x
  double *zw, *uw;            // 6 each: (z_f, z_τ), (u_f, u_τ)
  double* L;                  // 21: Cholesky factor of S, lower triangle row-major, the diagonal stored as 1/L_ii
  int s;
};
CDX_HD int wr_mem_doubles(int T) { return 15 * T + 33; }
CDX_HD size_t wr_mem_bytes(int T) { return (size_t)wr_mem_doubles(T) * 8; }
// The arrays of `lane` among `s` lanes in a block of wr_mem_bytes(T)·s bytes (8-byte aligned).
CDX_HD WrMem wr_mem_at(void* base, int T, int lane, int s) {
  WrMem m;
  double* d = (double*)base + lane;
  const size_t n = (size_t)(3 * T) * s;
  m.n = d;
  m.r = d + n;
  m.x = d + 2 * n;
  m.z = d + 3 * n;
  m.u = d + 4 * n;
  d += 5 * n;
  m.zw = d;
  m.uw = d + (size_t)6 * s;
  m.L = d + (size_t)12 * s;
  m.s = s;
  return m;
}

// 0, or CDX_EINVAL for a null or out-of-range parameter set.
CDX_HD int wr_params_code(const cdx_wrench_params* p) {
  if (!p) return CDX_EINVAL;
  if (p->n_tips < 1 || p->n_tips > CDX_MAX_TIPS || p->max_iters < 0 || p->check_every < 1) return CDX_EINVAL;
  const double pos[4] = {p->mu, p->reg, p->rho, p->tol};
  for (int i = 0; i < 4; ++i)
    if (!(__builtin_isfinite(pos[i]) && pos[i] > 0.0)) return CDX_EINVAL;
  if (!(__builtin_isfinite(p->min_force) && p->min_force >= 0.0)) return CDX_EINVAL;
  return CDX_OK;
}

CDX_HD double wr_norm3(const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
CDX_HD void wr_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// out = P_C(v): the projection of the force v onto the truncated friction cone of the unit normal n.
CDX_HD void mw_project(const double* v, const double* n, double mu, double fmin, double* out) {
  const double a = -((v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]);
  const double t[3] = {-v[0] - a * n[0], -v[1] - a * n[1], -v[2] - a * n[2]};
  const double tn = wr_norm3(t);
  double a2, sc;
  if (tn <= mu * a) {
    a2 = a;
    sc = 1.0;
  } else if (mu * tn <= -a) {
    a2 = 0.0;
    sc = 0.0;
  } else {
    a2 = (mu * tn + a) / (1.0 + mu * mu);
    sc = mu * a2 / tn;
  }
  if (!(a2 >= fmin)) {
    const double rad = mu * fmin;
    a2 = fmin;
    sc = tn > rad ? rad / tn : 1.0;
  }
  for (int k = 0; k < 3; ++k) out[k] = -(a2 * n[k] + sc * t[k]);
}

// P(F) of F = m.z and D(y).
CDX_HD void mw_certificate(const cdx_wrench_params& p, const WrMem& m, const double* y, double* P, double* D) {
  const int T = p.n_tips, s = m.s;
  double sf[3] = {0.0, 0.0, 0.0}, st[3] = {0.0, 0.0, 0.0}, sq = 0.0, d = 0.0;
  for (int i = 0; i < T; ++i) {
    double F[3], r[3], n[3], c[3], g[3], v[3], x[3];
    CDX_WR_UNROLL
    for (int k = 0; k < 3; ++k) {
      F[k] = m.z[(size_t)(3 * i + k) * s];
      r[k] = m.r[(size_t)(3 * i + k) * s];
      n[k] = m.n[(size_t)(3 * i + k) * s];
    }
    wr_cross(r, F, c);
    for (int k = 0; k < 3; ++k) {
      sf[k] += F[k];
      st[k] += c[k];
    }
    sq += (F[0] * F[0] + F[1] * F[1]) + F[2] * F[2];
    wr_cross(y + 3, r, c);
    for (int k = 0; k < 3; ++k) {
      g[k] = y[k] + c[k];
      v[k] = -g[k] / p.reg;
    }
    mw_project(v, n, p.mu, p.min_force, x);
    d += (0.5 * p.reg) * ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + ((g[0] * x[0] + g[1] * x[1]) + g[2] * x[2]);
  }
  *P = (0.5 * wr_norm3(sf) + 0.5 * wr_norm3(st)) + (0.5 * p.reg) * sq;
  *D = d;
}

// One row of the solve (p: passed wr_params_code).  tips / normals / forces / margin / grad: the row's [T][3] or [T]
// (grad nullable), dual [6]; returns the status.
CDX_HD int mw_row(const cdx_wrench_params& p, const double* tips, const double* normals, const WrMem& m,
                  double* forces, double* wrench, double* margin, double* dual, double* gap, int32_t* iters,
                  double* grad) {
  const int T = p.n_tips, s = m.s;
  const double rho = p.rho, kappa = p.reg + p.rho, cc = 1.0 / sqrt(1.0 + p.mu * p.mu);
  bool ok = true;
  double mean[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < T; ++i) {
    const double n[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    ok = ok && __builtin_isfinite(nn) && nn > 0.0;
    const double len = sqrt(nn);
    for (int k = 0; k < 3; ++k) {
      ok = ok && __builtin_isfinite(tips[3 * i + k]);
      mean[k] += tips[3 * i + k];
      m.n[(size_t)(3 * i + k) * s] = n[k] / len;
    }
  }
  *iters = 0;
  if (!ok) {
    for (int i = 0; i < 3 * T; ++i) {
      forces[i] = NAN;
      if (grad) grad[i] = NAN;
    }
    for (int i = 0; i < T; ++i) margin[i] = NAN;
    for (int i = 0; i < 6; ++i) dual[i] = NAN;
    *wrench = NAN;
    *gap = NAN;
    return 2;
  }
  for (int k = 0; k < 3; ++k) mean[k] = mean[k] / (double)T;
  double l2 = 0.0;
  for (int i = 0; i < T; ++i) {
    double r[3];
    for (int k = 0; k < 3; ++k) {
      r[k] = tips[3 * i + k] - mean[k];
      m.r[(size_t)(3 * i + k) * s] = r[k];
    }
    l2 += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
  }
  l2 = l2 / (double)T;
  const double ell = l2 > 0.0 ? sqrt(l2) : 1.0, il = 1.0 / ell;
  // S = (κ/ρ)·I + Σ A_i·A_iᵀ (lower triangle), then its Cholesky factor
  {
    double S[21];
    CDX_WR_UNROLL
    for (int a = 0; a < 6; ++a)
      CDX_WR_UNROLL
      for (int b = 0; b <= a; ++b) S[a * (a + 1) / 2 + b] = a == b ? kappa / rho : 0.0;
    for (int i = 0; i < T; ++i) {
      const double r[3] = {m.r[(size_t)(3 * i) * s] * il, m.r[(size_t)(3 * i + 1) * s] * il,
                           m.r[(size_t)(3 * i + 2) * s] * il};
      // rows of A_i: the identity, then skew(r/ℓ)
      const double A[6][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0},
                              {0.0, -r[2], r[1]}, {r[2], 0.0, -r[0]}, {-r[1], r[0], 0.0}};
      CDX_WR_UNROLL
      for (int a = 0; a < 6; ++a)
        CDX_WR_UNROLL
        for (int b = 0; b <= a; ++b) S[a * (a + 1) / 2 + b] += (A[a][0] * A[b][0] + A[a][1] * A[b][1]) + A[a][2] * A[b][2];
    }
    CDX_WR_UNROLL
    for (int a = 0; a < 6; ++a)
      CDX_WR_UNROLL
      for (int b = 0; b <= a; ++b) {
        double sum = S[a * (a + 1) / 2 + b];
        CDX_WR_UNROLL
        for (int k = 0; k < b; ++k) sum -= S[a * (a + 1) / 2 + k] * S[b * (b + 1) / 2 + k];
        S[a * (a + 1) / 2 + b] = a == b ? 1.0 / sqrt(sum) : sum * S[b * (b + 1) / 2 + b];
      }
    CDX_WR_UNROLL
    for (int a = 0; a < 21; ++a) m.L[(size_t)a * s] = S[a];
  }
  for (int i = 0; i < T; ++i)
    for (int k = 0; k < 3; ++k) {
      m.z[(size_t)(3 * i + k) * s] = -(p.min_force * m.n[(size_t)(3 * i + k) * s]);
      m.u[(size_t)(3 * i + k) * s] = 0.0;
    }
  for (int a = 0; a < 6; ++a) {
    m.zw[(size_t)a * s] = 0.0;
    m.uw[(size_t)a * s] = 0.0;
  }
  double best = INFINITY, bestP = 0.0;
  int it = 0, status;
  double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (;;) {
    // check(y)
    double P, D;
    mw_certificate(p, m, y, &P, &D);
    if (P - D < best) {
      best = P - D;
      bestP = P;
      for (int i = 0; i < 3 * T; ++i) forces[i] = m.z[(size_t)i * s];
      for (int a = 0; a < 6; ++a) dual[a] = y[a];
    }
    if (best <= p.tol * fmax(1.0, fabs(bestP))) {
      status = 0;
      break;
    }
    if (it >= p.max_iters) {
      status = 1;
      break;
    }
    // iterations up to the next check
    do {
      ++it;
      double df[3], dt[3], h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      CDX_WR_UNROLL
      for (int k = 0; k < 3; ++k) {
        df[k] = m.zw[(size_t)k * s] - m.uw[(size_t)k * s];
        dt[k] = (m.zw[(size_t)(3 + k) * s] - m.uw[(size_t)(3 + k) * s]) * il;
      }
      for (int i = 0; i < T; ++i) {
        double r[3], c[3], b[3];
        CDX_WR_UNROLL
        for (int k = 0; k < 3; ++k) r[k] = m.r[(size_t)(3 * i + k) * s];
        wr_cross(dt, r, c);
        CDX_WR_UNROLL
        for (int k = 0; k < 3; ++k) {
          b[k] = rho * ((df[k] + c[k]) + (m.z[(size_t)(3 * i + k) * s] - m.u[(size_t)(3 * i + k) * s]));
          m.x[(size_t)(3 * i + k) * s] = b[k];
          h[k] += b[k];
        }
        wr_cross(r, b, c);
        for (int k = 0; k < 3; ++k) h[3 + k] += c[k];
      }
      for (int k = 0; k < 3; ++k) h[3 + k] = h[3 + k] * il;
      // w = S⁻¹·h
      CDX_WR_UNROLL
      for (int a = 0; a < 6; ++a) {
        double sum = h[a];
        CDX_WR_UNROLL
        for (int k = 0; k < a; ++k) sum -= m.L[(size_t)(a * (a + 1) / 2 + k) * s] * h[k];
        h[a] = sum * m.L[(size_t)(a * (a + 1) / 2 + a) * s];
      }
      CDX_WR_UNROLL
      for (int a = 5; a >= 0; --a) {
        double sum = h[a];
        CDX_WR_UNROLL
        for (int k = a + 1; k < 6; ++k) sum -= m.L[(size_t)(k * (k + 1) / 2 + a) * s] * h[k];
        h[a] = sum * m.L[(size_t)(a * (a + 1) / 2 + a) * s];
      }
      const double wt[3] = {h[3] * il, h[4] * il, h[5] * il};
      double kf[3] = {0.0, 0.0, 0.0}, kt[3] = {0.0, 0.0, 0.0};
      for (int i = 0; i < T; ++i) {
        double r[3], n[3], c[3], x[3], v[3], z[3];
        CDX_WR_UNROLL
        for (int k = 0; k < 3; ++k) {
          r[k] = m.r[(size_t)(3 * i + k) * s];
          n[k] = m.n[(size_t)(3 * i + k) * s];
        }
        wr_cross(wt, r, c);
        CDX_WR_UNROLL
        for (int k = 0; k < 3; ++k) {
          x[k] = (m.x[(size_t)(3 * i + k) * s] - (h[k] + c[k])) / kappa;
          kf[k] += x[k];
          v[k] = x[k] + m.u[(size_t)(3 * i + k) * s];
        }
        wr_cross(r, x, c);
        for (int k = 0; k < 3; ++k) kt[k] += c[k];
        mw_project(v, n, p.mu, p.min_force, z);
        CDX_WR_UNROLL
        for (int k = 0; k < 3; ++k) {
          m.z[(size_t)(3 * i + k) * s] = z[k];
          m.u[(size_t)(3 * i + k) * s] = v[k] - z[k];
        }
      }
      CDX_WR_UNROLL
      for (int blk = 0; blk < 2; ++blk) {
        const double thr = blk == 0 ? 0.5 / rho : (0.5 * ell) / rho;
        double v[3];
        CDX_WR_UNROLL
        for (int k = 0; k < 3; ++k) v[k] = (blk == 0 ? kf[k] : kt[k] * il) + m.uw[(size_t)(3 * blk + k) * s];
        const double vn = wr_norm3(v), sc = vn <= thr ? 0.0 : 1.0 - thr / vn;
        CDX_WR_UNROLL
        for (int k = 0; k < 3; ++k) {
          const double z = v[k] * sc;
          m.zw[(size_t)(3 * blk + k) * s] = z;
          m.uw[(size_t)(3 * blk + k) * s] = v[k] - z;
        }
      }
    } while (it < p.max_iters && it % p.check_every != 0);
    // y of the iterate
    CDX_WR_UNROLL
    for (int blk = 0; blk < 2; ++blk) {
      double v[3];
      CDX_WR_UNROLL
      for (int k = 0; k < 3; ++k) v[k] = rho * m.uw[(size_t)(3 * blk + k) * s] * (blk == 0 ? 1.0 : il);
      const double vn = wr_norm3(v), sc = vn > 0.5 ? 0.5 / vn : 1.0;
      for (int k = 0; k < 3; ++k) y[3 * blk + k] = vn > 0.5 ? v[k] * sc : v[k];
    }
  }
  // outputs from the returned forces
  double sf[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < T; ++i) {
    const double F[3] = {forces[3 * i], forces[3 * i + 1], forces[3 * i + 2]};
    const double r[3] = {m.r[(size_t)(3 * i) * s], m.r[(size_t)(3 * i + 1) * s], m.r[(size_t)(3 * i + 2) * s]};
    double c[3];
    wr_cross(r, F, c);
    for (int k = 0; k < 3; ++k) {
      sf[k] += F[k];
      tau[k] += c[k];
    }
    const double fn = wr_norm3(F);
    const double dn = (F[0] * m.n[(size_t)(3 * i) * s] + F[1] * m.n[(size_t)(3 * i + 1) * s]) + F[2] * m.n[(size_t)(3 * i + 2) * s];
    margin[i] = fn > 0.0 ? -dn / fn - cc : 0.0;
  }
  const double tn = wr_norm3(tau);
  *wrench = wr_norm3(sf) + tn;
  *gap = best;
  *iters = it;
  if (grad) {
    const double th[3] = {tn > 0.0 ? tau[0] / tn : 0.0, tn > 0.0 ? tau[1] / tn : 0.0, tn > 0.0 ? tau[2] / tn : 0.0};
    double mc[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < T; ++i) {
      double c[3];
      wr_cross(forces + 3 * i, th, c);
      for (int k = 0; k < 3; ++k) {
        grad[3 * i + k] = c[k];
        mc[k] += c[k];
      }
    }
    for (int i = 0; i < T; ++i)
      for (int k = 0; k < 3; ++k) grad[3 * i + k] = grad[3 * i + k] - mc[k] / (double)T;
  }
  return status;
}

}  // namespace cdx
