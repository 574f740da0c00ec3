// Batched disturbance-load test: the spring equilibrium of a compliant grasp under a dead load, the rule shared by the
// kernels (cdx_equil.hip) and the host build (host_ref.cpp: cdxh_grasp_equilibrium, cdxh_equil_reduce).  The model is the
// reference's quasi-static one (force_eq_reward, optimize_pregrasp.py:73-118): contacts stick, every fingertip is a
// spring of its own stiffness towards its target, the object settles where springs and load balance.  The reference
// evaluates it for one load only (gravity along −z, as a 2 m dummy spring, through its Kabsch with squared weights and
// unweighted centroids); here the load is any dead load and the equilibrium is solved exactly.  The reference's
// "does it stay in the hand" is a PyBullet rollout (verify_pregrasp.py:82-121); parity with it is not attempted.
//
// Problem.  Per item (e, w): grasp row e, load w; independent of every other item.  All float64.
//   Row inputs, T contacts (1 ≤ T ≤ 8): contact points p_i, spring targets g_i, stiffness k_i > 0, outward surface
//   normals n_i, used as n̂_i = n_i / sqrt((nx² + ny²) + nz²).  Item inputs: a force f (world frame, constant) acting at
//   the body-fixed point c, given in world coordinates at the nominal pose.  Per call: friction mu > 0.
//   K = Σ k_i,  o = (Σ k_i·p_i)/K (the stiffness centre),  P_i = p_i − o,  G_i = g_i − o,  C = c − o.
//   State: a rotation matrix R (row-major, start I) and a vector t (start 0).  a_i = R·P_i, b = R·C, x_i = a_i + t,
//   r_i = x_i − G_i.
//       U(R, t) = ½·Σ k_i·|r_i|² − f·(b + t)
//   Scales: ℓ = max(max_i |P_i|, |C|), 1 if that is 0;  Fs = Σ k_i·|P_i − G_i| + |f|.
//   Sums over the contacts run i = 0 … T−1 left to right; a norm is sqrt((x² + y²) + z²), a dot product
//   (x·x′ + y·y′) + z·z′; P_i and G_i are formed anew from p_i, g_i and o wherever they are used.
//
// Loop: Levenberg–Marquardt with the μ schedule of ik_lm_row (cdx_ik.h) and its accept test (every pivot > 0 and the
//   true cost falls; how the fall is evaluated is step 6), one trial per iteration.
//   μ = mu0, iters = 0.  Repeat:
//   1. g_v = Σ k_i·r_i − f,   g_ω = Σ k_i·(a_i × r_i) − b × f.
//   2. The exact Hessian in the unknowns (δω, δv) of x_i ← Cay(δω)·a_i + t + δv, lower triangle:
//        ωω: Σ k_i·((a_i·a_i)·I − a_i·a_iᵀ) + Σ k_i·(½(a_i·r_iᵀ + r_i·a_iᵀ) − (a_i·r_i)·I) − (½(b·fᵀ + f·bᵀ) − (b·f)·I)
//        vω: −[s]×, s = Σ k_i·a_i      vv: K·I
//      (the first ωω sum, vω and vv are Σ k_i·J_iᵀJ_i with J_i = [−[a_i]×, I], the Gauss–Newton matrix; the preload
//      |r_i| is of the size of the arms |a_i|, so the second-order terms are not small and Gauss–Newton alone crawls).
//      The ω rows and columns are then divided by ℓ (g̃_ω = g_ω/ℓ).
//   3. |g_v| ≤ tol·Fs and |g_ω| ≤ tol·Fs·ℓ: status 0, stop.  Else iters == max_iters: status 1, stop.
//      On either stop, stable = the Cholesky factorisation of this (undamped, scaled) Hessian has six pivots > 0.
//   4. iters += 1.  μ·K is added to the six diagonal entries; Cholesky L·Lᵀ, all six pivots written out; pd = every
//      pivot > 0.  Not pd: μ ← min(μ·ν, μ_max), next iteration.  Else δ = −(L·Lᵀ)⁻¹·(g̃_ω, g_v) by two substitutions,
//      δω = δ_ω/ℓ, δv = δ_v.
//   5. Trial point: t′ = t + δv;  R′ = Cay(δω)·R with a = ½·δω, s = (ax² + ay²) + az²,
//      Cay = ((1 − s)·I + 2·a·aᵀ + 2·[a]×)/(1 + s), entry by entry as in ik_pose_trial (cdx_ik.h): plain arithmetic, no
//      trigonometric call, no re-orthonormalisation — the drift is a few roundings per accepted step.
//   6. The change of energy ΔU = U(R′, t′) − U(R, t) is formed from the step itself, not as the difference of two
//      rounded energies (whose last place, ε·U, hides the decrease of a step once |g_v| ≲ sqrt(2·K·ε·U) — about
//      1e-8·Fs on a hand-sized grasp, which is the default tol): with D = Cay − I = (2·a·aᵀ + 2·[a]× − 2s·I)/(1 + s)
//      and d_i = D·a_i + δv = x_i′ − x_i,
//          ΔU = Σ k_i·(d_i·(r_i + ½·d_i)) − f·(D·b + δv).
//      ΔU < 0: (R, t) ← (R′, t′), μ ← max(μ/ν, μ_min).  Else μ ← min(μ·ν, μ_max).
//      The accepted energy never rises; a NaN anywhere in a trial fails the comparison and is rejected.
//
// Outputs per item.  rot [9] = R and trans [3] = (o + t) − R·o, the world convention x_i = rot·p_i + trans;
//   force_i = k_i·(G_i − x_i), the force of spring i on the object;  with m_i = R·n̂_i:
//   normal_force_i = −(force_i·m_i);  margin_i = −(force_i·m_i)/|force_i| − 1/sqrt(1 + mu²) (compute_margin's
//   definition in float64, not the reference's float32 cos_mu), 0 for a zero force;  shift = |t|, the displacement of
//   the stiffness centre;  chord = sqrt(max(3 − ((R00 + R11) + R22), 0)): for a rotation by θ, 3 − tr R = 2 − 2cos θ =
//   4·sin²(θ/2), so chord = 2·sin(θ/2), the convention of rot_err in solve_ik_frames (the subtraction from 3 leaves it
//   an absolute accuracy of about 1e-8);  stable (uint8), iters, status.
//   Status 2, float outputs NaN, stable 0, iters 0: for all W items of a row with a non-finite p, g, k or n, a k_i ≤ 0 or
//   a normal whose squared length is 0 or not finite; for one item with a non-finite f or c.
//
// Reduction per row (equil_reduce_row), over the row's W items in the order w = 0 … W−1, i = 0 … T−1:
//   worst_margin = the least margin_i over the items with status ≠ 2 (NaN if there is none; a NaN margin never wins),
//   worst_load / worst_tip its (w, i), the first in that order on a tie, −1 if none; max_shift / max_chord the largest
//   over the same items (NaN if none); n_failed the number of items that do not hold; holds = (n_failed == 0).
//   An item holds when status = 0 and stable, every margin_i > margin_min, every normal_force_i ≥ min_normal_force,
//   shift ≤ max_shift_allowed and chord ≤ max_chord_allowed (a NaN fails each of them).
//
// Storage.  The pose, its trial copy, the gradient and the 6 × 6 system (21 doubles, factored in place) are addressed by
// constants only and live in registers.  The loops over the contacts index at run time and read p, g, k straight from
// the row's inputs (global memory on the device: the lanes of a wave that share a row read the same addresses); no
// per-item array indexed at run time exists, so the kernel needs neither LDS nor scratch.
#pragma once
#include "cdx_hd.h"

#if defined(__HIPCC__)
#define CDX_EQ_UNROLL _Pragma("unroll")
#else
#define CDX_EQ_UNROLL
#endif

namespace cdx {

// 0, or CDX_EINVAL for a null or out-of-range parameter set.
CDX_HD int eq_params_code(const cdx_equil_params* p) {
  if (!p) return CDX_EINVAL;
  if (p->n_tips < 1 || p->n_tips > CDX_MAX_TIPS || p->max_iters < 0) return CDX_EINVAL;
  const double pos[6] = {p->mu, p->tol, p->mu0, p->mu_min, p->mu_max, p->nu};
  for (int i = 0; i < 6; ++i)
    if (!(__builtin_isfinite(pos[i]) && pos[i] > 0.0)) return CDX_EINVAL;
  return CDX_OK;
}

CDX_HD double eq_norm3(const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
CDX_HD double eq_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
CDX_HD void eq_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
CDX_HD void eq_rot(const double* R, const double* v, double* out) {
  CDX_EQ_UNROLL
  for (int i = 0; i < 3; ++i) out[i] = (R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2];
}

// One row's inputs and what every item of the row derives from them.
struct EqRow {
  const double *p, *g, *k;  // [T][3], [T][3], [T]
  double o[3], K, lmax, F0;  // stiffness centre, Σk, max |P_i|, Σ k_i·|P_i − G_i|
};

// Fills o, K, lmax, F0; false for a row of status 2.
CDX_HD bool eq_row_prepare(int T, const double* p, const double* g, const double* k, const double* n, EqRow* r) {
  bool ok = true;
  double K = 0.0, so[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < T; ++i) {
    const double ki = k[i];
    const double nn = (n[3 * i] * n[3 * i] + n[3 * i + 1] * n[3 * i + 1]) + n[3 * i + 2] * n[3 * i + 2];
    ok = ok && __builtin_isfinite(ki) && ki > 0.0 && __builtin_isfinite(nn) && nn > 0.0;
    K += ki;
    CDX_EQ_UNROLL
    for (int j = 0; j < 3; ++j) {
      ok = ok && __builtin_isfinite(p[3 * i + j]) && __builtin_isfinite(g[3 * i + j]);
      so[j] += ki * p[3 * i + j];
    }
  }
  r->p = p;
  r->g = g;
  r->k = k;
  r->K = K;
  CDX_EQ_UNROLL
  for (int j = 0; j < 3; ++j) r->o[j] = so[j] / K;
  double lmax = 0.0, F0 = 0.0;
  for (int i = 0; i < T; ++i) {
    const double P[3] = {p[3 * i] - r->o[0], p[3 * i + 1] - r->o[1], p[3 * i + 2] - r->o[2]};
    const double d[3] = {p[3 * i] - g[3 * i], p[3 * i + 1] - g[3 * i + 1], p[3 * i + 2] - g[3 * i + 2]};
    const double l = eq_norm3(P);
    lmax = l > lmax ? l : lmax;
    F0 += k[i] * eq_norm3(d);
  }
  r->lmax = lmax;
  r->F0 = F0;
  return ok;
}

// ΔU of the step (D, dv) from (R, t).
CDX_HD double eq_energy_change(int T, const EqRow& r, const double* f, const double* C, const double* R, const double* t,
                               const double* D, const double* dv) {
  double acc = 0.0;
  for (int i = 0; i < T; ++i) {
    const double P[3] = {r.p[3 * i] - r.o[0], r.p[3 * i + 1] - r.o[1], r.p[3 * i + 2] - r.o[2]};
    double a[3], d[3], m[3];
    eq_rot(R, P, a);
    eq_rot(D, a, d);
    CDX_EQ_UNROLL
    for (int j = 0; j < 3; ++j) {
      d[j] = d[j] + dv[j];
      m[j] = ((a[j] + t[j]) - (r.g[3 * i + j] - r.o[j])) + 0.5 * d[j];
    }
    acc += r.k[i] * eq_dot3(d, m);
  }
  double b[3], db[3];
  eq_rot(R, C, b);
  eq_rot(D, b, db);
  const double dbt[3] = {db[0] + dv[0], db[1] + dv[1], db[2] + dv[2]};
  return acc - eq_dot3(f, dbt);
}

// The Cholesky factorisation of the lower triangle A (row-major, 21 entries) in place, the diagonal stored as 1/L_aa;
// true when every pivot is > 0.
CDX_HD bool eq_cholesky(double* A) {
  bool pd = true;
  CDX_EQ_UNROLL
  for (int a = 0; a < 6; ++a)
    CDX_EQ_UNROLL
    for (int b = 0; b <= a; ++b) {
      double sum = A[a * (a + 1) / 2 + b];
      CDX_EQ_UNROLL
      for (int c = 0; c < b; ++c) sum -= A[a * (a + 1) / 2 + c] * A[b * (b + 1) / 2 + c];
      if (a == b) {
        pd = pd && sum > 0.0;
        A[a * (a + 1) / 2 + b] = 1.0 / sqrt(sum);
      } else {
        A[a * (a + 1) / 2 + b] = sum * A[b * (b + 1) / 2 + b];
      }
    }
  return pd;
}

// One item of the solve (p: passed eq_params_code; row: after eq_row_prepare, row_ok its result; n: the row's normals
// [T][3]; f, c: the item's load).  rot / trans / force may be null.  Returns the status.
CDX_HD int equil_row(const cdx_equil_params& p, const EqRow& row, bool row_ok, const double* n, const double* f,
                     const double* c, double* rot, double* trans, double* force, double* normal_force, double* margin,
                     double* shift, double* chord, uint8_t* stable, int32_t* iters) {
  const int T = p.n_tips;
  bool ok = row_ok;
  CDX_EQ_UNROLL
  for (int j = 0; j < 3; ++j) ok = ok && __builtin_isfinite(f[j]) && __builtin_isfinite(c[j]);
  if (!ok) {
    if (rot)
      for (int j = 0; j < 9; ++j) rot[j] = NAN;
    if (trans)
      for (int j = 0; j < 3; ++j) trans[j] = NAN;
    if (force)
      for (int j = 0; j < 3 * T; ++j) force[j] = NAN;
    for (int i = 0; i < T; ++i) {
      normal_force[i] = NAN;
      margin[i] = NAN;
    }
    *shift = NAN;
    *chord = NAN;
    *stable = 0;
    *iters = 0;
    return 2;
  }
  const double C[3] = {c[0] - row.o[0], c[1] - row.o[1], c[2] - row.o[2]};
  const double lc = eq_norm3(C), l0 = row.lmax > lc ? row.lmax : lc;
  const double ell = l0 > 0.0 ? l0 : 1.0, il = 1.0 / ell;
  const double Fs = row.F0 + eq_norm3(f);
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  double mu = p.mu0;
  int it = 0, status;
  bool stab;
  for (;;) {
    // gradient and Hessian at (R, t)
    double gv[3] = {0.0, 0.0, 0.0}, gw[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
    double Q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // ωω, lower triangle: 00, 10, 11, 20, 21, 22
    for (int i = 0; i < T; ++i) {
      const double ki = row.k[i];
      const double P[3] = {row.p[3 * i] - row.o[0], row.p[3 * i + 1] - row.o[1], row.p[3 * i + 2] - row.o[2]};
      double a[3], r[3], x[3];
      eq_rot(R, P, a);
      CDX_EQ_UNROLL
      for (int j = 0; j < 3; ++j) r[j] = (a[j] + t[j]) - (row.g[3 * i + j] - row.o[j]);
      eq_cross(a, r, x);
      const double aa = eq_dot3(a, a), ar = eq_dot3(a, r);
      CDX_EQ_UNROLL
      for (int j = 0; j < 3; ++j) {
        gv[j] += ki * r[j];
        gw[j] += ki * x[j];
        s[j] += ki * a[j];
      }
      CDX_EQ_UNROLL
      for (int m = 0; m < 3; ++m)
        CDX_EQ_UNROLL
        for (int q = 0; q <= m; ++q) {
          const double sym = 0.5 * (a[m] * r[q] + r[m] * a[q]) - a[m] * a[q];
          Q[m * (m + 1) / 2 + q] += ki * (m == q ? (aa - ar) + sym : sym);
        }
    }
    double b[3], x[3];
    eq_rot(R, C, b);
    eq_cross(b, f, x);
    const double bf = eq_dot3(b, f);
    CDX_EQ_UNROLL
    for (int j = 0; j < 3; ++j) {
      gv[j] = gv[j] - f[j];
      gw[j] = gw[j] - x[j];
    }
    CDX_EQ_UNROLL
    for (int m = 0; m < 3; ++m)
      CDX_EQ_UNROLL
      for (int q = 0; q <= m; ++q) {
        const double sym = 0.5 * (b[m] * f[q] + f[m] * b[q]);
        Q[m * (m + 1) / 2 + q] = Q[m * (m + 1) / 2 + q] - (m == q ? sym - bf : sym);
      }
    // the scaled system, lower triangle row-major over (ω0, ω1, ω2, v0, v1, v2)
    const double il2 = il * il;
    double A[21] = {Q[0] * il2,
                    Q[1] * il2, Q[2] * il2,
                    Q[3] * il2, Q[4] * il2, Q[5] * il2,
                    0.0, s[2] * il, -s[1] * il, row.K,
                    -s[2] * il, 0.0, s[0] * il, 0.0, row.K,
                    s[1] * il, -s[0] * il, 0.0, 0.0, 0.0, row.K};
    const double h[6] = {gw[0] * il, gw[1] * il, gw[2] * il, gv[0], gv[1], gv[2]};
    const bool conv = eq_norm3(gv) <= p.tol * Fs && eq_norm3(gw) <= (p.tol * Fs) * ell;
    if (conv || it >= p.max_iters) {
      status = conv ? 0 : 1;
      stab = eq_cholesky(A);
      break;
    }
    ++it;
    const double damp = mu * row.K;
    CDX_EQ_UNROLL
    for (int a = 0; a < 6; ++a) A[a * (a + 1) / 2 + a] += damp;
    bool accept = false;
    double Rn[9], tn[3];
    if (eq_cholesky(A)) {
      double d[6];
      CDX_EQ_UNROLL
      for (int a = 0; a < 6; ++a) {
        double sum = -h[a];
        CDX_EQ_UNROLL
        for (int q = 0; q < a; ++q) sum -= A[a * (a + 1) / 2 + q] * d[q];
        d[a] = sum * A[a * (a + 1) / 2 + a];
      }
      CDX_EQ_UNROLL
      for (int a = 5; a >= 0; --a) {
        double sum = d[a];
        CDX_EQ_UNROLL
        for (int q = a + 1; q < 6; ++q) sum -= A[q * (q + 1) / 2 + a] * d[q];
        d[a] = sum * A[a * (a + 1) / 2 + a];
      }
      CDX_EQ_UNROLL
      for (int j = 0; j < 3; ++j) tn[j] = t[j] + d[3 + j];
      const double a[3] = {0.5 * (d[0] * il), 0.5 * (d[1] * il), 0.5 * (d[2] * il)};
      const double ss = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], den = 1.0 + ss, one = 1.0 - ss;
      const double Cy[9] = {(one + 2.0 * (a[0] * a[0])) / den,        (2.0 * (a[0] * a[1]) - 2.0 * a[2]) / den,
                            (2.0 * (a[0] * a[2]) + 2.0 * a[1]) / den, (2.0 * (a[1] * a[0]) + 2.0 * a[2]) / den,
                            (one + 2.0 * (a[1] * a[1])) / den,        (2.0 * (a[1] * a[2]) - 2.0 * a[0]) / den,
                            (2.0 * (a[2] * a[0]) - 2.0 * a[1]) / den, (2.0 * (a[2] * a[1]) + 2.0 * a[0]) / den,
                            (one + 2.0 * (a[2] * a[2])) / den};
      const double Dm[9] = {(2.0 * (a[0] * a[0]) - 2.0 * ss) / den,   Cy[1], Cy[2], Cy[3],
                            (2.0 * (a[1] * a[1]) - 2.0 * ss) / den,   Cy[5], Cy[6], Cy[7],
                            (2.0 * (a[2] * a[2]) - 2.0 * ss) / den};
      CDX_EQ_UNROLL
      for (int m = 0; m < 3; ++m)
        CDX_EQ_UNROLL
        for (int q = 0; q < 3; ++q)
          Rn[3 * m + q] = (Cy[3 * m] * R[q] + Cy[3 * m + 1] * R[3 + q]) + Cy[3 * m + 2] * R[6 + q];
      accept = eq_energy_change(T, row, f, C, R, t, Dm, d + 3) < 0.0;
    }
    if (accept) {
      CDX_EQ_UNROLL
      for (int j = 0; j < 9; ++j) R[j] = Rn[j];
      CDX_EQ_UNROLL
      for (int j = 0; j < 3; ++j) t[j] = tn[j];
      mu = mu / p.nu;
      mu = mu > p.mu_min ? mu : p.mu_min;
    } else {
      mu = mu * p.nu;
      mu = mu < p.mu_max ? mu : p.mu_max;
    }
  }
  // outputs at (R, t)
  const double cc = 1.0 / sqrt(1.0 + p.mu * p.mu);
  for (int i = 0; i < T; ++i) {
    const double ki = row.k[i];
    const double P[3] = {row.p[3 * i] - row.o[0], row.p[3 * i + 1] - row.o[1], row.p[3 * i + 2] - row.o[2]};
    const double nv[3] = {n[3 * i], n[3 * i + 1], n[3 * i + 2]};
    const double len = eq_norm3(nv);
    const double nh[3] = {nv[0] / len, nv[1] / len, nv[2] / len};
    double a[3], m[3], F[3];
    eq_rot(R, P, a);
    eq_rot(R, nh, m);
    CDX_EQ_UNROLL
    for (int j = 0; j < 3; ++j) F[j] = ki * ((row.g[3 * i + j] - row.o[j]) - (a[j] + t[j]));
    const double dn = eq_dot3(F, m), fn = eq_norm3(F);
    normal_force[i] = -dn;
    margin[i] = fn > 0.0 ? -dn / fn - cc : 0.0;
    if (force)
      for (int j = 0; j < 3; ++j) force[3 * i + j] = F[j];
  }
  if (rot)
    for (int j = 0; j < 9; ++j) rot[j] = R[j];
  if (trans) {
    double Ro[3];
    eq_rot(R, row.o, Ro);
    for (int j = 0; j < 3; ++j) trans[j] = (row.o[j] + t[j]) - Ro[j];
  }
  *shift = eq_norm3(t);
  const double ch = 3.0 - ((R[0] + R[4]) + R[8]);
  *chord = sqrt(ch > 0.0 ? ch : 0.0);
  *stable = stab ? 1 : 0;
  *iters = it;
  return status;
}

// The reduction of one row: its W items' margin / normal_force [W][T], shift / chord / stable / status [W].
CDX_HD void equil_reduce_row(int64_t W, int T, const double* margin, const double* normal_force, const double* shift,
                             const double* chord, const uint8_t* stable, const int32_t* status,
                             const cdx_equil_limits& lim, double* worst_margin, int32_t* worst_load,
                             int32_t* worst_tip, double* max_shift, double* max_chord, int32_t* n_failed,
                             uint8_t* holds) {
  double wm = NAN, ms = NAN, mc = NAN;
  int32_t wl = -1, wt = -1, nf = 0;
  for (int64_t w = 0; w < W; ++w) {
    const int32_t st = status[w];
    bool hold = st == 0 && stable[w] != 0 && shift[w] <= lim.max_shift && chord[w] <= lim.max_chord;
    for (int i = 0; i < T; ++i) {
      const double m = margin[w * T + i];
      hold = hold && m > lim.margin_min && normal_force[w * T + i] >= lim.min_normal_force;
      if (st != 2 && (m < wm || (wl < 0 && m == m))) {
        wm = m;
        wl = (int32_t)w;
        wt = i;
      }
    }
    if (st != 2) {
      ms = (shift[w] > ms || ms != ms) ? shift[w] : ms;
      mc = (chord[w] > mc || mc != mc) ? chord[w] : mc;
    }
    nf += hold ? 0 : 1;
  }
  *worst_margin = wm;
  *worst_load = wl;
  *worst_tip = wt;
  *max_shift = ms;
  *max_chord = mc;
  *n_failed = nf;
  *holds = nf == 0 ? 1 : 0;
}

}  // namespace cdx
