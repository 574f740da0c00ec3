// Approach trajectories: the CHOMP rule shared by the kernels (cdx_traj.hip) and the host build (host_ref.cpp:
// cdxh_traj_seed / cdxh_traj_step, the CPU yardstick of those kernels).  The reference leaves this to cuRobo's
// MotionGen (traj_gen.py); parity with it is not attempted.  Both builds compile this header without FMA contraction,
// and it calls no libm function.
//
// A row is q[T][D] float64, q[0] and q[T−1] fixed, the n = T − 2 interior waypoints the unknowns.
//   Smooth   virtual points q[−1] = q[0], q[T] = q[T−1] (rest to rest);  a_t = (q[t−1] − 2·q[t]) + q[t+1], t = 0…T−1;
//            U_s = ½·Σ_d Σ_t a_t,d²;  ∂U_s/∂q[t] = (a_{t−1} − 2·a_t) + a_{t+1} on the interior.  Per joint its Hessian
//            in the unknowns is the n×n Toeplitz pentadiagonal A_T = [1 −4 6 −4 1], symmetric positive definite.
//   Limits   on the interior:  p = max(q − (upper − m_lim), 0) − max((lower + m_lim) − q, 0);  U_l = ½·Σ p²;  ∂ = p.
//            (The endpoints are given: their hinges would add a constant.)  ±inf bounds switch a side off.
//   Collide  U_c = Σ_t cost_t over all T waypoints, t ascending, one accumulator;  ∂U_c/∂q[t] = g_c[t] on the interior.
//   Total    U = (w_s·U_s + w_c·U_c) + w_l·U_l;   g = (w_s·∂U_s + w_c·g_c) + w_l·p.
//   Step     per joint solve A_T·x = g by the LDLᵀ factors of traj_factor (no pivoting, O(n)): forward
//            y_i = (g_i − e_i·y_{i−1}) − f_i·y_{i−2}, z_i = y_i / d_i, backward x_i = (z_i − e_{i+1}·x_{i+1}) − f_{i+2}·x_{i+2};
//            then q[t] ← q[t] − step·x_{t−1}.
//   Best     U is the cost of the iterate the step starts from; it replaces the row's best when U < best (strict, so a
//            NaN never wins), and the row BEFORE the step is what is kept.
//   Sums     lane d owns joint d and adds over t ascending; the D lane sums are joined by the tree x[l] += x[l + off],
//            off = 16, 8, 4, 2, 1, over CDX_TRAJ_LANES = 32 slots (slots ≥ D hold 0), as cdx_hand.h joins its lanes; the
//            ½ is applied to the joined sum.
//   Bad rows a non-finite value anywhere in q, g_c or cost_t: the interior and the three costs become NaN, best stays.
//   Seed     row (g, s), joint d:  i = (g·seeds + s)·D + d;  r = Philox4x32-10(counter (i lo, i hi, 0, 0), key (seed lo,
//            seed hi));  U01 = (r0 + 0.5)·2⁻³²;  a_d = s == 0 ? 0 : amp·(2·U01 − 1);  u = t / (T − 1);  w = u·(1 − u);
//            q[t] = (q_start + u·(q_goal − q_start)) + a_d·(16·(w·w)) for 0 < t < T − 1, q[0] = q_start, q[T−1] = q_goal.
//            The bump 16u²(1−u)² has zero value and slope at both ends and is 1 in the middle.
#pragma once
#include "cdx_hd.h"
#include "cdx_sample.h"

namespace cdx {

CDX_HD bool traj_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }  // false for NaN and ±inf

// LDLᵀ of A_T (n = T − 2 unknowns): A = L·D·Lᵀ, L unit lower triangular with sub-diagonals e (L[i][i−1]) and f
// (L[i][i−2]).  e[0], f[0], f[1] are 0.  Filled on the host by both builds and handed to the row code by value.
struct TrajFactor {
  double d[CDX_TRAJ_MAX_T - 2], e[CDX_TRAJ_MAX_T - 2], f[CDX_TRAJ_MAX_T - 2];
};

inline void traj_factor(int n, TrajFactor* F) {
  for (int i = 0; i < CDX_TRAJ_MAX_T - 2; ++i) F->d[i] = F->e[i] = F->f[i] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double fi = i >= 2 ? 1.0 / F->d[i - 2] : 0.0;
    double ei = 0.0;
    if (i >= 1) ei = (i >= 2 ? -4.0 - (fi * F->d[i - 2]) * F->e[i - 1] : -4.0) / F->d[i - 1];
    double di = 6.0;
    if (i >= 1) di -= (ei * ei) * F->d[i - 1];
    if (i >= 2) di -= (fi * fi) * F->d[i - 2];
    F->d[i] = di;
    F->e[i] = ei;
    F->f[i] = fi;
  }
}

CDX_HD int traj_shape_code(int32_t T, int32_t D) {
  return (T < 3 || T > CDX_TRAJ_MAX_T || D < 1 || D > CDX_MAX_DOFS) ? CDX_EINVAL : CDX_OK;
}

CDX_HD int traj_params_code(const cdx_traj_params* p) {
  if (!p) return CDX_EINVAL;
  if (traj_shape_code(p->T, p->n_dofs)) return CDX_EINVAL;
  for (int d = 0; d < p->n_dofs; ++d)
    if (!(p->lower[d] <= p->upper[d])) return CDX_EINVAL;  // (a NaN bound fails the comparison)
  if (!traj_finite(p->w_smooth) || !traj_finite(p->w_col) || !traj_finite(p->w_lim) || !traj_finite(p->m_lim) ||
      !traj_finite(p->step))
    return CDX_EINVAL;
  return CDX_OK;
}

CDX_HD int traj_step_code(const cdx_traj_params* p, int64_t E, const double* traj, const double* g_c,
                          const double* cost_t, const double* cost, const double* best_cost, const int32_t* best_iter,
                          const double* best_traj) {
  const int rc = traj_params_code(p);
  if (rc) return rc;
  if (E < 0 || E > 0x7fffffff || (g_c == nullptr) != (cost_t == nullptr)) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!traj || !cost || !best_cost || !best_iter || !best_traj) return CDX_EINVAL;
  return CDX_OK;
}

CDX_HD int traj_seed_code(int64_t G, int32_t seeds, int32_t T, int32_t D, const double* q_start, const double* q_goal,
                          double amp, const double* traj) {
  if (traj_shape_code(T, D) || seeds < 1 || G < 0 || !traj_finite(amp)) return CDX_EINVAL;
  if (G * (int64_t)seeds > 0x7fffffff) return CDX_EINVAL;
  if (G == 0) return CDX_OK;
  if (!q_start || !q_goal || !traj) return CDX_EINVAL;
  return CDX_OK;
}

CDX_HD double traj_hinge(double x) { return x > 0.0 ? x : 0.0; }

// Joint d of a row, first half: q and x are the row's [T][D] arrays (x holds g_c on entry; the caller zero-fills it
// without a collision term).  Leaves the gradient g in x[t][d] for the interior t, returns the lane's Σ a² in *us and
// Σ p² in *ul, and false if a value it read was not finite.
CDX_HD bool traj_gradient_column(const cdx_traj_params& P, int d, const double* q, double* x, double* us, double* ul) {
  const int T = P.T, D = P.n_dofs;
  const double hi = P.upper[d] - P.m_lim, lo = P.lower[d] + P.m_lim;
  bool ok = true;
  // accelerations with the virtual points: a_prev = a_{t−1}, a_cur = a_t, a_next = a_{t+1}
  double qm = q[d], qc = q[d], qp = q[D + d];
  double a_prev = 0.0, a_cur = (qm - 2.0 * qc) + qp;
  double s2 = a_cur * a_cur, l2 = 0.0;
  ok = ok && traj_finite(qc) && traj_finite(x[d]);
  for (int t = 1; t < T; ++t) {
    qm = qc;
    qc = qp;
    qp = q[(t + 1 < T ? t + 1 : T - 1) * D + d];
    const double a_next = (qm - 2.0 * qc) + qp;  // a_t
    s2 += a_next * a_next;
    ok = ok && traj_finite(qc) && traj_finite(x[t * D + d]);
    if (t >= 2) {  // the gradient at t − 1 needs a_{t−2}, a_{t−1}, a_t
      const int k = t - 1;
      const double qk = qm;
      const double p = traj_hinge(qk - hi) - traj_hinge(lo - qk);
      l2 += p * p;
      const double gs = (a_prev - 2.0 * a_cur) + a_next;
      x[k * D + d] = (P.w_smooth * gs + P.w_col * x[k * D + d]) + P.w_lim * p;
    }
    a_prev = a_cur;
    a_cur = a_next;
  }
  *us = s2;
  *ul = l2;
  return ok;
}

// Second half: x[t][d] ← (A_T⁻¹·x[·][d])_t on the interior.  The forward pass carries y in registers and leaves
// z_i = y_i / d_i behind; the backward pass turns z into the solution.
CDX_HD void traj_solve_column(const cdx_traj_params& P, const TrajFactor& F, int d, double* x) {
  const int D = P.n_dofs, n = P.T - 2;
  double y1 = 0.0, y2 = 0.0;  // y_{i−1}, y_{i−2}
  for (int i = 0; i < n; ++i) {
    const double y = (x[(i + 1) * D + d] - F.e[i] * y1) - F.f[i] * y2;
    x[(i + 1) * D + d] = y / F.d[i];
    y2 = y1;
    y1 = y;
  }
  double x1 = 0.0, x2 = 0.0;  // x_{i+1}, x_{i+2}
  for (int i = n - 1; i >= 0; --i) {
    const double e1 = i + 1 < n ? F.e[i + 1] : 0.0, f2 = i + 2 < n ? F.f[i + 2] : 0.0;
    const double xi = (x[(i + 1) * D + d] - e1 * x1) - f2 * x2;
    x[(i + 1) * D + d] = xi;
    x2 = x1;
    x1 = xi;
  }
}

CDX_HD bool traj_column(const cdx_traj_params& P, const TrajFactor& F, int d, const double* q, double* x, double* us,
                        double* ul) {
  const bool ok = traj_gradient_column(P, d, q, x, us, ul);
  traj_solve_column(P, F, d, x);
  return ok;
}

// U_c: Σ cost_t, t ascending; false if a cost is not finite.  cost_t nullptr: 0.
CDX_HD bool traj_collision_sum(const double* cost_t, int T, double* uc) {
  double s = 0.0;
  bool ok = true;
  for (int t = 0; cost_t && t < T; ++t) {
    ok = ok && traj_finite(cost_t[t]);
    s += cost_t[t];
  }
  *uc = s;
  return ok;
}

CDX_HD double traj_total(const cdx_traj_params& P, double us, double uc, double ul) {
  return (P.w_smooth * us + P.w_col * uc) + P.w_lim * ul;
}

CDX_HD double traj_moved(const cdx_traj_params& P, double q, double x, bool bad) {
  return bad ? (double)NAN : q - P.step * x;
}

// One row on the host, in the kernel's order.
inline void traj_step_row(const cdx_traj_params& P, const TrajFactor& F, double* traj, const double* g_c,
                          const double* cost_t, int32_t iteration, double* cost, double* best_cost, int32_t* best_iter,
                          double* best_traj) {
  const int T = P.T, D = P.n_dofs;
  double x[CDX_TRAJ_MAX_T * CDX_MAX_DOFS], rs[CDX_TRAJ_LANES], rl[CDX_TRAJ_LANES];
  for (int i = 0; i < T * D; ++i) x[i] = g_c ? g_c[i] : 0.0;
  bool ok = true;
  for (int l = 0; l < CDX_TRAJ_LANES; ++l) {
    rs[l] = rl[l] = 0.0;
    if (l < D) ok = traj_column(P, F, l, traj, x, rs + l, rl + l) && ok;
  }
  double uc;
  ok = traj_collision_sum(cost_t, T, &uc) && ok;
  for (int off = CDX_TRAJ_LANES / 2; off; off >>= 1)
    for (int l = 0; l < off; ++l) {
      rs[l] += rs[l + off];
      rl[l] += rl[l + off];
    }
  const double us = 0.5 * rs[0], ul = 0.5 * rl[0];
  const bool bad = !ok;
  cost[0] = bad ? (double)NAN : us;
  cost[1] = bad ? (double)NAN : uc;
  cost[2] = bad ? (double)NAN : ul;
  const double U = traj_total(P, us, uc, ul);
  if (!bad && U < *best_cost) {
    *best_cost = U;
    *best_iter = iteration;
    for (int i = 0; i < T * D; ++i) best_traj[i] = traj[i];
  }
  for (int i = D; i < (T - 1) * D; ++i) traj[i] = traj_moved(P, traj[i], x[i], bad);
}

// a_d of the seed rule.
CDX_HD double traj_seed_amp(uint64_t seed, int64_t row, int32_t s, int32_t D, int32_t d, double amp) {
  if (s == 0) return 0.0;
  const uint64_t i = (uint64_t)row * (uint64_t)D + (uint64_t)d;
  uint32_t r[4];
  philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const double u01 = ((double)r[0] + 0.5) * 0x1p-32;
  return amp * (2.0 * u01 - 1.0);
}

CDX_HD double traj_seed_value(double qs, double qg, double a, int t, int T, bool bad) {
  if (bad) return (double)NAN;
  if (t == 0) return qs;
  if (t == T - 1) return qg;
  const double u = (double)t / (double)(T - 1), w = u * (1.0 - u);
  return (qs + u * (qg - qs)) + a * (16.0 * (w * w));
}

inline void traj_seed_row(int64_t row, int32_t s, int32_t T, int32_t D, const double* qs, const double* qg, double amp,
                          uint64_t seed, double* out) {
  bool bad = false;
  for (int d = 0; d < D; ++d) bad = bad || !traj_finite(qs[d]) || !traj_finite(qg[d]);
  for (int d = 0; d < D; ++d) {
    const double a = traj_seed_amp(seed, row, s, D, d, amp);
    for (int t = 0; t < T; ++t) out[t * D + d] = traj_seed_value(qs[d], qg[d], a, t, T, bad);
  }
}

}  // namespace cdx
