// Fingertip Jacobians and batched inverse kinematics: the rule shared by the kernels (cdx_ik.hip) and the host build
// (host_ref.cpp: cdxh_fk_jacobian, cdxh_ik_solve, cdxh_ik_solve_pose, cdxh_ik_solve_frames, the CPU yardsticks of those
// kernels).  The
// reference turns fingertips back into a hand pose with PyBullet's calculateInverseKinematics (verify_pregrasp.py:50-53,
// bullet_robot.py:262-280) and has compute_endeffector_jacobian (robot_model.py:643-683); parity with PyBullet's solver
// is unpinned.
//
// Jacobian.  For tip k of the chain at joint row q (float32), with p the tip position of cdx_fk_forward (offset
//   included), and for every moving joint j on the tip's path its world axis ω_j = R_parent·F_j·e_axis and world
//   origin o_j (what fk_tip_walk3s keeps):
//     lin[:, dof_j] = sign_j · ω_j × (p − o_j),   ang[:, dof_j] = sign_j · ω_j        (robot_model.py:677-678)
//   all in float32 with the functions of the FK kernels (chain_step, tip_from_pose); the columns of joints off the
//   path are exactly 0.  Two walks of the path: the first gives p, the second the columns — no per-level storage.
//   This is the TRUE derivative of the fingertip position.  It is deliberately NOT cdx_fk_backward's, which
//   reproduces the reference autograd's detached quaternion scale (cdx_fk.h) and so differs wherever a tip offset is
//   set.
//
// Inverse kinematics.  Per candidate row, independent of every other row.  Inputs: q0 [D] (float64, or float32
//   widened), target [T][3], palm [6] = position + XYZ Euler angles (null: identity), w [T] (null: all 1), and per call
//   palm_offset [3] and cdx_ik_params.  A row with a non-finite q0 (as given or rounded to float32), target, palm or w
//   has status 2: its q is q0 unchanged, its err NaN, its iters 0.  w ≥ 0 is the caller's contract and is not checked.
//   Fingertips.  tip_k(q) = (Rp·double(FK_f32(q)_k) + palm_pos) + palm_offset, Rp = euler_xyz(palm[3:6]) in float64
//     (cdx_cost.h), the products summed left to right.  d_k = target_k − tip_k, e_k = sqrt((dx² + dy²) + dz²),
//     r_k = w_k·d_k, cost(q) = ½·Σ_k ((rx² + ry²) + rz²) + ½·ρ·Σ_d (q_d − ref_d)², emax = max_k w_k·e_k.
//   Bounds.  lower / upper are rounded INWARD to float32 once (ik_prepare), so a float32 q never leaves the float64 box;
//     if that crosses them (lower == upper not a float32) both become float(lower).  q ← clamp(float(q0)).
//   Loop, with μ = mu0 and iters = 0:
//     if emax ≤ tol: status 0, stop.   if iters == max_iters: status 1, stop.   iters += 1.
//     Jl [3T × D] = lin of every tip at q, widened.  The weighted world Jacobian is Jw = diag(w)·blockdiag(Rp)·Jl; Rp is
//       orthogonal and w is constant per tip, so Jw·Jwᵀ + κI = blockdiag(Rp)·(W·Jl·Jlᵀ·W + κI)·blockdiag(Rp)ᵀ and the
//       whole step is taken in the palm frame with u_k = w_k·Rpᵀ·r_k: the same step up to rounding, Jl kept as the
//       float32 it is.
//     g_d = Σ_rows Jl[row][d]·u[row] + ρ·(ref_d − q_d).
//     A joint with q_d ≤ lower_d and g_d < 0, or q_d ≥ upper_d and g_d > 0, is fixed for this step: g_d = 0 and column d
//       of Jl is zeroed.
//     κ = μ + ρ.  A = W·Jl·Jlᵀ·W + κI (3T × 3T, lower triangle, A_ab = (w_a·w_b)·Σ_d Jl[a][d]·Jl[b][d]);
//       b_a = w_a·Σ_d Jl[a][d]·g_d;  A = L·Lᵀ by Cholesky (row by row), y = A⁻¹·b by two substitutions;
//       δ_d = (g_d − Σ_a Jl[a][d]·(w_a·y_a)) / κ — the damped step (JwᵀJw + κI)⁻¹·g through the 3T × 3T system.
//     q′_d = float(clamp(double(q_d) + δ_d, lower_d, upper_d)).
//     Accepted if every pivot was > 0 and cost(q′) < cost(q): q ← q′, μ ← max(μ/ν, μ_min).  Else μ ← min(μ·ν, μ_max).
//     The accepted cost never rises.
//   Outputs: q (float32 values), err_k = e_k at the returned q (unweighted), iters, status.
//
// Free-wrist inverse kinematics (ik_pose_row).  The same solve with the palm's rigid pose an unknown next to the joints:
//   per row, independent of every other row.  State: q float32 [D] clamped as above, pp double [3], Rp double [9]
//   (row-major).  Inputs as above without `palm`, plus palm0_pos [3] / palm0_rot [9] (both or neither).  A row with a
//   non-finite q0, target, w, palm0_pos or palm0_rot has status 2: q = q0, NaN in palm_pos / palm_rot / err, iters 0.
//   Fingertips, residuals, cost, emax: exactly ik_eval's with the current (Rp, pp):
//     tip_k = (Rp·double(FK_f32(q)_k) + pp) + palm_offset.  The pose carries no cost term of its own.
//   Start.  With palm0_pos / palm0_rot: (pp, Rp) are those values as they are — an orthogonal palm0_rot is the caller's
//     contract, nothing re-orthonormalises it.  Without: the weighted Kabsch fit of the start's own fingertips onto the
//     targets.  v_k = double(FK_f32(q)_k) at the clamped q0, t_k = target_k − palm_offset, W = Σ_k w_k (k ascending),
//     c_v = (Σ w_k·v_k)/W, c_t = (Σ w_k·t_k)/W, H = Σ_k (w_k·(v_k − c_v))·(t_k − c_t)ᵀ,
//     Rp = kabsch_rotation<double>(H, zero noise) = V·diag(1, 1, d)·Uᵀ of H = U·S·Vᵀ (cdx_cost.h), which takes v onto t,
//     pp = c_t − Rp·c_v.  Fallback — fewer than three tips with w_k > 0, W not > 0, or a non-finite entry in Rp —:
//     Rp = I, pp = c_t − c_v, and pp = 0 where W is not > 0.
//   No trigonometric function is called anywhere in the row: the pose is a matrix from start to end.
//   Loop: the fixed-palm loop with D′ = D + 6 columns.  The step's unknowns are (δq [D], t_b [3], ω_b [3]), the pose
//     increment written in the PALM frame, so the step stays the palm-frame step above: rows 3k..3k+2 of Jl gain six
//     float32 columns after the joint columns, t_b: I₃, ω_b: −[v_k]× = [[0, vz, −vy], [−vz, 0, vx], [vy, −vx, 0]] with v_k
//     the float32 FK tip — exact entries.  u as above.
//     g_d for d < D as above (ρ term, bounds);  g_d = Σ_rows Jl[row][d]·u[row] for the six pose columns: no ρ term, and
//       a pose column is never fixed on a bound.
//     κ = μ + ρ damps all D′ columns.  On the pose columns ρ is a step damping only (it shortens the step as it does the
//       joints'), never a pull towards a rest pose.  A, b, the Cholesky, the substitutions and δ [D′] as above.
//     Trial point: q′ as above;  pp′ = pp + Rp·t_b;  with a = ½·ω_b, s = (ax² + ay²) + az², the Cayley rotation
//       C = ((1 − s)·I + 2·a·aᵀ + 2·[a]×)/(1 + s), entry by entry C_ii = ((1 − s) + 2·a_i²)/(1 + s),
//       C_ij = (2·a_i·a_j ∓ 2·a_k)/(1 + s) (− for ij = 01, 12, 20) — plain arithmetic, orthogonal before rounding;
//       Rp′ = Rp·C (mat3_mul).  No re-orthonormalisation: the drift is a few roundings per ACCEPTED step.
//     Accepted as above (every pivot > 0 and cost(q′, Rp′, pp′) < cost): (q, Rp, pp) ← (q′, Rp′, pp′).  The μ schedule,
//       the stop tests and the statuses are the fixed-palm ones.
//   Outputs: q, palm_pos = pp, palm_rot = Rp, err (unweighted, at the returned q and pose), iters, status.
//   The pose and its trial copy (2 × 12 doubles) are indexed by constants only and live in registers.
//
// Pose targets and held joints (frame_ik_row).  The fixed-palm solve (ik_row) with two additions; whatever is not named
//   here is ik_row's: the start, the bounds rounded inward, the μ schedule, the accept test on the true cost, the
//   statuses.  Per call (64-bit words at the C ABI, 32 bits here once checked): rot_mask (bit k: tip k carries
//   orientation rows) and dof_mask (bit d: joint d is solved).  Per row besides ik_row's inputs (`palm` is the pose of
//   the chain's root — for an arm its base): target_rot [T][9]
//   (row-major, world frame; an orthogonal matrix is the caller's contract; may be null where rot_mask is 0) and wr [T]
//   in metres per radian, ≥ 0 (null: all 0.1).  A non-finite entry anywhere in target_rot or wr gives status 2 as well,
//   and rot_err is then NaN like err.
//   Target quaternions.  Once per row, for every tip in rot_mask: Rt′ = Rpᵀ·Rt (the products summed as mat3_mul's) becomes
//     a unit quaternion t (xyzw) in float64 by Shepperd's rule (shepperd_quat: the branch on the largest of the trace and
//     the three diagonal entries, ties to the first; one sqrt, no trigonometric function).
//   Orientation residual, at every evaluation: the FK's float32 quaternion c of the tip's link, widened, divided by its
//     float64 norm sqrt(((x² + y²) + z²) + w²);  e = t ⊗ conj(c):
//       e_w = ((t_w·c_w + t_x·c_x) + t_y·c_y) + t_z·c_z,   e_xyz = (c_w·t_v − t_w·c_v) − t_v × c_v;
//     ρ_k = 2·s·e_xyz with s = −1 if e_w < 0, else +1: the rotation vector from the current onto the target frame in the
//     root's frame, of length 2·sin(θ/2);  rot_err_k = sqrt((ρx² + ρy²) + ρz²), a chord ≤ 2.
//     cost = ½·(Σ_k |w_k·d_k|² + Σ_{k∈mask} |wr_k·ρ_k|²) + ½·ρ·Σ_{d∈dof_mask} (q_d − ref_d)²,
//     emax = max(max_k w_k·e_k, max_{k∈mask} wr_k·rot_err_k): the one tol stops both, wr carrying the units.
//   Rows.  M = 3T + 3·popcount(rot_mask), packed: the 3T position rows, then three rows per tip of the mask in tip order,
//     holding the tip's float32 `ang` columns (fk_tip_columns) as they are — the exact Jacobian of ρ at θ = 0, a
//     Gauss–Newton model elsewhere; the accept test keeps the cost from rising.  Row weights: w_k on a position row,
//     wr_k on an orientation row.  y (ik_row's u) is w_k·Rpᵀ·(w_k·d_k) on the position rows and wr_k·(wr_k·ρ_k) on the
//     orientation rows (ρ is already in the root's frame).  g, A, b, the Cholesky, the substitutions, δ and the trial
//     point are ik_row's with M for 3T and these row weights.
//   Held joints.  A joint outside dof_mask keeps clamp(float(q0_d)) to the end: in every iteration its column of Jl is
//     zeroed and g_d = 0 (as for a joint fixed on a bound), its trial value is its value, and it is left out of the
//     rest-pose sum of the cost and of g.
//   With rot_mask = 0 and every joint in dof_mask the row is ik_row's bit for bit.
//   Outputs: q, err, rot_err [T] (the chord; 0 for a tip outside rot_mask), iters, status.
//
// One loop.  The three solves are ik_lm_row<V>, written once; a variant V (IkFixed, IkPose, IkFrames) is two
// compile-time flags, and everything stated above as a variant's own sits behind `if constexpr (V::pose)` or
// `if constexpr (V::frames)` there and in ik_eval<V>.  ik_row, ik_pose_row and frame_ik_row name their inputs and call it.
//
// Storage.  One layout (ik_mem_at<V>) over n rows and Dc columns: n = 3T and Dc = D for the fixed palm, Dc = D + 6 for
// the free wrist, n = M for pose targets.  Doubles: A [n(n+1)/2] (lower triangle, row-major), g [Dc], y [n], dv [2n]
// (the residuals of the current and of the trial point), then for pose targets only tq [4·popcount(rot_mask)] (the
// target quaternions, xyzw) and rw [M] (the row weights).  Floats after all doubles: J [n·Dc] (row-major), q [Dc],
// qn [Dc] (the free wrist uses their first D).  Every array is addressed as base[i·s]: s = 1 on the host, and on the
// device the arrays of the lanes of a workgroup are interleaved in LDS (s = lanes, base shifted by the lane), so no
// array indexed at run time lives in registers (it would go to scratch).
#pragma once
#include "cdx_cost.h"

// The inner loops of the solve run over run-time bounds and read LDS: unrolled by four, the loads of four terms are in
// flight together while the sums keep their order (the same bits).
#if defined(__HIPCC__)
#define CDX_IK_UNROLL _Pragma("unroll 4")
#else
#define CDX_IK_UNROLL
#endif

namespace cdx {

// q[i] of a strided float row.
struct QStride {
  const float* p;
  int s;
  CDX_HDM float operator[](int i) const { return p[(size_t)i * s]; }
};

// q0[i] as a double from a float64 or float32 row.
struct Q0Row {
  const void* p;
  int f64;
  CDX_HDM double operator[](int i) const { return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i]; }
};

// The Jacobian columns of tip k at q, given its position p (fk_tip): col(dof, lin[3], ang[3]) once per moving joint on
// the path, in root→tip order.  The poses are chain_step's, as in the FK kernels.
template <class Q, class COL>
CDX_HD void fk_tip_columns(const cdx_chain& c, int k, const Q& q, const float* p, COL&& col) {
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, t[3] = {0.f, 0.f, 0.f};
  for (uint32_t m = chain_path_mask(c, c.tip_body[k]); m; m &= m - 1) {
    const cdx_body& b = c.bodies[low_bit(m)];
    float Rn[9], tn[3];
    chain_step(b, q, R, t, Rn, tn);
    if (b.dof >= 0) {
      const int ax = b.axis;  // (selects, not an index: see fk_tip_bwd2)
      const float fa[3] = {ax == 0 ? b.F[0] : (ax == 1 ? b.F[1] : b.F[2]), ax == 0 ? b.F[3] : (ax == 1 ? b.F[4] : b.F[5]),
                           ax == 0 ? b.F[6] : (ax == 1 ? b.F[7] : b.F[8])};
      float om[3];
      mat3_vec(R, fa, om);
      const float d[3] = {p[0] - tn[0], p[1] - tn[1], p[2] - tn[2]};
      const float lin[3] = {b.sign * (om[1] * d[2] - om[2] * d[1]), b.sign * (om[2] * d[0] - om[0] * d[2]),
                            b.sign * (om[0] * d[1] - om[1] * d[0])};
      const float ang[3] = {b.sign * om[0], b.sign * om[1], b.sign * om[2]};
      col((int)b.dof, lin, ang);
    }
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    for (int i = 0; i < 3; ++i) t[i] = tn[i];
  }
}

// lin / ang [3][D] of one (row, tip); ang nullable.
template <class Q>
CDX_HD void fk_jacobian_tip(const cdx_chain& c, int k, const Q& q, float* lin, float* ang) {
  const int D = c.n_dofs;
  for (int i = 0; i < 3 * D; ++i) {
    lin[i] = 0.f;
    if (ang) ang[i] = 0.f;
  }
  float p[3];
  fk_tip(c, k, q, p, nullptr);
  fk_tip_columns(c, k, q, p, [&](int d, const float* l, const float* a) {
    for (int i = 0; i < 3; ++i) {
      lin[i * D + d] = l[i];
      if (ang) ang[i * D + d] = a[i];
    }
  });
}


// The variants of the solve (see "One loop" above).
struct IkFixed {
  static constexpr bool pose = false, frames = false;
};
struct IkPose {
  static constexpr bool pose = true, frames = false;
};
struct IkFrames {
  static constexpr bool pose = false, frames = true;
};
template <class V>
CDX_HD int ik_rows(int T, uint32_t rot_mask) {
  return 3 * T + (V::frames ? 3 * __builtin_popcount(rot_mask) : 0);
}
template <class V>
CDX_HD int ik_cols(int D) {
  return D + (V::pose ? 6 : 0);
}

// Per-row storage of the solve (see "Storage" above), element i at base[i·s].  tq and rw: pose targets only.
struct IkMem {
  double *A, *g, *y, *dv, *tq, *rw;
  float *J, *q, *qn;
  int s;
};
template <class V>
CDX_HD int ik_mem_doubles(int n, int Dc, int R) {
  return n * (n + 1) / 2 + Dc + n + 2 * n + (V::frames ? 4 * R + n : 0);
}
template <class V>
CDX_HD size_t ik_mem_bytes(int T, int D, uint32_t rot_mask) {
  const int n = ik_rows<V>(T, rot_mask), Dc = ik_cols<V>(D);
  return (size_t)ik_mem_doubles<V>(n, Dc, __builtin_popcount(rot_mask)) * 8 + (size_t)(n * Dc + 2 * Dc) * 4;
}
// The arrays of `lane` among `s` lanes in a block of ik_mem_bytes<V>(T, D, rot_mask)·s bytes (8-byte aligned).
template <class V>
CDX_HD IkMem ik_mem_at(void* base, int T, int D, uint32_t rot_mask, int lane, int s) {
  const int n = ik_rows<V>(T, rot_mask), Dc = ik_cols<V>(D), R = __builtin_popcount(rot_mask);
  IkMem m;
  double* d = (double*)base + lane;
  m.A = d;
  d += (size_t)(n * (n + 1) / 2) * s;
  m.g = d;
  d += (size_t)Dc * s;
  m.y = d;
  d += (size_t)n * s;
  m.dv = d;
  d += (size_t)(2 * n) * s;
  m.tq = d;
  d += (size_t)(V::frames ? 4 * R : 0) * s;
  m.rw = d;
  float* f = (float*)((double*)base + (size_t)ik_mem_doubles<V>(n, Dc, R) * s) + lane;
  m.J = f;
  f += (size_t)(n * Dc) * s;
  m.q = f;
  f += (size_t)Dc * s;
  m.qn = f;
  m.s = s;
  return m;
}

// Checks the parameters and rounds the bounds inward to float32 (see above).  0, CDX_EINVAL, or CDX_ECHAIN for null.
CDX_HD int ik_prepare(const cdx_ik_params* in, int D, cdx_ik_params* out) {
  if (!in) return CDX_ECHAIN;
  *out = *in;
  if (in->max_iters < 0) return CDX_EINVAL;
  const double pos[5] = {in->tol, in->mu0, in->mu_min, in->mu_max, in->nu};
  for (int i = 0; i < 5; ++i)
    if (!(__builtin_isfinite(pos[i]) && pos[i] > 0.0)) return CDX_EINVAL;
  if (!(__builtin_isfinite(in->rho) && in->rho >= 0.0)) return CDX_EINVAL;
  for (int d = 0; d < D; ++d) {
    const double lo = in->lower[d], hi = in->upper[d];
    if (!(lo <= hi) || !__builtin_isfinite(in->ref_q[d])) return CDX_EINVAL;  // (a NaN bound fails lo <= hi)
    float l = (float)lo, h = (float)hi;
    if ((double)l < lo) l = nextafterf(l, INFINITY);
    if ((double)h > hi) h = nextafterf(h, -INFINITY);
    if (l > h) l = h = (float)lo;
    out->lower[d] = (double)l;
    out->upper[d] = (double)h;
  }
  return CDX_OK;
}

// One row's inputs and outputs, as stated at the top.  A variant reads only the fields named for it.
struct IkRow {
  Q0Row q0;
  const double *target, *w;
  double* err;
  const double* palm;                    // fixed palm, pose targets
  const double *palm0_pos, *palm0_rot;   // free wrist
  double *palm_pos, *palm_rot;           //
  const double *target_rot, *wr;         // pose targets
  uint32_t rot_mask, dof_mask;           //
  double* rot_err;                       //
};

// Whether joint d is solved: the dof_mask of pose targets, every joint otherwise.
template <class V>
CDX_HD bool ik_solved(const IkRow& r, int d) {
  if constexpr (V::frames)
    return (r.dof_mask >> d) & 1u;
  else
    return true;
}

// d = target − tip(q) into dv [0, 3T) (stride s), cost(q) and emax at the pose (Rp, pp).  Pose targets: also ρ_k of
// the oriented tips into dv [3T, M) in mask order, against the target quaternions tq.
template <class V, class Q>
CDX_HD double ik_eval(const cdx_chain& c, const cdx_ik_params& p, const Q& q, const IkRow& r, const double* Rp,
                      const double* pp, const double* po, const double* tq, double* dv, int s, double* emax) {
  const int T = c.n_tips;
  double ss = 0.0, sr = 0.0, em = 0.0;
  int j = 0;
  for (int k = 0; k < T; ++k) {
    float pf[3], cf[4];
    fk_tip(c, k, q, pf, V::frames ? cf : nullptr);
    const double v[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
    double x[3];
    mat3_vec(Rp, v, x);
    const double wk = r.w ? r.w[k] : 1.0;
    double d[3];
    for (int i = 0; i < 3; ++i) {
      d[i] = r.target[3 * k + i] - ((x[i] + pp[i]) + po[i]);
      dv[(size_t)(3 * k + i) * s] = d[i];
    }
    const double e = wk * sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    em = e > em ? e : em;
    const double rd[3] = {wk * d[0], wk * d[1], wk * d[2]};
    ss += (rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2];
    if constexpr (V::frames) {
      if ((r.rot_mask >> k) & 1u) {
        const double cx = (double)cf[0], cy = (double)cf[1], cz = (double)cf[2], cw = (double)cf[3];
        const double nn = sqrt(((cx * cx + cy * cy) + cz * cz) + cw * cw);
        const double ax = cx / nn, ay = cy / nn, az = cz / nn, aw = cw / nn;
        const double tx = tq[(size_t)(4 * j) * s], ty = tq[(size_t)(4 * j + 1) * s], tz = tq[(size_t)(4 * j + 2) * s],
                     tw = tq[(size_t)(4 * j + 3) * s];
        const double ew = ((tw * aw + tx * ax) + ty * ay) + tz * az;
        const double ex = (aw * tx - tw * ax) - (ty * az - tz * ay);
        const double ey = (aw * ty - tw * ay) - (tz * ax - tx * az);
        const double ez = (aw * tz - tw * az) - (tx * ay - ty * ax);
        const double sg = ew < 0.0 ? -2.0 : 2.0;
        const double ro[3] = {sg * ex, sg * ey, sg * ez};
        for (int i = 0; i < 3; ++i) dv[(size_t)(3 * T + 3 * j + i) * s] = ro[i];
        const double wrk = r.wr ? r.wr[k] : 0.1;
        const double er = wrk * sqrt((ro[0] * ro[0] + ro[1] * ro[1]) + ro[2] * ro[2]);
        em = er > em ? er : em;
        const double rr[3] = {wrk * ro[0], wrk * ro[1], wrk * ro[2]};
        sr += (rr[0] * rr[0] + rr[1] * rr[1]) + rr[2] * rr[2];
        ++j;
      }
    }
  }
  double sq = 0.0;
  for (int d = 0; d < c.n_dofs; ++d) {
    if (!ik_solved<V>(r, d)) continue;
    const double dq = (double)q[d] - p.ref_q[d];
    sq += dq * dq;
  }
  *emax = em;
  return 0.5 * (V::frames ? ss + sr : ss) + (0.5 * p.rho) * sq;
}

// The damped system of one step over the first D columns of every row of m.J (row stride D): A = W·J·Jᵀ·W + κI and
// b = W·J·g, A = L·Lᵀ in place, y = A⁻¹·b by two substitutions, then y ← w·y in m.y (the header's order of operations).
// False if a pivot was not > 0.  rw(a) is the weight of row a: IkTipW for three rows per tip (null: all 1), IkRowW for
// the packed rows of frame_ik_row.
struct IkTipW {
  const double* w;
  CDX_HDM double operator()(int a) const { return w ? w[a / 3] : 1.0; }
};
struct IkRowW {
  const double* p;
  int s;
  CDX_HDM double operator()(int a) const { return p[(size_t)a * s]; }
};
template <class RW>
CDX_HD bool ik_gram_solve(const IkMem& m, const RW& rw, int n, int D, double kappa) {
  const int s = m.s;
  // A and b
  for (int a = 0; a < n; ++a) {
    const double wa = rw(a);
    for (int b = 0; b <= a; ++b) {
      const double wb = rw(b);
      double acc = 0.0;
      CDX_IK_UNROLL
      for (int d = 0; d < D; ++d) acc += (double)m.J[(size_t)(a * D + d) * s] * (double)m.J[(size_t)(b * D + d) * s];
      acc = (wa * wb) * acc;
      if (a == b) acc += kappa;
      m.A[(size_t)(a * (a + 1) / 2 + b) * s] = acc;
    }
    double acc = 0.0;
    CDX_IK_UNROLL
    for (int d = 0; d < D; ++d) acc += (double)m.J[(size_t)(a * D + d) * s] * m.g[(size_t)d * s];
    m.y[(size_t)a * s] = wa * acc;
  }
  // A = L·Lᵀ in place
  bool pd = true;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double sum = m.A[(size_t)(i * (i + 1) / 2 + j) * s];
      CDX_IK_UNROLL
      for (int k = 0; k < j; ++k) sum -= m.A[(size_t)(i * (i + 1) / 2 + k) * s] * m.A[(size_t)(j * (j + 1) / 2 + k) * s];
      if (i == j) {
        pd = pd && sum > 0.0;
        m.A[(size_t)(i * (i + 1) / 2 + j) * s] = sqrt(sum);
      } else {
        m.A[(size_t)(i * (i + 1) / 2 + j) * s] = sum / m.A[(size_t)(j * (j + 1) / 2 + j) * s];
      }
    }
  for (int i = 0; i < n; ++i) {
    double sum = m.y[(size_t)i * s];
    CDX_IK_UNROLL
    for (int k = 0; k < i; ++k) sum -= m.A[(size_t)(i * (i + 1) / 2 + k) * s] * m.y[(size_t)k * s];
    m.y[(size_t)i * s] = sum / m.A[(size_t)(i * (i + 1) / 2 + i) * s];
  }
  for (int i = n - 1; i >= 0; --i) {
    double sum = m.y[(size_t)i * s];
    CDX_IK_UNROLL
    for (int k = i + 1; k < n; ++k) sum -= m.A[(size_t)(k * (k + 1) / 2 + i) * s] * m.y[(size_t)k * s];
    m.y[(size_t)i * s] = sum / m.A[(size_t)(i * (i + 1) / 2 + i) * s];
  }
  for (int a = 0; a < n; ++a) m.y[(size_t)a * s] = rw(a) * m.y[(size_t)a * s];
  return pd;
}

// The Kabsch start of ik_pose_row (see above): v [3T] (stride s) holds double(FK_f32(q)_k).
CDX_HD void ik_pose_start(int T, const double* v, int s, const double* target, const double* po, const double* w,
                          double* Rp, double* pp) {
  double cv[3] = {0.0, 0.0, 0.0}, ct[3] = {0.0, 0.0, 0.0}, W = 0.0;
  int npos = 0;
  for (int k = 0; k < T; ++k) {
    const double wk = w ? w[k] : 1.0;
    W += wk;
    npos += wk > 0.0 ? 1 : 0;
    for (int i = 0; i < 3; ++i) {
      cv[i] += wk * v[(size_t)(3 * k + i) * s];
      ct[i] += wk * (target[3 * k + i] - po[i]);
    }
  }
  for (int i = 0; i < 9; ++i) Rp[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (!(W > 0.0)) {
    for (int i = 0; i < 3; ++i) pp[i] = 0.0;
    return;
  }
  for (int i = 0; i < 3; ++i) {
    cv[i] /= W;
    ct[i] /= W;
  }
  if (npos >= 3) {
    double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < T; ++k) {
      const double wk = w ? w[k] : 1.0;
      for (int r = 0; r < 3; ++r) {
        const double a = wk * (v[(size_t)(3 * k + r) * s] - cv[r]);
        for (int i = 0; i < 3; ++i) H[3 * r + i] += a * ((target[3 * k + i] - po[i]) - ct[i]);
      }
    }
    const double noise[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    KabschTape tp;
    double R[9];
    kabsch_rotation<double>(H, noise, tp, R);
    bool fin = true;
    for (int i = 0; i < 9; ++i) fin = fin && __builtin_isfinite(R[i]);
    if (fin)
      for (int i = 0; i < 9; ++i) Rp[i] = R[i];
  }
  double x[3];
  mat3_vec(Rp, cv, x);
  for (int i = 0; i < 3; ++i) pp[i] = ct[i] - x[i];
}

// The masks of a call: 0, or CDX_EINVAL for a rot_mask bit at or above T, a dof_mask with no bit below D or one at or
// above D.
CDX_HD int ik_frames_mask_code(int T, int D, uint64_t rot_mask, uint64_t dof_mask) {
  if ((rot_mask >> T) || (dof_mask >> D)) return CDX_EINVAL;
  if (!dof_mask) return CDX_EINVAL;
  return CDX_OK;
}

// Shepperd's rule: the unit quaternion (x, y, z, w) of an orthogonal R (row-major entries r00 … r22) in float64.  The
// branch is on the largest of the trace tr = (r00 + r11) + r22 and the three diagonal entries, ties to the first.  Trace:
// r = sqrt(1 + tr), w = ½·r, (x, y, z) = (r21 − r12, r02 − r20, r10 − r01)·(½/r).  Entry ii, with (i, j, k) the cyclic
// order from i: r = sqrt(((1 + r_ii) − r_jj) − r_kk), q_i = ½·r, q_j = (r_ij + r_ji)·(½/r), q_k = (r_ik + r_ki)·(½/r),
// w = (r_kj − r_jk)·(½/r).  One sqrt, one division; written with selects on scalars only, so nothing is indexed at run
// time.
CDX_HD void shepperd_quat(double r00, double r01, double r02, double r10, double r11, double r12, double r20, double r21,
                          double r22, double& x, double& y, double& z, double& w) {
  const double tr = (r00 + r11) + r22;
  int br = -1;
  double best = tr;
  if (r00 > best) { br = 0; best = r00; }
  if (r11 > best) { br = 1; best = r11; }
  if (r22 > best) { br = 2; }
  const double dii = br == 0 ? r00 : (br == 1 ? r11 : r22), djj = br == 0 ? r11 : (br == 1 ? r22 : r00),
               dkk = br == 0 ? r22 : (br == 1 ? r00 : r11);
  const double rad = br < 0 ? 1.0 + tr : ((1.0 + dii) - djj) - dkk;
  const double r = sqrt(rad), f = 0.5 / r, h = 0.5 * r;
  const double s01 = (r01 + r10) * f, s12 = (r12 + r21) * f, s20 = (r20 + r02) * f;
  const double a0 = (r21 - r12) * f, a1 = (r02 - r20) * f, a2 = (r10 - r01) * f;
  x = br < 0 ? a0 : (br == 0 ? h : (br == 1 ? s01 : s20));
  y = br < 0 ? a1 : (br == 0 ? s01 : (br == 1 ? h : s12));
  z = br < 0 ? a2 : (br == 0 ? s20 : (br == 1 ? s12 : h));
  w = br < 0 ? h : (br == 0 ? a0 : (br == 1 ? a1 : a2));
}

// The free wrist's trial pose (Rn, pn) from (Rp, pp) and the step st = (t_b, ω_b): see "Trial point" at the top.
CDX_HD void ik_pose_trial(const double* Rp, const double* pp, const double* st, double* Rn, double* pn) {
  double x[3];
  mat3_vec(Rp, st, x);
  for (int i = 0; i < 3; ++i) pn[i] = pp[i] + x[i];
  const double a[3] = {0.5 * st[3], 0.5 * st[4], 0.5 * st[5]};
  const double ss = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], den = 1.0 + ss, one = 1.0 - ss;
  const double C[9] = {(one + 2.0 * (a[0] * a[0])) / den,        (2.0 * (a[0] * a[1]) - 2.0 * a[2]) / den,
                       (2.0 * (a[0] * a[2]) + 2.0 * a[1]) / den, (2.0 * (a[1] * a[0]) + 2.0 * a[2]) / den,
                       (one + 2.0 * (a[1] * a[1])) / den,        (2.0 * (a[1] * a[2]) - 2.0 * a[0]) / den,
                       (2.0 * (a[2] * a[0]) - 2.0 * a[1]) / den, (2.0 * (a[2] * a[1]) + 2.0 * a[0]) / den,
                       (one + 2.0 * (a[2] * a[2])) / den};
  mat3_mul(Rp, C, Rn);
}

// One row of the solve of variant V (p: after ik_prepare; po: 3 doubles; the masks: after ik_frames_mask_code;
// m: ik_mem_at<V>).  Leaves the result in m.q, writes the variant's outputs and *iters, returns the status.  Status 2
// leaves m untouched.
template <class V>
CDX_HD int ik_lm_row(const cdx_chain& c, const cdx_ik_params& p, const double* po, const IkRow& r, const IkMem& m,
                     int32_t* iters) {
  const int T = c.n_tips, D = c.n_dofs, Dc = ik_cols<V>(D), n = ik_rows<V>(T, r.rot_mask), s = m.s;
  const double* w = r.w;
  bool fin = true;
  for (int d = 0; d < D; ++d) {
    const double v = r.q0[d];
    fin = fin && __builtin_isfinite(v) && __builtin_isfinite((float)v);
  }
  for (int i = 0; i < 3 * T; ++i) fin = fin && __builtin_isfinite(r.target[i]);
  if (w)
    for (int k = 0; k < T; ++k) fin = fin && __builtin_isfinite(w[k]);
  if constexpr (V::pose) {
    if (r.palm0_pos) {
      for (int i = 0; i < 3; ++i) fin = fin && __builtin_isfinite(r.palm0_pos[i]);
      for (int i = 0; i < 9; ++i) fin = fin && __builtin_isfinite(r.palm0_rot[i]);
    }
  } else {
    if (r.palm)
      for (int i = 0; i < 6; ++i) fin = fin && __builtin_isfinite(r.palm[i]);
  }
  if constexpr (V::frames) {
    if (r.target_rot)
      for (int i = 0; i < 9 * T; ++i) fin = fin && __builtin_isfinite(r.target_rot[i]);
    if (r.wr)
      for (int k = 0; k < T; ++k) fin = fin && __builtin_isfinite(r.wr[k]);
  }
  *iters = 0;
  if (!fin) {
    for (int k = 0; k < T; ++k) r.err[k] = NAN;
    if constexpr (V::pose) {
      for (int i = 0; i < 3; ++i) r.palm_pos[i] = NAN;
      for (int i = 0; i < 9; ++i) r.palm_rot[i] = NAN;
    }
    if constexpr (V::frames)
      for (int k = 0; k < T; ++k) r.rot_err[k] = NAN;
    return 2;
  }
  for (int d = 0; d < D; ++d) {
    const float f = (float)r.q0[d], lo = (float)p.lower[d], hi = (float)p.upper[d];
    m.q[(size_t)d * s] = f < lo ? lo : (f > hi ? hi : f);
  }
  const QStride q{m.q, s}, qn{m.qn, s};
  // the pose: given, or the free wrist's start; Rn / pn: the free wrist's trial copy
  double Rp[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, pp[3] = {0.0, 0.0, 0.0}, Rn[9], pn[3];
  if constexpr (V::pose) {
    if (r.palm0_pos) {
      for (int i = 0; i < 9; ++i) Rp[i] = r.palm0_rot[i];
      for (int i = 0; i < 3; ++i) pp[i] = r.palm0_pos[i];
    } else {
      double* v = m.dv + (size_t)n * s;  // (the second residual buffer: free until the first trial point)
      for (int k = 0; k < T; ++k) {
        float pf[3];
        fk_tip(c, k, q, pf, nullptr);
        for (int i = 0; i < 3; ++i) v[(size_t)(3 * k + i) * s] = (double)pf[i];
      }
      ik_pose_start(T, v, s, r.target, po, w, Rp, pp);
    }
  } else {
    if (r.palm) {
      euler_xyz(r.palm + 3, Rp, nullptr, nullptr, nullptr);
      for (int i = 0; i < 3; ++i) pp[i] = r.palm[i];
    }
  }
  // pose targets: the target quaternions and the row weights, once
  if constexpr (V::frames) {
    int j = 0;
    for (int k = 0; k < T; ++k) {
      const double wk = w ? w[k] : 1.0;
      for (int i = 0; i < 3; ++i) m.rw[(size_t)(3 * k + i) * s] = wk;
      if ((r.rot_mask >> k) & 1u) {
        // (Rpᵀ·Rt entry by entry, indexed by constants only: the matrix stays in registers)
        const double* B = r.target_rot + 9 * k;
        auto el = [&](int i, int c3) { return (Rp[i] * B[c3] + Rp[3 + i] * B[3 + c3]) + Rp[6 + i] * B[6 + c3]; };
        double t[4];
        shepperd_quat(el(0, 0), el(0, 1), el(0, 2), el(1, 0), el(1, 1), el(1, 2), el(2, 0), el(2, 1), el(2, 2), t[0], t[1],
                      t[2], t[3]);
        const double wrk = r.wr ? r.wr[k] : 0.1;
        m.tq[(size_t)(4 * j) * s] = t[0];
        m.tq[(size_t)(4 * j + 1) * s] = t[1];
        m.tq[(size_t)(4 * j + 2) * s] = t[2];
        m.tq[(size_t)(4 * j + 3) * s] = t[3];
        for (int i = 0; i < 3; ++i) m.rw[(size_t)(3 * T + 3 * j + i) * s] = wrk;
        ++j;
      }
    }
  }
  int cur = 0;
  double emax;
  double cost = ik_eval<V>(c, p, q, r, Rp, pp, po, m.tq, m.dv, s, &emax);
  double mu = p.mu0;
  int it = 0, status;
  for (;;) {
    if (emax <= p.tol) { status = 0; break; }
    if (it >= p.max_iters) { status = 1; break; }
    ++it;
    // Jl at q: lin of every tip; the free wrist's t_b and ω_b columns; ang of the oriented tips
    CDX_IK_UNROLL
    for (int i = 0; i < n * Dc; ++i) m.J[(size_t)i * s] = 0.f;
    for (int k = 0, j = 0; k < T; ++k) {
      const bool rot = V::frames && ((r.rot_mask >> k) & 1u);
      float pf[3];
      fk_tip(c, k, q, pf, nullptr);
      fk_tip_columns(c, k, q, pf, [&](int d, const float* l, const float* a) {
        for (int i = 0; i < 3; ++i) m.J[(size_t)((3 * k + i) * Dc + d) * s] = l[i];
        if (rot)
          for (int i = 0; i < 3; ++i) m.J[(size_t)((3 * T + 3 * j + i) * Dc + d) * s] = a[i];
      });
      if constexpr (V::pose) {
        float* r0 = m.J + (size_t)((3 * k) * Dc + D) * s;
        float* r1 = m.J + (size_t)((3 * k + 1) * Dc + D) * s;
        float* r2 = m.J + (size_t)((3 * k + 2) * Dc + D) * s;
        r0[0] = 1.f; r1[(size_t)1 * s] = 1.f; r2[(size_t)2 * s] = 1.f;
        r0[(size_t)4 * s] = pf[2];  r0[(size_t)5 * s] = -pf[1];
        r1[(size_t)3 * s] = -pf[2]; r1[(size_t)5 * s] = pf[0];
        r2[(size_t)3 * s] = pf[1];  r2[(size_t)4 * s] = -pf[0];
      }
      j += rot ? 1 : 0;
    }
    // u = w·Rpᵀ·(w·d) of the position rows, and wr·(wr·ρ) of the orientation rows, into y
    const double* dc = m.dv + (size_t)(cur * n) * s;
    for (int k = 0; k < T; ++k) {
      const double wk = w ? w[k] : 1.0;
      const double rd[3] = {wk * dc[(size_t)(3 * k) * s], wk * dc[(size_t)(3 * k + 1) * s], wk * dc[(size_t)(3 * k + 2) * s]};
      double u[3];
      mat3t_vec(Rp, rd, u);
      for (int i = 0; i < 3; ++i) m.y[(size_t)(3 * k + i) * s] = wk * u[i];
    }
    if constexpr (V::frames)
      for (int a = 3 * T; a < n; ++a) {
        const double wa = m.rw[(size_t)a * s];
        m.y[(size_t)a * s] = wa * (wa * dc[(size_t)a * s]);
      }
    // g: the joints with their ρ term, held or fixed on their bounds; the free wrist's pose columns bare
    for (int d = 0; d < Dc; ++d) {
      double acc = 0.0;
      CDX_IK_UNROLL
      for (int a = 0; a < n; ++a) acc += (double)m.J[(size_t)(a * Dc + d) * s] * m.y[(size_t)a * s];
      double g = acc;
      if (d < D) {
        const double qd = (double)q[d];
        g = acc + p.rho * (p.ref_q[d] - qd);
        if (!ik_solved<V>(r, d) || (qd <= p.lower[d] && g < 0.0) || (qd >= p.upper[d] && g > 0.0)) {
          g = 0.0;
          for (int a = 0; a < n; ++a) m.J[(size_t)(a * Dc + d) * s] = 0.f;
        }
      }
      m.g[(size_t)d * s] = g;
    }
    const double kappa = mu + p.rho;
    bool pd;
    if constexpr (V::frames)
      pd = ik_gram_solve(m, IkRowW{m.rw, s}, n, Dc, kappa);
    else
      pd = ik_gram_solve(m, IkTipW{w}, n, Dc, kappa);
    // the trial point
    for (int d = 0; d < D; ++d) {
      double acc = 0.0;
      CDX_IK_UNROLL
      for (int a = 0; a < n; ++a) acc += (double)m.J[(size_t)(a * Dc + d) * s] * m.y[(size_t)a * s];
      const double v = (double)q[d] + (m.g[(size_t)d * s] - acc) / kappa;
      const float vn = (float)(v < p.lower[d] ? p.lower[d] : (v > p.upper[d] ? p.upper[d] : v));
      m.qn[(size_t)d * s] = ik_solved<V>(r, d) ? vn : m.q[(size_t)d * s];
    }
    if constexpr (V::pose) {
      double st[6];
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int j = 0; j < 6; ++j) {
        double acc = 0.0;
        CDX_IK_UNROLL
        for (int a = 0; a < n; ++a) acc += (double)m.J[(size_t)(a * Dc + D + j) * s] * m.y[(size_t)a * s];
        st[j] = (m.g[(size_t)(D + j) * s] - acc) / kappa;
      }
      ik_pose_trial(Rp, pp, st, Rn, pn);
    }
    double emn;
    const double cn = ik_eval<V>(c, p, qn, r, V::pose ? Rn : Rp, V::pose ? pn : pp, po, m.tq,
                                 m.dv + (size_t)((1 - cur) * n) * s, s, &emn);
    if (pd && cn < cost) {
      for (int d = 0; d < D; ++d) m.q[(size_t)d * s] = m.qn[(size_t)d * s];
      if constexpr (V::pose) {
        for (int i = 0; i < 9; ++i) Rp[i] = Rn[i];
        for (int i = 0; i < 3; ++i) pp[i] = pn[i];
      }
      cur = 1 - cur;
      cost = cn;
      emax = emn;
      mu = mu / p.nu;
      mu = mu > p.mu_min ? mu : p.mu_min;
    } else {
      mu = mu * p.nu;
      mu = mu < p.mu_max ? mu : p.mu_max;
    }
  }
  const double* dc = m.dv + (size_t)(cur * n) * s;
  for (int k = 0, j = 0; k < T; ++k) {
    const double d[3] = {dc[(size_t)(3 * k) * s], dc[(size_t)(3 * k + 1) * s], dc[(size_t)(3 * k + 2) * s]};
    r.err[k] = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if constexpr (V::frames) {
      r.rot_err[k] = 0.0;
      if ((r.rot_mask >> k) & 1u) {
        const double* ro = dc + (size_t)(3 * T + 3 * j) * s;
        const double a = ro[0], b = ro[(size_t)s], cc = ro[(size_t)2 * s];
        r.rot_err[k] = sqrt((a * a + b * b) + cc * cc);
        ++j;
      }
    }
  }
  if constexpr (V::pose) {
    for (int i = 0; i < 3; ++i) r.palm_pos[i] = pp[i];
    for (int i = 0; i < 9; ++i) r.palm_rot[i] = Rp[i];
  }
  *iters = it;
  return status;
}

// The three solves: what each takes and writes (null as stated at the top).
CDX_HD int ik_row(const cdx_chain& c, const cdx_ik_params& p, const double* po, const Q0Row& q0, const double* target,
                  const double* palm, const double* w, const IkMem& m, double* err, int32_t* iters) {
  IkRow r{};
  r.q0 = q0, r.target = target, r.w = w, r.err = err, r.palm = palm;
  return ik_lm_row<IkFixed>(c, p, po, r, m, iters);
}
CDX_HD int ik_pose_row(const cdx_chain& c, const cdx_ik_params& p, const double* po, const Q0Row& q0,
                       const double* target, const double* palm0_pos, const double* palm0_rot, const double* w,
                       const IkMem& m, double* palm_pos, double* palm_rot, double* err, int32_t* iters) {
  IkRow r{};
  r.q0 = q0, r.target = target, r.w = w, r.err = err;
  r.palm0_pos = palm0_pos, r.palm0_rot = palm0_rot, r.palm_pos = palm_pos, r.palm_rot = palm_rot;
  return ik_lm_row<IkPose>(c, p, po, r, m, iters);
}
CDX_HD int frame_ik_row(const cdx_chain& c, const cdx_ik_params& p, const double* po, const Q0Row& q0,
                        const double* target, const double* target_rot, const double* palm, const double* w,
                        const double* wr, uint32_t rot_mask, uint32_t dof_mask, const IkMem& m, double* err,
                        double* rot_err, int32_t* iters) {
  IkRow r{};
  r.q0 = q0, r.target = target, r.w = w, r.err = err, r.palm = palm;
  r.target_rot = target_rot, r.wr = wr, r.rot_mask = rot_mask, r.dof_mask = dof_mask, r.rot_err = rot_err;
  return ik_lm_row<IkFrames>(c, p, po, r, m, iters);
}

// What every entry of the solves checks first, device and host, in this order: the chain (chain_code, cdx_fk.h: null →
// CDX_ECHAIN, sizes over the descriptor's → CDX_EINVAL, a malformed tree or an over-deep tip → CDX_ECHAIN), the
// parameters (ik_prepare, into *p), then E and q_dtype.
CDX_HD int ik_call_code(const cdx_chain* c, const cdx_ik_params* params, int64_t E, int32_t q_dtype, cdx_ik_params* p) {
  int rc = chain_code(c);
  if (rc) return rc;
  rc = ik_prepare(params, c->n_dofs, p);
  if (rc) return rc;
  if (E < 0 || (q_dtype != CDX_DTYPE_F32 && q_dtype != CDX_DTYPE_F64)) return CDX_EINVAL;
  return CDX_OK;
}

// po [3] = palm_offset, or 0 for null; CDX_EINVAL for a non-finite entry.
CDX_HD int ik_offset_code(const double* palm_offset, double* po) {
  for (int i = 0; i < 3; ++i) {
    po[i] = palm_offset ? palm_offset[i] : 0.0;
    if (!__builtin_isfinite(po[i])) return CDX_EINVAL;
  }
  return CDX_OK;
}

// Row e of the batch's q0 [E][D], and of its q: m.q, or q0 as it was given for a status-2 row.
CDX_HD Q0Row ik_q0_row(const void* q0, int f64, int64_t e, int D) {
  return Q0Row{f64 ? (const void*)((const double*)q0 + e * D) : (const void*)((const float*)q0 + e * D), f64};
}
CDX_HD void ik_store_q(void* q, const void* q0, int f64, int64_t e, int D, int st, const IkMem& m) {
  for (int d = 0; d < D; ++d) {
    if (f64)
      ((double*)q)[e * D + d] = st == 2 ? ((const double*)q0)[e * D + d] : (double)m.q[(size_t)d * m.s];
    else
      ((float*)q)[e * D + d] = st == 2 ? ((const float*)q0)[e * D + d] : m.q[(size_t)d * m.s];
  }
}

}  // namespace cdx
