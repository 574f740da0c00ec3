// Rigid-body dynamics of a chain: the per-row rule shared by the kernels (cdx_dyn.hip) and the host build (host_ref.cpp:
// cdxh_dyn_inverse, cdxh_dyn_inertia, cdxh_dyn_forward).  The reference's compute_inverse_dynamics,
// compute_lagrangian_inertia_matrix and compute_forward_dynamics (robot_model.py:266-640, with the spatial algebra of
// spatial_vector_algebra.py:175-372), Featherstone's recursive Newton–Euler algorithm in body coordinates.
//
// Joint convention (that of cdx_ik.h).  q is rounded to float32, the angle is the float32 product sign·q, its sine and
//   cosine are float32, taken as the DEVICE's cdx_sinf / cdx_cosf take them — the float64 function, rounded — on both
//   builds (dyn_sinf / dyn_cosf: the host's cdx_sinf is the C library's sinf, which differs from that in the last bit
//   for one angle in a hundred, and the host build here is held to the device bit for bit); everything after that is
//   float64: the joint pose E_i = F_i·A(axis, c, s) with F_i
//   the descriptor's float32 fixed rotation widened, p_i its float32 origin widened, the joint's motion subspace
//   S_i = sign_i·e_axis (angular; the reference's raw URDF axis, rigid_body.py:133).  A fixed body has c = 1, s = 0
//   (E_i = F_i exactly), a moving joint whose sign is 0 never moves (E_i = F_i, S_i = 0).
//
// Inverse dynamics (dyn_rnea), bodies in descriptor (URDF) order, parents first:
//   forward   (ω, v, α, a)_0 = (0, 0, 0, −g)  — gravity is the base's acceleration (robot_model.py:360-366) —, and with
//             λ the parent, w = S·q̇, z = S·q̈:
//               ω_i = Eᵀω_λ + w,              v_i = Eᵀ(v_λ + ω_λ × p),
//               α_i = Eᵀα_λ + z + ω_i × w,    a_i = Eᵀ(a_λ + α_λ × p) + v_i × w             (:278-293)
//   own force n_i = Īα + mc × a + ω × (Īω + mc × v) + v × (m·v − mc × ω),
//             f_i = m·a − mc × α + ω × (m·v − mc × ω)                                          (:300-309)
//             with Ī = I + m·[c]ₓ[c]ₓᵀ and mc = m·c from the cdx_dyn descriptor; written over the body's (ω, v, α, a):
//             nothing needs those once the forward sweep is over, so a body keeps 12 doubles, not 18;
//   tips      an external force F_t (base frame) at tip t of body b, offset o_t: with R_b the body's rotation in the
//             base frame (the product of the E on its path, walked up the parents — no depth limit),
//             f_b −= R_bᵀF_t,  n_b −= o_t × (R_bᵀF_t): the torque returned is what the joints must supply,
//             τ_RNEA − Σ_t J_tᵀF_t, and no Jacobian is formed;
//   backward  i = n−1 … 1:  τ_dof(i) = sign·n_i[axis] (+ damping·q̇);  f_λ += E·f_i,  n_λ += E·n_i + p × (E·f_i)  (:312-317,
//             :369-389).
// Inertia matrix (dyn_inertia): column j is dyn_rnea at q̇ = 0, q̈ = e_j, g = 0 (what the reference's D + 1 passes
//   reduce to, :419-466); rows i ≥ j are kept and mirrored, so H is symmetric bit for bit.
// Forward dynamics (dyn_forward): q̈ = H⁻¹·(f − damping·q̇ − nle), nle = dyn_rnea at q̈ = 0 without damping, H as above
//   into the lower triangle, H = L·Lᵀ row by row, two substitutions (ik_gram_solve's order).  The reference's
//   articulated-body sweep (:504-640) solves the same system.
//
// Storage (DynMem).  Every per-row array is addressed as base[i·s]: s = 1 on the host; on the device the arrays of the
// lanes of a workgroup are interleaved in LDS (s = lanes, base shifted by the lane), as cdx_ik.h's IkMem.  Per body 12
// doubles and the cached (c, s) as two floats; the forward dynamics adds the D(D + 1)/2 + D doubles of its system.
#pragma once
#include "cdx_ik.h"

namespace cdx {

struct DynMem {
  double *B, *A, *y;  // B: 12·n_bodies, A: D(D+1)/2 (lower triangle, row-major), y: D  (A, y: forward dynamics only)
  float* cs;          // 2·n_bodies
  int s;
};
CDX_HD int dyn_mem_doubles(int n, int D, int fwd) { return 12 * n + (fwd ? D * (D + 1) / 2 + D : 0); }
CDX_HD size_t dyn_mem_bytes(int n, int D, int fwd) { return (size_t)dyn_mem_doubles(n, D, fwd) * 8 + (size_t)(2 * n) * 4; }
// The arrays of `lane` among `s` lanes in a block of dyn_mem_bytes(n, D, fwd)·s bytes (8-byte aligned).
CDX_HD DynMem dyn_mem_at(void* base, int n, int D, int fwd, int lane, int s) {
  DynMem m;
  double* d = (double*)base + lane;
  m.B = d;
  d += (size_t)(12 * n) * s;
  m.A = d;
  d += (size_t)(fwd ? D * (D + 1) / 2 : 0) * s;
  m.y = d;
  m.cs = (float*)((double*)base + (size_t)dyn_mem_doubles(n, D, fwd) * s) + lane;
  m.s = s;
  return m;
}

// The chain check of the three entries: chain_code's without its limit on a tip's depth (the state is per body, not
// per level) and with no tip required.  null → CDX_ECHAIN, sizes over the descriptor's → CDX_EINVAL, a malformed tree →
// CDX_ECHAIN.
CDX_HD int dyn_chain_code(const cdx_chain* c, const cdx_dyn* dy) {
  if (!c || !dy) return CDX_ECHAIN;
  if (c->n_bodies <= 0 || c->n_bodies > CDX_MAX_BODIES || c->n_dofs < 0 || c->n_dofs > CDX_MAX_DOFS || c->n_tips < 0 ||
      c->n_tips > CDX_MAX_TIPS)
    return CDX_EINVAL;
  for (int i = 1; i < c->n_bodies; ++i)
    if (c->bodies[i].parent < 0 || c->bodies[i].parent >= i || c->bodies[i].dof >= c->n_dofs || c->bodies[i].axis < 0 ||
        c->bodies[i].axis > 2)
      return CDX_ECHAIN;
  for (int k = 0; k < c->n_tips; ++k)
    if (c->tip_body[k] < 0 || c->tip_body[k] >= c->n_bodies) return CDX_ECHAIN;
  return CDX_OK;
}
// True if a moving joint has sign 0: its row of H is zero and the forward dynamics has no solution.
CDX_HD bool dyn_has_dead_joint(const cdx_chain& c) {
  for (int i = 1; i < c.n_bodies; ++i)
    if (c.bodies[i].dof >= 0 && c.bodies[i].sign == 0.f) return true;
  return false;
}

// Row readers: element i of a float64 / float32 row as a double (null: 0), all zero, a unit vector.
struct DynVec {
  const void* p;
  int f64;
  CDX_HDM double operator[](int i) const {
    return !p ? 0.0 : (f64 ? ((const double*)p)[i] : (double)((const float*)p)[i]);
  }
};
struct DynUnit {
  int j;
  CDX_HDM double operator[](int i) const { return i == j ? 1.0 : 0.0; }
};

// cdx_sinf / cdx_cosf as the device defines them (cdx_hd.h), on both builds.
CDX_HD float dyn_sinf(float x) { return (float)sin((double)x); }
CDX_HD float dyn_cosf(float x) { return (float)cos((double)x); }

CDX_HD void dyn_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// E = F·A(axis, c, s) in float64 (selects, not indices or branches: a register array indexed at run time would go to scratch).
CDX_HD void dyn_joint_E(const cdx_body& b, double c, double s, double* E) {
  const int ax = b.axis;
  for (int r = 0; r < 3; ++r) {
    const double F0 = (double)b.F[3 * r], F1 = (double)b.F[3 * r + 1], F2 = (double)b.F[3 * r + 2];
    // with (u, v, w) = (axis, axis + 1, axis + 2) mod 3: column u = F_u, v = F_v·c + F_w·s, w = F_w·c − F_v·s
    const double Fu = ax == 0 ? F0 : (ax == 1 ? F1 : F2), Fv = ax == 0 ? F1 : (ax == 1 ? F2 : F0),
                 Fw = ax == 0 ? F2 : (ax == 1 ? F0 : F1);
    const double ev = Fv * c + Fw * s, ew = Fw * c - Fv * s;
    E[3 * r] = ax == 0 ? Fu : (ax == 1 ? ew : ev);
    E[3 * r + 1] = ax == 0 ? ev : (ax == 1 ? Fu : ew);
    E[3 * r + 2] = ax == 0 ? ew : (ax == 1 ? ev : Fu);
  }
}
CDX_HD void dyn_body_E(const cdx_chain& c, const DynMem& m, int i, double* E) {
  dyn_joint_E(c.bodies[i], (double)m.cs[(size_t)(2 * i) * m.s], (double)m.cs[(size_t)(2 * i + 1) * m.s], E);
}
// S·x: x on the joint's axis.
CDX_HD void dyn_axis_vec(int ax, double x, double* o) {
  o[0] = ax == 0 ? x : 0.0;
  o[1] = ax == 1 ? x : 0.0;
  o[2] = ax == 2 ? x : 0.0;
}
// (Ī·w + mc × u, m·u − mc × w): the spatial inertia of body i on the motion (w angular, u linear).
CDX_HD void dyn_inertia_mul(const cdx_dyn& dy, int i, const double* w, const double* u, double* n, double* f) {
  const double* I = dy.inertia[i];
  const double* mc = dy.mcom[i];
  const double ms = dy.mass[i];
  double x[3], y[3];
  dyn_cross(mc, u, x);
  dyn_cross(mc, w, y);
  n[0] = ((I[0] * w[0] + I[1] * w[1]) + I[2] * w[2]) + x[0];
  n[1] = ((I[1] * w[0] + I[3] * w[1]) + I[4] * w[2]) + x[1];
  n[2] = ((I[2] * w[0] + I[4] * w[1]) + I[5] * w[2]) + x[2];
  for (int k = 0; k < 3; ++k) f[k] = ms * u[k] - y[k];
}

// The cached (c, s) of every body at the row's q (rounded to float32).
template <class Q>
CDX_HD void dyn_trig(const cdx_chain& c, const Q& q, const DynMem& m) {
  for (int i = 0; i < c.n_bodies; ++i) {
    const cdx_body& b = c.bodies[i];
    float cc = 1.f, ss = 0.f;
    if (i > 0 && b.dof >= 0) {
      const float th = b.sign * (float)q[b.dof];
      cc = dyn_cosf(th);
      ss = dyn_sinf(th);
    }
    m.cs[(size_t)(2 * i) * m.s] = cc;
    m.cs[(size_t)(2 * i + 1) * m.s] = ss;
  }
}

// One inverse-dynamics pass after dyn_trig (see above): out(dof, τ) once per moving joint, without the damping term.
// g: the gravity vector in the base frame (3 doubles), tipF: [n_tips][3] or null.
template <class QD, class QDD, class OUT>
CDX_HD void dyn_rnea(const cdx_chain& c, const cdx_dyn& dy, const DynMem& m, const QD& qd, const QDD& qdd,
                     const double* g, const double* tipF, OUT&& out) {
  const int n = c.n_bodies, s = m.s;
  for (int k = 0; k < 9; ++k) m.B[(size_t)k * s] = 0.0;
  for (int k = 0; k < 3; ++k) m.B[(size_t)(9 + k) * s] = -g[k];
  for (int i = 1; i < n; ++i) {
    const cdx_body& b = c.bodies[i];
    const double* P = m.B + (size_t)(12 * b.parent) * s;
    double* X = m.B + (size_t)(12 * i) * s;
    double E[9], st[12];
    dyn_body_E(c, m, i, E);
    for (int k = 0; k < 12; ++k) st[k] = P[(size_t)k * s];
    const double p[3] = {(double)b.t[0], (double)b.t[1], (double)b.t[2]};
    const double sg = (double)b.sign;
    double wj[3], zj[3];
    dyn_axis_vec(b.axis, b.dof >= 0 ? sg * qd[b.dof] : 0.0, wj);
    dyn_axis_vec(b.axis, b.dof >= 0 ? sg * qdd[b.dof] : 0.0, zj);
    double x[3], y[3], w[3], v[3], al[3], a[3];
    mat3t_vec(E, st, w);
    for (int k = 0; k < 3; ++k) w[k] = w[k] + wj[k];
    dyn_cross(st, p, x);
    for (int k = 0; k < 3; ++k) y[k] = st[3 + k] + x[k];
    mat3t_vec(E, y, v);
    mat3t_vec(E, st + 6, al);
    dyn_cross(w, wj, x);
    for (int k = 0; k < 3; ++k) al[k] = (al[k] + zj[k]) + x[k];
    dyn_cross(st + 6, p, x);
    for (int k = 0; k < 3; ++k) y[k] = st[9 + k] + x[k];
    mat3t_vec(E, y, a);
    dyn_cross(v, wj, x);
    for (int k = 0; k < 3; ++k) a[k] = a[k] + x[k];
    for (int k = 0; k < 3; ++k) {
      X[(size_t)k * s] = w[k];
      X[(size_t)(3 + k) * s] = v[k];
      X[(size_t)(6 + k) * s] = al[k];
      X[(size_t)(9 + k) * s] = a[k];
    }
  }
  // own forces over the motion state: slots 0..2 = n_i, 3..5 = f_i
  for (int i = 1; i < n; ++i) {
    double* X = m.B + (size_t)(12 * i) * s;
    double st[12];
    for (int k = 0; k < 12; ++k) st[k] = X[(size_t)k * s];
    double na[3], fa[3], hn[3], hf[3], x[3], y[3], z[3];
    dyn_inertia_mul(dy, i, st + 6, st + 9, na, fa);
    dyn_inertia_mul(dy, i, st, st + 3, hn, hf);
    dyn_cross(st, hn, x);
    dyn_cross(st + 3, hf, y);
    dyn_cross(st, hf, z);
    for (int k = 0; k < 3; ++k) {
      X[(size_t)k * s] = na[k] + (x[k] + y[k]);
      X[(size_t)(3 + k) * s] = fa[k] + z[k];
    }
  }
  if (tipF)
    for (int t = 0; t < c.n_tips; ++t) {
      const int body = c.tip_body[t];
      if (body <= 0) continue;  // (a force on the base loads no joint)
      double R[9], E[9], Rn[9];
      dyn_body_E(c, m, body, R);
      for (int b = c.bodies[body].parent; b > 0; b = c.bodies[b].parent) {
        dyn_body_E(c, m, b, E);
        mat3_mul(E, R, Rn);
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
      }
      double fl[3], fn[3] = {0.0, 0.0, 0.0};
      mat3t_vec(R, tipF + 3 * t, fl);
      if (c.has_offsets) {
        const double o[3] = {(double)c.tip_offset[t][0], (double)c.tip_offset[t][1], (double)c.tip_offset[t][2]};
        dyn_cross(o, fl, fn);
      }
      double* X = m.B + (size_t)(12 * body) * s;
      for (int k = 0; k < 3; ++k) {
        X[(size_t)k * s] = X[(size_t)k * s] - fn[k];
        X[(size_t)(3 + k) * s] = X[(size_t)(3 + k) * s] - fl[k];
      }
    }
  for (int i = n - 1; i >= 1; --i) {
    const cdx_body& b = c.bodies[i];
    const double* X = m.B + (size_t)(12 * i) * s;
    double f[6];
    for (int k = 0; k < 6; ++k) f[k] = X[(size_t)k * s];
    if (b.dof >= 0) {
      const int ax = b.axis;
      out((int)b.dof, (double)b.sign * (ax == 0 ? f[0] : (ax == 1 ? f[1] : f[2])));
    }
    if (b.parent > 0) {
      double E[9], En[3], Ef[3], x[3];
      dyn_body_E(c, m, i, E);
      mat3_vec(E, f, En);
      mat3_vec(E, f + 3, Ef);
      const double p[3] = {(double)b.t[0], (double)b.t[1], (double)b.t[2]};
      dyn_cross(p, Ef, x);
      double* P = m.B + (size_t)(12 * b.parent) * s;
      for (int k = 0; k < 3; ++k) {
        P[(size_t)k * s] = P[(size_t)k * s] + (En[k] + x[k]);
        P[(size_t)(3 + k) * s] = P[(size_t)(3 + k) * s] + Ef[k];
      }
    }
  }
}

// Writers of a row's outputs in the I/O dtype.
struct DynOut {
  void* p;
  int f64;
  CDX_HDM void set(int64_t i, double v) const {
    if (f64)
      ((double*)p)[i] = v;
    else
      ((float*)p)[i] = (float)v;
  }
};

// The gravity of a row: g [3] of the call (device or host memory of the caller's side), or zero.
CDX_HD void dyn_gravity(int include_gravity, const double* gravity, double* g) {
  g[0] = g[1] = g[2] = 0.0;
  if (!include_gravity) return;
  if (gravity) {
    for (int k = 0; k < 3; ++k) g[k] = gravity[k];
  } else {
    g[2] = -9.81;
  }
}

// One row of cdx_dyn_inverse: tau [D] (row-relative writer).
CDX_HD void dyn_inverse_row(const cdx_chain& c, const cdx_dyn& dy, const DynMem& m, const DynVec& q, const DynVec& qd,
                            const DynVec& qdd, const double* g, int use_damping, const double* tipF, const DynOut& tau) {
  dyn_trig(c, q, m);
  dyn_rnea(c, dy, m, qd, qdd, g, tipF, [&](int d, double v) {
    // (robot_model.py:383-389; a null q̇ reads as 0)
    tau.set(d, use_damping ? v + dy.damping[d] * qd[d] : v);
  });
}

// One row of cdx_dyn_inertia: H [D][D].
CDX_HD void dyn_inertia_row(const cdx_chain& c, const cdx_dyn& dy, const DynMem& m, const DynVec& q, const DynOut& H) {
  const int D = c.n_dofs;
  const double g[3] = {0.0, 0.0, 0.0};
  const DynVec zero{nullptr, 1};
  dyn_trig(c, q, m);
  for (int j = 0; j < D; ++j)
    dyn_rnea(c, dy, m, zero, DynUnit{j}, g, nullptr, [&](int i, double v) {
      if (i >= j) {
        H.set((int64_t)i * D + j, v);
        H.set((int64_t)j * D + i, v);
      }
    });
}

// One row of cdx_dyn_forward: qdd [D].  The chain has no dead joint (dyn_has_dead_joint: the entry refuses it).
CDX_HD void dyn_forward_row(const cdx_chain& c, const cdx_dyn& dy, const DynMem& m, const DynVec& q, const DynVec& qd,
                            const DynVec& f, const double* g, int use_damping, const DynOut& qdd) {
  const int D = c.n_dofs, s = m.s;
  const double g0[3] = {0.0, 0.0, 0.0};
  const DynVec zero{nullptr, 1};
  dyn_trig(c, q, m);
  dyn_rnea(c, dy, m, qd, zero, g, nullptr, [&](int d, double v) {
    const double fd = use_damping ? f[d] - dy.damping[d] * qd[d] : f[d];
    m.y[(size_t)d * s] = fd - v;
  });
  for (int j = 0; j < D; ++j)
    dyn_rnea(c, dy, m, zero, DynUnit{j}, g0, nullptr, [&](int i, double v) {
      if (i >= j) m.A[(size_t)(i * (i + 1) / 2 + j) * s] = v;
    });
  // H = L·Lᵀ in place, then the two substitutions (ik_gram_solve's order)
  for (int i = 0; i < D; ++i)
    for (int j = 0; j <= i; ++j) {
      double sum = m.A[(size_t)(i * (i + 1) / 2 + j) * s];
      CDX_IK_UNROLL
      for (int k = 0; k < j; ++k) sum -= m.A[(size_t)(i * (i + 1) / 2 + k) * s] * m.A[(size_t)(j * (j + 1) / 2 + k) * s];
      if (i == j)
        m.A[(size_t)(i * (i + 1) / 2 + j) * s] = sqrt(sum);
      else
        m.A[(size_t)(i * (i + 1) / 2 + j) * s] = sum / m.A[(size_t)(j * (j + 1) / 2 + j) * s];
    }
  for (int i = 0; i < D; ++i) {
    double sum = m.y[(size_t)i * s];
    CDX_IK_UNROLL
    for (int k = 0; k < i; ++k) sum -= m.A[(size_t)(i * (i + 1) / 2 + k) * s] * m.y[(size_t)k * s];
    m.y[(size_t)i * s] = sum / m.A[(size_t)(i * (i + 1) / 2 + i) * s];
  }
  for (int i = D - 1; i >= 0; --i) {
    double sum = m.y[(size_t)i * s];
    CDX_IK_UNROLL
    for (int k = i + 1; k < D; ++k) sum -= m.A[(size_t)(k * (k + 1) / 2 + i) * s] * m.y[(size_t)k * s];
    m.y[(size_t)i * s] = sum / m.A[(size_t)(i * (i + 1) / 2 + i) * s];
  }
  for (int d = 0; d < D; ++d) qdd.set(d, m.y[(size_t)d * s]);
}

}  // namespace cdx
