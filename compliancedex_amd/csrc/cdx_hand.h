// Whole-hand sphere collision model: sphere placement, the penetration cost with its gradient with respect to the sphere
// centres, and the pull-back of that gradient to the joint angles and the palm pose.  Shared by the gfx950 kernels
// (cdx_hand.hip) and the host test build (host_ref.cpp), which therefore run the same operations in the same order.
//
//   placement  every body's pose by chain_step on (float)q along its root path — the recurrence fk_tip runs, so a body's
//              pose has the bits of fk_tip's final pose of a walk to that body — then c_h = R_b·c_local + t_b in float32
//              and c = Rp·(double)c_h + palm_pos in float64 (as collision_candidate promotes its anchors).
//   cost       float64 quadratic hinges p₊ = max(p, 0), C¹ in the centres:
//                object  p = r_s + m_obj − d_s              cost += w_obj·½p₊²    ∂/∂c_s = −w_obj·p₊·∇d_s
//                self    p = r_a + r_b + m_self − ‖c_a−c_b‖ cost += w_self·½p₊²   ∂/∂c_a = −w_self·p₊·(c_a−c_b)/ρ = −∂/∂c_b
//                floor   p = r_s + m_floor − (c_s.z − z₀)   cost += w_floor·½p₊²  ∂/∂c_s.z = −w_floor·p₊
//              and per class the largest penetration at zero margin with the sphere / pair that attains it.
//   pull-back  g_q[dof_j] = ω_j·Σ_s (c_h,s − o_j) × (Rpᵀ·g_s) over the spheres below joint j, g_pp = Σ g_s,
//              g_po[a] = Σ g_sᵀ·(∂Rp/∂a)·c_h,s — the true derivative (no quaternion is involved).
//
// Order of summation (what makes the device and the host build agree bit for bit, and a row's bits independent of the
// batch): a candidate is worked by CDX_HAND_LANES = 64 lanes; lane l owns the spheres l, l + 64, l + 128, l + 192 and
// adds their terms in that order — a sphere's own terms as object, floor, then its partners in ascending pair index (a
// pair's cost is counted on its lower sphere, its gradient on both: both sides compute the same p from the same
// squares) — and the 64 lane sums are joined by the fixed tree x[l] += x[l + off], off = 32, 16, …, 1.  A maximum is
// joined the same way with "larger value, then smaller index", which no order can change.
//
// The palm's sines and cosines come from hand_sincos, plain double arithmetic (fdlibm's reduction and kernels) that both
// builds round identically; the math libraries of the two differ in the last bit.  The formulas are euler_xyz's.
//
// A row with a non-finite input (centre, distance, distance gradient, pose, cotangent or palm angle; an angle beyond
// ±1e6 rad counts as one) is NaN in all of its float outputs, worst = −1: it never reaches another row.
#pragma once
#include "cdx_fk.h"

namespace cdx {

// ------------------------------------------------------------------ deterministic sin / cos (float64)
CDX_HD void hand_sincos(double x, double* sn, double* cs) {
  if (!(fabs(x) <= 1e6)) {
    *sn = *cs = (double)NAN;
    return;
  }
  const double fn = rint(x * 6.36619772367581382433e-01);
  // three-part π/2 (33 + 33 + 53 bits): fn·p1 and fn·p2 are exact for |fn| < 2²⁰
  const double r = (x - fn * 1.57079632673412561417e+00) - fn * 6.07710050630396597660e-11;
  const double w = fn * 2.02226624879595063154e-21;
  const double y0 = r - w, y1 = (r - y0) - w;
  const double z = y0 * y0;
  const double v = z * y0;
  const double rs = 8.33333333332248946124e-03 +
                    z * (-1.98412698298579493134e-04 +
                         z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double ks = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * -1.66666666666666324348e-01);
  const double rc = z * (4.16666666666666019037e-02 +
                         z * (-1.38888888888741095749e-03 +
                              z * (2.48015872894767294178e-05 +
                                   z * (-2.75573143513906633035e-07 +
                                        z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, wc = 1.0 - hz;
  const double kc = wc + (((1.0 - wc) - hz) + (z * rc - y0 * y1));
  const int n = (int)((long long)fn & 3);
  *sn = n == 0 ? ks : (n == 1 ? kc : (n == 2 ? -ks : -kc));
  *cs = n == 0 ? kc : (n == 1 ? -ks : (n == 2 ? -kc : ks));
}

CDX_HD void hand_rot_axis(int axis, double a, double* R, double* dR) {
  double s, c;
  hand_sincos(a, &s, &c);
  for (int i = 0; i < 9; ++i) { R[i] = 0.0; dR[i] = 0.0; }
  if (axis == 0) {
    R[0] = 1; R[4] = c; R[5] = -s; R[7] = s; R[8] = c;
    dR[4] = -s; dR[5] = -c; dR[7] = c; dR[8] = -s;
  } else if (axis == 1) {
    R[0] = c; R[2] = s; R[4] = 1; R[6] = -s; R[8] = c;
    dR[0] = -s; dR[2] = c; dR[6] = -c; dR[8] = -s;
  } else {
    R[0] = c; R[1] = -s; R[3] = s; R[4] = c; R[8] = 1;
    dR[0] = -s; dR[1] = -c; dR[3] = c; dR[4] = -s;
  }
}

// euler_xyz (cdx_cost.h) on hand_sincos: R = (Rx(a)·Ry(b))·Rz(c) and, optionally, its three partials.
CDX_HD void hand_euler(const double* ang, double* R, double* dRa, double* dRb, double* dRc) {
  double X[9], dX[9], Y[9], dY[9], Z[9], dZ[9], XY[9];
  hand_rot_axis(0, ang[0], X, dX);
  hand_rot_axis(1, ang[1], Y, dY);
  hand_rot_axis(2, ang[2], Z, dZ);
  mat3_mul(X, Y, XY);
  mat3_mul(XY, Z, R);
  if (dRa) {
    double t[9];
    mat3_mul(dX, Y, t); mat3_mul(t, Z, dRa);
    mat3_mul(X, dY, t); mat3_mul(t, Z, dRb);
    mat3_mul(XY, dZ, dRc);
  }
}

CDX_HD bool hand_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }  // false for NaN and ±inf

// ------------------------------------------------------------------ tables
// The chain check of the three entries: chain_code's without its tips, and with EVERY body at most CDX_MAX_DEPTH
// levels below the root (chain_path_mask stops there).
CDX_HD int hand_chain_code(const cdx_chain* c) {
  if (!c) return CDX_ECHAIN;
  if (c->n_bodies <= 0 || c->n_bodies > CDX_MAX_BODIES || c->n_dofs < 0 || c->n_dofs > CDX_MAX_DOFS) return CDX_EINVAL;
  for (int i = 1; i < c->n_bodies; ++i) {
    if (c->bodies[i].parent < 0 || c->bodies[i].parent >= i || c->bodies[i].dof >= c->n_dofs || c->bodies[i].dof < -1 ||
        c->bodies[i].axis < 0 || c->bodies[i].axis > 2)
      return CDX_ECHAIN;
    int depth = 0;
    for (int b = i; b > 0; b = c->bodies[b].parent) ++depth;
    if (depth > CDX_MAX_DEPTH) return CDX_ECHAIN;
  }
  return CDX_OK;
}

// Slots of the partner table: a group of 64 spheres (one per lane) keeps entry k of its sphere l at base + 64k + l, so
// a wave reads consecutive words; a group is as long as its longest list, at most min(S − 1, P).
CDX_HD int hand_entries(int S, int P) {
  const int groups = (S + CDX_HAND_LANES - 1) / CDX_HAND_LANES, longest = P < S - 1 ? P : S - 1;
  return groups * CDX_HAND_LANES * longest;
}

// What the entries can see of a prepared model (its tables are in device memory).
CDX_HD int hand_code(const cdx_hand* h) {
  if (!h) return CDX_EINVAL;
  if (h->n_spheres < 1 || h->n_spheres > CDX_MAX_SPHERES || h->n_pairs < 0 || h->n_pairs > CDX_HAND_MAX_PAIRS ||
      h->n_bodies < 1 || h->n_bodies > CDX_MAX_BODIES)
    return CDX_EINVAL;
  if (!h->local || !h->radius || !h->body || !h->len || (h->n_pairs > 0 && (!h->pairs || !h->entry))) return CDX_EINVAL;
  for (int g = 0; g < CDX_MAX_SPHERES / CDX_HAND_LANES; ++g)
    if (h->group_base[g] < 0 || h->group_base[g] > hand_entries(h->n_spheres, h->n_pairs)) return CDX_EINVAL;
  return CDX_OK;
}

CDX_HD size_t hand_up8(size_t n) { return (n + 7) & ~(size_t)7; }
CDX_HD size_t hand_bytes(int S, int P) {
  if (S < 1 || S > CDX_MAX_SPHERES || P < 0 || P > CDX_HAND_MAX_PAIRS) return 0;
  return (size_t)S * 8 + hand_up8((size_t)S * 12) + 2 * hand_up8((size_t)S * 4) + hand_up8((size_t)P * 8) +
         hand_up8((size_t)hand_entries(S, P) * 4);
}
// The descriptor of tables laid out at `base` (radius, local, body, len, pairs, entry); group_base is left to hand_fill.
CDX_HD void hand_layout(int n_bodies, int S, int P, char* base, cdx_hand* h) {
  h->n_spheres = S;
  h->n_pairs = P;
  h->n_bodies = n_bodies;
  h->_pad = 0;
  char* p = base;
  h->radius = (const double*)p; p += (size_t)S * 8;
  h->local = (const float*)p; p += hand_up8((size_t)S * 12);
  h->body = (const int32_t*)p; p += hand_up8((size_t)S * 4);
  h->len = (const int32_t*)p; p += hand_up8((size_t)S * 4);
  h->pairs = (const int32_t*)p; p += hand_up8((size_t)P * 8);
  h->entry = (const int32_t*)p;
}

// Checks the caller's tables and fills the ones at `base` (HOST memory, hand_bytes(S, P) bytes) and h->group_base:
// spheres sorted by body, finite centres, finite radii > 0, pairs 0 ≤ a < b < S; every sphere's partner list in
// ascending pair index, an entry = partner | pair << 8.  CDX_EINVAL otherwise, with nothing written.
inline int hand_fill(int n_bodies, int S, const float* local, const double* radius, const int32_t* body, int P,
                     const int32_t* pairs, char* base, cdx_hand* h) {
  if (n_bodies < 1 || n_bodies > CDX_MAX_BODIES || hand_bytes(S, P) == 0 || !local || !radius || !body || !base || !h ||
      (P > 0 && !pairs))
    return CDX_EINVAL;
  for (int s = 0; s < S; ++s) {
    if (body[s] < 0 || body[s] >= n_bodies || (s > 0 && body[s] < body[s - 1])) return CDX_EINVAL;
    if (!hand_finite(radius[s]) || !(radius[s] > 0.0)) return CDX_EINVAL;
    for (int i = 0; i < 3; ++i)
      if (!hand_finite((double)local[3 * s + i])) return CDX_EINVAL;
  }
  int32_t count[CDX_MAX_SPHERES];
  for (int s = 0; s < S; ++s) count[s] = 0;
  for (int p = 0; p < P; ++p) {
    if (pairs[2 * p] < 0 || pairs[2 * p] >= pairs[2 * p + 1] || pairs[2 * p + 1] >= S) return CDX_EINVAL;
    ++count[pairs[2 * p]];
    ++count[pairs[2 * p + 1]];
  }
  // (a list is at most min(S − 1, P) long only if no pair repeats: a longer one is refused)
  const int longest = P < S - 1 ? P : S - 1;
  for (int s = 0; s < S; ++s)
    if (count[s] > longest) return CDX_EINVAL;
  hand_layout(n_bodies, S, P, base, h);
  double* r = const_cast<double*>(h->radius);
  float* l = const_cast<float*>(h->local);
  int32_t* b = const_cast<int32_t*>(h->body);
  int32_t* len = const_cast<int32_t*>(h->len);
  int32_t* pr = const_cast<int32_t*>(h->pairs);
  int32_t* en = const_cast<int32_t*>(h->entry);
  for (int s = 0; s < S; ++s) {
    r[s] = radius[s];
    b[s] = body[s];
    len[s] = 0;
    for (int i = 0; i < 3; ++i) l[3 * s + i] = local[3 * s + i];
  }
  int at = 0;
  for (int g = 0; g < CDX_MAX_SPHERES / CDX_HAND_LANES; ++g) {
    h->group_base[g] = at;
    int m = 0;
    for (int s = g * CDX_HAND_LANES; s < S && s < (g + 1) * CDX_HAND_LANES; ++s) m = count[s] > m ? count[s] : m;
    at += m * CDX_HAND_LANES;
  }
  for (int i = 0; i < hand_entries(S, P); ++i) en[i] = -1;
  for (int p = 0; p < P; ++p) {
    pr[2 * p] = pairs[2 * p];
    pr[2 * p + 1] = pairs[2 * p + 1];
    for (int side = 0; side < 2; ++side) {
      const int s = pairs[2 * p + side], k = len[s]++;
      en[h->group_base[s / CDX_HAND_LANES] + k * CDX_HAND_LANES + s % CDX_HAND_LANES] = pairs[2 * p + 1 - side] | (p << 8);
    }
  }
  return CDX_OK;
}

// ------------------------------------------------------------------ placement
// Pose of `body` in the hand frame, pose[12] = R row-major then t: fk_tip's walk to that body.
template <class Q>
CDX_HD void hand_body_pose(const cdx_chain& c, int body, const Q& q, float* pose) {
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, t[3] = {0.f, 0.f, 0.f};
  for (uint32_t m = chain_path_mask(c, body); m; m &= m - 1) {
    float Rn[9], tn[3];
    chain_step(c.bodies[low_bit(m)], q, R, t, Rn, tn);
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    for (int i = 0; i < 3; ++i) t[i] = tn[i];
  }
  for (int i = 0; i < 9; ++i) pose[i] = R[i];
  for (int i = 0; i < 3; ++i) pose[9 + i] = t[i];
}

// c_h = R_b·c_local + t_b in float32.
CDX_HD void hand_center_local(const float* pose, const float* cl, float* ch) {
  float v[3];
  mat3_vec(pose, cl, v);
  for (int i = 0; i < 3; ++i) ch[i] = v[i] + pose[9 + i];
}

// c = Rp·(double)c_h + pp.
CDX_HD void hand_center_world(const double* Rp, const double* pp, const float* ch, double* c) {
  const double v[3] = {(double)ch[0], (double)ch[1], (double)ch[2]};
  double w[3];
  mat3_vec(Rp, v, w);
  for (int i = 0; i < 3; ++i) c[i] = w[i] + pp[i];
}

// ------------------------------------------------------------------ cost
struct HandBest {
  double v;
  int32_t i;
};
CDX_HD bool hand_beats(double v, int32_t i, double bv, int32_t bi) { return v > bv || (v == bv && i < bi); }
CDX_HD void hand_offer(HandBest& b, double v, int32_t i) {
  if (hand_beats(v, i, b.v, b.i)) { b.v = v; b.i = i; }
}
CDX_HD double hand_hinge(double p) { return p > 0.0 ? p : (p == p ? 0.0 : p); }

// One sphere's terms.  cen / rad: the row's centres [S·3] and the radii [S] (LDS on the device).  cost and the three
// bests are accumulated into; g [3] is written.  Returns false when an input of this sphere is not finite.
CDX_HD bool hand_sphere_terms(const cdx_hand& H, const cdx_hand_params& P, int s, const double* cen, const double* rad,
                              const double* dist, const double* gdist, double& cost, double* g, HandBest& bo,
                              HandBest& bs, HandBest& bf) {
  const double c[3] = {cen[3 * s], cen[3 * s + 1], cen[3 * s + 2]};
  const double r = rad[s];
  bool ok = hand_finite(c[0]) && hand_finite(c[1]) && hand_finite(c[2]);
  g[0] = g[1] = g[2] = 0.0;
  if (dist) {
    const double d = dist[s], gd[3] = {gdist[3 * s], gdist[3 * s + 1], gdist[3 * s + 2]};
    ok = ok && hand_finite(d) && hand_finite(gd[0]) && hand_finite(gd[1]) && hand_finite(gd[2]);
    const double ph = hand_hinge((r + P.m_obj) - d);
    cost += P.w_obj * 0.5 * (ph * ph);
    const double k = P.w_obj * ph;
    for (int i = 0; i < 3; ++i) g[i] -= k * gd[i];
    hand_offer(bo, r - d, s);
  }
  if (P.floor_on) {
    const double h = c[2] - P.floor_z;
    const double ph = hand_hinge((r + P.m_floor) - h);
    cost += P.w_floor * 0.5 * (ph * ph);
    g[2] -= P.w_floor * ph;
    hand_offer(bf, r - h, s);
  }
  const int32_t* list = H.entry + H.group_base[s / CDX_HAND_LANES] + s % CDX_HAND_LANES;
  for (int k = 0, n = H.len[s]; k < n; ++k) {
    const int32_t en = list[k * CDX_HAND_LANES];
    const int o = en & 255;
    const double d[3] = {c[0] - cen[3 * o], c[1] - cen[3 * o + 1], c[2] - cen[3 * o + 2]};
    const double rho = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const double rr = r + rad[o];
    const double ph = hand_hinge((rr + P.m_self) - rho);
    if (rho > 0.0) {
      const double f = (P.w_self * ph) / rho;
      for (int i = 0; i < 3; ++i) g[i] -= f * d[i];
    }
    if (s < o) {
      cost += P.w_self * 0.5 * (ph * ph);
      hand_offer(bs, rr - rho, en >> 8);
    }
  }
  return ok;
}

// One step of the lane tree on the four reduced quantities: rv [4][64] = cost and the three class maxima, ri [3][64]
// their indices.
CDX_HD void hand_cost_join(double* rv, int32_t* ri, int l, int off) {
  rv[l] += rv[l + off];
  for (int k = 0; k < 3; ++k) {
    const double v = rv[(1 + k) * CDX_HAND_LANES + l + off];
    const int32_t i = ri[k * CDX_HAND_LANES + l + off];
    if (hand_beats(v, i, rv[(1 + k) * CDX_HAND_LANES + l], ri[k * CDX_HAND_LANES + l])) {
      rv[(1 + k) * CDX_HAND_LANES + l] = v;
      ri[k * CDX_HAND_LANES + l] = i;
    }
  }
}

// Lane l's share of a row: its spheres' gradients into g_centers, its sums into slot l of rv / ri.
CDX_HD bool hand_cost_lane(const cdx_hand& H, const cdx_hand_params& P, int l, const double* cen, const double* rad,
                           const double* dist, const double* gdist, double* g_centers, double* rv, int32_t* ri) {
  const double ninf = -(double)INFINITY;
  double cost = 0.0;
  HandBest bo{ninf, -1}, bs{ninf, -1}, bf{ninf, -1};
  bool ok = true;
  for (int s = l; s < H.n_spheres; s += CDX_HAND_LANES) {
    double g[3];
    ok = hand_sphere_terms(H, P, s, cen, rad, dist, gdist, cost, g, bo, bs, bf) && ok;
    for (int i = 0; i < 3; ++i) g_centers[3 * s + i] = g[i];
  }
  rv[l] = cost;
  rv[CDX_HAND_LANES + l] = bo.v; ri[l] = bo.i;
  rv[2 * CDX_HAND_LANES + l] = bs.v; ri[CDX_HAND_LANES + l] = bs.i;
  rv[3 * CDX_HAND_LANES + l] = bf.v; ri[2 * CDX_HAND_LANES + l] = bf.i;
  return ok;
}

// The row's results from slot 0 after the tree (bad: an input of the row was not finite).
CDX_HD void hand_cost_finish(bool bad, const double* rv, const int32_t* ri, double* cost, double* depth, int32_t* worst) {
  *cost = bad ? (double)NAN : rv[0];
  for (int k = 0; k < 3; ++k) {
    depth[k] = bad ? (double)NAN : rv[(1 + k) * CDX_HAND_LANES];
    worst[k] = bad ? -1 : ri[k * CDX_HAND_LANES];
  }
}

// ------------------------------------------------------------------ pull-back
// Lane l's spheres: c_h and Rpᵀ·g into st [S·6] (c_h, then g_h), their bodies into sb [S], and its sums of g_s (3) and g_sᵀ·dR_a·c_h (3) into
// slot l of rv [6][64].
CDX_HD bool hand_pull_lane(const cdx_hand& H, int l, const float* poses, const double* g_centers, const double* Rp,
                           const double* dRa, const double* dRb, const double* dRc, double* st, int32_t* sb, double* rv) {
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = true;
  for (int s = l; s < H.n_spheres; s += CDX_HAND_LANES) {
    float chf[3];
    const int32_t b = H.body[s];
    sb[s] = b;
    hand_center_local(poses + 12 * b, H.local + 3 * s, chf);
    const double ch[3] = {(double)chf[0], (double)chf[1], (double)chf[2]};
    const double g[3] = {g_centers[3 * s], g_centers[3 * s + 1], g_centers[3 * s + 2]};
    double gh[3], v[3];
    mat3t_vec(Rp, g, gh);
    for (int i = 0; i < 3; ++i) {
      ok = ok && hand_finite(ch[i]) && hand_finite(g[i]);
      st[6 * s + i] = ch[i];
      st[6 * s + 3 + i] = gh[i];
      acc[i] += g[i];
    }
    mat3_vec(dRa, ch, v); acc[3] += dot3(g, v);
    mat3_vec(dRb, ch, v); acc[4] += dot3(g, v);
    mat3_vec(dRc, ch, v); acc[5] += dot3(g, v);
  }
  for (int k = 0; k < 6; ++k) rv[k * CDX_HAND_LANES + l] = acc[k];
  return ok;
}

// g_q of DOF d: over the bodies it moves (one in a well-formed chain), ω_j·Σ_s (c_h,s − o_j) × g_h,s in ascending s
// over the spheres whose body has j on its root path (mask [n_bodies]: chain_path_mask of every body; sb [S]: the
// spheres' bodies).  The lanes of a wave search their bodies first and then walk the spheres together: st, sb and
// mask are read at one address by all of them.
CDX_HD double hand_pull_dof(const cdx_chain& c, const cdx_hand& H, int d, const float* poses, const uint32_t* mask,
                            const double* st, const int32_t* sb, bool* ok) {
  double gq = 0.0;
  int j = 0;
  for (;;) {
    for (++j; j < c.n_bodies && !(c.bodies[j].dof == d && c.bodies[j].sign != 0.f); ++j) {}
    if (j >= c.n_bodies) break;
    const float* pj = poses + 12 * j;
    const int ax = c.bodies[j].axis;
    const double sg = (double)c.bodies[j].sign;
    const double om[3] = {sg * (double)pj[ax], sg * (double)pj[3 + ax], sg * (double)pj[6 + ax]};
    const double o[3] = {(double)pj[9], (double)pj[10], (double)pj[11]};
    for (int i = 0; i < 3; ++i) *ok = *ok && hand_finite(om[i]) && hand_finite(o[i]);
    double a[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < H.n_spheres; ++s) {
      if (!((mask[sb[s]] >> j) & 1u)) continue;
      const double r[3] = {st[6 * s] - o[0], st[6 * s + 1] - o[1], st[6 * s + 2] - o[2]};
      const double* g = st + 6 * s + 3;
      a[0] += r[1] * g[2] - r[2] * g[1];
      a[1] += r[2] * g[0] - r[0] * g[2];
      a[2] += r[0] * g[1] - r[1] * g[0];
    }
    gq += dot3(om, a);
  }
  return gq;
}

// ------------------------------------------------------------------ whole rows (the host build; the kernels run the
// same pieces across lanes)
inline void hand_spheres_row(const cdx_chain& c, const cdx_hand& H, const double* q, const double* pp, const double* po,
                             float* poses, double* centers) {
  const double zero[3] = {0.0, 0.0, 0.0};
  double Rp[9];
  hand_euler(po ? po : zero, Rp, nullptr, nullptr, nullptr);
  for (int b = 0; b < c.n_bodies; ++b) hand_body_pose(c, b, QRowD{q}, poses + 12 * b);
  for (int s = 0; s < H.n_spheres; ++s) {
    float ch[3];
    hand_center_local(poses + 12 * H.body[s], H.local + 3 * s, ch);
    hand_center_world(Rp, pp ? pp : zero, ch, centers + 3 * s);
  }
}

inline void hand_cost_row(const cdx_hand& H, const cdx_hand_params& P, const double* centers, const double* dist,
                          const double* gdist, double* cost, double* depth, int32_t* worst, double* g_centers) {
  double rv[4 * CDX_HAND_LANES];
  int32_t ri[3 * CDX_HAND_LANES];
  bool ok = true;
  for (int l = 0; l < CDX_HAND_LANES; ++l)
    ok = hand_cost_lane(H, P, l, centers, H.radius, dist, gdist, g_centers, rv, ri) && ok;
  for (int off = CDX_HAND_LANES / 2; off; off >>= 1)
    for (int l = 0; l < off; ++l) hand_cost_join(rv, ri, l, off);
  hand_cost_finish(!ok, rv, ri, cost, depth, worst);
  if (!ok)
    for (int i = 0; i < 3 * H.n_spheres; ++i) g_centers[i] = (double)NAN;
}

inline void hand_pullback_row(const cdx_chain& c, const cdx_hand& H, const float* poses, const double* g_centers,
                              const double* po, double* g_q, double* g_pp, double* g_po) {
  const double zero[3] = {0.0, 0.0, 0.0};
  double Rp[9], dRa[9], dRb[9], dRc[9];
  hand_euler(po ? po : zero, Rp, dRa, dRb, dRc);
  bool ok = true;
  for (int i = 0; i < 9; ++i) ok = ok && hand_finite(Rp[i]);
  double st[6 * CDX_MAX_SPHERES], rv[6 * CDX_HAND_LANES];
  int32_t sb[CDX_MAX_SPHERES];
  uint32_t mask[CDX_MAX_BODIES];
  for (int b = 0; b < c.n_bodies; ++b) mask[b] = chain_path_mask(c, b);
  for (int l = 0; l < CDX_HAND_LANES; ++l) ok = hand_pull_lane(H, l, poses, g_centers, Rp, dRa, dRb, dRc, st, sb, rv) && ok;
  for (int off = CDX_HAND_LANES / 2; off; off >>= 1)
    for (int l = 0; l < off; ++l)
      for (int k = 0; k < 6; ++k) rv[k * CDX_HAND_LANES + l] += rv[k * CDX_HAND_LANES + l + off];
  for (int d = 0; d < c.n_dofs; ++d) g_q[d] = hand_pull_dof(c, H, d, poses, mask, st, sb, &ok);
  for (int i = 0; i < 3; ++i) {
    g_pp[i] = rv[i * CDX_HAND_LANES];
    g_po[i] = rv[(3 + i) * CDX_HAND_LANES];
  }
  if (!ok) {
    for (int d = 0; d < c.n_dofs; ++d) g_q[d] = (double)NAN;
    for (int i = 0; i < 3; ++i) g_pp[i] = g_po[i] = (double)NAN;
  }
}

// ------------------------------------------------------------------ the term (cdx_hand_term)
// The cost and its pull-back as one weighted term of a caller's loss: x is what hand_cost_row and hand_pullback_row
// give (g_centers never leaves the row's worker), and every output element is weight·x, or old + weight·x when the
// term accumulates — two roundings, the product first (the file is compiled without contraction).  A bad row is NaN.
CDX_HD double hand_term_out(double old, double x, double weight, bool accumulate, bool bad) {
  if (bad) return (double)NAN;
  const double wx = weight * x;
  return accumulate ? old + wx : wx;
}

inline void hand_term_row(const cdx_chain& c, const cdx_hand& H, const cdx_hand_params& P, const float* poses,
                          const double* centers, const double* dist, const double* gdist, const double* po,
                          double weight, bool accumulate, double* loss, double* g_q, double* g_pp, double* g_po,
                          double* depth, int32_t* worst) {
  double gc[3 * CDX_MAX_SPHERES], cost, dp[3], gq[CDX_MAX_DOFS > 0 ? CDX_MAX_DOFS : 1], gpp[3], gpo[3];
  int32_t wi[3];
  hand_cost_row(H, P, centers, dist, gdist, &cost, dp, wi, gc);
  hand_pullback_row(c, H, poses, gc, po, gq, gpp, gpo);
  *loss = hand_term_out(accumulate ? *loss : 0.0, cost, weight, accumulate, !(cost == cost));
  for (int k = 0; k < 3; ++k) {
    if (depth) depth[k] = dp[k];
    if (worst) worst[k] = wi[k];
  }
  for (int d = 0; d < c.n_dofs && g_q; ++d)
    g_q[d] = hand_term_out(accumulate ? g_q[d] : 0.0, gq[d], weight, accumulate, !(gq[d] == gq[d]));
  for (int i = 0; i < 3; ++i) {
    if (g_pp) g_pp[i] = hand_term_out(accumulate ? g_pp[i] : 0.0, gpp[i], weight, accumulate, !(gpp[i] == gpp[i]));
    if (g_po) g_po[i] = hand_term_out(accumulate ? g_po[i] : 0.0, gpo[i], weight, accumulate, !(gpo[i] == gpo[i]));
  }
}

// Argument checks of cdx_hand_term after the chain, model and parameter codes (0 ≤ E checked by the caller).
CDX_HD int hand_term_code(const cdx_chain* c, const cdx_hand* h, int64_t E, const float* poses, const double* centers,
                          const double* dist, const double* gdist, double weight, int32_t accumulate,
                          const double* loss, const double* g_q) {
  if (h->n_bodies != c->n_bodies || E < 0 || E > 0x7fffffff || (dist == nullptr) != (gdist == nullptr)) return CDX_EINVAL;
  if (!hand_finite(weight) || (accumulate != 0 && accumulate != 1)) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!poses || !centers || !loss || (!g_q && c->n_dofs > 0)) return CDX_EINVAL;
  return CDX_OK;
}

// Argument checks shared by the device entries and the host build (after the chain / model codes).
CDX_HD int hand_params_code(const cdx_hand_params* p) {
  if (!p) return CDX_EINVAL;
  const double v[7] = {p->m_obj, p->m_self, p->m_floor, p->w_obj, p->w_self, p->w_floor, p->floor_z};
  for (int i = 0; i < 7; ++i)
    if (!hand_finite(v[i])) return CDX_EINVAL;
  return CDX_OK;
}

}  // namespace cdx
