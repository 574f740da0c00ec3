// Per-candidate math of the GPIS-mode optimisers (GPISGraspOptimizer, optimize_pregrasp.py:322-406, mode 0;
// KinGPISGraspOptimizer, :408-511, mode 1): the iteration's loss and its gradient in closed form from the
// per-point GPIS data (mean / ∇mean / normal / std / ∇std at the fingertips, mean / ∇mean at the targets), and the
// optimiser step (best iterate, RMSprop, clamps, next fingertips).  Everything is f64, as the reference runs
// these two modes; the FK of mode 1 and its backward are f32 like robot_model._FK.  Shared by cdx_gpis_mode.hip
// and the host build (libcdx_host.so), so the CPU tests check this very code against autograd.
//
//   mode 0:  l = −25·reward + 1000·Σ|mean| + 10·Σ tmean + 10·‖mean_t tip − mean_t target‖
//                − Σ_t min(fn_t·softmin(fn)_t, 1) + uncertainty·Σ std                               (:374-383)
//   mode 1:  l = −5·reward + 1000·Σ|mean| + 10·Σ tmean + (centre) + (force) + 20·‖q − ref_q‖
//                + max_t uncertainty·log(100·std_t)                                                (:473-486)
// Gradient rules (torch autograd's): sign(0) = 0, a zero 2-norm gives a zero gradient, clamp(max = 1) passes the
// gradient where it does not clamp, the max sends its gradient to the first maximal fingertip, normals are
// detached, the force term goes through ForceEq::backward as g_force_norm.
#pragma once
#include "cdx_cost.h"

namespace cdx {

CDX_HD uint64_t gm_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Element i of candidate e's Kabsch noise: the tape's value, or the counter-based draw keyed by (seed, row) of
// cdx_force_eq_* / cdx_kin_cost.
CDX_HD double gm_noise(const double* noise, uint64_t seed, int64_t e, int i) {
  return noise ? noise[e * 9 + i] : (double)(gm_mix(seed ^ gm_mix((uint64_t)(e * 9 + i))) >> 11) * 0x1.0p-53;
}

// Per-DOF accumulator of the f32 FK backward with a stride (a lane's column of an LDS array on the device).
struct GqStride {
  float* g;
  int stride;
  CDX_HDM void operator()(int d, float v) const { g[d * stride] += v; }
};

// Loss and gradients of candidate e.  FK: mode 1 (chain, q, ref_cost, log-variance max).  fk_g: D zeroed floats at
// `fk_stride` apart, scratch for the FK backward's per-DOF sums.  Writes loss[e], margin[e·T…], normal_out (the
// fingertip normals copied to the iteration's slot, nullable), g_target, g_comp, g_tip (mode 0: the pose gradient)
// and, FK, g_q.
template <int NT, int MAXD, bool FK>
CDX_HD void gpis_mode_cost_candidate(const cdx_chain& chain, const cdx_gpis_mode_params& p, int T_rt, int64_t e,
                                     const double* q, const double* tip, const double* target, const double* comp,
                                     const double* noise, uint64_t seed, const double* mean, const double* gmean,
                                     const double* normal, const double* std_, const double* gstd,
                                     const double* tmean, const double* tgmean, double* loss, double* margin,
                                     double* normal_out, double* g_q, double* g_target, double* g_comp, double* g_tip,
                                     float* fk_g, int fk_stride) {
  constexpr int NTA = NT > 0 ? NT : CDX_MAX_TIPS;
  const int T = NT > 0 ? NT : T_rt, D = FK ? chain.n_dofs : 0;
  // the candidate's rows are read in place (ForceEq keeps its own copies on its tape; the compliances are read again
  // by the backward): no second copy of them is held in registers across the reward
  const double(*tp)[3] = reinterpret_cast<const double(*)[3]>(tip + e * T * 3);
  const double(*nr)[3] = reinterpret_cast<const double(*)[3]>(normal + e * T * 3);
  const double* tg = target + e * T * 3;
  const double* cp = comp + e * T;
  if (normal_out)
    for (int i = 0; i < 3 * T; ++i) normal_out[e * T * 3 + i] = normal[e * T * 3 + i];
  double nz[9];
  for (int i = 0; i < 9; ++i) nz[i] = gm_noise(noise, seed, e, i);
  ForceEqParams fp;
  fp.cos_mu = (double)p.fe.cos_mu;
  fp.gravity = p.fe.gravity;
  for (int i = 0; i < 3; ++i) fp.com[i] = (double)p.fe.com[i];
  fp.dummy_target_z = (double)p.fe.dummy_target_z;
  fp.dummy_comp = (double)p.fe.dummy_comp;
  ForceEq<NT> fe;
  fe.forward(fp, T, tp, tg, cp, nr, nz);

  // ---- forward
  double ct[3] = {0, 0, 0}, cg[3] = {0, 0, 0};
  for (int f = 0; f < T; ++f)
    for (int i = 0; i < 3; ++i) { ct[i] += fe.S1[f][i]; cg[i] += fe.S2[f][i]; }
  double cd[3];
  for (int i = 0; i < 3; ++i) cd[i] = ct[i] / T - cg[i] / T;
  const double cn = sqrt(cd[0] * cd[0] + cd[1] * cd[1] + cd[2] * cd[2]);
  double qn = 0.0;
  if (FK) {
    double dq2 = 0.0;
    for (int i = 0; i < D; ++i) {
      const double d = q[e * D + i] - p.ref_q[i];
      dq2 += d * d;
    }
    qn = sqrt(dq2);
  }
  // distance, target-distance and variance terms; mode 1's max keeps its first maximal fingertip (a NaN wins, as
  // torch.max propagates it)
  double dcost = 0.0, tcost = 0.0, vsum = 0.0, vmax = 0.0;
  int fmax = 0;
  for (int f = 0; f < T; ++f) {
    const int64_t r = e * T + f;
    const double m = mean[r];
    dcost += m < 0 ? -m : m;
    tcost += tmean[r];
    if (FK) {
      const double v = p.uncertainty * log(100.0 * std_[r]);
      if (f == 0 || v > vmax || (v != v && vmax == vmax)) { vmax = v; fmax = f; }
    } else {
      vsum += std_[r];
    }
  }
  const double* fn = fe.fn;
  double zmax = -fn[0];
  for (int f = 1; f < T; ++f) zmax = -fn[f] > zmax ? -fn[f] : zmax;
  double ez[NTA], esum = 0.0;
  for (int f = 0; f < T; ++f) { ez[f] = exp(-fn[f] - zmax); esum += ez[f]; }
  double sm[NTA], v[NTA], fcost = 0.0;
  for (int f = 0; f < T; ++f) {
    sm[f] = ez[f] / esum;
    v[f] = fn[f] * sm[f];
    fcost += v[f] > 1.0 ? 1.0 : v[f];
  }
  const double g_rw = FK ? -5.0 : -25.0;
  loss[e] = FK ? fe.reward * g_rw + 1000.0 * dcost + 10.0 * tcost + cn * 10.0 - fcost + qn * 20.0 + vmax
               : fe.reward * g_rw + 1000.0 * dcost + 10.0 * tcost + cn * 10.0 - fcost + p.uncertainty * vsum;
  for (int f = 0; f < T; ++f) margin[e * T + f] = fe.margin[f];

  // ---- backward (dl = 1): the reward and force terms first (ForceEq accumulates into zeroed gradients), then the
  // cost terms' own gradients, whose operands are loaded only now instead of being held across the reward's backward
  double g_fn[NTA], gt[NTA][3], gg[NTA][3], gc[NTA];
  {
    double g_sm[NTA], gsm_dot = 0.0;
    for (int f = 0; f < T; ++f) {
      const double gvf = v[f] <= 1.0 ? -1.0 : 0.0;
      g_fn[f] = gvf * sm[f];
      g_sm[f] = gvf * fn[f];
      gsm_dot += g_sm[f] * sm[f];
    }
    for (int f = 0; f < T; ++f) g_fn[f] += -(sm[f] * (g_sm[f] - gsm_dot));
  }
  for (int f = 0; f < T; ++f) {
    gc[f] = 0.0;
    for (int i = 0; i < 3; ++i) gt[f][i] = gg[f][i] = 0.0;
  }
  fe.backward(g_rw, g_fn, cp, gt, gg, gc);
  for (int f = 0; f < T; ++f) {
    const int64_t r = e * T + f;
    const double m = mean[r];
    const double gd = 1000.0 * (double)((0.0 < m) - (m < 0.0));  // torch's sgn: 0 at 0
    double gv;  // d l / d std_f
    if (FK) {
      // log(100·std): autograd divides by the log's argument, then multiplies by 100
      gv = f == fmax ? (p.uncertainty / (100.0 * std_[r])) * 100.0 : 0.0;
    } else {
      gv = p.uncertainty;
    }
    for (int i = 0; i < 3; ++i) {
      const double gcen = cn > 0 ? 10.0 * cd[i] / cn / T : 0.0;
      gt[f][i] += gd * gmean[3 * r + i] + gcen + gv * gstd[3 * r + i];  // (0·∇std where the max is elsewhere, as autograd)
      gg[f][i] += 10.0 * tgmean[3 * r + i] - gcen;
    }
  }
  if (FK) {
    // g_tip (f64) → f32 → the f32 FK backward → f64, fingertip by fingertip like cdx_fk_backward
    for (int i = 0; i < D; ++i) fk_g[i * fk_stride] = 0.f;
    for (int f = 0; f < T; ++f) {
      const float gpos[3] = {(float)gt[f][0], (float)gt[f][1], (float)gt[f][2]};
      // hands (≤ 8 levels): cdx_fk_backward's walk, which keeps every level's rotation in registers; deeper chains
      // (arm + hand): the closed form with no per-level state (two walks; the same gradient to f32 rounding) — 16
      // levels of rotations on top of the reward's tape do not fit the register file
      if (MAXD <= 8) fk_tip_bwd<MAXD>(chain, f, QRowD{q + e * D}, gpos, GqStride{fk_g, fk_stride});
      else fk_tip_bwd2<MAXD>(chain, f, QRowD{q + e * D}, gpos, GqStride{fk_g, fk_stride});
    }
    for (int i = 0; i < D; ++i) {
      const double d = q[e * D + i] - p.ref_q[i];
      const double gq = qn > 0 ? 20.0 * d / qn : 0.0;
      g_q[e * D + i] = gq + (double)fk_g[i * fk_stride];
    }
  }
  for (int f = 0; f < T; ++f) {
    const int64_t r = e * T + f;
    g_comp[r] = gc[f];
    for (int i = 0; i < 3; ++i) {
      g_target[3 * r + i] = gg[f][i];
      if (g_tip) g_tip[3 * r + i] = gt[f][i];
    }
  }
}

// torch.optim.RMSprop (no momentum, not centred) in f64, the single-tensor order: v.mul_(α).addcmul_(g, g, 1 − α);
// p.addcdiv_(g, sqrt(v) + eps, −lr)
CDX_HD double gm_rmsprop(double p, double g, double& v, double a, double w2, double eps, double mlr) {
  v = v * a + (w2 * g) * g;
  const double avg = sqrt(v) + eps;
  return p + mlr * (g / avg);
}

CDX_HD double gm_clamp(double x, double lo, double hi) {  // torch.clamp: NaN stays NaN
  x = x < lo ? lo : x;
  return x > hi ? hi : x;
}

// Candidate e's step after its cost: the best iterate (on the parameters the loss was computed on), RMSprop, the
// clamps and — FK — the next fingertips.  Returns whether the candidate improved (the caller's `any` flag).
template <bool FK>
CDX_HD bool gpis_mode_step_candidate(const cdx_chain& chain, const cdx_gpis_mode_params& p, const cdx_gpis_mode_opt& cfg,
                                     const cdx_gpis_mode_buffers& b, int T, int64_t e) {
  const int D = FK ? chain.n_dofs : 0;
  const int np = FK ? D : 3 * T;  // pose entries of a candidate
  const double l = b.loss[e];
  const bool flag = l < b.opt_value[e];  // (false for a non-finite loss)
  if (flag) {
    b.opt_value[e] = l;
    for (int i = 0; i < np; ++i) b.opt_pose[e * np + i] = b.pose[e * np + i];
    for (int i = 0; i < 3 * T; ++i) b.opt_target[e * 3 * T + i] = b.target[e * 3 * T + i];
    for (int f = 0; f < T; ++f) b.opt_comp[e * T + f] = b.comp[e * T + f];
  }
  const double a = cfg.alpha, w2 = 1.0 - cfg.alpha, eps = cfg.eps;
  if (cfg.lr[0] != 0.0)
    for (int i = 0; i < np; ++i) {
      const int64_t k = e * np + i;
      double v = b.v_pose[k];
      b.pose[k] = gm_rmsprop(b.pose[k], b.g_pose[k], v, a, w2, eps, -cfg.lr[0]);
      b.v_pose[k] = v;
    }
  if (cfg.lr[1] != 0.0)
    for (int i = 0; i < 3 * T; ++i) {
      const int64_t k = e * 3 * T + i;
      double v = b.v_target[k];
      b.target[k] = gm_rmsprop(b.target[k], b.g_target[k], v, a, w2, eps, -cfg.lr[1]);
      b.v_target[k] = v;
    }
  if (cfg.lr[2] != 0.0)
    for (int f = 0; f < T; ++f) {
      const int64_t k = e * T + f;
      double v = b.v_comp[k];
      b.comp[k] = gm_rmsprop(b.comp[k], b.g_comp[k], v, a, w2, eps, -cfg.lr[2]);
      b.v_comp[k] = v;
    }
  // mode 0: tips into the box, comp ≥ comp_min (:399-401); mode 1: comp ≥ comp_min, TARGETS into the box whether
  // or not they are optimised (:503-505)
  double* boxed = FK ? b.target : b.pose;
  for (int i = 0; i < 3 * T; ++i) {
    const int64_t k = e * 3 * T + i;
    boxed[k] = gm_clamp(boxed[k], cfg.box_lb[i], cfg.box_ub[i]);
  }
  for (int f = 0; f < T; ++f) {
    const double c = b.comp[e * T + f];
    b.comp[e * T + f] = c < cfg.comp_min ? cfg.comp_min : c;
  }
  if (FK && b.tips)  // the next iteration's fingertips: double(FK_f32(float(q))) + palm_offset
    for (int f = 0; f < T; ++f) {
      float pos[3];
      fk_tip(chain, f, QRowD{b.pose + e * D}, pos, nullptr);
      for (int i = 0; i < 3; ++i) b.tips[(e * T + f) * 3 + i] = (double)pos[i] + p.palm_offset[i];
    }
  return flag;
}

// The late commit of the step (cdx_kin_step's rule): candidate e's rows of the previous iteration's margin /
// normal slot into opt_margin / opt_normal.
CDX_HD void gpis_mode_commit(const cdx_gpis_mode_buffers& b, int T, int64_t e, int slot) {
  for (int f = 0; f < T; ++f) {
    const int64_t r = e * T + f;
    b.opt_margin[r] = b.margin[slot][r];
    for (int i = 0; i < 3; ++i) b.opt_normal[3 * r + i] = b.normal_slot[slot][3 * r + i];
  }
}

// Argument checks shared by the device entry points and the host build (0 = fine).
CDX_HD int gpis_mode_check(const cdx_chain* chain, const cdx_gpis_mode_params* p, int64_t E, int n_tips) {
  if (!p || E < 0 || n_tips < 1 || n_tips > CDX_MAX_TIPS || (p->mode != 0 && p->mode != 1) || p->fe.n_tips != n_tips)
    return CDX_EINVAL;
  if (p->mode == 1 && (!chain || chain->n_tips != n_tips || chain->n_dofs < 1 || chain->n_dofs > CDX_MAX_DOFS ||
                       chain->n_bodies < 1 || chain->n_bodies > CDX_MAX_BODIES))
    return CDX_EINVAL;
  return CDX_OK;
}
// After gpis_mode_check: the chain's tree (parent order, DOF / tip range, depth) in mode 1 → CDX_ECHAIN.
CDX_HD int gpis_mode_check_chain(const cdx_chain* chain, const cdx_gpis_mode_params* p) {
  return p->mode == 1 && chain_code(chain) ? CDX_ECHAIN : CDX_OK;
}
CDX_HD int gpis_mode_check_cost(const cdx_gpis_mode_params* p, const cdx_gpis_mode_buffers* b) {
  if (!b || !b->pose || !b->target || !b->comp || !b->mean || !b->gmean || !b->normal || !b->std || !b->gstd ||
      !b->tmean || !b->tgmean || !b->loss || !b->g_pose || !b->g_target || !b->g_comp || !b->margin[0] || !b->margin[1] ||
      (p->mode == 1 && !b->tips))
    return CDX_EINVAL;
  return CDX_OK;
}
CDX_HD int gpis_mode_check_step(const cdx_gpis_mode_opt* cfg, const cdx_gpis_mode_buffers* b, int iteration,
                                int finalize) {
  if (!cfg || !b || iteration < 0) return CDX_EINVAL;
  if (!b->margin[0] || !b->margin[1] || !b->normal_slot[0] || !b->normal_slot[1] || !b->opt_margin || !b->opt_normal ||
      !b->any)
    return CDX_EINVAL;
  if (!finalize && (!b->pose || !b->target || !b->comp || !b->g_pose || !b->g_target || !b->g_comp || !b->v_pose ||
                    !b->v_target || !b->v_comp || !b->loss || !b->opt_value || !b->opt_pose || !b->opt_target ||
                    !b->opt_comp))
    return CDX_EINVAL;
  return CDX_OK;
}

}  // namespace cdx
