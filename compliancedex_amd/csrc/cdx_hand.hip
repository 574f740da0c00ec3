// Whole-hand sphere collision on gfx950 (the rule, and the order of every sum: cdx_hand.h).
//
//   hand_spheres_kernel   256 lanes work 8 candidates.  Phase 1: lane (candidate, body) walks that body's root path with
//                         a running pose (chain_step, no per-level storage, no array indexed at run time) and leaves the
//                         pose in LDS and in `poses`; the candidate's body-0 lane also leaves the palm rotation there.
//                         Phase 2: the block's lanes stride over (candidate, sphere), read the body's pose from LDS and
//                         write the world centre.  A body's walk repeats its ancestors' steps (depth × the work of one
//                         walk over all bodies) in exchange for lanes that never wait on a parent: 8 × 1.5 KB of LDS.
//   hand_cost_kernel      one wave per candidate.  The row's centres and the radii are staged in LDS (8 KB); lane l
//                         owns the spheres l + 64k: their object and floor terms and their partner lists (read from the
//                         model's device table, which keeps entry k of a wave's 64 lists in 64 consecutive words, one
//                         word = partner and pair; the partner's centre from LDS), so every g_centers entry has
//                         one writer and no atomic exists.  Cost and the three class maxima are joined over the lanes by
//                         a fixed tree in LDS.
//   hand_pullback_kernel  one wave per candidate.  Lanes over spheres leave c_h and Rpᵀ·g in LDS (12 KB) and their palm
//                         sums in the tree; then lane d < n_dofs sums its joint's spheres in ascending order (membership:
//                         a bit test on the body's path mask; masks and the spheres' bodies are kept in LDS and the lanes
//                         walk the spheres together, each reading the same address).  No trigonometric library call: the palm's
//                         sines and cosines are hand_sincos.
//   hand_term_kernel      one wave per candidate: the two kernels above back to back with g_centers in LDS, every output
//                         weight·x or old + weight·x (the optimisers' loops add the term into their own buffers).
#include <hip/hip_runtime.h>

#include <vector>

#include "cdx_hand.h"

namespace {

constexpr int SP_G = 8;  // candidates per workgroup of hand_spheres_kernel (32 body lanes each)
static_assert(CDX_MAX_BODIES == 32 && CDX_HAND_LANES == 64, "lane maps of the hand kernels");

__global__ __launch_bounds__(256) void hand_spheres_kernel(cdx_chain c, cdx_hand H, int64_t E, const double* __restrict__ q,
                                                           const double* __restrict__ pp, const double* __restrict__ po,
                                                           float* __restrict__ poses, double* __restrict__ centers) {
  __shared__ float pose[SP_G][CDX_MAX_BODIES][12];
  __shared__ double palm[SP_G][12];
  const int t = (int)threadIdx.x, g = t >> 5, b = t & 31;
  const int64_t e0 = (int64_t)blockIdx.x * SP_G, e = e0 + g;
  if (e < E && b < c.n_bodies) {
    cdx::hand_body_pose(c, b, cdx::QRowD{q + e * c.n_dofs}, pose[g][b]);
    float* out = poses + (e * c.n_bodies + b) * 12;
    for (int i = 0; i < 12; ++i) out[i] = pose[g][b][i];
  }
  if (e < E && b == 0) {
    const double ang[3] = {po ? po[3 * e] : 0.0, po ? po[3 * e + 1] : 0.0, po ? po[3 * e + 2] : 0.0};
    double Rp[9];
    cdx::hand_euler(ang, Rp, nullptr, nullptr, nullptr);
    for (int i = 0; i < 9; ++i) palm[g][i] = Rp[i];
    for (int i = 0; i < 3; ++i) palm[g][9 + i] = pp ? pp[3 * e + i] : 0.0;
  }
  __syncthreads();
  const int S = H.n_spheres;
  const int64_t left = E - e0;
  const int n = (int)(left < SP_G ? left : SP_G) * S;
  for (int i = t; i < n; i += 256) {
    const int gg = i / S, s = i - gg * S;
    float ch[3];
    cdx::hand_center_local(pose[gg][H.body[s]], H.local + 3 * s, ch);
    double cw[3];
    cdx::hand_center_world(palm[gg], palm[gg] + 9, ch, cw);
    double* out = centers + ((e0 + gg) * S + s) * 3;
    for (int k = 0; k < 3; ++k) out[k] = cw[k];
  }
}

__global__ __launch_bounds__(CDX_HAND_LANES) void hand_cost_kernel(cdx_hand H, cdx_hand_params P,
                                                                   const double* __restrict__ centers,
                                                                   const double* __restrict__ dist,
                                                                   const double* __restrict__ gdist,
                                                                   double* __restrict__ cost, double* __restrict__ depth,
                                                                   int32_t* __restrict__ worst, double* g_centers) {
  __shared__ double cen[3 * CDX_MAX_SPHERES];
  __shared__ double rad[CDX_MAX_SPHERES];
  __shared__ double rv[4 * CDX_HAND_LANES];
  __shared__ int32_t ri[3 * CDX_HAND_LANES];
  __shared__ int bad;
  const int l = (int)threadIdx.x, S = H.n_spheres;
  const int64_t e = blockIdx.x;
  for (int i = l; i < 3 * S; i += CDX_HAND_LANES) cen[i] = centers[e * S * 3 + i];
  for (int i = l; i < S; i += CDX_HAND_LANES) rad[i] = H.radius[i];
  if (l == 0) bad = 0;
  __syncthreads();
  double* g = g_centers + e * S * 3;
  const bool ok = cdx::hand_cost_lane(H, P, l, cen, rad, dist ? dist + e * S : nullptr, gdist ? gdist + e * S * 3 : nullptr,
                                      g, rv, ri);
  if (!ok) bad = 1;
  __syncthreads();
  for (int off = CDX_HAND_LANES / 2; off; off >>= 1) {
    if (l < off) cdx::hand_cost_join(rv, ri, l, off);
    __syncthreads();
  }
  const bool row_bad = bad != 0;
  if (l == 0) cdx::hand_cost_finish(row_bad, rv, ri, cost + e, depth + 3 * e, worst + 3 * e);
  if (row_bad)
    for (int i = l; i < 3 * S; i += CDX_HAND_LANES) g[i] = (double)NAN;
}

__global__ __launch_bounds__(CDX_HAND_LANES) void hand_pullback_kernel(cdx_chain c, cdx_hand H,
                                                                       const float* __restrict__ poses,
                                                                       const double* __restrict__ g_centers,
                                                                       const double* __restrict__ po,
                                                                       double* __restrict__ g_q, double* __restrict__ g_pp,
                                                                       double* __restrict__ g_po) {
  __shared__ double st[6 * CDX_MAX_SPHERES];
  __shared__ double rv[6 * CDX_HAND_LANES];
  __shared__ double rot[36];
  __shared__ uint32_t mask[CDX_MAX_BODIES];
  __shared__ int32_t sb[CDX_MAX_SPHERES];
  __shared__ int bad;
  const int l = (int)threadIdx.x;
  const int64_t e = blockIdx.x;
  const float* pe = poses + e * c.n_bodies * 12;
  if (l == 0) {
    const double ang[3] = {po ? po[3 * e] : 0.0, po ? po[3 * e + 1] : 0.0, po ? po[3 * e + 2] : 0.0};
    double Rp[9], dRa[9], dRb[9], dRc[9];
    cdx::hand_euler(ang, Rp, dRa, dRb, dRc);
    bool ok = true;
    for (int i = 0; i < 9; ++i) {
      ok = ok && cdx::hand_finite(Rp[i]);
      rot[i] = Rp[i];
      rot[9 + i] = dRa[i];
      rot[18 + i] = dRb[i];
      rot[27 + i] = dRc[i];
    }
    bad = ok ? 0 : 1;
  }
  if (l < c.n_bodies) mask[l] = cdx::chain_path_mask(c, l);
  __syncthreads();
  bool ok = cdx::hand_pull_lane(H, l, pe, g_centers + e * H.n_spheres * 3, rot, rot + 9, rot + 18, rot + 27, st, sb,
                                rv);
  __syncthreads();
  double gq = 0.0;
  if (l < c.n_dofs) gq = cdx::hand_pull_dof(c, H, l, pe, mask, st, sb, &ok);
  if (!ok) bad = 1;
  for (int off = CDX_HAND_LANES / 2; off; off >>= 1) {
    if (l < off)
      for (int k = 0; k < 6; ++k) rv[k * CDX_HAND_LANES + l] += rv[k * CDX_HAND_LANES + l + off];
    __syncthreads();
  }
  const bool row_bad = bad != 0;
  if (l < c.n_dofs) g_q[e * c.n_dofs + l] = row_bad ? (double)NAN : gq;
  if (l < 3) {
    g_pp[3 * e + l] = row_bad ? (double)NAN : rv[l * CDX_HAND_LANES];
    g_po[3 * e + l] = row_bad ? (double)NAN : rv[(3 + l) * CDX_HAND_LANES];
  }
}

// hand_cost_kernel, then hand_pullback_kernel, in one wave per candidate with g_centers kept in LDS (hand_term_kernel
// in the head comment of cdx_hand.h's term section).  LDS: g_centers (6 KB), then one region the two phases use in
// turn — the cost's centres, radii and tree (10.75 KB), the pull-back's c_h / Rpᵀ·g and tree (15 KB) — and the
// pull-back's small tables: 22.5 KB.  The same cdx_hand.h pieces run in the same order as in the two kernels above, so
// x has their bits; lane 0 owns loss (and depth / worst), lane d < n_dofs g_q[d], lane i < 3 g_palm_pos[i] and
// g_palm_ori[i].
constexpr int TERM_COST_WORDS = 3 * CDX_MAX_SPHERES + CDX_MAX_SPHERES + 4 * CDX_HAND_LANES + 2 * CDX_HAND_LANES;
constexpr int TERM_PULL_WORDS = 6 * CDX_MAX_SPHERES + 6 * CDX_HAND_LANES;
constexpr int TERM_WORDS = TERM_COST_WORDS > TERM_PULL_WORDS ? TERM_COST_WORDS : TERM_PULL_WORDS;

__global__ __launch_bounds__(CDX_HAND_LANES) void hand_term_kernel(
    cdx_chain c, cdx_hand H, cdx_hand_params P, const float* __restrict__ poses, const double* __restrict__ centers,
    const double* __restrict__ dist, const double* __restrict__ gdist, const double* __restrict__ po, double weight,
    int accumulate, double* loss, double* g_q, double* g_pp, double* g_po, double* __restrict__ depth,
    int32_t* __restrict__ worst) {
  __shared__ double gc[3 * CDX_MAX_SPHERES];
  __shared__ double work[TERM_WORDS];
  __shared__ double rot[36];
  __shared__ uint32_t mask[CDX_MAX_BODIES];
  __shared__ int32_t sb[CDX_MAX_SPHERES];
  __shared__ int bad;
  const int l = (int)threadIdx.x, S = H.n_spheres;
  const int64_t e = blockIdx.x;
  // ---- the cost (hand_cost_kernel)
  double* cen = work;
  double* rad = cen + 3 * CDX_MAX_SPHERES;
  double* rv = rad + CDX_MAX_SPHERES;
  int32_t* ri = reinterpret_cast<int32_t*>(rv + 4 * CDX_HAND_LANES);  // [3][64] in 2·64 doubles
  for (int i = l; i < 3 * S; i += CDX_HAND_LANES) cen[i] = centers[e * S * 3 + i];
  for (int i = l; i < S; i += CDX_HAND_LANES) rad[i] = H.radius[i];
  if (l == 0) bad = 0;
  __syncthreads();
  const bool okc = cdx::hand_cost_lane(H, P, l, cen, rad, dist ? dist + e * S : nullptr,
                                       gdist ? gdist + e * S * 3 : nullptr, gc, rv, ri);
  if (!okc) bad = 1;
  __syncthreads();
  for (int off = CDX_HAND_LANES / 2; off; off >>= 1) {
    if (l < off) cdx::hand_cost_join(rv, ri, l, off);
    __syncthreads();
  }
  const bool cost_bad = bad != 0;
  if (l == 0) {
    double cost, dp[3];
    int32_t wi[3];
    cdx::hand_cost_finish(cost_bad, rv, ri, &cost, dp, wi);
    loss[e] = cdx::hand_term_out(accumulate ? loss[e] : 0.0, cost, weight, accumulate != 0, cost_bad);
    for (int k = 0; k < 3; ++k) {
      if (depth) depth[3 * e + k] = dp[k];
      if (worst) worst[3 * e + k] = wi[k];
    }
  }
  if (cost_bad)
    for (int i = l; i < 3 * S; i += CDX_HAND_LANES) gc[i] = (double)NAN;
  // ---- the pull-back (hand_pullback_kernel)
  const float* pe = poses + e * c.n_bodies * 12;
  if (l == 0) {
    const double ang[3] = {po ? po[3 * e] : 0.0, po ? po[3 * e + 1] : 0.0, po ? po[3 * e + 2] : 0.0};
    double Rp[9], dRa[9], dRb[9], dRc[9];
    cdx::hand_euler(ang, Rp, dRa, dRb, dRc);
    bool ok = true;
    for (int i = 0; i < 9; ++i) {
      ok = ok && cdx::hand_finite(Rp[i]);
      rot[i] = Rp[i];
      rot[9 + i] = dRa[i];
      rot[18 + i] = dRb[i];
      rot[27 + i] = dRc[i];
    }
    if (!ok) bad = 1;
  }
  if (l < c.n_bodies) mask[l] = cdx::chain_path_mask(c, l);
  __syncthreads();  // (the cost's region is free: its tree was read before this barrier)
  double* st = work;
  double* pv = st + 6 * CDX_MAX_SPHERES;
  bool ok = cdx::hand_pull_lane(H, l, pe, gc, rot, rot + 9, rot + 18, rot + 27, st, sb, pv);
  __syncthreads();
  double gq = 0.0;
  if (l < c.n_dofs) gq = cdx::hand_pull_dof(c, H, l, pe, mask, st, sb, &ok);
  if (!ok) bad = 1;
  for (int off = CDX_HAND_LANES / 2; off; off >>= 1) {
    if (l < off)
      for (int k = 0; k < 6; ++k) pv[k * CDX_HAND_LANES + l] += pv[k * CDX_HAND_LANES + l + off];
    __syncthreads();
  }
  const bool row_bad = bad != 0;
  const bool acc = accumulate != 0;
  if (l < c.n_dofs && g_q) {
    double* o = g_q + e * c.n_dofs + l;
    *o = cdx::hand_term_out(acc ? *o : 0.0, gq, weight, acc, row_bad);
  }
  if (l < 3) {
    if (g_pp) {
      double* o = g_pp + 3 * e + l;
      *o = cdx::hand_term_out(acc ? *o : 0.0, pv[l * CDX_HAND_LANES], weight, acc, row_bad);
    }
    if (g_po) {
      double* o = g_po + 3 * e + l;
      *o = cdx::hand_term_out(acc ? *o : 0.0, pv[(3 + l) * CDX_HAND_LANES], weight, acc, row_bad);
    }
  }
}

int launched() { return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH; }

}  // namespace

extern "C" {

size_t cdx_hand_bytes(int32_t S, int32_t P) { return cdx::hand_bytes(S, P); }

void cdx_hand_abi_sizes(size_t* out2) {
  out2[0] = sizeof(cdx_hand);
  out2[1] = sizeof(cdx_hand_params);
}

int cdx_hand_prepare(int32_t n_bodies, int32_t S, const float* local, const double* radius, const int32_t* body,
                     int32_t P, const int32_t* pairs, void* tables, cdx_hand* out, cdx_stream_t stream) {
  const size_t bytes = cdx::hand_bytes(S, P);
  if (!bytes || !tables || !out) return CDX_EINVAL;
  std::vector<char> host(bytes, 0);
  cdx_hand h;
  const int rc = cdx::hand_fill(n_bodies, S, local, radius, body, P, pairs, host.data(), &h);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(tables, host.data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess) return CDX_ELAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return CDX_ELAUNCH;
  cdx::hand_layout(n_bodies, S, P, static_cast<char*>(tables), &h);  // (the same offsets at the device address)
  *out = h;
  return CDX_OK;
}

int cdx_hand_spheres(const cdx_chain* chain, const cdx_hand* h, int64_t E, const double* q, const double* palm_pos,
                     const double* palm_ori, float* poses, double* centers, cdx_stream_t stream) {
  int rc = cdx::hand_chain_code(chain);
  if (rc) return rc;
  rc = cdx::hand_code(h);
  if (rc) return rc;
  if (h->n_bodies != chain->n_bodies || E < 0) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if ((!q && chain->n_dofs > 0) || !poses || !centers) return CDX_EINVAL;
  const int64_t blocks = (E + SP_G - 1) / SP_G;
  if (blocks > 0x7fffffff) return CDX_EINVAL;
  hipLaunchKernelGGL(hand_spheres_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     *chain, *h, E, q, palm_pos, palm_ori, poses, centers);
  return launched();
}

int cdx_hand_cost(const cdx_hand* h, const cdx_hand_params* p, int64_t E, const double* centers, const double* dist,
                  const double* gdist, double* cost, double* depth, int32_t* worst, double* g_centers,
                  cdx_stream_t stream) {
  int rc = cdx::hand_code(h);
  if (rc) return rc;
  rc = cdx::hand_params_code(p);
  if (rc) return rc;
  if (E < 0 || E > 0x7fffffff || (dist == nullptr) != (gdist == nullptr)) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!centers || !cost || !depth || !worst || !g_centers) return CDX_EINVAL;
  hipLaunchKernelGGL(hand_cost_kernel, dim3((unsigned)E), dim3(CDX_HAND_LANES), 0, reinterpret_cast<hipStream_t>(stream),
                     *h, *p, centers, dist, gdist, cost, depth, worst, g_centers);
  return launched();
}

int cdx_hand_pullback(const cdx_chain* chain, const cdx_hand* h, int64_t E, const float* poses, const double* g_centers,
                      const double* palm_ori, double* g_q, double* g_palm_pos, double* g_palm_ori, cdx_stream_t stream) {
  int rc = cdx::hand_chain_code(chain);
  if (rc) return rc;
  rc = cdx::hand_code(h);
  if (rc) return rc;
  if (h->n_bodies != chain->n_bodies || E < 0 || E > 0x7fffffff) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!poses || !g_centers || (!g_q && chain->n_dofs > 0) || !g_palm_pos || !g_palm_ori) return CDX_EINVAL;
  hipLaunchKernelGGL(hand_pullback_kernel, dim3((unsigned)E), dim3(CDX_HAND_LANES), 0,
                     reinterpret_cast<hipStream_t>(stream), *chain, *h, poses, g_centers, palm_ori, g_q, g_palm_pos,
                     g_palm_ori);
  return launched();
}

int cdx_hand_term(const cdx_chain* chain, const cdx_hand* h, const cdx_hand_params* p, int64_t E, const float* poses,
                  const double* centers, const double* dist, const double* gdist, const double* palm_ori, double weight,
                  int32_t accumulate, double* loss, double* g_q, double* g_palm_pos, double* g_palm_ori, double* depth,
                  int32_t* worst, cdx_stream_t stream) {
  int rc = cdx::hand_chain_code(chain);
  if (rc) return rc;
  rc = cdx::hand_code(h);
  if (rc) return rc;
  rc = cdx::hand_params_code(p);
  if (rc) return rc;
  rc = cdx::hand_term_code(chain, h, E, poses, centers, dist, gdist, weight, accumulate, loss, g_q);
  if (rc || E == 0) return rc;
  hipLaunchKernelGGL(hand_term_kernel, dim3((unsigned)E), dim3(CDX_HAND_LANES), 0, reinterpret_cast<hipStream_t>(stream),
                     *chain, *h, *p, poses, centers, dist, gdist, palm_ori, weight, (int)accumulate, loss, g_q,
                     g_palm_pos, g_palm_ori, depth, worst);
  return launched();
}

}  // extern "C"
