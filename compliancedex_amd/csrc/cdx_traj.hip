// Approach trajectories on gfx950 (the rule, and the order of every sum: cdx_traj.h).
//
//   traj_seed_kernel   one workgroup of 64 lanes per row (g, s).  Lanes d < D test the row's start and goal and draw
//                      a_d (one Philox block each) into LDS; then the 64 lanes stride over the row's T·D values, so the
//                      stores are consecutive.
//   traj_step_kernel   one workgroup of 64 lanes (one wave) per row.  The row's T·D doubles and its g_c are staged in
//                      LDS by consecutive loads (2·T·D·8 bytes, 32 KB at T = 64, D = 32, sized at launch).  Lane d < D
//                      then works column d alone — accelerations, gradient, limit hinges and the pentadiagonal solve, in
//                      place in the g_c copy; lanes of a wave read consecutive doubles of one waypoint, so no two lanes
//                      meet in a bank.  The lane sums are joined by the 32-slot tree, lane 0 adds cost_t and runs the
//                      best-iterate comparison, and the 64 lanes copy the staged row to best_traj (on a win) and write
//                      the moved interior back, both with consecutive stores.  No atomics; the LDLᵀ factors arrive by
//                      value (1.5 KB of kernel arguments, read with uniform addresses).
//                      One row per wave also when D ≤ 32 leaves half the wave idle in the column phase: kept, because
//                      a row's bits then depend on nothing but the row by construction and the launch is a small share
//                      of an iteration next to the three hand launches.
#include <hip/hip_runtime.h>

#include "cdx_traj.h"

namespace {

constexpr int TRAJ_BLOCK = 64;
static_assert(CDX_MAX_DOFS <= CDX_TRAJ_LANES && CDX_TRAJ_LANES <= TRAJ_BLOCK, "lane map of the trajectory kernels");

__global__ __launch_bounds__(TRAJ_BLOCK) void traj_seed_kernel(int32_t seeds, int32_t T, int32_t D,
                                                               const double* __restrict__ q_start,
                                                               const double* __restrict__ q_goal, double amp,
                                                               uint64_t seed, double* __restrict__ traj) {
  __shared__ double qs[CDX_MAX_DOFS], qg[CDX_MAX_DOFS], a[CDX_MAX_DOFS];
  __shared__ int bad;
  const int l = (int)threadIdx.x;
  const int64_t row = blockIdx.x, g = row / seeds;
  const int32_t s = (int32_t)(row - g * seeds);
  if (l == 0) bad = 0;
  __syncthreads();
  if (l < D) {
    qs[l] = q_start[g * D + l];
    qg[l] = q_goal[g * D + l];
    a[l] = cdx::traj_seed_amp(seed, row, s, D, l, amp);
    if (!cdx::traj_finite(qs[l]) || !cdx::traj_finite(qg[l])) bad = 1;
  }
  __syncthreads();
  const bool row_bad = bad != 0;
  double* out = traj + row * T * D;
  for (int i = l; i < T * D; i += TRAJ_BLOCK) {
    const int t = i / D, d = i - t * D;
    out[i] = cdx::traj_seed_value(qs[d], qg[d], a[d], t, T, row_bad);
  }
}

__global__ __launch_bounds__(TRAJ_BLOCK) void traj_step_kernel(cdx_traj_params P, cdx::TrajFactor F, double* traj,
                                                               const double* __restrict__ g_c,
                                                               const double* __restrict__ cost_t, int32_t iteration,
                                                               double* __restrict__ cost, double* best_cost,
                                                               int32_t* best_iter, double* __restrict__ best_traj) {
  extern __shared__ double lds[];  // q [T·D], then x [T·D]
  __shared__ double rs[CDX_TRAJ_LANES], rl[CDX_TRAJ_LANES];
  __shared__ int bad, win;
  const int l = (int)threadIdx.x, T = P.T, D = P.n_dofs, n = T * D;
  const int64_t e = blockIdx.x;
  double* q = lds;
  double* x = lds + n;
  double* row = traj + e * n;
  for (int i = l; i < n; i += TRAJ_BLOCK) {
    q[i] = row[i];
    x[i] = g_c ? g_c[e * n + i] : 0.0;
  }
  if (l == 0) bad = win = 0;
  __syncthreads();
  if (l < CDX_TRAJ_LANES) {
    double us = 0.0, ul = 0.0;
    if (l < D && !cdx::traj_column(P, F, l, q, x, &us, &ul)) bad = 1;
    rs[l] = us;
    rl[l] = ul;
  }
  double uc = 0.0;
  if (l == 0 && !cdx::traj_collision_sum(cost_t ? cost_t + e * T : nullptr, T, &uc)) bad = 1;
  __syncthreads();
  for (int off = CDX_TRAJ_LANES / 2; off; off >>= 1) {
    if (l < off) {
      rs[l] += rs[l + off];
      rl[l] += rl[l + off];
    }
    __syncthreads();
  }
  const bool row_bad = bad != 0;
  if (l == 0) {
    const double us = 0.5 * rs[0], ul = 0.5 * rl[0];
    cost[3 * e] = row_bad ? (double)NAN : us;
    cost[3 * e + 1] = row_bad ? (double)NAN : uc;
    cost[3 * e + 2] = row_bad ? (double)NAN : ul;
    const double U = cdx::traj_total(P, us, uc, ul);
    if (!row_bad && U < best_cost[e]) {
      best_cost[e] = U;
      best_iter[e] = iteration;
      win = 1;
    }
  }
  __syncthreads();
  if (win) {
    double* best = best_traj + e * n;
    for (int i = l; i < n; i += TRAJ_BLOCK) best[i] = q[i];
  }
  for (int i = D + l; i < n - D; i += TRAJ_BLOCK) row[i] = cdx::traj_moved(P, q[i], x[i], row_bad);
}

int launched() { return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH; }

}  // namespace

extern "C" {

void cdx_traj_abi_sizes(size_t* out1) { out1[0] = sizeof(cdx_traj_params); }

int cdx_traj_seed(int64_t G, int32_t seeds, int32_t T, int32_t n_dofs, const double* q_start, const double* q_goal,
                  double amp, uint64_t seed, double* traj, cdx_stream_t stream) {
  const int rc = cdx::traj_seed_code(G, seeds, T, n_dofs, q_start, q_goal, amp, traj);
  if (rc || G == 0) return rc;
  hipLaunchKernelGGL(traj_seed_kernel, dim3((unsigned)(G * seeds)), dim3(TRAJ_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), seeds, T, n_dofs, q_start, q_goal, amp, seed, traj);
  return launched();
}

int cdx_traj_step(const cdx_traj_params* p, int64_t E, double* traj, const double* g_c, const double* cost_t,
                  int32_t iteration, double* cost, double* best_cost, int32_t* best_iter, double* best_traj,
                  cdx_stream_t stream) {
  const int rc = cdx::traj_step_code(p, E, traj, g_c, cost_t, cost, best_cost, best_iter, best_traj);
  if (rc || E == 0) return rc;
  cdx::TrajFactor F;
  cdx::traj_factor(p->T - 2, &F);
  const size_t lds = (size_t)2 * p->T * p->n_dofs * sizeof(double);
  hipLaunchKernelGGL(traj_step_kernel, dim3((unsigned)E), dim3(TRAJ_BLOCK), lds, reinterpret_cast<hipStream_t>(stream),
                     *p, F, traj, g_c, cost_t, iteration, cost, best_cost, best_iter, best_traj);
  return launched();
}

}  // extern "C"
