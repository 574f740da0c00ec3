// Batched disturbance-load test on gfx950 (the rule: cdx_equil.h).
//
//   grasp_equilibrium_kernel  one lane per (grasp, load) item, item e·W + w, the WHOLE solve (the row's stiffness centre
//                             and scales, every Levenberg–Marquardt iteration on the exact 6 × 6 Hessian, the outputs)
//                             in one launch.  The pose, its trial copy and the 6 × 6 system are registers addressed by
//                             constants; the loops over the contacts read the row's p, g, k from global memory, where
//                             the lanes of a wave that share a row (consecutive items) read the same addresses — one
//                             request a wave and row, served by the caches after the first pass.  No LDS, no barrier,
//                             no cross-lane operation: an item cannot steer another.  The workgroup is one wave: with
//                             nothing shared a larger one would only hold finished waves until its slowest ends.  A
//                             wave lasts as long as its slowest lane.
//   equil_reduce_kernel       one lane per grasp row, its W items in order: a running minimum with its place, two maxima
//                             and a count, no atomics.
#include <hip/hip_runtime.h>

#include "cdx_equil.h"

namespace {

constexpr int EQ_LANES = 64;

__global__ __launch_bounds__(EQ_LANES) void grasp_equilibrium_kernel(
    cdx_equil_params p, int64_t N, int64_t W, const double* __restrict__ contact, const double* __restrict__ target,
    const double* __restrict__ stiffness, const double* __restrict__ normal, const double* __restrict__ load_force,
    const double* __restrict__ load_point, int shared, double* __restrict__ rot, double* __restrict__ trans,
    double* __restrict__ force, double* __restrict__ normal_force, double* __restrict__ margin,
    double* __restrict__ shift, double* __restrict__ chord, uint8_t* __restrict__ stable, int32_t* __restrict__ iters,
    int32_t* __restrict__ status) {
  const int64_t item = (int64_t)blockIdx.x * EQ_LANES + (int64_t)threadIdx.x;
  if (item >= N) return;
  const int T = p.n_tips;
  const int64_t e = item / W, l = shared ? item - e * W : item;
  cdx::EqRow row;
  const bool ok = cdx::eq_row_prepare(T, contact + e * T * 3, target + e * T * 3, stiffness + e * T, normal + e * T * 3, &row);
  int32_t it;
  uint8_t stab;
  const int st = cdx::equil_row(p, row, ok, normal + e * T * 3, load_force + l * 3, load_point + l * 3,
                                rot ? rot + item * 9 : nullptr, trans ? trans + item * 3 : nullptr,
                                force ? force + item * T * 3 : nullptr, normal_force + item * T, margin + item * T,
                                shift + item, chord + item, &stab, &it);
  stable[item] = stab;
  iters[item] = it;
  status[item] = st;
}

__global__ __launch_bounds__(EQ_LANES) void equil_reduce_kernel(
    cdx_equil_limits lim, int64_t E, int64_t W, int T, const double* __restrict__ margin,
    const double* __restrict__ normal_force, const double* __restrict__ shift, const double* __restrict__ chord,
    const uint8_t* __restrict__ stable, const int32_t* __restrict__ status, double* __restrict__ worst_margin,
    int32_t* __restrict__ worst_load, int32_t* __restrict__ worst_tip, double* __restrict__ max_shift,
    double* __restrict__ max_chord, int32_t* __restrict__ n_failed, uint8_t* __restrict__ holds) {
  const int64_t e = (int64_t)blockIdx.x * EQ_LANES + (int64_t)threadIdx.x;
  if (e >= E) return;
  const int64_t at = e * W;
  cdx::equil_reduce_row(W, T, margin + at * T, normal_force + at * T, shift + at, chord + at, stable + at, status + at,
                        lim, worst_margin + e, worst_load + e, worst_tip + e, max_shift + e, max_chord + e,
                        n_failed + e, holds + e);
}

}  // namespace

extern "C" {

void cdx_equil_abi_sizes(size_t* out) {
  if (!out) return;
  out[0] = sizeof(cdx_equil_params);
  out[1] = sizeof(cdx_equil_limits);
}

int cdx_grasp_equilibrium(const cdx_equil_params* params, int64_t E, int64_t W, const double* contact,
                          const double* target, const double* stiffness, const double* normal,
                          const double* load_force, const double* load_point, int32_t loads_shared, double* rot,
                          double* trans, double* force, double* normal_force, double* margin, double* shift,
                          double* chord, uint8_t* stable, int32_t* iters, int32_t* status, cdx_stream_t stream) {
  const int rc = cdx::eq_params_code(params);
  if (rc) return rc;
  if (E < 0 || W < 0) return CDX_EINVAL;
  if (E == 0 || W == 0) return CDX_OK;
  if (!contact || !target || !stiffness || !normal || !load_force || !load_point || !normal_force || !margin ||
      !shift || !chord || !stable || !iters || !status)
    return CDX_EINVAL;
  if (E > 0x7fffffff / W || E * W > 0x7fffffff / params->n_tips) return CDX_EINVAL;
  const int64_t N = E * W, blocks = (N + EQ_LANES - 1) / EQ_LANES;
  hipLaunchKernelGGL(grasp_equilibrium_kernel, dim3((unsigned)blocks), dim3(EQ_LANES), 0,
                     reinterpret_cast<hipStream_t>(stream), *params, N, W, contact, target, stiffness, normal,
                     load_force, load_point, loads_shared != 0 ? 1 : 0, rot, trans, force, normal_force, margin, shift,
                     chord, stable, iters, status);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_equil_reduce(const cdx_equil_limits* limits, int64_t E, int64_t W, int32_t n_tips, const double* margin,
                     const double* normal_force, const double* shift, const double* chord, const uint8_t* stable,
                     const int32_t* status, double* worst_margin, int32_t* worst_load, int32_t* worst_tip,
                     double* max_shift, double* max_chord, int32_t* n_failed, uint8_t* holds, cdx_stream_t stream) {
  if (!limits || E < 0 || W < 0 || W > 0x7fffffff || n_tips < 1 || n_tips > CDX_MAX_TIPS) return CDX_EINVAL;
  if (E == 0 || W == 0) return CDX_OK;
  if (!margin || !normal_force || !shift || !chord || !stable || !status || !worst_margin || !worst_load ||
      !worst_tip || !max_shift || !max_chord || !n_failed || !holds)
    return CDX_EINVAL;
  const int64_t blocks = (E + EQ_LANES - 1) / EQ_LANES;
  if (blocks > 0x7fffffff) return CDX_EINVAL;
  hipLaunchKernelGGL(equil_reduce_kernel, dim3((unsigned)blocks), dim3(EQ_LANES), 0,
                     reinterpret_cast<hipStream_t>(stream), *limits, E, W, (int)n_tips, margin, normal_force, shift,
                     chord, stable, status, worst_margin, worst_load, worst_tip, max_shift, max_chord, n_failed, holds);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
