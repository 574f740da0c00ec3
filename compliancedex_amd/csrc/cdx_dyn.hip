// Rigid-body dynamics of a chain on gfx950 (the rule: cdx_dyn.h).
//
//   dyn_inverse_kernel  one lane per row: the trigonometry of the row's joints once, then the forward sweep, the own
//                       forces, the tip forces and the backward sweep of recursive Newton–Euler.
//   dyn_inertia_kernel  one lane per row: D such passes at unit accelerations, the lower triangle written and mirrored.
//   dyn_forward_kernel  one lane per row: the non-linear effects, H into LDS, its Cholesky factor and two substitutions.
// Everything a row indexes at run time (12 doubles and a float (c, s) pair per body; for the forward dynamics also the
// D(D + 1)/2 + D doubles of the system) lives in LDS, the lanes of a workgroup interleaved element by element as in
// cdx_ik.hip: a lane touches only its own slots, so there is no barrier, no cross-lane operation and no atomic, and a
// row cannot steer another.  The chain is read in place from the kernel-argument segment; the inertial constants
// (cdx_dyn, 2.8 KB — with the chain more than the segment holds) from the caller's device copy, uniform loads.  The
// workgroup is sized by the LDS a row needs (dyn_lanes), the rule of ik_lanes.
#include <hip/hip_runtime.h>

#include "cdx_dyn.h"

namespace {

extern __shared__ __attribute__((aligned(16))) char dyn_lds[];

__device__ __forceinline__ const void* row_ptr(const void* p, int f64, int64_t e, int D) {
  return !p ? nullptr : (f64 ? (const void*)((const double*)p + e * D) : (const void*)((const float*)p + e * D));
}
__device__ __forceinline__ void* out_ptr(void* p, int f64, int64_t e, int64_t D) {
  return f64 ? (void*)((double*)p + e * D) : (void*)((float*)p + e * D);
}

__global__ __launch_bounds__(64) void dyn_inverse_kernel(cdx_chain c, const cdx_dyn* __restrict__ dy, int64_t B,
                                                         const void* __restrict__ q, const void* __restrict__ qd,
                                                         const void* __restrict__ qdd, int f64, int include_gravity,
                                                         int use_damping, const double* __restrict__ gravity,
                                                         int gravity_per_row, const double* __restrict__ tip_forces,
                                                         void* __restrict__ tau) {
  const cdx_chain& kc = *(const cdx_chain*)(__builtin_amdgcn_kernarg_segment_ptr());
  const int lanes = (int)blockDim.x, lane = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * lanes + lane;
  if (e >= B) return;
  const int D = kc.n_dofs, T = kc.n_tips;
  const cdx::DynMem m = cdx::dyn_mem_at(dyn_lds, kc.n_bodies, D, 0, lane, lanes);
  double g[3];
  cdx::dyn_gravity(include_gravity, gravity ? gravity + (gravity_per_row ? e * 3 : 0) : nullptr, g);
  cdx::dyn_inverse_row(kc, *dy, m, cdx::DynVec{row_ptr(q, f64, e, D), f64}, cdx::DynVec{row_ptr(qd, f64, e, D), f64},
                       cdx::DynVec{row_ptr(qdd, f64, e, D), f64}, g, use_damping,
                       tip_forces ? tip_forces + e * T * 3 : nullptr, cdx::DynOut{out_ptr(tau, f64, e, D), f64});
}

__global__ __launch_bounds__(64) void dyn_inertia_kernel(cdx_chain c, const cdx_dyn* __restrict__ dy, int64_t B,
                                                         const void* __restrict__ q, int f64, void* __restrict__ H) {
  const cdx_chain& kc = *(const cdx_chain*)(__builtin_amdgcn_kernarg_segment_ptr());
  const int lanes = (int)blockDim.x, lane = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * lanes + lane;
  if (e >= B) return;
  const int D = kc.n_dofs;
  const cdx::DynMem m = cdx::dyn_mem_at(dyn_lds, kc.n_bodies, D, 0, lane, lanes);
  cdx::dyn_inertia_row(kc, *dy, m, cdx::DynVec{row_ptr(q, f64, e, D), f64},
                       cdx::DynOut{out_ptr(H, f64, e, (int64_t)D * D), f64});
}

__global__ __launch_bounds__(64) void dyn_forward_kernel(cdx_chain c, const cdx_dyn* __restrict__ dy, int64_t B,
                                                         const void* __restrict__ q, const void* __restrict__ qd,
                                                         const void* __restrict__ f, int f64, int include_gravity,
                                                         int use_damping, const double* __restrict__ gravity,
                                                         int gravity_per_row, void* __restrict__ qdd) {
  const cdx_chain& kc = *(const cdx_chain*)(__builtin_amdgcn_kernarg_segment_ptr());
  const int lanes = (int)blockDim.x, lane = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * lanes + lane;
  if (e >= B) return;
  const int D = kc.n_dofs;
  const cdx::DynMem m = cdx::dyn_mem_at(dyn_lds, kc.n_bodies, D, 1, lane, lanes);
  double g[3];
  cdx::dyn_gravity(include_gravity, gravity ? gravity + (gravity_per_row ? e * 3 : 0) : nullptr, g);
  cdx::dyn_forward_row(kc, *dy, m, cdx::DynVec{row_ptr(q, f64, e, D), f64}, cdx::DynVec{row_ptr(qd, f64, e, D), f64},
                       cdx::DynVec{row_ptr(f, f64, e, D), f64}, g, use_damping,
                       cdx::DynOut{out_ptr(qdd, f64, e, D), f64});
}

// Lanes (rows) per workgroup: the largest power of two ≤ 64 whose rows fit in 40 KB of LDS (four workgroups on a
// compute unit's 160 KB), at least 1 — ik_lanes' rule.
int dyn_lanes(int n, int D, int fwd) {
  const size_t row = cdx::dyn_mem_bytes(n, D, fwd);
  int lanes = 64;
  while (lanes > 1 && row * lanes > 40960) lanes >>= 1;
  return lanes;
}

// The checks every entry shares; 1: nothing to do (B = 0).
int dyn_check(const cdx_chain* chain, const cdx_dyn* dyn, int64_t B, int32_t dtype) {
  const int rc = cdx::dyn_chain_code(chain, dyn);
  if (rc) return rc;
  if (B < 0 || (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64)) return CDX_EINVAL;
  return B == 0 ? 1 : CDX_OK;
}

}  // namespace

extern "C" {

int32_t cdx_dyn_rows_per_block(int32_t n_bodies, int32_t n_dofs, int32_t entry) {
  if (n_bodies <= 0 || n_bodies > CDX_MAX_BODIES || n_dofs < 0 || n_dofs > CDX_MAX_DOFS || entry < 0 || entry > 2)
    return 0;
  return dyn_lanes(n_bodies, n_dofs, entry == 2);
}

size_t cdx_dyn_abi_size(void) { return sizeof(cdx_dyn); }

int cdx_dyn_inverse(const cdx_chain* chain, const cdx_dyn* dyn, int64_t B, const void* q, const void* qd,
                    const void* qdd, int32_t dtype, int32_t include_gravity, int32_t use_damping, const double* gravity,
                    int32_t gravity_per_row, const double* tip_forces, void* tau, cdx_stream_t stream) {
  const int rc = dyn_check(chain, dyn, B, dtype);
  if (rc) return rc < 0 ? rc : CDX_OK;
  if (!q || !tau) return CDX_ECHAIN;
  const int n = chain->n_bodies, D = chain->n_dofs, lanes = dyn_lanes(n, D, 0);
  const size_t lds = cdx::dyn_mem_bytes(n, D, 0) * lanes;
  const int64_t blocks = (B + lanes - 1) / lanes;
  if (blocks > 0x7fffffff || lds > 65536) return CDX_EINVAL;
  hipLaunchKernelGGL(dyn_inverse_kernel, dim3((unsigned)blocks), dim3((unsigned)lanes), lds,
                     reinterpret_cast<hipStream_t>(stream), *chain, dyn, B, q, qd, qdd, (int)(dtype == CDX_DTYPE_F64),
                     (int)(include_gravity != 0), (int)(use_damping != 0), gravity, (int)(gravity_per_row != 0),
                     chain->n_tips > 0 ? tip_forces : nullptr, tau);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_dyn_inertia(const cdx_chain* chain, const cdx_dyn* dyn, int64_t B, const void* q, int32_t dtype, void* H,
                    cdx_stream_t stream) {
  const int rc = dyn_check(chain, dyn, B, dtype);
  if (rc) return rc < 0 ? rc : CDX_OK;
  if (!q || !H) return CDX_ECHAIN;
  const int n = chain->n_bodies, D = chain->n_dofs, lanes = dyn_lanes(n, D, 0);
  const size_t lds = cdx::dyn_mem_bytes(n, D, 0) * lanes;
  const int64_t blocks = (B + lanes - 1) / lanes;
  if (blocks > 0x7fffffff || lds > 65536) return CDX_EINVAL;
  hipLaunchKernelGGL(dyn_inertia_kernel, dim3((unsigned)blocks), dim3((unsigned)lanes), lds,
                     reinterpret_cast<hipStream_t>(stream), *chain, dyn, B, q, (int)(dtype == CDX_DTYPE_F64), H);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_dyn_forward(const cdx_chain* chain, const cdx_dyn* dyn, int64_t B, const void* q, const void* qd, const void* f,
                    int32_t dtype, int32_t include_gravity, int32_t use_damping, const double* gravity,
                    int32_t gravity_per_row, void* qdd, cdx_stream_t stream) {
  const int rc = dyn_check(chain, dyn, B, dtype);
  if (rc < 0) return rc;
  if (cdx::dyn_has_dead_joint(*chain)) return CDX_EINVAL;
  if (rc) return CDX_OK;
  if (!q || !f || !qdd) return CDX_ECHAIN;
  const int n = chain->n_bodies, D = chain->n_dofs, lanes = dyn_lanes(n, D, 1);
  const size_t lds = cdx::dyn_mem_bytes(n, D, 1) * lanes;
  const int64_t blocks = (B + lanes - 1) / lanes;
  if (blocks > 0x7fffffff || lds > 65536) return CDX_EINVAL;
  hipLaunchKernelGGL(dyn_forward_kernel, dim3((unsigned)blocks), dim3((unsigned)lanes), lds,
                     reinterpret_cast<hipStream_t>(stream), *chain, dyn, B, q, qd, f, (int)(dtype == CDX_DTYPE_F64),
                     (int)(include_gravity != 0), (int)(use_damping != 0), gravity, (int)(gravity_per_row != 0), qdd);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
