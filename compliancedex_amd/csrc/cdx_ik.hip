// Fingertip Jacobians and batched inverse kinematics on gfx950 (the rule: cdx_ik.h).
//
//   fk_jacobian_kernel  one lane per (row, tip): two walks of the tip's path with a running pose, the columns written
//                       straight to the outputs.
//   ik_solve_kernel     one lane per candidate, the WHOLE Levenberg–Marquardt solve in one launch.  Everything a row
//                       indexes at run time (Jl, the 3T × 3T system, g, y, the two residual buffers, q and the trial q)
//                       lives in LDS, the lanes of a workgroup interleaved element by element (element i of lane l at
//                       i·lanes + l: consecutive lanes on consecutive banks); a lane touches only its own slots, so the
//                       kernel has no barrier and no cross-lane operation, and a row cannot steer another.  The loop of a
//                       wave ends when its last row stops (rows that stopped sit masked off).  The workgroup is sized
//                       by the LDS a row needs (ik_lanes): the largest power of two ≤ 64 lanes that leaves room for four
//                       workgroups on a compute unit — a hand's row needs 1.9 KB, so 16 rows share a workgroup.
//   ik_pose_kernel      the same layout for the free-wrist solve (ik_pose_row): six more columns per row of Jl (a hand's
//                       row needs 2.3 KB, still 16 rows a workgroup; iiwa7_allegro 2.8 KB, 8 rows), the palm pose and
//                       its trial copy in registers.
//   ik_frames_kernel    the same layout for pose targets and held joints (frame_ik_row): three more rows of Jl per
//                       oriented tip, the target quaternions and the row weights in LDS as well (iiwa7_allegro's palm
//                       link, one oriented tip: 1.3 KB a row, 16 rows a workgroup).
#include <hip/hip_runtime.h>

#include "cdx_ik.h"

namespace {

struct IkArgs {
  cdx_chain c;
  cdx_ik_params p;
  double po[3];
};

// (the chain read in place from the kernel-argument segment — the first argument, offset 0 —, as fk_backward_kernel
// does: indexed per body, a by-value copy would go to scratch)
__global__ __launch_bounds__(64) void fk_jacobian_kernel(cdx_chain c, const float* __restrict__ q, int64_t B,
                                                         float* __restrict__ lin, float* __restrict__ ang) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const cdx_chain& kc = *(const cdx_chain*)(__builtin_amdgcn_kernarg_segment_ptr());
  const int T = kc.n_tips, D = kc.n_dofs;
  if (t >= B * T) return;
  const int64_t b = t / T;
  const int k = (int)(t - b * T);
  cdx::fk_jacobian_tip(kc, k, q + b * D, lin + t * 3 * D, ang ? ang + t * 3 * D : nullptr);
}

extern __shared__ __attribute__((aligned(16))) char ik_lds[];

__global__ __launch_bounds__(64) void ik_solve_kernel(IkArgs a, int64_t E, const void* __restrict__ q0, int q_f64,
                                                      const double* __restrict__ target,
                                                      const double* __restrict__ palm, const double* __restrict__ w,
                                                      void* __restrict__ q, double* __restrict__ err,
                                                      int32_t* __restrict__ iters, int32_t* __restrict__ status) {
  const IkArgs& ka = *(const IkArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
  const int lanes = (int)blockDim.x, lane = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * lanes + lane;
  if (e >= E) return;
  const int T = ka.c.n_tips, D = ka.c.n_dofs;
  const cdx::IkMem m = cdx::ik_mem_at(ik_lds, T, D, lane, lanes);
  const cdx::Q0Row q0r{q_f64 ? (const void*)((const double*)q0 + e * D) : (const void*)((const float*)q0 + e * D), q_f64};
  int32_t it;
  const int st = cdx::ik_row(ka.c, ka.p, ka.po, q0r, target + e * T * 3, palm ? palm + e * 6 : nullptr,
                             w ? w + e * T : nullptr, m, err + e * T, &it);
  for (int d = 0; d < D; ++d) {
    if (q_f64)
      ((double*)q)[e * D + d] = st == 2 ? ((const double*)q0)[e * D + d] : (double)m.q[(size_t)d * lanes];
    else
      ((float*)q)[e * D + d] = st == 2 ? ((const float*)q0)[e * D + d] : m.q[(size_t)d * lanes];
  }
  iters[e] = it;
  status[e] = st;
}

// The free-wrist solve (ik_pose_row): the layout of ik_solve_kernel with D + 6 columns per row of Jl; the pose and its
// trial copy are indexed by constants and stay in registers.
__global__ __launch_bounds__(64) void ik_pose_kernel(IkArgs a, int64_t E, const void* __restrict__ q0, int q_f64,
                                                     const double* __restrict__ target,
                                                     const double* __restrict__ palm0_pos,
                                                     const double* __restrict__ palm0_rot, const double* __restrict__ w,
                                                     void* __restrict__ q, double* __restrict__ palm_pos,
                                                     double* __restrict__ palm_rot, double* __restrict__ err,
                                                     int32_t* __restrict__ iters, int32_t* __restrict__ status) {
  const IkArgs& ka = *(const IkArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
  const int lanes = (int)blockDim.x, lane = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * lanes + lane;
  if (e >= E) return;
  const int T = ka.c.n_tips, D = ka.c.n_dofs;
  const cdx::IkMem m = cdx::ik_mem_at(ik_lds, T, D + 6, lane, lanes);
  const cdx::Q0Row q0r{q_f64 ? (const void*)((const double*)q0 + e * D) : (const void*)((const float*)q0 + e * D), q_f64};
  int32_t it;
  double pp[3], Rp[9];
  const int st = cdx::ik_pose_row(ka.c, ka.p, ka.po, q0r, target + e * T * 3, palm0_pos ? palm0_pos + e * 3 : nullptr,
                                  palm0_rot ? palm0_rot + e * 9 : nullptr, w ? w + e * T : nullptr, m, pp, Rp,
                                  err + e * T, &it);
  for (int d = 0; d < D; ++d) {
    if (q_f64)
      ((double*)q)[e * D + d] = st == 2 ? ((const double*)q0)[e * D + d] : (double)m.q[(size_t)d * lanes];
    else
      ((float*)q)[e * D + d] = st == 2 ? ((const float*)q0)[e * D + d] : m.q[(size_t)d * lanes];
  }
  for (int i = 0; i < 3; ++i) palm_pos[e * 3 + i] = pp[i];
  for (int i = 0; i < 9; ++i) palm_rot[e * 9 + i] = Rp[i];
  iters[e] = it;
  status[e] = st;
}

// The pose-target solve (frame_ik_row): the layout of ik_solve_kernel over M = 3T + 3·popcount(rot_mask) packed rows,
// with the target quaternions and the row weights next to them in LDS (IkFrameMem).
__global__ __launch_bounds__(64) void ik_frames_kernel(IkArgs a, int64_t E, const void* __restrict__ q0, int q_f64,
                                                       const double* __restrict__ target,
                                                       const double* __restrict__ target_rot,
                                                       const double* __restrict__ palm, const double* __restrict__ w,
                                                       const double* __restrict__ wr, uint32_t rot_mask,
                                                       uint32_t dof_mask, void* __restrict__ q, double* __restrict__ err,
                                                       double* __restrict__ rot_err, int32_t* __restrict__ iters,
                                                       int32_t* __restrict__ status) {
  const IkArgs& ka = *(const IkArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
  const int lanes = (int)blockDim.x, lane = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * lanes + lane;
  if (e >= E) return;
  const int T = ka.c.n_tips, D = ka.c.n_dofs;
  const cdx::IkFrameMem f = cdx::ik_frames_mem_at(ik_lds, T, D, rot_mask, lane, lanes);
  const cdx::Q0Row q0r{q_f64 ? (const void*)((const double*)q0 + e * D) : (const void*)((const float*)q0 + e * D), q_f64};
  int32_t it;
  const int st = cdx::frame_ik_row(ka.c, ka.p, ka.po, q0r, target + e * T * 3,
                                   target_rot ? target_rot + e * T * 9 : nullptr, palm ? palm + e * 6 : nullptr,
                                   w ? w + e * T : nullptr, wr ? wr + e * T : nullptr, rot_mask, dof_mask, f,
                                   err + e * T, rot_err + e * T, &it);
  for (int d = 0; d < D; ++d) {
    if (q_f64)
      ((double*)q)[e * D + d] = st == 2 ? ((const double*)q0)[e * D + d] : (double)f.m.q[(size_t)d * lanes];
    else
      ((float*)q)[e * D + d] = st == 2 ? ((const float*)q0)[e * D + d] : f.m.q[(size_t)d * lanes];
  }
  iters[e] = it;
  status[e] = st;
}

// Lanes (rows) per workgroup: the largest power of two ≤ 64 whose rows of `row` bytes fit in 40 KB of LDS (four
// workgroups on a compute unit's 160 KB), at least 1.
int ik_lanes_bytes(size_t row) {
  int lanes = 64;
  while (lanes > 1 && row * lanes > 40960) lanes >>= 1;
  return lanes;
}
int ik_lanes(int T, int D) { return ik_lanes_bytes(cdx::ik_mem_bytes(T, D)); }

}  // namespace

extern "C" {

int cdx_fk_jacobian(const cdx_chain* chain, const float* q, int64_t B, float* lin, float* ang, cdx_stream_t stream) {
  const int rc = cdx::ik_chain_code(chain);
  if (rc) return rc;
  if (B < 0) return CDX_EINVAL;
  if (B == 0) return CDX_OK;
  if (!q || !lin) return CDX_ECHAIN;
  const int64_t n = B * chain->n_tips;
  if ((n + 63) / 64 > 0x7fffffff) return CDX_EINVAL;
  hipLaunchKernelGGL(fk_jacobian_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), *chain, q, B, lin, ang);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

size_t cdx_ik_workspace(int64_t, int32_t, int32_t) { return 0; }

int32_t cdx_ik_rows_per_block(int32_t n_tips, int32_t n_dofs) {
  if (n_tips <= 0 || n_tips > CDX_MAX_TIPS || n_dofs < 0 || n_dofs > CDX_MAX_DOFS) return 0;
  return ik_lanes(n_tips, n_dofs);
}

size_t cdx_ik_abi_size(void) { return sizeof(cdx_ik_params); }

int cdx_ik_solve(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                 const double* target, const double* palm, const double* palm_offset, const double* w, void*,
                 void* q, double* err, int32_t* iters, int32_t* status, cdx_stream_t stream) {
  int rc = cdx::ik_chain_code(chain);
  if (rc) return rc;
  IkArgs a;
  rc = cdx::ik_prepare(params, chain->n_dofs, &a.p);
  if (rc) return rc;
  if (E < 0 || (q_dtype != CDX_DTYPE_F32 && q_dtype != CDX_DTYPE_F64)) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!q0 || !target || !q || !err || !iters || !status) return CDX_ECHAIN;
  a.c = *chain;
  for (int i = 0; i < 3; ++i) {
    a.po[i] = palm_offset ? palm_offset[i] : 0.0;
    if (!__builtin_isfinite(a.po[i])) return CDX_EINVAL;
  }
  const int T = chain->n_tips, D = chain->n_dofs, lanes = ik_lanes(T, D);
  const size_t lds = cdx::ik_mem_bytes(T, D) * lanes;
  const int64_t blocks = (E + lanes - 1) / lanes;
  if (blocks > 0x7fffffff || lds > 65536) return CDX_EINVAL;
  hipLaunchKernelGGL(ik_solve_kernel, dim3((unsigned)blocks), dim3((unsigned)lanes), lds,
                     reinterpret_cast<hipStream_t>(stream), a, E, q0, (int)(q_dtype == CDX_DTYPE_F64), target, palm, w, q,
                     err, iters, status);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int32_t cdx_ik_pose_rows_per_block(int32_t n_tips, int32_t n_dofs) {
  if (n_tips <= 0 || n_tips > CDX_MAX_TIPS || n_dofs < 0 || n_dofs > CDX_MAX_DOFS) return 0;
  return ik_lanes(n_tips, n_dofs + 6);
}

int cdx_ik_solve_pose(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                      const double* target, const double* palm0_pos, const double* palm0_rot, const double* palm_offset,
                      const double* w, void*, void* q, double* palm_pos, double* palm_rot, double* err, int32_t* iters,
                      int32_t* status, cdx_stream_t stream) {
  int rc = cdx::ik_chain_code(chain);
  if (rc) return rc;
  IkArgs a;
  rc = cdx::ik_prepare(params, chain->n_dofs, &a.p);
  if (rc) return rc;
  if (E < 0 || (q_dtype != CDX_DTYPE_F32 && q_dtype != CDX_DTYPE_F64)) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!q0 || !target || !q || !palm_pos || !palm_rot || !err || !iters || !status) return CDX_ECHAIN;
  if (!palm0_pos != !palm0_rot) return CDX_ECHAIN;
  a.c = *chain;
  for (int i = 0; i < 3; ++i) {
    a.po[i] = palm_offset ? palm_offset[i] : 0.0;
    if (!__builtin_isfinite(a.po[i])) return CDX_EINVAL;
  }
  const int T = chain->n_tips, D = chain->n_dofs + 6, lanes = ik_lanes(T, D);
  const size_t lds = cdx::ik_mem_bytes(T, D) * lanes;
  const int64_t blocks = (E + lanes - 1) / lanes;
  if (blocks > 0x7fffffff || lds > 65536) return CDX_EINVAL;
  hipLaunchKernelGGL(ik_pose_kernel, dim3((unsigned)blocks), dim3((unsigned)lanes), lds,
                     reinterpret_cast<hipStream_t>(stream), a, E, q0, (int)(q_dtype == CDX_DTYPE_F64), target, palm0_pos,
                     palm0_rot, w, q, palm_pos, palm_rot, err, iters, status);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int32_t cdx_ik_frames_rows_per_block(int32_t n_tips, int32_t n_dofs, uint64_t rot_mask) {
  if (n_tips <= 0 || n_tips > CDX_MAX_TIPS || n_dofs < 0 || n_dofs > CDX_MAX_DOFS || (rot_mask >> n_tips)) return 0;
  const size_t row = cdx::ik_frames_bytes(n_tips, n_dofs, (uint32_t)rot_mask);
  return row > 65536 ? 0 : ik_lanes_bytes(row);
}

int cdx_ik_solve_frames(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                        const double* target_pos, const double* target_rot, const double* palm,
                        const double* palm_offset, const double* w, const double* wr, uint64_t rot_mask64,
                        uint64_t dof_mask64, void*, void* q, double* err, double* rot_err, int32_t* iters, int32_t* status,
                        cdx_stream_t stream) {
  int rc = cdx::ik_chain_code(chain);
  if (rc) return rc;
  IkArgs a;
  rc = cdx::ik_prepare(params, chain->n_dofs, &a.p);
  if (rc) return rc;
  if (E < 0 || (q_dtype != CDX_DTYPE_F32 && q_dtype != CDX_DTYPE_F64)) return CDX_EINVAL;
  const int T = chain->n_tips, D = chain->n_dofs;
  rc = cdx::ik_frames_mask_code(T, D, rot_mask64, dof_mask64);
  if (rc) return rc;
  const uint32_t rot_mask = (uint32_t)rot_mask64, dof_mask = (uint32_t)dof_mask64;
  const size_t row = cdx::ik_frames_bytes(T, D, rot_mask);
  if (row > 65536) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!q0 || !target_pos || !q || !err || !rot_err || !iters || !status || (rot_mask && !target_rot)) return CDX_ECHAIN;
  a.c = *chain;
  for (int i = 0; i < 3; ++i) {
    a.po[i] = palm_offset ? palm_offset[i] : 0.0;
    if (!__builtin_isfinite(a.po[i])) return CDX_EINVAL;
  }
  const int lanes = ik_lanes_bytes(row);
  const size_t lds = row * lanes;
  const int64_t blocks = (E + lanes - 1) / lanes;
  if (blocks > 0x7fffffff || lds > 65536) return CDX_EINVAL;
  hipLaunchKernelGGL(ik_frames_kernel, dim3((unsigned)blocks), dim3((unsigned)lanes), lds,
                     reinterpret_cast<hipStream_t>(stream), a, E, q0, (int)(q_dtype == CDX_DTYPE_F64), target_pos,
                     target_rot, palm, w, wr, rot_mask, dof_mask, q, err, rot_err, iters, status);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
