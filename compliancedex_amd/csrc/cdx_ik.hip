// Fingertip Jacobians and batched inverse kinematics on gfx950 (the rule: cdx_ik.h).
//
//   fk_jacobian_kernel  one lane per (row, tip): two walks of the tip's path with a running pose, the columns written
//                       straight to the outputs.
//   the solve kernels   one lane per candidate, the WHOLE Levenberg–Marquardt solve in one launch.  Everything a row
//                       indexes at run time (cdx_ik.h, "Storage") lives in LDS, the lanes of a workgroup interleaved
//                       element by element (element i of lane l at i·lanes + l: consecutive lanes on consecutive
//                       banks); a lane touches only its own slots, so the kernels have no barrier and no cross-lane
//                       operation, and a row cannot steer another.  The loop of a wave ends when its last row stops
//                       (rows that stopped sit masked off).  The workgroup is sized by the LDS a row needs
//                       (ik_lanes): the largest power of two ≤ 64 lanes that leaves room for four workgroups on
//                       a compute unit.  The three kernels share their start (ik_lane), the row function
//                       (cdx::ik_lm_row) and the write-back of q (cdx::ik_store_q); each names its own arrays:
//   ik_solve_kernel     the fixed palm (ik_row): a hand's row needs 1.9 KB, so 16 rows share a workgroup.
//   ik_pose_kernel      the free wrist (ik_pose_row): six more columns per row of Jl (a hand's row needs 2.3 KB, still
//                       16 rows a workgroup; iiwa7_allegro 2.8 KB, 8 rows), the palm pose and its trial copy in
//                       registers.
//   ik_frames_kernel    pose targets and held joints (frame_ik_row): three more rows of Jl per oriented tip, the target
//                       quaternions and the row weights in LDS as well (iiwa7_allegro's palm link, one oriented tip:
//                       1.3 KB a row, 16 rows a workgroup).
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

// What a solve kernel starts with: the arguments read in place (as above), the lane's row e (≥ E: nothing to do), its
// storage in LDS and its row of q0.
struct IkLane {
  const IkArgs* a;
  int64_t e;
  cdx::IkMem m;
  cdx::Q0Row q0;
};
template <class V>
__device__ __forceinline__ IkLane ik_lane(const void* q0, int q_f64, uint32_t rot_mask) {
  IkLane l;
  l.a = (const IkArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
  const int lanes = (int)blockDim.x, lane = (int)threadIdx.x;
  l.e = (int64_t)blockIdx.x * lanes + lane;
  l.m = cdx::ik_mem_at<V>(ik_lds, l.a->c.n_tips, l.a->c.n_dofs, rot_mask, lane, lanes);
  l.q0 = cdx::ik_q0_row(q0, q_f64, l.e, l.a->c.n_dofs);
  return l;
}

__global__ __launch_bounds__(64) void ik_solve_kernel(IkArgs a, int64_t E, const void* __restrict__ q0, int q_f64,
                                                      const double* __restrict__ target,
                                                      const double* __restrict__ palm, const double* __restrict__ w,
                                                      void* __restrict__ q, double* __restrict__ err,
                                                      int32_t* __restrict__ iters, int32_t* __restrict__ status) {
  const IkLane l = ik_lane<cdx::IkFixed>(q0, q_f64, 0);
  if (l.e >= E) return;
  const int64_t e = l.e;
  const int T = l.a->c.n_tips;
  int32_t it;
  const int st = cdx::ik_row(l.a->c, l.a->p, l.a->po, l.q0, target + e * T * 3, palm ? palm + e * 6 : nullptr,
                             w ? w + e * T : nullptr, l.m, err + e * T, &it);
  cdx::ik_store_q(q, q0, q_f64, e, l.a->c.n_dofs, st, l.m);
  iters[e] = it;
  status[e] = st;
}

__global__ __launch_bounds__(64) void ik_pose_kernel(IkArgs a, int64_t E, const void* __restrict__ q0, int q_f64,
                                                     const double* __restrict__ target,
                                                     const double* __restrict__ palm0_pos,
                                                     const double* __restrict__ palm0_rot, const double* __restrict__ w,
                                                     void* __restrict__ q, double* __restrict__ palm_pos,
                                                     double* __restrict__ palm_rot, double* __restrict__ err,
                                                     int32_t* __restrict__ iters, int32_t* __restrict__ status) {
  const IkLane l = ik_lane<cdx::IkPose>(q0, q_f64, 0);
  if (l.e >= E) return;
  const int64_t e = l.e;
  const int T = l.a->c.n_tips;
  int32_t it;
  const int st = cdx::ik_pose_row(l.a->c, l.a->p, l.a->po, l.q0, target + e * T * 3,
                                  palm0_pos ? palm0_pos + e * 3 : nullptr, palm0_rot ? palm0_rot + e * 9 : nullptr,
                                  w ? w + e * T : nullptr, l.m, palm_pos + e * 3, palm_rot + e * 9, err + e * T, &it);
  cdx::ik_store_q(q, q0, q_f64, e, l.a->c.n_dofs, st, l.m);
  iters[e] = it;
  status[e] = st;
}

__global__ __launch_bounds__(64) void ik_frames_kernel(IkArgs a, int64_t E, const void* __restrict__ q0, int q_f64,
                                                       const double* __restrict__ target,
                                                       const double* __restrict__ target_rot,
                                                       const double* __restrict__ palm, const double* __restrict__ w,
                                                       const double* __restrict__ wr, uint32_t rot_mask,
                                                       uint32_t dof_mask, void* __restrict__ q, double* __restrict__ err,
                                                       double* __restrict__ rot_err, int32_t* __restrict__ iters,
                                                       int32_t* __restrict__ status) {
  const IkLane l = ik_lane<cdx::IkFrames>(q0, q_f64, rot_mask);
  if (l.e >= E) return;
  const int64_t e = l.e;
  const int T = l.a->c.n_tips;
  int32_t it;
  const int st = cdx::frame_ik_row(l.a->c, l.a->p, l.a->po, l.q0, target + e * T * 3,
                                   target_rot ? target_rot + e * T * 9 : nullptr, palm ? palm + e * 6 : nullptr,
                                   w ? w + e * T : nullptr, wr ? wr + e * T : nullptr, rot_mask, dof_mask, l.m,
                                   err + e * T, rot_err + e * T, &it);
  cdx::ik_store_q(q, q0, q_f64, e, l.a->c.n_dofs, st, l.m);
  iters[e] = it;
  status[e] = st;
}

// Lanes (rows) per workgroup: the largest power of two ≤ 64 whose rows of `row` bytes fit in 40 KB of LDS (four
// workgroups on a compute unit's 160 KB), at least 1.
int ik_lanes(size_t row) {
  int lanes = 64;
  while (lanes > 1 && row * lanes > 40960) lanes >>= 1;
  return lanes;
}

// One launch of a solve kernel over E rows of `row` bytes each: CDX_EINVAL if the grid or a workgroup's LDS is too
// large.
template <class K, class... A>
int ik_launch(K kernel, size_t row, int64_t E, cdx_stream_t stream, const A&... args) {
  const int lanes = ik_lanes(row);
  const size_t lds = row * lanes;
  const int64_t blocks = (E + lanes - 1) / lanes;
  if (blocks > 0x7fffffff || lds > 65536) return CDX_EINVAL;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)lanes), lds, reinterpret_cast<hipStream_t>(stream),
                     args...);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

bool ik_sizes_ok(int32_t n_tips, int32_t n_dofs) {
  return n_tips > 0 && n_tips <= CDX_MAX_TIPS && n_dofs >= 0 && n_dofs <= CDX_MAX_DOFS;
}

}  // namespace

extern "C" {

int cdx_fk_jacobian(const cdx_chain* chain, const float* q, int64_t B, float* lin, float* ang, cdx_stream_t stream) {
  const int rc = cdx::chain_code(chain);
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
  return ik_sizes_ok(n_tips, n_dofs) ? ik_lanes(cdx::ik_mem_bytes<cdx::IkFixed>(n_tips, n_dofs, 0)) : 0;
}

size_t cdx_ik_abi_size(void) { return sizeof(cdx_ik_params); }

int cdx_ik_solve(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                 const double* target, const double* palm, const double* palm_offset, const double* w, void*,
                 void* q, double* err, int32_t* iters, int32_t* status, cdx_stream_t stream) {
  IkArgs a;
  int rc = cdx::ik_call_code(chain, params, E, q_dtype, &a.p);
  if (rc || E == 0) return rc;
  if (!q0 || !target || !q || !err || !iters || !status) return CDX_ECHAIN;
  rc = cdx::ik_offset_code(palm_offset, a.po);
  if (rc) return rc;
  a.c = *chain;
  return ik_launch(ik_solve_kernel, cdx::ik_mem_bytes<cdx::IkFixed>(chain->n_tips, chain->n_dofs, 0), E, stream, a, E, q0,
                   (int)(q_dtype == CDX_DTYPE_F64), target, palm, w, q, err, iters, status);
}

int32_t cdx_ik_pose_rows_per_block(int32_t n_tips, int32_t n_dofs) {
  return ik_sizes_ok(n_tips, n_dofs) ? ik_lanes(cdx::ik_mem_bytes<cdx::IkPose>(n_tips, n_dofs, 0)) : 0;
}

int cdx_ik_solve_pose(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                      const double* target, const double* palm0_pos, const double* palm0_rot, const double* palm_offset,
                      const double* w, void*, void* q, double* palm_pos, double* palm_rot, double* err, int32_t* iters,
                      int32_t* status, cdx_stream_t stream) {
  IkArgs a;
  int rc = cdx::ik_call_code(chain, params, E, q_dtype, &a.p);
  if (rc || E == 0) return rc;
  if (!q0 || !target || !q || !palm_pos || !palm_rot || !err || !iters || !status) return CDX_ECHAIN;
  if (!palm0_pos != !palm0_rot) return CDX_ECHAIN;
  rc = cdx::ik_offset_code(palm_offset, a.po);
  if (rc) return rc;
  a.c = *chain;
  return ik_launch(ik_pose_kernel, cdx::ik_mem_bytes<cdx::IkPose>(chain->n_tips, chain->n_dofs, 0), E, stream, a, E, q0,
                   (int)(q_dtype == CDX_DTYPE_F64), target, palm0_pos, palm0_rot, w, q, palm_pos, palm_rot, err, iters,
                   status);
}

int32_t cdx_ik_frames_rows_per_block(int32_t n_tips, int32_t n_dofs, uint64_t rot_mask) {
  if (!ik_sizes_ok(n_tips, n_dofs) || (rot_mask >> n_tips)) return 0;
  const size_t row = cdx::ik_mem_bytes<cdx::IkFrames>(n_tips, n_dofs, (uint32_t)rot_mask);
  return row > 65536 ? 0 : ik_lanes(row);
}

int cdx_ik_solve_frames(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                        const double* target_pos, const double* target_rot, const double* palm,
                        const double* palm_offset, const double* w, const double* wr, uint64_t rot_mask64,
                        uint64_t dof_mask64, void*, void* q, double* err, double* rot_err, int32_t* iters, int32_t* status,
                        cdx_stream_t stream) {
  IkArgs a;
  int rc = cdx::ik_call_code(chain, params, E, q_dtype, &a.p);
  if (rc) return rc;
  rc = cdx::ik_frames_mask_code(chain->n_tips, chain->n_dofs, rot_mask64, dof_mask64);
  if (rc) return rc;
  const uint32_t rot_mask = (uint32_t)rot_mask64, dof_mask = (uint32_t)dof_mask64;
  const size_t row = cdx::ik_mem_bytes<cdx::IkFrames>(chain->n_tips, chain->n_dofs, rot_mask);
  if (row > 65536) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!q0 || !target_pos || !q || !err || !rot_err || !iters || !status || (rot_mask && !target_rot)) return CDX_ECHAIN;
  rc = cdx::ik_offset_code(palm_offset, a.po);
  if (rc) return rc;
  a.c = *chain;
  return ik_launch(ik_frames_kernel, row, E, stream, a, E, q0, (int)(q_dtype == CDX_DTYPE_F64), target_pos, target_rot,
                   palm, w, wr, rot_mask, dof_mask, q, err, rot_err, iters, status);
}

}  // extern "C"
