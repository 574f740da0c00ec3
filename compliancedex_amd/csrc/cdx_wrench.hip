// Batched minimum-wrench contact forces on gfx950 (the rule: cdx_wrench.h).
//
//   min_wrench_kernel   one lane per candidate, the WHOLE solve (set-up, 6 × 6 factorisation, every ADMM iteration, the
//                       duality-gap checks, the outputs) in one launch.  The layout is ik_solve_kernel's: everything a
//                       row indexes at run time (n̂, r, x, z, u, the two 6-vectors and the factor: 15T + 33 doubles)
//                       lives in LDS, the lanes of a workgroup interleaved element by element (element i of lane l at
//                       i·lanes + l: consecutive lanes on consecutive 8-byte slots, conflict-free ds_read_b64); a lane
//                       touches only its own slots, so the kernel has no barrier and no cross-lane operation, and a
//                       row cannot steer another.  The best pair checked so far is kept in the row's own outputs
//                       (forces, dual) in global memory, not in LDS.  The loop of a wave ends when its last row stops.
//                       The workgroup is the largest power of two ≤ 64 lanes whose rows fit in 48 KB (three workgroups
//                       on a compute unit's 160 KB): a whole wave up to four tips (744 B a row), 32 lanes beyond.
#include <hip/hip_runtime.h>

#include "cdx_wrench.h"

namespace {

extern __shared__ __attribute__((aligned(16))) char wr_lds[];

__global__ __launch_bounds__(64) void min_wrench_kernel(cdx_wrench_params p, int64_t E, const double* __restrict__ tips,
                                                        const double* __restrict__ normals, double* forces,
                                                        double* __restrict__ wrench, double* __restrict__ margin,
                                                        double* dual, double* __restrict__ gap,
                                                        int32_t* __restrict__ iters, int32_t* __restrict__ status,
                                                        double* __restrict__ grad) {
  const int lanes = (int)blockDim.x, lane = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * lanes + lane;
  if (e >= E) return;
  const int T = p.n_tips;
  const cdx::WrMem m = cdx::wr_mem_at(wr_lds, T, lane, lanes);
  int32_t it;
  const int st = cdx::mw_row(p, tips + e * T * 3, normals + e * T * 3, m, forces + e * T * 3, wrench + e, margin + e * T,
                             dual + e * 6, gap + e, &it, grad ? grad + e * T * 3 : nullptr);
  iters[e] = it;
  status[e] = st;
}

int wr_lanes(int T) {
  const size_t row = cdx::wr_mem_bytes(T);
  int lanes = 64;
  while (lanes > 1 && row * lanes > 49152) lanes >>= 1;
  return lanes;
}

}  // namespace

extern "C" {

int32_t cdx_wrench_rows_per_block(int32_t n_tips) {
  if (n_tips < 1 || n_tips > CDX_MAX_TIPS) return 0;
  return wr_lanes(n_tips);
}

size_t cdx_wrench_abi_size(void) { return sizeof(cdx_wrench_params); }

int cdx_min_wrench(const cdx_wrench_params* params, int64_t E, const double* tips, const double* normals,
                   double* forces, double* wrench, double* margin, double* dual, double* gap, int32_t* iters,
                   int32_t* status, double* grad_tips, cdx_stream_t stream) {
  const int rc = cdx::wr_params_code(params);
  if (rc) return rc;
  if (E < 0) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!tips || !normals || !forces || !wrench || !margin || !dual || !gap || !iters || !status) return CDX_EINVAL;
  const int T = params->n_tips, lanes = wr_lanes(T);
  const size_t lds = cdx::wr_mem_bytes(T) * lanes;
  const int64_t blocks = (E + lanes - 1) / lanes;
  if (blocks > 0x7fffffff || lds > 65536) return CDX_EINVAL;
  hipLaunchKernelGGL(min_wrench_kernel, dim3((unsigned)blocks), dim3((unsigned)lanes), lds,
                     reinterpret_cast<hipStream_t>(stream), *params, E, tips, normals, forces, wrench, margin, dual, gap,
                     iters, status, grad_tips);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
