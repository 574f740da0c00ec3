// GPIS-mode optimiser iteration for gfx950 (GPISGraspOptimizer, optimize_pregrasp.py:322-406; KinGPISGraspOptimizer,
// :408-511): the per-candidate cost-and-backward and the step of cdx_gpis_mode.h, one lane per candidate, as two
// launches (cdx_gpis_mode_cost, cdx_gpis_mode_step) or one (cdx_gpis_mode_iteration, four fingertips).
//
// Lane layout: one lane per candidate (kin_cost_kernel's): the simpler of the two layouts the project has, chosen
// because the iteration's long pole is the exact-variance GEMM over E·T rows, not this launch; kin_cost4_kernel's four
// lanes per candidate were not measured here.  Register budget: the reward's tape fills most of the file, so the cost
// terms read the candidate's rows in place, add their own gradients after ForceEq's backward instead of holding them
// across it, and the one-launch form fences the step's loads behind the cost.  A lane reads and writes only its
// own candidate's rows (and its own column of the LDS scratch), so there is no barrier; lanes past E are predicated
// off and only take part in the wave vote of the `any` flag.  The one-launch form runs the same two device
// functions back to back in the same lane — the step re-reads the gradients the lane has just stored — hence the
// same bits as the two launches.
#include <hip/hip_runtime.h>

#include "cdx_gpis_mode.h"

#pragma clang fp contract(off)

namespace {

enum { PHASE_COST = 1, PHASE_STEP = 2 };

// chain first: the FK walks read it in place from the kernel-argument segment (indexed by a per-lane body index, a
// by-value copy goes to scratch)
template <int NT, int MAXD, bool FK, int PHASE>
__global__ __launch_bounds__(64) void gpis_mode_kernel(cdx_chain chain_, cdx_gpis_mode_params p, cdx_gpis_mode_opt cfg,
                                                       cdx_gpis_mode_buffers b, int64_t E, int T_rt,
                                                       const double* noise, uint64_t seed, int s, int finalize) {
  __shared__ float s_fk[FK && (PHASE & PHASE_COST) ? CDX_MAX_DOFS : 1][64];  // the FK backward's per-DOF sums
  const cdx_chain& chain = *(const cdx_chain*)(__builtin_amdgcn_kernarg_segment_ptr());
  (void)chain_;
  const int T = NT > 0 ? NT : T_rt;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = e < E;
  bool flag = false;
  if (on) {
    if constexpr ((PHASE & PHASE_COST) != 0) {
      const int slot = s & 1;
      cdx::gpis_mode_cost_candidate<NT, MAXD, FK>(
          chain, p, T, e, FK ? b.pose : nullptr, FK ? b.tips : b.pose, b.target, b.comp, noise, seed, b.mean, b.gmean,
          b.normal, b.std, b.gstd, b.tmean, b.tgmean, b.loss, b.margin[slot], b.normal_slot[slot], FK ? b.g_pose : nullptr,
          b.g_target, b.g_comp, FK ? b.g_tip : b.g_pose, &s_fk[0][threadIdx.x], 64);
    }
    // (one launch: the step's loads are not to be hoisted into the cost, whose registers are all in use)
    if constexpr (PHASE == (PHASE_COST | PHASE_STEP)) __builtin_amdgcn_sched_barrier(0);
    if constexpr ((PHASE & PHASE_STEP) != 0) {
      // commit the previous iteration's margin / normal if some candidate improved in it (its flags are final: that
      // launch has finished)
      if (s > 0 && b.any[(s - 1) % 3]) cdx::gpis_mode_commit(b, T, e, (s - 1) & 1);
      if (!finalize) {
        if (e == 0) b.any[(s + 1) % 3] = 0u;  // (written at s − 2, read at s − 1: free now)
        flag = cdx::gpis_mode_step_candidate<FK>(chain, p, cfg, b, T, e);
      }
    }
  }
  if constexpr ((PHASE & PHASE_STEP) != 0) {
    if (__any(flag) && (threadIdx.x & 63) == 0) atomicOr(b.any + s % 3, 1u);
  }
}

template <int PHASE>
int launch(const cdx_chain* chain, const cdx_gpis_mode_params* p, const cdx_gpis_mode_opt* cfg,
           const cdx_gpis_mode_buffers* buf, int64_t E, int T, const double* noise, uint64_t seed, int s, int finalize,
           cdx_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((E + 63) / 64));
  const bool fk = p->mode == 1;
  const cdx_chain c = fk ? *chain : cdx_chain{};
  const cdx_gpis_mode_opt o = cfg ? *cfg : cdx_gpis_mode_opt{};
  const bool shallow = !fk || cdx::chain_max_depth(*chain) <= 8;
#define CDX_GM_LAUNCH(NT, MAXD, FK)                                                                                  \
  hipLaunchKernelGGL((gpis_mode_kernel<NT, MAXD, FK, PHASE>), grid, dim3(64), 0, st, c, *p, o, *buf, E, T, noise, seed, \
                     s, finalize)
  if constexpr (PHASE == PHASE_STEP) {  // (the step has no fingertip-count or depth specialisation)
    if (fk) CDX_GM_LAUNCH(0, 8, true);
    else CDX_GM_LAUNCH(0, 8, false);
  } else {
    if (!fk && T == 4) CDX_GM_LAUNCH(4, 8, false);
    else if (!fk) CDX_GM_LAUNCH(0, 8, false);
    else if (T == 4 && shallow) CDX_GM_LAUNCH(4, 8, true);
    else if (T == 4) CDX_GM_LAUNCH(4, CDX_MAX_DEPTH, true);
    else if (shallow) CDX_GM_LAUNCH(0, 8, true);
    else CDX_GM_LAUNCH(0, CDX_MAX_DEPTH, true);
  }
#undef CDX_GM_LAUNCH
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // namespace

extern "C" int cdx_gpis_mode_cost(const cdx_chain* chain, const cdx_gpis_mode_params* p, const cdx_gpis_mode_buffers* buf,
                                  int64_t E, int32_t n_tips, const double* noise, uint64_t seed, int32_t iteration,
                                  cdx_stream_t stream) {
  if (cdx::gpis_mode_check(chain, p, E, n_tips) || iteration < 0) return CDX_EINVAL;
  if (cdx::gpis_mode_check_chain(chain, p)) return CDX_ECHAIN;
  if (E == 0) return CDX_OK;
  if (cdx::gpis_mode_check_cost(p, buf)) return CDX_EINVAL;
  return launch<PHASE_COST>(chain, p, nullptr, buf, E, n_tips, noise, seed, iteration, 0, stream);
}

extern "C" int cdx_gpis_mode_step(const cdx_chain* chain, const cdx_gpis_mode_params* p, const cdx_gpis_mode_opt* opt,
                                  const cdx_gpis_mode_buffers* buf, int64_t E, int32_t n_tips, int32_t iteration,
                                  int32_t finalize, cdx_stream_t stream) {
  if (cdx::gpis_mode_check(chain, p, E, n_tips) || !opt) return CDX_EINVAL;
  if (cdx::gpis_mode_check_chain(chain, p)) return CDX_ECHAIN;
  if (E == 0) return CDX_OK;
  if (cdx::gpis_mode_check_step(opt, buf, iteration, finalize)) return CDX_EINVAL;
  return launch<PHASE_STEP>(chain, p, opt, buf, E, n_tips, nullptr, 0, iteration, finalize, stream);
}

extern "C" int cdx_gpis_mode_iteration(const cdx_chain* chain, const cdx_gpis_mode_params* p,
                                       const cdx_gpis_mode_opt* opt, const cdx_gpis_mode_buffers* buf, int64_t E,
                                       int32_t n_tips, const double* noise, uint64_t seed, int32_t iteration,
                                       cdx_stream_t stream) {
  if (cdx::gpis_mode_check(chain, p, E, n_tips) || !opt) return CDX_EINVAL;
  if (cdx::gpis_mode_check_chain(chain, p)) return CDX_ECHAIN;
  if (E == 0) return CDX_OK;
  if (cdx::gpis_mode_check_cost(p, buf) || cdx::gpis_mode_check_step(opt, buf, iteration, 0)) return CDX_EINVAL;
  if (n_tips != 4) {  // the two launches
    const int rc = launch<PHASE_COST>(chain, p, nullptr, buf, E, n_tips, noise, seed, iteration, 0, stream);
    if (rc) return rc;
    return launch<PHASE_STEP>(chain, p, opt, buf, E, n_tips, nullptr, 0, iteration, 0, stream);
  }
  return launch<PHASE_COST | PHASE_STEP>(chain, p, opt, buf, E, n_tips, noise, seed, iteration, 0, stream);
}

extern "C" void cdx_gpis_mode_abi_sizes(size_t* out) {
  out[0] = sizeof(cdx_gpis_mode_params);
  out[1] = sizeof(cdx_gpis_mode_opt);
  out[2] = sizeof(cdx_gpis_mode_buffers);
}
