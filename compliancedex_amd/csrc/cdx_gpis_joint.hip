// The GPIS posterior covariance of (f, ∇f) on gfx950 (the rule: cdx_gpis_joint.h): Σ(x) = P0 − WᵀW with
// W = L⁻¹·[k, ∂ₓk, ∂ᵧk, ∂_z k], a sibling of the whitened std pass with four columns a query instead of one.
//
//   gpis_joint_kernel    one wave per tile of 4 queries and per split of the state's columns; a workgroup is 4 waves
//                        with 4 neighbouring tiles.  The product W = B·L⁻ᵀ runs on v_mfma_f64_16x16x4_f64 with the 16
//                        rows of the A tile ordered row = q + 4·c (4 queries q, 4 components c), every lane generating
//                        its own A element from its (q, j, c) on chip.  The f64 C/D map (col = lane & 15, row =
//                        (lane >> 4) + 4·reg) then leaves in one lane's four accumulators exactly one query's
//                        (k, ∂ₓ, ∂ᵧ, ∂_z) column of W against one column n of L⁻ᵀ: the 10 products of the Gram matrix
//                        are lane-local FMAs, accumulated over the 8 column tiles of a 128-column block and over the
//                        split's blocks, then summed over the 16 lanes that share lane >> 4 by xor-shuffles.  L⁻ᵀ is
//                        upper triangular: a block starting at column nb needs the rows j < nb + 128 only, and past
//                        row nb a column tile n0 takes part while j ≤ n0 + 15.  No LDS, no barrier, no atomics.
//   gpis_joint_finalize  one lane per output entry: prior − Σ_s partial[s] in the order of s.
//
// How the columns are split (cdx::joint_splits) depends on N alone and a query's row of the A tile meets no other
// query's data, so a row's 10 outputs have the same bits whatever M, the row's place and its neighbours.  The pad
// rows of the last tile replicate query M − 1 and are not written.
#include <hip/hip_runtime.h>

#include "cdx_gpis_joint.h"

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

constexpr int JT_WAVES = 4;                      // query tiles per workgroup
constexpr int JT_TILES = cdx::JOINT_BLOCK / 16;  // MFMA column tiles per block

// One K-step (the four inducing points j0 … j0 + 3) of a block: the lane's A element against the block's column
// tiles.  DIAG: past the block's first column only the tiles with j0 ≤ n0 + 15 are non-zero.
template <int KT, bool DIAG>
__device__ __forceinline__ void joint_kstep(const double* __restrict__ X1, const double* __restrict__ Bp, int j0,
                                            int rel, double x0, double x1, double x2, int c, double R,
                                            double inv_s2, int64_t ld, dbl4 (&acc)[JT_TILES]) {
  const double* xj = X1 + 3 * (int64_t)j0;
  const double a = cdx::gpis_joint_entry<KT, true>(x0 - xj[0], x1 - xj[1], x2 - xj[2], c, R, inv_s2);
  const double* bp = Bp + (int64_t)j0 * ld;
#pragma unroll
  for (int t = 0; t < JT_TILES; ++t) {
    if (DIAG && rel >= 16 * (t + 1)) continue;  // wave-uniform
    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bp[16 * t], acc[t], 0, 0, 0);
  }
}

template <int KT>
__global__ __launch_bounds__(64 * JT_WAVES) void gpis_joint_kernel(const cdx_gpis g, const double* __restrict__ X,
                                                                   int64_t M, int64_t tiles, int splits,
                                                                   double* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * JT_WAVES + (threadIdx.x >> 6);
  if (tile >= tiles) return;
  const int split = blockIdx.y;
  const int N = g.N;
  const int64_t ld = g.N_pad;
  const double R = g.R, inv_s2 = 1.0 / (g.sigma * g.sigma);
  // A operand: row = lane & 15 = q + 4·c, k = lane >> 4
  const int c = (lane & 15) >> 2, kk = lane >> 4;
  int64_t ma = tile * 4 + (lane & 3);
  ma = ma < M ? ma : M - 1;
  const double x0 = X[3 * ma], x1 = X[3 * ma + 1], x2 = X[3 * ma + 2];
  const double* X1 = g.X1 + 3 * kk;                     // the lane's inducing point of a K-step
  const double* B = g.Linv_t + (int64_t)kk * ld + (lane & 15);  // B[k = lane >> 4][col = lane & 15]
  const int kend = (N + 3) & ~3;                        // rows ≥ N of L⁻ᵀ are zero (kend ≤ N_pad)
  double gram[cdx::JOINT_OUT] = {};
  const int blocks = cdx::joint_blocks(N);
  for (int blk = split; blk < blocks; blk += splits) {
    const int nb = blk * cdx::JOINT_BLOCK;
    dbl4 acc[JT_TILES];
#pragma unroll
    for (int t = 0; t < JT_TILES; ++t) acc[t] = dbl4{0, 0, 0, 0};
    const double* Bp = B + nb;
    for (int j0 = 0; j0 < nb; j0 += 4) joint_kstep<KT, false>(X1, Bp, j0, 0, x0, x1, x2, c, R, inv_s2, ld, acc);
    const int jend = kend < nb + cdx::JOINT_BLOCK ? kend : nb + cdx::JOINT_BLOCK;
    for (int j0 = nb; j0 < jend; j0 += 4) joint_kstep<KT, true>(X1, Bp, j0, j0 - nb, x0, x1, x2, c, R, inv_s2, ld, acc);
    // acc[t][r]: component r of query lane >> 4 against column nb + 16·t + (lane & 15)
#pragma unroll
    for (int t = 0; t < JT_TILES; ++t) {
      const double w[4] = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
      cdx::gpis_joint_gram(w, gram);
    }
  }
#pragma unroll
  for (int e = 0; e < cdx::JOINT_OUT; ++e)
#pragma unroll
    for (int w = 1; w < 16; w <<= 1) gram[e] += __shfl_xor(gram[e], w);
  const int64_t mo = tile * 4 + kk;
  if ((lane & 15) == 0 && mo < M) {
    double* p = partial + ((int64_t)split * M + mo) * cdx::JOINT_OUT;
#pragma unroll
    for (int e = 0; e < cdx::JOINT_OUT; ++e) p[e] = gram[e];
  }
}

template <int KT>
__global__ __launch_bounds__(256) void gpis_joint_finalize(const double* __restrict__ partial, int64_t M, int splits,
                                                           double R, double sigma, double* __restrict__ cov) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = M * cdx::JOINT_OUT;
  if (i >= n) return;
  double s = 0.0;
  for (int k = 0; k < splits; ++k) s += partial[(int64_t)k * n + i];
  cov[i] = cdx::gpis_joint_prior<KT>((int)(i % cdx::JOINT_OUT), R, 1.0 / (sigma * sigma)) - s;
}

template <int KT>
void joint_launch(const cdx_gpis& g, const double* X, int64_t M, double* cov, double* partial, hipStream_t s) {
  const int64_t tiles = (M + 3) / 4;
  const int splits = cdx::joint_splits(g.N);
  hipLaunchKernelGGL(gpis_joint_kernel<KT>, dim3((unsigned)((tiles + JT_WAVES - 1) / JT_WAVES), (unsigned)splits),
                     dim3(64 * JT_WAVES), 0, s, g, X, M, tiles, splits, partial);
  hipLaunchKernelGGL(gpis_joint_finalize<KT>, dim3((unsigned)((M * cdx::JOINT_OUT + 255) / 256)), dim3(256), 0, s,
                     partial, M, splits, g.R, g.sigma, cov);
}

bool joint_state_ok(const cdx_gpis* g) {
  return g && g->X1 && g->Linv_t && g->N > 0 && g->N_pad >= g->N && g->N_pad % CDX_NPAD_ALIGN == 0 && g->kernel >= 0 &&
         g->kernel <= 2;
}

constexpr int64_t JOINT_MAX_M = (int64_t)1 << 32;  // keeps both grids within 2³¹ − 1 workgroups

}  // namespace

extern "C" {

size_t cdx_gpis_joint_workspace(const cdx_gpis* g, int64_t M) {
  if (!g || M <= 0 || M > JOINT_MAX_M || g->N <= 0) return 0;
  return (size_t)cdx::joint_splits(g->N) * (size_t)M * cdx::JOINT_OUT * sizeof(double);
}

int cdx_gpis_joint(const cdx_gpis* g, const double* X, int64_t M, double* cov, void* workspace, cdx_stream_t stream) {
  if (!joint_state_ok(g)) return g && (g->kernel < 0 || g->kernel > 2) ? CDX_EKERNEL : CDX_EINVAL;
  if (M < 0 || M > JOINT_MAX_M || (M > 0 && (!X || !cov || !workspace))) return CDX_EINVAL;
  if (M == 0) return CDX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* partial = static_cast<double*>(workspace);
  switch (g->kernel) {
    case CDX_KERNEL_TPS: joint_launch<CDX_KERNEL_TPS>(*g, X, M, cov, partial, s); break;
    case CDX_KERNEL_RBF: joint_launch<CDX_KERNEL_RBF>(*g, X, M, cov, partial, s); break;
    default: joint_launch<CDX_KERNEL_JOINT>(*g, X, M, cov, partial, s); break;
  }
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
