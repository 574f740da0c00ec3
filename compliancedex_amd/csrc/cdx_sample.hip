// Area-weighted surface sampling for gfx950: a cloud of a mesh's whole surface, the step in front of the Poisson-disk
// cloud every run of the reference on a mesh object opens with (optimize_pregrasp.py:887, gpis.py:199-263).  The rule
// is csrc/cdx_sample.h; everything below gives its bits whatever the launch shape.
//
//   Prepare, once per mesh (five launches on the caller's stream, integers from the second on, no float atomics):
//     sample_area_kernel     area of every face into the workspace, the largest of each workgroup's SAMPLE_FACES faces
//     sample_max_kernel      one workgroup: the largest area A, and info = (A == 0)
//     sample_scan_kernel<0>  weights floor(area/A·2³²), their sum per workgroup
//     sample_offsets_kernel  one workgroup: exclusive prefix sums of those sums (the pattern of cdx_field.hip's
//                            surface_scan_kernel)
//     sample_scan_kernel<1>  the weights again, scanned in the workgroup on top of its offset: C [F] uint64
//   Draw, one lane per sample, workgroups striding over tiles of their size:
//     sample_draw_kernel<T, CAP>  LDS holds NS ≤ CAP splitters of C, the last entry of every run of `stride` faces
//                            (stride the smallest power of two with ceil(F / stride) ≤ CAP).  Philox in registers,
//                            __umul64hi, a binary search of the splitters in LDS; with stride > 1 the search ends in the
//                            run's `stride` entries of C in global memory.  Then the face gather, the point, and the
//                            outputs through an LDS transpose so that consecutive lanes store consecutive doubles.
//       mode 1 (table)       CAP = 16384: C whole in 128 KiB of LDS, one workgroup of 1024 lanes alone on its CU
//       mode 2 (splitters)   CAP = 2048: 16 KiB, workgroups of 256 lanes, seven a CU; whole tables up to 2048 faces
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cdx_sample.h"

namespace {

constexpr int SAMPLE_BLOCK = 256;  // prepare
constexpr int SAMPLE_WAVES = SAMPLE_BLOCK / 64;
constexpr int SAMPLE_PER = 4;
constexpr int SAMPLE_FACES = SAMPLE_BLOCK * SAMPLE_PER;  // faces per workgroup of the scan

constexpr int SAMPLE_TABLE_CAP = 16384;  // mode 1: entries of C in LDS (128 KiB of the CU's 160 KiB)
constexpr int SAMPLE_TABLE_BLOCK = 1024;
constexpr int SAMPLE_SPLIT_CAP = 2048;  // mode 2: 16 KiB
constexpr int SAMPLE_SPLIT_BLOCK = 256;
constexpr int SAMPLE_CUS = 256;  // MI355X
constexpr int64_t SAMPLE_MAX_FACES = 0x7fffffff / 9;

int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

template <typename T>
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_area_kernel(const T* __restrict__ faces, int64_t F,
                                                                   double* __restrict__ area,
                                                                   double* __restrict__ bmax) {
  __shared__ double s_m[SAMPLE_BLOCK];
  const int tid = threadIdx.x;
  double m = 0.0;
#pragma unroll
  for (int u = 0; u < SAMPLE_PER; ++u) {
    const int64_t f = (int64_t)blockIdx.x * SAMPLE_FACES + u * SAMPLE_BLOCK + tid;
    if (f < F) {
      const double a = cdx::sample_area(cdx::sample_face(faces + 9 * f));
      area[f] = a;
      m = fmax(m, a);
    }
  }
  s_m[tid] = m;
  __syncthreads();
  for (int off = SAMPLE_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) s_m[tid] = fmax(s_m[tid], s_m[tid + off]);
    __syncthreads();
  }
  if (tid == 0) bmax[blockIdx.x] = s_m[0];
}

// Areas are finite and ≥ 0, so the maximum does not depend on the order it is taken in.
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_max_kernel(const double* __restrict__ bmax, int64_t G,
                                                                  double* __restrict__ amax,
                                                                  int32_t* __restrict__ info) {
  __shared__ double s_m[SAMPLE_BLOCK];
  const int tid = threadIdx.x;
  double m = 0.0;
  for (int64_t g = tid; g < G; g += SAMPLE_BLOCK) m = fmax(m, bmax[g]);
  s_m[tid] = m;
  __syncthreads();
  for (int off = SAMPLE_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) s_m[tid] = fmax(s_m[tid], s_m[tid + off]);
    __syncthreads();
  }
  if (tid == 0) {
    *amax = s_m[0];
    *info = s_m[0] > 0.0 ? 0 : 1;
  }
}

// Inclusive scan of one value per thread over the workgroup; `total` is the workgroup's sum.  All threads call it.
__device__ __forceinline__ uint64_t sample_block_scan(uint64_t v, uint64_t* s_w, uint64_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) {
    if (w < wave) v += s_w[w];
    total += s_w[w];
  }
  __syncthreads();  // s_w is free again
  return v;
}

// FINAL: C of the workgroup's faces on top of its offset; otherwise the workgroup's sum of weights.
template <bool FINAL>
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_scan_kernel(const double* __restrict__ area, int64_t F,
                                                                   const double* __restrict__ amax,
                                                                   uint64_t* __restrict__ bsum,
                                                                   uint64_t* __restrict__ cdf) {
  __shared__ uint64_t s_w[SAMPLE_WAVES];
  const int tid = threadIdx.x;
  const double A = *amax;
  uint64_t carry = FINAL ? bsum[blockIdx.x] : 0;
#pragma unroll
  for (int u = 0; u < SAMPLE_PER; ++u) {
    const int64_t f = (int64_t)blockIdx.x * SAMPLE_FACES + u * SAMPLE_BLOCK + tid;
    const uint64_t w = f < F ? cdx::sample_weight(area[f], A) : 0;
    uint64_t total;
    const uint64_t c = sample_block_scan(w, s_w, total);
    if (FINAL && f < F) cdf[f] = carry + c;
    carry += total;
  }
  if (!FINAL && tid == 0) bsum[blockIdx.x] = carry;
}

// sums [G] → their exclusive prefix sums, in place.  One workgroup: each thread owns a contiguous segment.
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_offsets_kernel(uint64_t* __restrict__ sums, int64_t G) {
  __shared__ uint64_t s[SAMPLE_BLOCK];
  const int tid = threadIdx.x;
  const int64_t per = (G + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK;
  const int64_t lo = min((int64_t)tid * per, G), hi = min(lo + per, G);
  uint64_t sum = 0;
  for (int64_t q = lo; q < hi; ++q) sum += sums[q];
  s[tid] = sum;
  __syncthreads();
  for (int off = 1; off < SAMPLE_BLOCK; off <<= 1) {
    const uint64_t v = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  uint64_t base = s[tid] - sum;
  for (int64_t q = lo; q < hi; ++q) {
    const uint64_t w = sums[q];
    sums[q] = base;
    base += w;
  }
}

// One output of `W` doubles a sample, through LDS: lane l of the tile holds row l, and stores doubles l, l + BLOCK, …
// of the tile's W·BLOCK.  All threads of the workgroup call it.
template <int W, int BLOCK>
__device__ __forceinline__ void sample_store(double* __restrict__ out, int64_t tile_row, int64_t K, const double* v,
                                             double* s_out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < W; ++k) s_out[W * tid + k] = v[k];
  __syncthreads();
  const int64_t base = tile_row * W, end = K * W;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const int64_t o = base + k * BLOCK + tid;
    if (o < end) out[o] = s_out[k * BLOCK + tid];
  }
  __syncthreads();
}

template <typename T, int CAP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void sample_draw_kernel(const T* __restrict__ faces, int64_t F,
                                                            const uint64_t* __restrict__ cdf, int stride, uint64_t seed,
                                                            uint64_t first, int64_t K, double* __restrict__ points,
                                                            int64_t* __restrict__ face, double* __restrict__ bary,
                                                            double* __restrict__ normal) {
  __shared__ uint64_t s_tab[CAP];
  __shared__ double s_out[3 * BLOCK];
  const int tid = threadIdx.x;
  const int NS = (int)((F + stride - 1) / stride);  // ≤ CAP, the launcher's choice of stride
  for (int j = tid; j < NS; j += BLOCK) s_tab[j] = cdf[min((int64_t)(j + 1) * stride, F) - 1];
  __syncthreads();
  const uint64_t total = s_tab[NS - 1];
  const int64_t tiles = (K + BLOCK - 1) / BLOCK;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row = tile * BLOCK + tid;
    uint64_t t;
    double uv[2], p[3], n[3];
    cdx::sample_uniforms(seed, first + (uint64_t)row, total, t, uv[0], uv[1]);
    int64_t f = -1;
    if (total != 0 && row < K) {  // t < total = C[F − 1]: the searches below always find an entry
      f = cdx::sample_upper(s_tab, 0, NS, t);
      if (stride > 1 && f < NS) {
        const int64_t lo = f * stride;
        f = cdx::sample_upper(cdf, lo, min(lo + stride, F), t);
      }
      if (f >= F) f = -1;  // only a table that cdx_sample_prepare did not write: no face is read out of bounds
    }
    if (f >= 0) {
      const cdx::SampleFace s = cdx::sample_face(faces + 9 * f);
      cdx::sample_point(s, uv[0], uv[1], p);
      if (normal) cdx::sample_normal(s, n);
    } else {
      const double nan = __builtin_nan("");
      uv[0] = uv[1] = p[0] = p[1] = p[2] = n[0] = n[1] = n[2] = nan;
    }
    if (face && row < K) face[row] = f;
    if (points) sample_store<3, BLOCK>(points, tile * BLOCK, K, p, s_out);
    if (bary) sample_store<2, BLOCK>(bary, tile * BLOCK, K, uv, s_out);
    if (normal) sample_store<3, BLOCK>(normal, tile * BLOCK, K, n, s_out);
  }
}

// Workspace of prepare: area [F], the workgroups' maxima [G], their sums then offsets [G], A [1], each on 256 bytes.
struct SampleLayout {
  int64_t G;
  size_t area, bmax, bsum, amax, bytes;
};

SampleLayout sample_layout(int64_t F) {
  SampleLayout l;
  l.G = (F + SAMPLE_FACES - 1) / SAMPLE_FACES;
  l.area = 0;
  l.bmax = l.area + (size_t)round_up(F * (int64_t)sizeof(double), 256);
  l.bsum = l.bmax + (size_t)round_up(l.G * (int64_t)sizeof(double), 256);
  l.amax = l.bsum + (size_t)round_up(l.G * (int64_t)sizeof(uint64_t), 256);
  l.bytes = l.amax + 256;
  return l;
}

bool sample_shape_ok(int64_t F) { return F >= 1 && F <= SAMPLE_MAX_FACES; }

// 0: bad mode, or mode 1 beyond its capacity.  Automatic is mode 2 at every F: at the table path's capacity the two
// draw 10⁷ samples in the same time (0.207 against 0.201–0.215 ms), and mode 2 leaves its CU to six more workgroups
// (DESIGN.md §5h).  Up to SAMPLE_SPLIT_CAP faces its splitters are the whole table; beyond, it finishes in global memory.
int sample_path(int64_t F, int32_t mode) {
  if (mode == 0) return 2;
  if (mode == 1) return F <= SAMPLE_TABLE_CAP ? 1 : 0;
  return mode == 2 ? 2 : 0;
}

template <typename T, int CAP, int BLOCK>
void draw_launch(const void* faces, int64_t F, const uint64_t* cdf, uint64_t seed, uint64_t first, int64_t K,
                 int per_cu, double* points, int64_t* face, double* bary, double* normal, hipStream_t s) {
  int stride = 1;
  while ((F + stride - 1) / stride > CAP) stride <<= 1;
  const int64_t tiles = (K + BLOCK - 1) / BLOCK;
  const unsigned grid = (unsigned)std::min<int64_t>(tiles, (int64_t)SAMPLE_CUS * per_cu);
  hipLaunchKernelGGL((sample_draw_kernel<T, CAP, BLOCK>), dim3(grid), dim3(BLOCK), 0, s, static_cast<const T*>(faces),
                     F, cdf, stride, seed, first, K, points, face, bary, normal);
}

template <typename T>
void draw_dispatch(int path, const void* faces, int64_t F, const uint64_t* cdf, uint64_t seed, uint64_t first,
                   int64_t K, double* points, int64_t* face, double* bary, double* normal, hipStream_t s) {
  if (path == 1)
    draw_launch<T, SAMPLE_TABLE_CAP, SAMPLE_TABLE_BLOCK>(faces, F, cdf, seed, first, K, 1, points, face, bary, normal,
                                                         s);
  else
    draw_launch<T, SAMPLE_SPLIT_CAP, SAMPLE_SPLIT_BLOCK>(faces, F, cdf, seed, first, K, 7, points, face, bary, normal,
                                                         s);
}

template <typename T>
void prepare_launch(const void* faces, int64_t F, void* ws, uint64_t* cdf, int32_t* info, hipStream_t s) {
  const SampleLayout l = sample_layout(F);
  char* w = static_cast<char*>(ws);
  double* area = reinterpret_cast<double*>(w + l.area);
  double* bmax = reinterpret_cast<double*>(w + l.bmax);
  uint64_t* bsum = reinterpret_cast<uint64_t*>(w + l.bsum);
  double* amax = reinterpret_cast<double*>(w + l.amax);
  const dim3 grid((unsigned)l.G), block(SAMPLE_BLOCK);
  hipLaunchKernelGGL(sample_area_kernel<T>, grid, block, 0, s, static_cast<const T*>(faces), F, area, bmax);
  hipLaunchKernelGGL(sample_max_kernel, dim3(1), block, 0, s, bmax, l.G, amax, info);
  hipLaunchKernelGGL(sample_scan_kernel<false>, grid, block, 0, s, area, F, amax, bsum, cdf);
  hipLaunchKernelGGL(sample_offsets_kernel, dim3(1), block, 0, s, bsum, l.G);
  hipLaunchKernelGGL(sample_scan_kernel<true>, grid, block, 0, s, area, F, amax, bsum, cdf);
}

}  // namespace

extern "C" {

int64_t cdx_sample_scan_faces(void) { return SAMPLE_FACES; }

int64_t cdx_sample_table_capacity(void) { return SAMPLE_TABLE_CAP; }

size_t cdx_sample_prepare_workspace(int64_t F) { return sample_shape_ok(F) ? sample_layout(F).bytes : 0; }

int cdx_sample_prepare(const void* faces, int32_t dtype, int64_t F, void* workspace, uint64_t* cdf, int32_t* info,
                       cdx_stream_t stream) {
  if (!faces || !workspace || !cdf || !info || !sample_shape_ok(F)) return CDX_EINVAL;
  if (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == CDX_DTYPE_F32) prepare_launch<float>(faces, F, workspace, cdf, info, s);
  else prepare_launch<double>(faces, F, workspace, cdf, info, s);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_sample_draw(const void* faces, int32_t dtype, int64_t F, const uint64_t* cdf, uint64_t seed, uint64_t first,
                    int64_t K, int32_t mode, double* points, int64_t* face, double* bary, double* normal,
                    cdx_stream_t stream) {
  if (!faces || !cdf || !sample_shape_ok(F) || K < 0) return CDX_EINVAL;
  if (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) return CDX_EINVAL;
  const int path = sample_path(F, mode);
  if (path == 0) return CDX_EINVAL;
  if (K == 0 || (!points && !face && !bary && !normal)) return CDX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == CDX_DTYPE_F32) draw_dispatch<float>(path, faces, F, cdf, seed, first, K, points, face, bary, normal, s);
  else draw_dispatch<double>(path, faces, F, cdf, seed, first, K, points, face, bary, normal, s);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
