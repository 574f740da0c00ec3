// GPIS field on a lattice and its surface cells for gfx950: get_visualization_data (gpis.py:113-125) and topcd
// (:127-150) without leaving the device.
//
//   cdx_gpis_field           the lattice's cells, `chunk` at a time: field_points_kernel writes their coordinates,
//                            the cdx_gpis_mean launch gives mean and normal in one pass (the mean alone:
//                            cdx::gpis_mean_only_launch), cdx::gpis_var_launch the whitened fp64 std with no stored V.
//                            All on the caller's stream: no sync, no allocation.
//   cdx_gpis_surface_count   surface_count_kernel: 256 consecutive cells (consecutive in k: coalesced reads) per
//                            workgroup, flag from the shared cell rule (cdx_field.h), per-wave __ballot popcounts, one
//                            count per workgroup; surface_scan_kernel: one-workgroup exclusive scan of the counts in
//                            place, and the total.
//   cdx_gpis_surface_place   surface_place_kernel: the flags again, rank = scan base + earlier waves + the wave
//                            prefix; cell index, point and gathered normal to row `rank`.
// No atomics: the rows are in C order of (i, j, k) by construction — numpy's boolean-mask order — and deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cdx_field.h"
#include "cdx_gpis_launch.h"

namespace {

constexpr int FIELD_BLOCK = 256;               // cells per workgroup of every kernel here
constexpr int FIELD_WAVES = FIELD_BLOCK / 64;
constexpr int64_t FIELD_WS_CAP = (int64_t)1 << 30;  // default chunk: workspace under 1 GiB

int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

int64_t cells_of(int steps) { return (int64_t)steps * steps * steps; }

bool field_gpis_ok(const cdx_gpis* g) {
  return g && g->X1 && g->alpha && g->N > 0 && g->N_pad >= g->N && g->N_pad % CDX_NPAD_ALIGN == 0 && g->kernel >= 0 &&
         g->kernel <= 2;
}

// Coordinates of n cells: cells[q], or start + q without a list.
__global__ __launch_bounds__(FIELD_BLOCK) void field_points_kernel(const double* __restrict__ ax,
                                                                   const double* __restrict__ ay,
                                                                   const double* __restrict__ az, int steps,
                                                                   const int64_t* __restrict__ cells, int64_t start,
                                                                   int64_t n, double* __restrict__ X) {
  const int64_t q = (int64_t)blockIdx.x * FIELD_BLOCK + threadIdx.x;
  if (q >= n) return;
  const int64_t c = cells ? cells[q] : start + q;
  if (c < 0 || c >= (int64_t)steps * steps * steps) {
    const double nan = __builtin_nan("");
    X[3 * q] = nan; X[3 * q + 1] = nan; X[3 * q + 2] = nan;
    return;
  }
  int i, j, k;
  cdx::field_cell(c, steps, i, j, k);
  X[3 * q] = ax[j];
  X[3 * q + 1] = ay[i];
  X[3 * q + 2] = az[k];
}

// Flag of this thread's cell, and the cell.
template <typename T>
__device__ __forceinline__ bool surface_flag(const T* __restrict__ mean, int steps, int flip_k, int64_t total,
                                             int64_t& c, int& i, int& j, int& k) {
  c = (int64_t)blockIdx.x * FIELD_BLOCK + threadIdx.x;
  i = j = k = 0;
  if (c >= total) return false;
  cdx::field_cell(c, steps, i, j, k);
  return cdx::field_surface_cell(mean, steps, i, j, k, flip_k);
}

template <typename T>
__global__ __launch_bounds__(FIELD_BLOCK) void surface_count_kernel(const T* __restrict__ mean, int steps, int flip_k,
                                                                    int64_t total, int64_t* __restrict__ counts) {
  __shared__ int wsum[FIELD_WAVES];
  int64_t c;
  int i, j, k;
  const bool f = surface_flag(mean, steps, flip_k, total, c, i, j, k);
  const unsigned long long b = __ballot(f);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < FIELD_WAVES; ++w) s += wsum[w];
    counts[blockIdx.x] = s;
  }
}

// counts [nb] → their exclusive prefix sums, in place; *total = Σ counts.  One workgroup: each thread owns a
// contiguous segment (its sum, a Hillis-Steele scan of the 256 sums in LDS, then the segment's prefixes).
__global__ __launch_bounds__(FIELD_BLOCK) void surface_scan_kernel(int64_t* __restrict__ counts, int64_t nb,
                                                                   int64_t* __restrict__ total) {
  __shared__ int64_t s[FIELD_BLOCK];
  const int tid = threadIdx.x;
  const int64_t per = (nb + FIELD_BLOCK - 1) / FIELD_BLOCK;
  const int64_t lo = min((int64_t)tid * per, nb), hi = min(lo + per, nb);
  int64_t sum = 0;
  for (int64_t q = lo; q < hi; ++q) sum += counts[q];
  s[tid] = sum;
  __syncthreads();
  for (int off = 1; off < FIELD_BLOCK; off <<= 1) {
    const int64_t v = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  int64_t base = s[tid] - sum;
  for (int64_t q = lo; q < hi; ++q) {
    const int64_t cnt = counts[q];
    counts[q] = base;
    base += cnt;
  }
  if (tid == FIELD_BLOCK - 1) *total = s[tid];
}

template <typename T>
__global__ __launch_bounds__(FIELD_BLOCK) void surface_place_kernel(const T* __restrict__ mean,
                                                                    const T* __restrict__ normal, int steps, int flip_k,
                                                                    int64_t total, const double* __restrict__ px,
                                                                    const double* __restrict__ py,
                                                                    const double* __restrict__ pz,
                                                                    const int64_t* __restrict__ offsets,
                                                                    int64_t capacity, int64_t* __restrict__ cells,
                                                                    double* __restrict__ points,
                                                                    T* __restrict__ normals) {
  __shared__ int wsum[FIELD_WAVES];
  int64_t c;
  int i, j, k;
  const bool f = surface_flag(mean, steps, flip_k, total, c, i, j, k);
  const unsigned long long b = __ballot(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  if (!f) return;
  int64_t rank = offsets[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += wsum[w];
  if (rank >= capacity) return;
  if (cells) cells[rank] = c;
  if (points) {
    points[3 * rank] = px[j];
    points[3 * rank + 1] = py[i];
    points[3 * rank + 2] = pz[k];
  }
  if (normals) {
    const int64_t src = cdx::field_src(steps, i, j, k, flip_k);
    normals[3 * rank] = normal[3 * src];
    normals[3 * rank + 1] = normal[3 * src + 1];
    normals[3 * rank + 2] = normal[3 * src + 2];
  }
}

// Bytes of one chunk of `m` cells: its coordinates, then the whitened pass's partial sums.
size_t chunk_x_bytes(int64_t m) { return (size_t)round_up(m * 3 * (int64_t)sizeof(double), 256); }

// The chunk a call uses: the caller's, or the default; never more than the lattice (rounded up to 128 for the default).
int64_t field_chunk(const cdx_gpis& g, int steps, int64_t chunk) {
  const int64_t total = cells_of(steps);
  if (chunk > 0) return std::min(chunk, total);
  // large chunks take one workgroup per (128 queries, 256-column stripe): 24 B of coordinates and one partial per
  // stripe for each cell, so the bound is linear; the loop only covers the roundings
  const int64_t per = 3 * (int64_t)sizeof(double) + (int64_t)(g.N_pad / CDX_NPAD_ALIGN) * (int64_t)sizeof(double);
  int64_t c = std::max<int64_t>(128, (FIELD_WS_CAP - 4096) / per / 128 * 128);
  while (c > 128 && chunk_x_bytes(c) + cdx::gpis_var_ws_bytes(g, c) > (size_t)FIELD_WS_CAP) c -= 128;
  return std::min(c, round_up(total, 128));
}

// Workspace of the whitened pass over chunks of m cells and the ragged last one (a small last chunk may take the
// split-K path, whose partials are larger than a full chunk's).
size_t field_var_bytes(const cdx_gpis& g, int steps, int64_t m) {
  const int64_t total = cells_of(steps), last = total % m;
  size_t b = cdx::gpis_var_ws_bytes(g, std::min(m, total));
  if (last) b = std::max(b, cdx::gpis_var_ws_bytes(g, last));
  return b;
}

template <typename T>
void count_launch(const void* mean, int steps, int flip_k, int64_t total, int64_t nb, int64_t* counts, int64_t* out,
                  hipStream_t s) {
  hipLaunchKernelGGL(surface_count_kernel<T>, dim3((unsigned)nb), dim3(FIELD_BLOCK), 0, s, static_cast<const T*>(mean),
                     steps, flip_k, total, counts);
  hipLaunchKernelGGL(surface_scan_kernel, dim3(1), dim3(FIELD_BLOCK), 0, s, counts, nb, out);
}

template <typename T>
void place_launch(const void* mean, const void* normal, int steps, int flip_k, int64_t total, int64_t nb,
                  const double* px, const double* py, const double* pz, const int64_t* offsets, int64_t capacity,
                  int64_t* cells, double* points, void* normals, hipStream_t s) {
  hipLaunchKernelGGL(surface_place_kernel<T>, dim3((unsigned)nb), dim3(FIELD_BLOCK), 0, s, static_cast<const T*>(mean),
                     static_cast<const T*>(normal), steps, flip_k, total, px, py, pz, offsets, capacity, cells, points,
                     static_cast<T*>(normals));
}

bool steps_ok(int32_t steps) { return steps >= 1 && steps <= CDX_FIELD_MAX_STEPS; }
bool dtype_ok(int32_t dtype) { return dtype == CDX_DTYPE_F32 || dtype == CDX_DTYPE_F64; }

}  // namespace

extern "C" {

size_t cdx_gpis_field_workspace(const cdx_gpis* g, int32_t steps, int64_t chunk) {
  if (!field_gpis_ok(g) || !steps_ok(steps) || chunk < 0) return 0;
  const int64_t m = field_chunk(*g, steps, chunk);
  return chunk_x_bytes(m) + field_var_bytes(*g, steps, m);
}

int cdx_gpis_field(const cdx_gpis* g, const double* ax, const double* ay, const double* az, int32_t steps,
                   int64_t chunk, double* mean, double* std_out, double* normal, void* workspace,
                   cdx_stream_t stream) {
  if (!field_gpis_ok(g)) return g && (g->kernel < 0 || g->kernel > 2) ? CDX_EKERNEL : CDX_EINVAL;
  if (!steps_ok(steps) || chunk < 0 || !ax || !ay || !az || !mean || !workspace) return CDX_EINVAL;
  if (std_out && !g->Linv_t) return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = cells_of(steps), m = field_chunk(*g, steps, chunk);
  double* X = static_cast<double*>(workspace);
  void* var_ws = static_cast<char*>(workspace) + chunk_x_bytes(m);
  for (int64_t c0 = 0; c0 < total; c0 += m) {
    const int64_t M = std::min(m, total - c0);
    hipLaunchKernelGGL(field_points_kernel, dim3((unsigned)((M + FIELD_BLOCK - 1) / FIELD_BLOCK)), dim3(FIELD_BLOCK), 0,
                       s, ax, ay, az, steps, (const int64_t*)nullptr, c0, M, X);
    int rc = normal ? cdx_gpis_mean(g, X, M, mean + c0, nullptr, normal + 3 * c0, stream)
                    : cdx::gpis_mean_only_launch(*g, X, M, mean + c0, s);
    if (rc) return rc;
    if (std_out) {
      rc = cdx::gpis_var_launch(*g, X, M, std_out + c0, nullptr, var_ws, s);
      if (rc) return rc;
    }
  }
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_gpis_field_points(const double* ax, const double* ay, const double* az, int32_t steps, const int64_t* cells,
                          int64_t n, double* X, cdx_stream_t stream) {
  if (!steps_ok(steps) || n < 0 || !ax || !ay || !az || (n > 0 && !X)) return CDX_EINVAL;
  if (!cells && n > cells_of(steps)) return CDX_EINVAL;
  if (n == 0) return CDX_OK;
  if ((n + FIELD_BLOCK - 1) / FIELD_BLOCK > 0x7fffffff) return CDX_EINVAL;
  hipLaunchKernelGGL(field_points_kernel, dim3((unsigned)((n + FIELD_BLOCK - 1) / FIELD_BLOCK)), dim3(FIELD_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ax, ay, az, steps, cells, (int64_t)0, n, X);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

size_t cdx_gpis_surface_workspace(int32_t steps) {
  if (!steps_ok(steps)) return 0;
  const int64_t nb = (cells_of(steps) + FIELD_BLOCK - 1) / FIELD_BLOCK;
  return (size_t)round_up(nb * (int64_t)sizeof(int64_t), 256);
}

int cdx_gpis_surface_count(const void* mean, int32_t dtype, int32_t steps, int32_t flip_k, void* workspace,
                           int64_t* total, cdx_stream_t stream) {
  if (!steps_ok(steps) || !dtype_ok(dtype) || !mean || !workspace || !total) return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (steps < 3)  // no interior cell
    return hipMemsetAsync(total, 0, sizeof(int64_t), s) == hipSuccess ? CDX_OK : CDX_ELAUNCH;
  const int64_t cells = cells_of(steps), nb = (cells + FIELD_BLOCK - 1) / FIELD_BLOCK;
  int64_t* counts = static_cast<int64_t*>(workspace);
  if (dtype == CDX_DTYPE_F32) count_launch<float>(mean, steps, flip_k ? 1 : 0, cells, nb, counts, total, s);
  else count_launch<double>(mean, steps, flip_k ? 1 : 0, cells, nb, counts, total, s);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_gpis_surface_place(const void* mean, const void* normal, int32_t dtype, int32_t steps, int32_t flip_k,
                           const double* px, const double* py, const double* pz, const void* workspace,
                           int64_t capacity, int64_t* cells, double* points, void* normals, cdx_stream_t stream) {
  if (!steps_ok(steps) || !dtype_ok(dtype) || !mean || !workspace || capacity < 0) return CDX_EINVAL;
  if ((points && (!px || !py || !pz)) || (normals && !normal)) return CDX_EINVAL;
  if (steps < 3 || capacity == 0 || (!cells && !points && !normals)) return CDX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = cells_of(steps), nb = (total + FIELD_BLOCK - 1) / FIELD_BLOCK;
  const int64_t* offsets = static_cast<const int64_t*>(workspace);
  if (dtype == CDX_DTYPE_F32)
    place_launch<float>(mean, normal, steps, flip_k ? 1 : 0, total, nb, px, py, pz, offsets, capacity, cells, points,
                        normals, s);
  else
    place_launch<double>(mean, normal, steps, flip_k ? 1 : 0, total, nb, px, py, pz, offsets, capacity, cells, points,
                         normals, s);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
