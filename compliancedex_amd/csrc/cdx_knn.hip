// k-nearest-neighbour search and cloud normals for gfx950.  The rule is csrc/cdx_knn.h; both query paths below give
// its bits.
//
//   knn_scan_kernel    every cloud row against every query: the statement of the rule on the device and the path of
//                      small clouds.  One wave per query, KNN_QPB queries a workgroup.  The sorted list lives one pair
//                      per lane (lane l holds the l-th smallest so far; K ≤ 64 = one wave).  The cloud passes through
//                      LDS in tiles of KNN_TILE rows shared by the workgroup's waves; a step gives every lane one
//                      candidate, a ballot against the K-th pair keeps the few that enter, and each of those is
//                      inserted with one wave-wide shift on the data-parallel path (DPP wave_shr:1, no LDS).
//   knn_grid_kernel    the same wave and list, fed from a prepared uniform grid (cdx_knn_prepare): cells at Chebyshev
//                      distance r = 0, 1, … from the query's cell, a column of cells along z being one contiguous run
//                      of the cell-ordered rows, until cdx::knn_ring_bound(r) is strictly above the K-th pair or
//                      above max_d2.
//   cdx_knn_prepare    bounding box of the finite rows (ordered-integer atomics), grid shape (one lane), cell keys and
//                      per-slab extrema, hipcub radix sort of (cell, row), rows gathered in cell order, cell starts by
//                      binary search, running extrema.  Launches on the caller's stream, no host synchronisation.
//   knn_normals_kernel one lane per row: two passes over its list (mean, covariance), Jacobi in registers.
// Nothing waits on another workgroup; every loop is bounded by a launch argument or a constant.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "cdx_knn.h"

namespace {

constexpr int KNN_BLOCK = 256;
constexpr int KNN_QPB = KNN_BLOCK / 64;  // queries per workgroup, one per wave
constexpr int KNN_TILE = 1024;           // cloud rows per LDS tile: 24 KiB of float64 coordinates
constexpr int KNN_NO_INDEX = 0x7fffffff;
// automatic mode with a prepared grid: the scan up to this many cloud rows.  Measured: the two queries tie
// at 1024 rows and the walk is 1.45× faster at 4096.
constexpr int64_t KNN_AUTO_ROWS = 1024;
constexpr int DPP_WAVE_SHR1 = 0x138;     // lane l reads lane l − 1; lane 0 keeps `old`

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- the list -----------------------------------------------------------------------------------------------------

__device__ __forceinline__ double knn_readlane(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}

__device__ __forceinline__ int knn_shr1(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, DPP_WAVE_SHR1, 0xf, 0xf, false);
}

// Every lane offers one candidate (cd, ci) (a NaN cd offers nothing); (ld, li) is this lane's pair of the sorted
// list.  All 64 lanes must be active.  At most 64 insertions.
__device__ __forceinline__ void knn_offer(double cd, int ci, double& ld, int& li, int K, double max_d2) {
  double kd = knn_readlane(ld, K - 1);
  int ki = __builtin_amdgcn_readlane(li, K - 1);
  unsigned long long mask = __ballot(!(cd > max_d2) && cdx::knn_before(cd, ci, kd, ki));
  while (mask) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
    mask &= mask - 1;
    const double bd = knn_readlane(cd, src);
    const int bi = __builtin_amdgcn_readlane(ci, src);
    if (!cdx::knn_before(bd, bi, kd, ki)) continue;  // the K-th pair moved up since the ballot
    const bool stay = cdx::knn_before(ld, li, bd, bi);
    const int pstay = knn_shr1(1, stay ? 1 : 0);
    const int plo = knn_shr1(0, __double2loint(ld)), phi = knn_shr1(0, __double2hiint(ld)), pi = knn_shr1(0, li);
    if (!stay) {
      ld = pstay ? bd : __hiloint2double(phi, plo);
      li = pstay ? bi : pi;
    }
    kd = knn_readlane(ld, K - 1);
    ki = __builtin_amdgcn_readlane(li, K - 1);
  }
}

__device__ __forceinline__ void knn_write(int64_t m, int lane, int K, double ld, int li, int64_t* __restrict__ idx,
                                          double* __restrict__ d2, int32_t* __restrict__ count) {
  const bool found = lane < K && li != KNN_NO_INDEX;
  const unsigned long long got = __ballot(found);
  if (lane < K) {
    idx[m * K + lane] = found ? (int64_t)li : (int64_t)-1;
    if (d2) d2[m * K + lane] = found ? ld : (double)INFINITY;
  }
  if (count && lane == 0) count[m] = __popcll(got);
}

template <typename T>
__global__ __launch_bounds__(KNN_BLOCK) void knn_scan_kernel(const T* __restrict__ X, int P, const T* __restrict__ Q,
                                                             int64_t M, int K, double max_d2,
                                                             int64_t* __restrict__ idx, double* __restrict__ d2,
                                                             int32_t* __restrict__ count) {
  __shared__ double sx[KNN_TILE], sy[KNN_TILE], sz[KNN_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = (int64_t)blockIdx.x * KNN_QPB + wave;
  const bool valid = m < M;
  const int64_t mq = valid ? m : 0;
  const double qx = (double)Q[3 * mq], qy = (double)Q[3 * mq + 1], qz = (double)Q[3 * mq + 2];
  const bool active = valid && cdx::knn_finite3(qx, qy, qz);
  double ld = (double)INFINITY;
  int li = KNN_NO_INDEX;
  const double nan = __builtin_nan("");
  for (int tile = 0; tile < P; tile += KNN_TILE) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < KNN_TILE / KNN_BLOCK; ++u) {
      const int jj = u * KNN_BLOCK + tid;
      const int64_t j = (int64_t)tile + jj;
      double x = nan, y = nan, z = nan;
      if (j < P) {
        x = (double)X[3 * j];
        y = (double)X[3 * j + 1];
        z = (double)X[3 * j + 2];
        if (!cdx::knn_finite3(x, y, z)) x = nan;  // never a neighbour: its d2 is NaN
      }
      sx[jj] = x;
      sy[jj] = y;
      sz[jj] = z;
    }
    __syncthreads();
    if (active) {
      const int rows = P - tile < KNN_TILE ? P - tile : KNN_TILE;
      for (int s = 0; s < rows; s += 64) {
        const int jj = s + lane;
        const double cd = cdx::fps_sqdist(sx[jj], sy[jj], sz[jj], qx, qy, qz);
        knn_offer(cd, tile + jj, ld, li, K, max_d2);
      }
    }
  }
  if (valid) knn_write(m, lane, K, ld, li, idx, d2, count);
}

// ---- the grid -----------------------------------------------------------------------------------------------------

// Caller-owned bytes of a prepared grid, every part on 256 bytes.
struct GridLayout {
  int n0;
  int64_t cells;  // n0³: cell ids 0 … cells−1, the key of a non-finite row is `cells`
  int bits;       // of the sort key
  size_t info, box, slab_lo, slab_hi, below, above, start, order, xyz, keys, vals, tmp, tmp_bytes, bytes;
};

// Everything but the sort's temporary storage, which comes last: all that a query reads.
bool grid_parts(int64_t P, GridLayout& l) {
  if (P < 1 || P >= ((int64_t)1 << 31) - KNN_TILE) return false;
  l.n0 = cdx::knn_grid_n0(P);
  l.cells = (int64_t)l.n0 * l.n0 * l.n0;
  l.bits = 1;
  while (((int64_t)1 << l.bits) <= l.cells) ++l.bits;
  size_t off = 0;
  l.info = off; off = align256(off + sizeof(cdx::KnnGrid));
  l.box = off; off = align256(off + 6 * sizeof(unsigned long long));
  l.slab_lo = off; off = align256(off + 3 * CDX_KNN_MAX_DIM * sizeof(unsigned long long));
  l.slab_hi = off; off = align256(off + 3 * CDX_KNN_MAX_DIM * sizeof(unsigned long long));
  l.below = off; off = align256(off + 3 * CDX_KNN_MAX_DIM * sizeof(double));
  l.above = off; off = align256(off + 3 * CDX_KNN_MAX_DIM * sizeof(double));
  l.start = off; off = align256(off + (size_t)(l.cells + 1) * sizeof(int));
  l.order = off; off = align256(off + (size_t)P * sizeof(int));
  l.xyz = off; off = align256(off + (size_t)P * 3 * sizeof(double));
  l.keys = off; off = align256(off + (size_t)P * 2 * sizeof(unsigned));
  l.vals = off; off = align256(off + (size_t)P * sizeof(int));
  l.tmp = off;
  l.tmp_bytes = 0;
  l.bytes = off;
  return true;
}

// The whole buffer, with hipcub's size query: prepare and cdx_knn_grid_bytes only.
bool grid_layout(int64_t P, GridLayout& l) {
  if (!grid_parts(P, l)) return false;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, l.tmp_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (int*)nullptr,
                                         (int*)nullptr, (int)P, 0, l.bits, (hipStream_t) nullptr) != hipSuccess)
    return false;
  l.bytes = l.tmp + align256(l.tmp_bytes);
  return true;
}

// float64 ↔ an unsigned integer of the same order, for atomicMin / atomicMax.
__device__ __forceinline__ unsigned long long knn_enc(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double knn_dec(unsigned long long u) {
  return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}
__device__ __forceinline__ void knn_amin(unsigned long long* p, unsigned long long v) {
  if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, v);
}
__device__ __forceinline__ void knn_amax(unsigned long long* p, unsigned long long v) {
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_grid_init_kernel(unsigned long long* box, unsigned long long* slab_lo,
                                                                  unsigned long long* slab_hi) {
  const int t = threadIdx.x;
  if (t < 3) box[t] = ~0ull;
  else if (t < 6) box[t] = 0ull;
  for (int i = t; i < 3 * CDX_KNN_MAX_DIM; i += KNN_BLOCK) {
    slab_lo[i] = ~0ull;
    slab_hi[i] = 0ull;
  }
}

template <typename T>
__global__ __launch_bounds__(KNN_BLOCK) void knn_grid_box_kernel(const T* __restrict__ X, int P,
                                                                 unsigned long long* box) {
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
  const int64_t stride = (int64_t)gridDim.x * KNN_BLOCK;
  for (int64_t j = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x; j < P; j += stride) {
    const double x = (double)X[3 * j], y = (double)X[3 * j + 1], z = (double)X[3 * j + 2];
    if (!cdx::knn_finite3(x, y, z)) continue;
    const unsigned long long e[3] = {knn_enc(x), knn_enc(y), knn_enc(z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = e[a] < lo[a] ? e[a] : lo[a];
      hi[a] = e[a] > hi[a] ? e[a] : hi[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    knn_amin(&box[a], lo[a]);
    knn_amax(&box[3 + a], hi[a]);
  }
}

__global__ void knn_grid_shape_kernel(const unsigned long long* box, int n0, cdx::KnnGrid* info) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  cdx::KnnGrid g;
  const bool any = box[0] <= box[3];  // a finite row was seen
  double ext = 0.0, hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = any ? knn_dec(box[a]) : 0.0;
    hi[a] = any ? knn_dec(box[3 + a]) : 0.0;
    const double e = hi[a] - g.lo[a];
    ext = e > ext ? e : ext;
  }
  g.inv = cdx::knn_grid_inv(ext, n0);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int n = cdx::knn_cell_raw(hi[a], g.lo[a], g.inv) + 1;
    g.n[a] = n < n0 ? n : n0;
  }
  g.pad = 0;
  *info = g;
}

template <typename T>
__global__ __launch_bounds__(KNN_BLOCK) void knn_grid_keys_kernel(const T* __restrict__ X, int P,
                                                                  const cdx::KnnGrid* __restrict__ info,
                                                                  unsigned none_key, unsigned* __restrict__ keys,
                                                                  int* __restrict__ vals, unsigned long long* slab_lo,
                                                                  unsigned long long* slab_hi) {
  const int64_t j = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (j >= P) return;
  const cdx::KnnGrid g = *info;
  const double p[3] = {(double)X[3 * j], (double)X[3 * j + 1], (double)X[3 * j + 2]};
  unsigned key = none_key;
  if (cdx::knn_finite3(p[0], p[1], p[2])) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = cdx::knn_cell(p[a], g.lo[a], g.inv, g.n[a]);
      const unsigned long long e = knn_enc(p[a]);
      knn_amin(&slab_lo[a * CDX_KNN_MAX_DIM + c[a]], e);
      knn_amax(&slab_hi[a * CDX_KNN_MAX_DIM + c[a]], e);
    }
    key = (unsigned)((c[0] * g.n[1] + c[1]) * g.n[2] + c[2]);
  }
  keys[j] = key;
  vals[j] = (int)j;
}

// Rows in cell order, and the first sorted position of every cell id 0 … cells (lower bound on the sorted keys).
template <typename T>
__global__ __launch_bounds__(KNN_BLOCK) void knn_grid_fill_kernel(const T* __restrict__ X, int P, int64_t cells,
                                                                  const unsigned* __restrict__ skeys,
                                                                  const int* __restrict__ order,
                                                                  double* __restrict__ xyz, int* __restrict__ start) {
  const int64_t t = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (t < P) {
    int j = order[t];
    j = j < 0 ? 0 : (j >= P ? P - 1 : j);
    xyz[3 * t] = (double)X[3 * (int64_t)j];
    xyz[3 * t + 1] = (double)X[3 * (int64_t)j + 1];
    xyz[3 * t + 2] = (double)X[3 * (int64_t)j + 2];
  }
  if (t <= cells) {
    int lo = 0, hi = P;
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const int mid = lo + (hi - lo) / 2;
      if (skeys[mid] < (unsigned)t) lo = mid + 1;
      else hi = mid;
    }
    start[t] = lo;
  }
}

__global__ void knn_grid_slabs_kernel(const unsigned long long* slab_lo, const unsigned long long* slab_hi,
                                      double* below, double* above) {
  const int a = threadIdx.x;
  if (a >= 3 || blockIdx.x != 0) return;
  double run = -(double)INFINITY;
  for (int c = 0; c < CDX_KNN_MAX_DIM; ++c) {
    const unsigned long long u = slab_hi[a * CDX_KNN_MAX_DIM + c];
    const double v = u == 0ull ? -(double)INFINITY : knn_dec(u);
    run = v > run ? v : run;
    below[a * CDX_KNN_MAX_DIM + c] = run;
  }
  run = (double)INFINITY;
  for (int c = CDX_KNN_MAX_DIM - 1; c >= 0; --c) {
    const unsigned long long u = slab_lo[a * CDX_KNN_MAX_DIM + c];
    const double v = u == ~0ull ? (double)INFINITY : knn_dec(u);
    run = v < run ? v : run;
    above[a * CDX_KNN_MAX_DIM + c] = run;
  }
}

// The sorted rows [s, e) against the wave's query.
__device__ __forceinline__ void knn_run(int s, int e, int P, int lane, const double* __restrict__ xyz,
                                        const int* __restrict__ order, double qx, double qy, double qz, double& ld,
                                        int& li, int K, double max_d2) {
  s = s < 0 ? 0 : s;
  e = e > P ? P : e;
  for (int i = s; i < e; i += 64) {
    const int t = i + lane;
    double cd = __builtin_nan("");
    int ci = KNN_NO_INDEX;
    if (t < e) {
      cd = cdx::fps_sqdist(xyz[3 * (int64_t)t], xyz[3 * (int64_t)t + 1], xyz[3 * (int64_t)t + 2], qx, qy, qz);
      ci = order[t];
    }
    knn_offer(cd, ci, ld, li, K, max_d2);
  }
}

template <typename T>
__global__ __launch_bounds__(KNN_BLOCK) void knn_grid_kernel(int P, int cells, const cdx::KnnGrid* __restrict__ info,
                                                             const double* __restrict__ below,
                                                             const double* __restrict__ above,
                                                             const int* __restrict__ start,
                                                             const int* __restrict__ order,
                                                             const double* __restrict__ xyz, const T* __restrict__ Q,
                                                             int64_t M, int K, double max_d2,
                                                             int64_t* __restrict__ idx, double* __restrict__ d2,
                                                             int32_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * KNN_QPB + (threadIdx.x >> 6);
  if (m >= M) return;  // the whole wave
  const double q[3] = {(double)Q[3 * m], (double)Q[3 * m + 1], (double)Q[3 * m + 2]};
  double ld = (double)INFINITY;
  int li = KNN_NO_INDEX;
  if (cdx::knn_finite3(q[0], q[1], q[2])) {
    cdx::KnnGrid g = *info;
#pragma unroll
    for (int a = 0; a < 3; ++a) g.n[a] = g.n[a] < 1 ? 1 : (g.n[a] > CDX_KNN_MAX_DIM ? CDX_KNN_MAX_DIM : g.n[a]);
    int cq[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) cq[a] = cdx::knn_cell(q[a], g.lo[a], g.inv, g.n[a]);
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    auto first = [&](int cell) { return start[cell < cells ? cell : cells]; };  // start holds cells + 1 entries
    const int rings = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
    for (int r = 0; r < rings; ++r) {
      const int z0 = cq[2] - r < 0 ? 0 : cq[2] - r, z1 = cq[2] + r >= nz ? nz - 1 : cq[2] + r;
      const int x0 = cq[0] - r < 0 ? 0 : cq[0] - r, x1 = cq[0] + r >= nx ? nx - 1 : cq[0] + r;
      const int y0 = cq[1] - r < 0 ? 0 : cq[1] - r, y1 = cq[1] + r >= ny ? ny - 1 : cq[1] + r;
      for (int x = x0; x <= x1; ++x) {
        for (int y = y0; y <= y1; ++y) {
          const int col = (x * ny + y) * nz;
          const bool border = x == cq[0] - r || x == cq[0] + r || y == cq[1] - r || y == cq[1] + r;
          if (border) {  // the whole column of the ring's cube
            knn_run(first(col + z0), first(col + z1 + 1), P, lane, xyz, order, q[0], q[1], q[2], ld, li, K, max_d2);
          } else {  // its two caps
            if (cq[2] - r >= 0)
              knn_run(first(col + z0), first(col + z0 + 1), P, lane, xyz, order, q[0], q[1], q[2], ld, li, K, max_d2);
            if (cq[2] + r < nz)
              knn_run(first(col + z1), first(col + z1 + 1), P, lane, xyz, order, q[0], q[1], q[2], ld, li, K, max_d2);
          }
        }
      }
      bool none;
      const double bound = cdx::knn_ring_bound(g, below, above, q, cq, r, &none);
      // every row out there has d2 ≥ bound: none can enter the list, or none is within the radius
      if (none || bound > knn_readlane(ld, K - 1) || bound > max_d2) break;
    }
  }
  knn_write(m, lane, K, ld, li, idx, d2, count);
}

// ---- normals ------------------------------------------------------------------------------------------------------

struct KnnEye {
  double p[3];
  int has;
};

template <typename T>
__global__ __launch_bounds__(KNN_BLOCK) void knn_normals_kernel(const T* __restrict__ X, int P,
                                                                const int64_t* __restrict__ idx,
                                                                const int32_t* __restrict__ count, int K, KnnEye eye,
                                                                double* __restrict__ normals,
                                                                double* __restrict__ eigenvalues) {
  const int64_t row = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (row >= P) return;
  int c = count[row];
  c = c < 0 ? 0 : (c > K ? K : c);
  const int64_t* list = idx + row * K;
  cdx::KnnMoments k;
  cdx::knn_moments_init(k);
  for (int t = 0; t < c; ++t) {
    const int64_t j = list[t];
    if (j < 0 || j >= P) {  // not a list of cdx_knn: it ends here
      c = t;
      break;
    }
    cdx::knn_moments_sum(k, (double)X[3 * j], (double)X[3 * j + 1], (double)X[3 * j + 2]);
  }
  if (c > 0) cdx::knn_moments_mean(k, c);
  for (int t = 0; t < c; ++t) {
    const int64_t j = list[t];
    cdx::knn_moments_cov(k, (double)X[3 * j], (double)X[3 * j + 1], (double)X[3 * j + 2]);
  }
  const double p[3] = {(double)X[3 * row], (double)X[3 * row + 1], (double)X[3 * row + 2]};
  double n[3], w[3];
  cdx::knn_normal_finish(k, c, p, eye.has != 0, eye.p, n, w, nullptr);
  normals[3 * row] = n[0];
  normals[3 * row + 1] = n[1];
  normals[3 * row + 2] = n[2];
  if (eigenvalues) {
    eigenvalues[3 * row] = w[0];
    eigenvalues[3 * row + 1] = w[1];
    eigenvalues[3 * row + 2] = w[2];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------

template <typename T>
int prepare_launch(const void* Xv, int64_t P, void* grid, hipStream_t s) {
  GridLayout l;
  if (!grid_layout(P, l)) return CDX_EINVAL;
  const T* X = static_cast<const T*>(Xv);
  char* b = static_cast<char*>(grid);
  cdx::KnnGrid* info = reinterpret_cast<cdx::KnnGrid*>(b + l.info);
  unsigned long long* box = reinterpret_cast<unsigned long long*>(b + l.box);
  unsigned long long* slab_lo = reinterpret_cast<unsigned long long*>(b + l.slab_lo);
  unsigned long long* slab_hi = reinterpret_cast<unsigned long long*>(b + l.slab_hi);
  unsigned* keys = reinterpret_cast<unsigned*>(b + l.keys);
  int* vals = reinterpret_cast<int*>(b + l.vals);
  int* order = reinterpret_cast<int*>(b + l.order);
  const unsigned rows = (unsigned)((P + KNN_BLOCK - 1) / KNN_BLOCK);
  hipLaunchKernelGGL(knn_grid_init_kernel, dim3(1), dim3(KNN_BLOCK), 0, s, box, slab_lo, slab_hi);
  hipLaunchKernelGGL(knn_grid_box_kernel<T>, dim3(rows < 1024u ? rows : 1024u), dim3(KNN_BLOCK), 0, s, X, (int)P, box);
  hipLaunchKernelGGL(knn_grid_shape_kernel, dim3(1), dim3(64), 0, s, box, l.n0, info);
  hipLaunchKernelGGL(knn_grid_keys_kernel<T>, dim3(rows), dim3(KNN_BLOCK), 0, s, X, (int)P, info, (unsigned)l.cells,
                     keys, vals, slab_lo, slab_hi);
  size_t tmp = l.tmp_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(b + l.tmp, tmp, keys, keys + P, vals, order, (int)P, 0, l.bits, s) !=
      hipSuccess)
    return CDX_ELAUNCH;
  const int64_t fill = (P > l.cells + 1 ? P : l.cells + 1);
  hipLaunchKernelGGL(knn_grid_fill_kernel<T>, dim3((unsigned)((fill + KNN_BLOCK - 1) / KNN_BLOCK)), dim3(KNN_BLOCK), 0,
                     s, X, (int)P, l.cells, keys + P, order, reinterpret_cast<double*>(b + l.xyz),
                     reinterpret_cast<int*>(b + l.start));
  hipLaunchKernelGGL(knn_grid_slabs_kernel, dim3(1), dim3(64), 0, s, slab_lo, slab_hi,
                     reinterpret_cast<double*>(b + l.below), reinterpret_cast<double*>(b + l.above));
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

template <typename T>
int knn_launch(const void* Xv, int64_t P, const void* grid, const void* Qv, int64_t M, int K, double max_d2, int path,
               int64_t* idx, double* d2, int32_t* count, hipStream_t s) {
  const T* X = static_cast<const T*>(Xv);
  const T* Q = Qv ? static_cast<const T*>(Qv) : X;
  const dim3 blocks((unsigned)((M + KNN_QPB - 1) / KNN_QPB));
  if (path == CDX_KNN_SCAN) {
    hipLaunchKernelGGL(knn_scan_kernel<T>, blocks, dim3(KNN_BLOCK), 0, s, X, (int)P, Q, M, K, max_d2, idx, d2, count);
  } else {
    GridLayout l;
    if (!grid_parts(P, l)) return CDX_EINVAL;
    const char* b = static_cast<const char*>(grid);
    hipLaunchKernelGGL(knn_grid_kernel<T>, blocks, dim3(KNN_BLOCK), 0, s, (int)P, (int)l.cells,
                       reinterpret_cast<const cdx::KnnGrid*>(b + l.info),
                       reinterpret_cast<const double*>(b + l.below), reinterpret_cast<const double*>(b + l.above),
                       reinterpret_cast<const int*>(b + l.start), reinterpret_cast<const int*>(b + l.order),
                       reinterpret_cast<const double*>(b + l.xyz), Q, M, K, max_d2, idx, d2, count);
  }
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

bool knn_dtype_ok(int32_t dtype) { return dtype == CDX_DTYPE_F32 || dtype == CDX_DTYPE_F64; }
// a row index plus a tile's width stays an int
bool knn_rows_ok(int64_t P) { return P >= 1 && P < ((int64_t)1 << 31) - KNN_TILE; }

}  // namespace

extern "C" {

int64_t cdx_knn_auto_rows(void) { return KNN_AUTO_ROWS; }

size_t cdx_knn_grid_bytes(int64_t P) {
  GridLayout l;
  return grid_layout(P, l) ? l.bytes : 0;
}

int cdx_knn_prepare(const void* X, int32_t dtype, int64_t P, void* grid, cdx_stream_t stream) {
  if (!X || !grid || !knn_rows_ok(P) || !knn_dtype_ok(dtype)) return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dtype == CDX_DTYPE_F32 ? prepare_launch<float>(X, P, grid, s) : prepare_launch<double>(X, P, grid, s);
}

size_t cdx_knn_workspace(int64_t P, int64_t M, int64_t K, int32_t mode) {
  if (!knn_rows_ok(P) || M < 0 || K < 1 || K > CDX_KNN_MAX_K || mode < CDX_KNN_AUTO || mode > CDX_KNN_GRID) return 0;
  return 256;  // both paths keep their lists in registers
}

int cdx_knn(const void* X, int32_t dtype, int64_t P, const void* grid, const void* Q, int64_t M, int64_t K,
            double max_d2, int32_t mode, void* workspace, int64_t* idx, double* d2, int32_t* count,
            cdx_stream_t stream) {
  (void)workspace;
  if (!X || !knn_rows_ok(P) || M < 0 || K < 1 || K > CDX_KNN_MAX_K || !knn_dtype_ok(dtype)) return CDX_EINVAL;
  if (mode < CDX_KNN_AUTO || mode > CDX_KNN_GRID || (mode == CDX_KNN_GRID && !grid)) return CDX_EINVAL;
  if (!Q) M = P;
  if (M > (int64_t)0x7fffffff * KNN_QPB || (M > 0 && !idx)) return CDX_EINVAL;
  if (M == 0) return CDX_OK;
  int path = mode;
  if (mode == CDX_KNN_AUTO) path = (grid && P > KNN_AUTO_ROWS) ? CDX_KNN_GRID : CDX_KNN_SCAN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dtype == CDX_DTYPE_F32
             ? knn_launch<float>(X, P, grid, Q, M, (int)K, max_d2, path, idx, d2, count, s)
             : knn_launch<double>(X, P, grid, Q, M, (int)K, max_d2, path, idx, d2, count, s);
}

int cdx_cloud_normals(const void* X, int32_t dtype, int64_t P, const int64_t* idx, const int32_t* count, int64_t K,
                      const double* eye, double* normals, double* eigenvalues, cdx_stream_t stream) {
  if (!X || !idx || !count || !normals || !knn_rows_ok(P) || K < 1 || K > CDX_KNN_MAX_K || !knn_dtype_ok(dtype))
    return CDX_EINVAL;
  KnnEye e;
  e.has = eye != nullptr;
  for (int a = 0; a < 3; ++a) e.p[a] = eye ? eye[a] : 0.0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 blocks((unsigned)((P + KNN_BLOCK - 1) / KNN_BLOCK));
  if (dtype == CDX_DTYPE_F32)
    hipLaunchKernelGGL(knn_normals_kernel<float>, blocks, dim3(KNN_BLOCK), 0, s, static_cast<const float*>(X), (int)P,
                       idx, count, (int)K, e, normals, eigenvalues);
  else
    hipLaunchKernelGGL(knn_normals_kernel<double>, blocks, dim3(KNN_BLOCK), 0, s, static_cast<const double*>(X),
                       (int)P, idx, count, (int)K, e, normals, eigenvalues);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
