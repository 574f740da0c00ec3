// Iso-surface mesh of a lattice field for gfx950: GPIS.tomesh / surface_mesh, marching tetrahedra by the rule of
// cdx_mesh.h as two ordered stream compactions in the shape of cdx_gpis_surface_count / _place (cdx_field.hip).
//
//   cdx_gpis_mesh_count   mesh_count_kernel: 256 consecutive nodes (consecutive in k: coalesced reads) per workgroup;
//                         a thread reads its node and the seven nodes of its cube once, and from them counts the
//                         node's crossing edges (0 … 7 vertices) and the cube's triangles (0 … 12).  The counts are
//                         summed per wave from __ballots of their bits, one pair of counts per workgroup;
//                         mesh_scan_kernel: two workgroups, each the exclusive scan of one array of counts in place,
//                         and its total.
//   cdx_gpis_mesh_place   mesh_vertex_place_kernel: the counts again, rank = scan base + earlier waves + the wave
//                         prefix (the same ballots under a lane mask); the node's first vertex number into base[c],
//                         its vertices and keys to rows rank ….  mesh_face_place_kernel: the cube's triangles to rows
//                         rank …, each corner's vertex number = base[node] + the node's crossing edges below d,
//                         recounted from the mean.
//   cdx_gpis_mesh_refine_init / _step   mesh_refine_kernel: one thread per vertex, the bracket state and the vertex
//                         of cdx::mesh_refine_vertex; the GPIS mean between two steps is the caller's cdx_gpis_mean.
// No atomics: vertices are in ascending key order and faces in (cube, tetrahedron, triangle) order by construction.
// The loads are plain cached loads: the 2×2 node rows a workgroup touches are shared with its neighbours through L2.
#include <hip/hip_runtime.h>

#include "cdx_mesh.h"

namespace {

constexpr int MESH_BLOCK = 256;  // nodes per workgroup of every kernel here
constexpr int MESH_WAVES = MESH_BLOCK / 64;
constexpr int64_t MESH_INDEX_LIMIT = (int64_t)1 << 31;  // vertex numbers are int32

int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
int64_t nodes_of(int steps) { return (int64_t)steps * steps * steps; }
int64_t blocks_of(int steps) { return (nodes_of(steps) + MESH_BLOCK - 1) / MESH_BLOCK; }

// Workspace: vertex counts / offsets [nb], face counts / offsets [nb], the two totals, then base [steps³] int32.
size_t base_offset(int64_t nb) { return (size_t)round_up((2 * nb + 2) * (int64_t)sizeof(int64_t), 256); }

// This thread's node, its cube's corner bits and which of them exist; false past the lattice.
template <typename T>
__device__ __forceinline__ bool mesh_node(const T* __restrict__ mean, int steps, int64_t total, int64_t& c, int& i,
                                          int& j, int& k, int& exists, int& bits) {
  c = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  i = j = k = exists = bits = 0;
  if (c >= total) return false;
  cdx::field_cell(c, steps, i, j, k);
  exists = cdx::mesh_exists(steps, i, j, k);
  bits = cdx::mesh_corner_bits(mean, steps, i, j, k, exists);
  return true;
}

// Sum over the wave of a per-lane count below 2^NBITS, and the sum over the lanes before this one.
template <int NBITS>
__device__ __forceinline__ void wave_count(int n, int lane, int& before, int& all) {
  before = all = 0;
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int b = 0; b < NBITS; ++b) {
    const unsigned long long m = __ballot((n >> b) & 1);
    all += __popcll(m) << b;
    before += __popcll(m & lt) << b;
  }
}

template <typename T>
__global__ __launch_bounds__(MESH_BLOCK) void mesh_count_kernel(const T* __restrict__ mean, int steps, int64_t total,
                                                                int64_t nb, int64_t* __restrict__ counts) {
  __shared__ int wv[MESH_WAVES], wf[MESH_WAVES];
  int64_t c;
  int i, j, k, exists, bits;
  const bool ok = mesh_node(mean, steps, total, c, i, j, k, exists, bits);
  const int nv = ok ? cdx::mesh_popc(cdx::mesh_cross_mask(bits, exists)) : 0;
  const int nf = ok && exists == 0xff ? cdx::mesh_cube_count(bits) : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before, all_v, all_f;
  wave_count<3>(nv, lane, before, all_v);
  wave_count<4>(nf, lane, before, all_f);
  if (lane == 0) { wv[wave] = all_v; wf[wave] = all_f; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int sv = 0, sf = 0;
#pragma unroll
    for (int w = 0; w < MESH_WAVES; ++w) { sv += wv[w]; sf += wf[w]; }
    counts[blockIdx.x] = sv;
    counts[nb + blockIdx.x] = sf;
  }
}

// Workgroup b: counts[b·nb …] [nb] → their exclusive prefix sums, in place; totals[b] and keep[b] = their sum.  Each
// thread owns a contiguous segment (its sum, a Hillis-Steele scan of the 256 sums in LDS, then the segment's prefixes).
__global__ __launch_bounds__(MESH_BLOCK) void mesh_scan_kernel(int64_t* __restrict__ counts, int64_t nb,
                                                               int64_t* __restrict__ totals,
                                                               int64_t* __restrict__ keep) {
  __shared__ int64_t s[MESH_BLOCK];
  counts += (int64_t)blockIdx.x * nb;
  const int tid = threadIdx.x;
  const int64_t per = (nb + MESH_BLOCK - 1) / MESH_BLOCK;
  const int64_t lo = min((int64_t)tid * per, nb), hi = min(lo + per, nb);
  int64_t sum = 0;
  for (int64_t q = lo; q < hi; ++q) sum += counts[q];
  s[tid] = sum;
  __syncthreads();
  for (int off = 1; off < MESH_BLOCK; off <<= 1) {
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
  if (tid == MESH_BLOCK - 1) { totals[blockIdx.x] = s[tid]; keep[blockIdx.x] = s[tid]; }
}

template <typename T>
__global__ __launch_bounds__(MESH_BLOCK) void mesh_vertex_place_kernel(
    const T* __restrict__ mean, int steps, int64_t total, const double* __restrict__ px, const double* __restrict__ py,
    const double* __restrict__ pz, const int64_t* __restrict__ offsets, int32_t* __restrict__ base, int64_t vcap,
    double* __restrict__ vertices, int64_t* __restrict__ edges) {
  __shared__ int wsum[MESH_WAVES];
  int64_t c;
  int i, j, k, exists, bits;
  const bool ok = mesh_node(mean, steps, total, c, i, j, k, exists, bits);
  const int cross = ok ? cdx::mesh_cross_mask(bits, exists) : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before, all;
  wave_count<3>(cdx::mesh_popc(cross), lane, before, all);
  if (lane == 0) wsum[wave] = all;
  __syncthreads();
  if (!ok) return;
  int64_t rank = offsets[blockIdx.x] + before;
  for (int w = 0; w < wave; ++w) rank += wsum[w];
  base[c] = (int32_t)rank;  // (the caller has checked V < 2³¹)
  for (int d = 0; d < 7; ++d) {
    if (!((cross >> d) & 1)) continue;
    if (rank < vcap) {
      double v[3];
      cdx::mesh_vertex(mean, steps, px, py, pz, i, j, k, d, v);
      vertices[3 * rank] = v[0];
      vertices[3 * rank + 1] = v[1];
      vertices[3 * rank + 2] = v[2];
      if (edges) edges[rank] = 7 * c + d;
    }
    ++rank;
  }
}

template <typename T>
__global__ __launch_bounds__(MESH_BLOCK) void mesh_face_place_kernel(const T* __restrict__ mean, int steps,
                                                                     int64_t total,
                                                                     const double* __restrict__ px,
                                                                     const double* __restrict__ py,
                                                                     const double* __restrict__ pz,
                                                                     const int64_t* __restrict__ offsets,
                                                                     const int32_t* __restrict__ base, int64_t fcap,
                                                                     int32_t* __restrict__ faces) {
  __shared__ int wsum[MESH_WAVES];
  int64_t c;
  int i, j, k, exists, bits;
  const bool ok = mesh_node(mean, steps, total, c, i, j, k, exists, bits) && exists == 0xff;
  const int nf = ok ? cdx::mesh_cube_count(bits) : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before, all;
  wave_count<4>(nf, lane, before, all);
  if (lane == 0) wsum[wave] = all;
  __syncthreads();
  if (nf == 0) return;
  int64_t rank = offsets[blockIdx.x] + before;
  for (int w = 0; w < wave; ++w) rank += wsum[w];
  const int axes_sign = cdx::mesh_axes_sign(px[steps - 1] - px[0], py[steps - 1] - py[0], pz[steps - 1] - pz[0]);
  for (int tet = 0; tet < 6; ++tet) {
    uint32_t tris;
    const int nt = cdx::mesh_tet_faces(cdx::mesh_tet_bits(tet, bits), cdx::mesh_tet_sign(tet) * axes_sign, tris);
    for (int t = 0; t < nt; ++t, ++rank) {
      if (rank >= fcap) return;
      for (int v = 0; v < 3; ++v) {
        int m, d;
        cdx::mesh_tet_edge_node(tet, (tris >> (4 * (3 * t + v))) & 15u, m, d);
        const int ni = i + (m & 1), nj = j + ((m >> 1) & 1), nk = k + ((m >> 2) & 1);
        faces[3 * rank + v] =
            base[cdx::field_src(steps, ni, nj, nk, 0)] + cdx::mesh_cross_below(mean, steps, ni, nj, nk, d);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(MESH_BLOCK) void mesh_refine_kernel(const T* __restrict__ mean, const double* __restrict__ fv,
                                                                 int steps, const double* __restrict__ px,
                                                                 const double* __restrict__ py,
                                                                 const double* __restrict__ pz,
                                                                 const int64_t* __restrict__ edges, int64_t V,
                                                                 double* __restrict__ state,
                                                                 double* __restrict__ vertices) {
  const int64_t r = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (r < V) cdx::mesh_refine_vertex(mean, fv, steps, px, py, pz, edges, V, r, state, vertices);
}

template <typename T>
void count_launch(const void* mean, int steps, int64_t total, int64_t nb, int64_t* counts, int64_t* totals,
                  hipStream_t s) {
  hipLaunchKernelGGL(mesh_count_kernel<T>, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, s, static_cast<const T*>(mean),
                     steps, total, nb, counts);
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(2), dim3(MESH_BLOCK), 0, s, counts, nb, totals, counts + 2 * nb);
}

template <typename T>
void place_launch(const void* mean, int steps, int64_t total, int64_t nb, const double* px, const double* py,
                  const double* pz, const int64_t* offsets, int32_t* base, int64_t vcap, int64_t fcap,
                  double* vertices, int64_t* edges, int32_t* faces, hipStream_t s) {
  const T* m = static_cast<const T*>(mean);
  hipLaunchKernelGGL(mesh_vertex_place_kernel<T>, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, s, m, steps, total, px, py,
                     pz, offsets, base, vcap, vertices, edges);
  if (fcap > 0)
    hipLaunchKernelGGL(mesh_face_place_kernel<T>, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, s, m, steps, total, px, py, pz,
                       offsets + nb, base, fcap, faces);
}

bool steps_ok(int32_t steps) { return steps >= 1 && steps <= CDX_FIELD_MAX_STEPS; }
bool dtype_ok(int32_t dtype) { return dtype == CDX_DTYPE_F32 || dtype == CDX_DTYPE_F64; }

}  // namespace

extern "C" {

size_t cdx_gpis_mesh_workspace(int32_t steps) {
  if (!steps_ok(steps)) return 0;
  return base_offset(blocks_of(steps)) + (size_t)round_up(nodes_of(steps) * (int64_t)sizeof(int32_t), 256);
}

int cdx_gpis_mesh_count(const void* mean, int32_t dtype, int32_t steps, void* workspace, int64_t* totals,
                        cdx_stream_t stream) {
  if (!steps_ok(steps) || !dtype_ok(dtype) || !mean || !workspace || !totals) return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (steps < 2)  // no edge
    return hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s) == hipSuccess ? CDX_OK : CDX_ELAUNCH;
  const int64_t total = nodes_of(steps), nb = blocks_of(steps);
  int64_t* counts = static_cast<int64_t*>(workspace);
  if (dtype == CDX_DTYPE_F32) count_launch<float>(mean, steps, total, nb, counts, totals, s);
  else count_launch<double>(mean, steps, total, nb, counts, totals, s);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_gpis_mesh_place(const void* mean, int32_t dtype, int32_t steps, const double* px, const double* py,
                        const double* pz, void* workspace, int64_t vcap, int64_t fcap, double* vertices,
                        int64_t* edges, int32_t* faces, cdx_stream_t stream) {
  if (!steps_ok(steps) || !dtype_ok(dtype) || !mean || !workspace || vcap < 0 || fcap < 0) return CDX_EINVAL;
  if (!px || !py || !pz || (vcap > 0 && !vertices) || (fcap > 0 && !faces)) return CDX_EINVAL;
  if (steps < 2) return CDX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = nodes_of(steps), nb = blocks_of(steps), cubes = nodes_of(steps - 1);
  int64_t* offsets = static_cast<int64_t*>(workspace);
  if (7 * total >= MESH_INDEX_LIMIT || 12 * cubes >= MESH_INDEX_LIMIT) {
    // only a lattice this large can overflow int32 vertex numbers: read the count's totals back (a wait on the stream)
    int64_t vf[2];
    if (hipMemcpyAsync(vf, offsets + 2 * nb, sizeof(vf), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return CDX_ELAUNCH;
    if (vf[0] >= MESH_INDEX_LIMIT || vf[1] >= MESH_INDEX_LIMIT) return CDX_EINVAL;
  }
  int32_t* base = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + base_offset(nb));
  if (dtype == CDX_DTYPE_F32)
    place_launch<float>(mean, steps, total, nb, px, py, pz, offsets, base, vcap, fcap, vertices, edges, faces, s);
  else
    place_launch<double>(mean, steps, total, nb, px, py, pz, offsets, base, vcap, fcap, vertices, edges, faces, s);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_gpis_mesh_refine_init(const void* mean, int32_t dtype, int32_t steps, const double* px, const double* py,
                              const double* pz, const int64_t* edges, int64_t V, double* state, double* vertices,
                              cdx_stream_t stream) {
  if (!steps_ok(steps) || !dtype_ok(dtype) || !mean || !px || !py || !pz || V < 0) return CDX_EINVAL;
  if (V == 0) return CDX_OK;
  if (!edges || !state || !vertices || (V + MESH_BLOCK - 1) / MESH_BLOCK > 0x7fffffff) return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((V + MESH_BLOCK - 1) / MESH_BLOCK));
  if (dtype == CDX_DTYPE_F32)
    hipLaunchKernelGGL(mesh_refine_kernel<float>, grid, dim3(MESH_BLOCK), 0, s, static_cast<const float*>(mean),
                       (const double*)nullptr, steps, px, py, pz, edges, V, state, vertices);
  else
    hipLaunchKernelGGL(mesh_refine_kernel<double>, grid, dim3(MESH_BLOCK), 0, s, static_cast<const double*>(mean),
                       (const double*)nullptr, steps, px, py, pz, edges, V, state, vertices);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_gpis_mesh_refine_step(const double* fv, int32_t steps, const double* px, const double* py, const double* pz,
                              const int64_t* edges, int64_t V, double* state, double* vertices, cdx_stream_t stream) {
  if (!steps_ok(steps) || !px || !py || !pz || V < 0) return CDX_EINVAL;
  if (V == 0) return CDX_OK;
  if (!fv || !edges || !state || !vertices || (V + MESH_BLOCK - 1) / MESH_BLOCK > 0x7fffffff) return CDX_EINVAL;
  hipLaunchKernelGGL(mesh_refine_kernel<double>, dim3((unsigned)((V + MESH_BLOCK - 1) / MESH_BLOCK)), dim3(MESH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), (const double*)nullptr, fv, steps, px, py, pz, edges, V, state,
                     vertices);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
