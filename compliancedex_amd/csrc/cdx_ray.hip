// Ray casting on triangle meshes for gfx950, and the depth camera on top of it: the second query on a prepared
// mesh's hierarchy (cdx_sdf_mesh_prepare), next to the point-to-mesh distance of cdx_sdf.hip.  The rule — the
// float64 Möller–Trumbore test with its determinant threshold, the first-hit order, the pixel rays and the depth
// unprojection — is csrc/cdx_ray.h, compiled here and by the host build (cdxh_ray_cast, cdxh_depth_unproject).
//
//   scan    one ray per lane, every face through 512-face LDS tiles in the faces' own order.  Any [F, 3, 3] float32
//           tensor, no preparation.
//   walk    one wave per 64 consecutive rays on a prepared mesh's ray records (cdx_ray_mesh_prepare: the bounding
//           balls of the 512-, 32- and 8-face nodes and the faces' vertices with their original index, in the k-d
//           order).  Top node → chunk → run → face; the loops are wave-uniform (a node is entered when some lane
//           needs it, node and face data are read at wave-uniform addresses), a lane evaluates the faces of the
//           runs it needs.  Top nodes are visited near to far along the wave's first ray (a better first hit
//           early prunes more).  A lane skips a node only when cdx::ray_ball_miss holds: the ray's points with
//           tmin ≤ s ≤ min(tmax, best t) all lie farther than R + κ·(|o − c|₁ + R) from the node's centre.  Every face
//           the rule accepts with a t that could still win or tie lies, with its rounding error, inside that ball
//           (DESIGN.md §5f), so the walk's holder ends equal to the scan's, bit for bit — the first-hit order does
//           not depend on the order of evaluation.  A ray outside cdx::ray_in_domain, and every ray on a mesh with
//           a NaN-capable face, skips nothing.
//   render  cdx_depth_render: the same two casts with the rays generated in the kernel (cdx::pixel_ray), one wave per
//           8×8 pixel tile; no ray buffer exists.
//   unproject  cdx_depth_count / cdx_depth_place: per-workgroup counts, a one-workgroup scan, ordered placement —
//           the scheme of cdx_field.hip's surface cells.  No atomics; row-major pixel order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cdx_ray.h"
#include "cdx_sdf.h"
#include "cdx_sdf_mesh.h"

#pragma clang fp contract(off)

namespace {

using namespace cdx::mesh;

constexpr int RAY_BLOCK = 256;              // rays (pixels) per workgroup: 4 waves
constexpr int RAY_WAVES = RAY_BLOCK / 64;
constexpr int RAY_TILE = 512;               // faces per LDS tile of the scan
constexpr int TILE_PX = 8;                  // a wave renders an 8×8 pixel tile
constexpr int REC_V4 = 3;                   // float4 words of a ray face record

// Ray records of a prepared mesh: [header: may-NaN flag, F][top balls: T float4][chunk balls: C float4]
// [run balls: C·RPC float4][face records: C·CHUNK × 3 float4 = (v0 xyz, v1 x | v1 yz, v2 xy | v2 z, index, 0, 0)],
// balls = (centre xyz, radius) of the mesh's nodes, faces in the mesh's k-d order.
size_t rm_top_off() { return 256; }
size_t rm_chunk_off(int64_t C) { return rm_top_off() + align256((size_t)((C + TOPB - 1) / TOPB) * sizeof(float4)); }
size_t rm_run_off(int64_t C) { return rm_chunk_off(C) + align256((size_t)C * sizeof(float4)); }
size_t rm_rec_off(int64_t C) { return rm_run_off(C) + align256((size_t)C * RPC * sizeof(float4)); }
size_t rm_bytes(int64_t F) {
  const int64_t C = n_chunks(F);
  return rm_rec_off(C) + align256((size_t)C * CHUNK * REC_V4 * sizeof(float4));
}

// What a cast reads.  Scan: faces, F.  Walk: the ray records.
struct MeshView {
  const float* faces;
  int F, C, T;
  const unsigned* hdr;
  const float4 *top, *chunk, *run, *rec;
};

// Diagnostic counters (cdx_ray_stats): [0] (ray, face) pairs the walk evaluated, [1] rays it cast.  Counted only
// while enabled (one atomic per wave).
__device__ unsigned long long g_ray_stats[2];
bool g_ray_count = false;

__global__ __launch_bounds__(256) void ray_prepare_kernel(const cdx::FaceRec* __restrict__ rec,
                                                          const Node* __restrict__ top, const Node* __restrict__ chunk,
                                                          const Node* __restrict__ run, const unsigned* __restrict__ mws,
                                                          int64_t F, int64_t C, int64_t T, unsigned* __restrict__ hdr,
                                                          float4* __restrict__ otop, float4* __restrict__ ochunk,
                                                          float4* __restrict__ orun, float4* __restrict__ orec) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) { hdr[0] = mws[6]; hdr[1] = (unsigned)F; }
  if (j < T) otop[j] = top[j].a;
  if (j < C) ochunk[j] = chunk[j].a;
  if (j < C * RPC) orun[j] = run[j].a;
  if (j < C * CHUNK) {
    const cdx::FaceRec& r = rec[j];
    const bool live = j < F;
    orec[3 * j] = make_float4(r.v1.x, r.v1.y, r.v1.z, r.v2.x);
    orec[3 * j + 1] = make_float4(r.v2.y, r.v2.z, r.v3.x, r.v3.y);
    orec[3 * j + 2] = make_float4(r.v3.z, __int_as_float(live ? r.idx : -1), 0.f, 0.f);
  }
}

// Scan: every thread of the workgroup takes part (the tiles are loaded together); a lane without a ray evaluates
// nothing.
__device__ __forceinline__ cdx::RayHit cast_scan(const MeshView& m, bool valid, const double* o, const double* d,
                                                 double tmin, double tmax, float* sf) {
  cdx::RayHit best = cdx::ray_miss();
  for (int f0 = 0; f0 < m.F; f0 += RAY_TILE) {
    const int nt = min(RAY_TILE, m.F - f0);
    __syncthreads();
    for (int j = threadIdx.x; j < nt * 9; j += RAY_BLOCK) sf[j] = m.faces[(int64_t)f0 * 9 + j];
    __syncthreads();
    if (valid)
      for (int s = 0; s < nt; ++s) cdx::ray_update(o, d, &sf[9 * s], f0 + s, tmin, tmax, best);
  }
  return best;
}

__device__ __forceinline__ unsigned ordered_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Walk: one wave, lane = ray.  Returns the lane's holder; *pairs counts the faces the lane evaluated.
__device__ __forceinline__ cdx::RayHit cast_walk(const MeshView& m, bool valid, const double* o, const double* d,
                                                 double tmin, double tmax, unsigned* pairs) {
  cdx::RayHit best = cdx::ray_miss();
  const int lane = threadIdx.x & 63;
  const unsigned long long vm = __ballot(valid);
  if (!vm) return best;
  // a lane may skip nodes only inside the domain of the margin proof, on a mesh without NaN-capable faces
  const bool dom = valid && cdx::ray_in_domain(o, d) && m.hdr[0] == 0u;
  const int T = m.T;
  // near-to-far order of the top nodes along the wave's first ray (T ≤ 64: lane t holds top t's key)
  const bool ordered = T <= 64;
  unsigned key = 0xFFFFFFFFu;
  if (ordered) {
    const int r0 = __builtin_ctzll(vm);
    double ro[3], rd[3];
    for (int k = 0; k < 3; ++k) { ro[k] = __shfl(o[k], r0); rd[k] = __shfl(d[k], r0); }
    if (lane < T) {
      const float4 b = m.top[lane];
      const double L[3] = {(double)b.x - ro[0], (double)b.y - ro[1], (double)b.z - ro[2]};
      const double along = cdx::ray_dot(L, rd) - (double)b.w * sqrt(cdx::ray_dot(rd, rd));
      key = (ordered_key((float)along) & ~63u) | (unsigned)lane;
    }
  }
  unsigned long long visited = 0ull;
  for (int it = 0; it < T; ++it) {
    int t = it;
    if (ordered) {
      unsigned k = ((visited >> lane) & 1ull) ? 0xFFFFFFFFu : key;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) k = min(k, (unsigned)__shfl_xor((int)k, off));
      k = __builtin_amdgcn_readfirstlane(k);
      t = (k & 63u) < (unsigned)T && !((visited >> (k & 63u)) & 1ull) ? (int)(k & 63u) : __builtin_ctzll(~visited);
      visited |= 1ull << t;
    }
    const float4 tb = m.top[t];
    const bool nt = valid && !(dom && cdx::ray_ball_miss(o, d, tmin, fmin(tmax, best.t), tb.x, tb.y, tb.z, tb.w));
    if (!__any(nt)) continue;
    const int c1 = min(m.C, (t + 1) * TOPB);
    for (int c = t * TOPB; c < c1; ++c) {
      const float4 cb = m.chunk[c];
      const bool nc = nt && !(dom && cdx::ray_ball_miss(o, d, tmin, fmin(tmax, best.t), cb.x, cb.y, cb.z, cb.w));
      if (!__any(nc)) continue;
      for (int r = 0; r < RPC; ++r) {
        const int j0 = c * CHUNK + r * RUN;
        if (j0 >= m.F) break;
        const float4 rb = m.run[c * RPC + r];
        const bool nr = nc && !(dom && cdx::ray_ball_miss(o, d, tmin, fmin(tmax, best.t), rb.x, rb.y, rb.z, rb.w));
        if (!__any(nr)) continue;
        const int nf = min(RUN, m.F - j0);
        for (int k = 0; k < nf; ++k) {
          const float4* q = m.rec + (int64_t)REC_V4 * (j0 + k);
          const float4 a = q[0], b = q[1], cc = q[2];
          if (nr) {
            const float f[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, cc.x};
            cdx::ray_update(o, d, f, __float_as_int(cc.y), tmin, tmax, best);
            ++*pairs;
          }
        }
      }
    }
  }
  return best;
}

template <bool WALK>
__device__ __forceinline__ cdx::RayHit cast(const MeshView& m, bool valid, const double* o, const double* d, double tmin,
                                            double tmax, float* sf, int count) {
  if (!WALK) return cast_scan(m, valid, o, d, tmin, tmax, sf);
  unsigned pairs = 0;
  const cdx::RayHit h = cast_walk(m, valid, o, d, tmin, tmax, &pairs);
  if (count) {
    unsigned long long p = pairs;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p += __shfl_xor(p, off);
    const unsigned long long nv = __popcll(__ballot(valid));
    if ((threadIdx.x & 63) == 0 && nv) {
      atomicAdd(&g_ray_stats[0], p);
      atomicAdd(&g_ray_stats[1], nv);
    }
  }
  return h;
}

// Rays from buffers: ray r on thread r of the grid (a wave holds 64 consecutive rays, in the caller's order).
template <bool WALK>
__global__ __launch_bounds__(RAY_BLOCK) void ray_cast_kernel(MeshView m, const double* __restrict__ origins,
                                                             const double* __restrict__ dirs, int64_t R, double tmin,
                                                             double tmax, double* __restrict__ out_t,
                                                             int32_t* __restrict__ out_face, double* __restrict__ out_uv,
                                                             int count) {
  __shared__ float sf[WALK ? 1 : RAY_TILE * 9];
  const int64_t r = (int64_t)blockIdx.x * RAY_BLOCK + threadIdx.x;
  const bool live = r < R;
  double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
  if (live)
    for (int k = 0; k < 3; ++k) { o[k] = origins[3 * r + k]; d[k] = dirs[3 * r + k]; }
  const bool valid = live && cdx::ray_valid(o, d);
  const cdx::RayHit h = cast<WALK>(m, valid, o, d, tmin, tmax, sf, count);
  if (!live) return;
  double t, u, v;
  int32_t face;
  cdx::ray_result(h, t, face, u, v);
  out_t[r] = t;
  out_face[r] = face;
  if (out_uv) { out_uv[2 * r] = u; out_uv[2 * r + 1] = v; }
}

struct CameraArgs { double intr[4]; double M[16]; };

// Depth render: wave w of workgroup b renders pixel tile 4·b + w (tiles in row-major order of the tile grid), lane l
// its pixel (l / 8, l % 8).
template <bool WALK>
__global__ __launch_bounds__(RAY_BLOCK) void depth_render_kernel(MeshView m, CameraArgs cam, int W, int H, int tiles_x,
                                                                 int64_t tiles, double tmin, double tmax,
                                                                 double* __restrict__ depth,
                                                                 int32_t* __restrict__ out_face, int count) {
  __shared__ float sf[WALK ? 1 : RAY_TILE * 9];
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * RAY_WAVES + (threadIdx.x >> 6);
  const int ty = (int)(tile / tiles_x), tx = (int)(tile % tiles_x);
  const int i = ty * TILE_PX + (lane >> 3), j = tx * TILE_PX + (lane & 7);
  const bool live = tile < tiles && i < H && j < W;
  double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
  if (live) cdx::pixel_ray(i, j, cam.intr, cam.M, o, d);
  const bool valid = live && cdx::ray_valid(o, d);
  const cdx::RayHit h = cast<WALK>(m, valid, o, d, tmin, tmax, sf, count);
  if (!live) return;
  double t, u, v;
  int32_t face;
  cdx::ray_result(h, t, face, u, v);
  const int64_t px = (int64_t)i * W + j;
  depth[px] = face >= 0 ? t : 0.0;
  if (out_face) out_face[px] = face;
}

// ---- depth unprojection

struct UnprojectArgs {
  double intr[4], M[16];
  double scale, trunc, z_max;
  int W, H, stride, Ws, has_M;
  int64_t n;  // pixels visited: ⌈H/stride⌉·⌈W/stride⌉
};

// Thread q's pixel and its point, if kept.
template <typename D, typename Z>
__device__ __forceinline__ bool unproject_one(const D* __restrict__ depth, const UnprojectArgs& a, double* out) {
  const int64_t q = (int64_t)blockIdx.x * RAY_BLOCK + threadIdx.x;
  if (q >= a.n) return false;
  const int i = (int)(q / a.Ws) * a.stride, j = (int)(q % a.Ws) * a.stride;
  return cdx::depth_point<Z>((Z)depth[(int64_t)i * a.W + j], i, j, a.intr, a.scale, a.trunc, a.z_max,
                             a.has_M ? a.M : nullptr, out);
}

template <typename D, typename Z>
__global__ __launch_bounds__(RAY_BLOCK) void depth_count_kernel(const D* __restrict__ depth, UnprojectArgs a,
                                                                int64_t* __restrict__ counts) {
  __shared__ int wsum[RAY_WAVES];
  double p[3];
  const bool f = unproject_one<D, Z>(depth, a, p);
  const unsigned long long b = __ballot(f);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < RAY_WAVES; ++w) s += wsum[w];
    counts[blockIdx.x] = s;
  }
}

// counts [nb] → their exclusive prefix sums, in place; *total = Σ counts.  One workgroup: each thread owns a
// contiguous segment (its sum, a Hillis-Steele scan of the 256 sums in LDS, then the segment's prefixes).
__global__ __launch_bounds__(RAY_BLOCK) void depth_scan_kernel(int64_t* __restrict__ counts, int64_t nb,
                                                               int64_t* __restrict__ total) {
  __shared__ int64_t s[RAY_BLOCK];
  const int tid = threadIdx.x;
  const int64_t per = (nb + RAY_BLOCK - 1) / RAY_BLOCK;
  const int64_t lo = min((int64_t)tid * per, nb), hi = min(lo + per, nb);
  int64_t sum = 0;
  for (int64_t q = lo; q < hi; ++q) sum += counts[q];
  s[tid] = sum;
  __syncthreads();
  for (int off = 1; off < RAY_BLOCK; off <<= 1) {
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
  if (tid == RAY_BLOCK - 1) *total = s[tid];
}

template <typename D, typename Z>
__global__ __launch_bounds__(RAY_BLOCK) void depth_place_kernel(const D* __restrict__ depth, UnprojectArgs a,
                                                                const int64_t* __restrict__ offsets, int64_t capacity,
                                                                double* __restrict__ points) {
  __shared__ int wsum[RAY_WAVES];
  double p[3];
  const bool f = unproject_one<D, Z>(depth, a, p);
  const unsigned long long b = __ballot(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  if (!f) return;
  int64_t rank = offsets[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += wsum[w];
  if (rank >= capacity) return;
  points[3 * rank] = p[0];
  points[3 * rank + 1] = p[1];
  points[3 * rank + 2] = p[2];
}

bool faces_ok(const float* faces, int64_t F) { return faces && F > 0 && F <= INT32_MAX / 9; }

// The view a cast reads; false for a bad combination.  mode 0: the walk when ray records are given.
bool mesh_view(const void* mesh, const void* ray_mesh, const float* faces, int64_t F, int32_t mode, MeshView& m,
               bool& walk) {
  if (!faces_ok(faces, F) || mode < CDX_RAY_AUTO || mode > CDX_RAY_WALK) return false;
  walk = mode == CDX_RAY_WALK || (mode == CDX_RAY_AUTO && mesh && ray_mesh);
  if (walk && (!mesh || !ray_mesh)) return false;
  const int64_t C = n_chunks(F);
  m.faces = faces;
  m.F = (int)F;
  m.C = (int)C;
  m.T = (int)n_tops(F);
  m.hdr = nullptr;
  m.top = m.chunk = m.run = m.rec = nullptr;
  if (walk) {
    const char* b = static_cast<const char*>(ray_mesh);
    m.hdr = reinterpret_cast<const unsigned*>(b);
    m.top = reinterpret_cast<const float4*>(b + rm_top_off());
    m.chunk = reinterpret_cast<const float4*>(b + rm_chunk_off(C));
    m.run = reinterpret_cast<const float4*>(b + rm_run_off(C));
    m.rec = reinterpret_cast<const float4*>(b + rm_rec_off(C));
  }
  return true;
}

bool unproject_args(int32_t dtype, int32_t W, int32_t H, int32_t stride, const double* intr, double scale, double trunc,
                    double z_max, const double* M, UnprojectArgs& a) {
  if ((dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64 && dtype != CDX_DEPTH_U16) || W < 1 || H < 1 || stride < 1)
    return false;
  for (int k = 0; k < 4; ++k) a.intr[k] = intr ? intr[k] : 1.0;
  for (int k = 0; k < 16; ++k) a.M[k] = M ? M[k] : 0.0;
  a.scale = scale; a.trunc = trunc; a.z_max = z_max;
  a.W = W; a.H = H; a.stride = stride;
  a.Ws = (W + stride - 1) / stride;
  a.has_M = M != nullptr;
  a.n = (int64_t)((H + stride - 1) / stride) * a.Ws;
  return (a.n + RAY_BLOCK - 1) / RAY_BLOCK <= 0x7fffffff;
}

}  // namespace

extern "C" {

size_t cdx_ray_mesh_bytes(int64_t F) { return F > 0 && F <= INT32_MAX / 9 ? rm_bytes(F) : 0; }

int cdx_ray_mesh_prepare(const void* mesh, int64_t F, void* ray_mesh, cdx_stream_t stream) {
  if (!mesh || !ray_mesh || F <= 0 || F > INT32_MAX / 9) return CDX_EINVAL;
  const int64_t C = n_chunks(F), T = n_tops(F);
  const char* b = static_cast<const char*>(mesh);
  char* o = static_cast<char*>(ray_mesh);
  hipLaunchKernelGGL(ray_prepare_kernel, dim3((unsigned)((C * CHUNK + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const cdx::FaceRec*>(b + mesh_rec_off()),
                     reinterpret_cast<const Node*>(b + mesh_top_off(C)),
                     reinterpret_cast<const Node*>(b + mesh_chunk_off(C)),
                     reinterpret_cast<const Node*>(b + mesh_run_off(C)), reinterpret_cast<const unsigned*>(b), F, C, T,
                     reinterpret_cast<unsigned*>(o), reinterpret_cast<float4*>(o + rm_top_off()),
                     reinterpret_cast<float4*>(o + rm_chunk_off(C)), reinterpret_cast<float4*>(o + rm_run_off(C)),
                     reinterpret_cast<float4*>(o + rm_rec_off(C)));
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_ray_cast(const void* mesh, const void* ray_mesh, const float* faces, int64_t F, const double* origins,
                 const double* dirs, int64_t R, double tmin, double tmax, int32_t mode, double* t, int32_t* face,
                 double* uv, cdx_stream_t stream) {
  MeshView m;
  bool walk = false;
  if (R < 0 || !mesh_view(mesh, ray_mesh, faces, F, mode, m, walk)) return CDX_EINVAL;
  if (R == 0) return CDX_OK;
  if (!origins || !dirs || !t || !face || (R + RAY_BLOCK - 1) / RAY_BLOCK > 0x7fffffff) return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((R + RAY_BLOCK - 1) / RAY_BLOCK));
  if (walk)
    hipLaunchKernelGGL(ray_cast_kernel<true>, grid, dim3(RAY_BLOCK), 0, s, m, origins, dirs, R, tmin, tmax, t, face, uv,
                       (int)g_ray_count);
  else
    hipLaunchKernelGGL(ray_cast_kernel<false>, grid, dim3(RAY_BLOCK), 0, s, m, origins, dirs, R, tmin, tmax, t, face,
                       uv, 0);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_depth_render(const void* mesh, const void* ray_mesh, const float* faces, int64_t F, int32_t W, int32_t H,
                     const double* intr, const double* cam_to_world, double tmin, double tmax, int32_t mode,
                     double* depth, int32_t* face, cdx_stream_t stream) {
  MeshView m;
  bool walk = false;
  if (W < 1 || H < 1 || !intr || !cam_to_world || !depth || !mesh_view(mesh, ray_mesh, faces, F, mode, m, walk))
    return CDX_EINVAL;
  CameraArgs cam;
  for (int k = 0; k < 4; ++k) cam.intr[k] = intr[k];
  for (int k = 0; k < 16; ++k) cam.M[k] = cam_to_world[k];
  const int tiles_x = (W + TILE_PX - 1) / TILE_PX;
  const int64_t tiles = (int64_t)tiles_x * ((H + TILE_PX - 1) / TILE_PX);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((tiles + RAY_WAVES - 1) / RAY_WAVES));
  if (walk)
    hipLaunchKernelGGL(depth_render_kernel<true>, grid, dim3(RAY_BLOCK), 0, s, m, cam, W, H, tiles_x, tiles, tmin, tmax,
                       depth, face, (int)g_ray_count);
  else
    hipLaunchKernelGGL(depth_render_kernel<false>, grid, dim3(RAY_BLOCK), 0, s, m, cam, W, H, tiles_x, tiles, tmin,
                       tmax, depth, face, 0);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

size_t cdx_depth_workspace(int32_t W, int32_t H, int32_t stride) {
  UnprojectArgs a;
  if (!unproject_args(CDX_DTYPE_F32, W, H, stride, nullptr, 1.0, 1.0, 1.0, nullptr, a)) return 0;
  return align256((size_t)((a.n + RAY_BLOCK - 1) / RAY_BLOCK) * sizeof(int64_t));
}

int cdx_depth_count(const void* depth, int32_t dtype, int32_t W, int32_t H, int32_t stride, double depth_scale,
                    double depth_trunc, double z_max, void* workspace, int64_t* total, cdx_stream_t stream) {
  UnprojectArgs a;
  if (!depth || !workspace || !total ||
      !unproject_args(dtype, W, H, stride, nullptr, depth_scale, depth_trunc, z_max, nullptr, a))
    return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t nb = (a.n + RAY_BLOCK - 1) / RAY_BLOCK;
  int64_t* counts = static_cast<int64_t*>(workspace);
  const dim3 grid((unsigned)nb), block(RAY_BLOCK);
  if (dtype == CDX_DTYPE_F32)
    hipLaunchKernelGGL((depth_count_kernel<float, float>), grid, block, 0, s, static_cast<const float*>(depth), a, counts);
  else if (dtype == CDX_DTYPE_F64)
    hipLaunchKernelGGL((depth_count_kernel<double, double>), grid, block, 0, s, static_cast<const double*>(depth), a,
                       counts);
  else
    hipLaunchKernelGGL((depth_count_kernel<uint16_t, float>), grid, block, 0, s, static_cast<const uint16_t*>(depth), a,
                       counts);
  hipLaunchKernelGGL(depth_scan_kernel, dim3(1), block, 0, s, counts, nb, total);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_depth_place(const void* depth, int32_t dtype, int32_t W, int32_t H, int32_t stride, const double* intr,
                    double depth_scale, double depth_trunc, double z_max, const double* transform,
                    const void* workspace, int64_t capacity, double* points, cdx_stream_t stream) {
  UnprojectArgs a;
  if (!depth || !workspace || !intr || capacity < 0 || (capacity > 0 && !points) ||
      !unproject_args(dtype, W, H, stride, intr, depth_scale, depth_trunc, z_max, transform, a))
    return CDX_EINVAL;
  if (capacity == 0) return CDX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t nb = (a.n + RAY_BLOCK - 1) / RAY_BLOCK;
  const int64_t* offsets = static_cast<const int64_t*>(workspace);
  const dim3 grid((unsigned)nb), block(RAY_BLOCK);
  if (dtype == CDX_DTYPE_F32)
    hipLaunchKernelGGL((depth_place_kernel<float, float>), grid, block, 0, s, static_cast<const float*>(depth), a,
                       offsets, capacity, points);
  else if (dtype == CDX_DTYPE_F64)
    hipLaunchKernelGGL((depth_place_kernel<double, double>), grid, block, 0, s, static_cast<const double*>(depth), a,
                       offsets, capacity, points);
  else
    hipLaunchKernelGGL((depth_place_kernel<uint16_t, float>), grid, block, 0, s, static_cast<const uint16_t*>(depth), a,
                       offsets, capacity, points);
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

int cdx_ray_stats(int32_t enable, uint64_t* out2, cdx_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (out2) {
    if (hipMemcpyFromSymbolAsync(out2, HIP_SYMBOL(g_ray_stats), 2 * sizeof(uint64_t), 0, hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return CDX_ELAUNCH;
  }
  if (enable >= 0) {
    const unsigned long long z[2] = {0, 0};
    if (enable && (hipMemcpyToSymbolAsync(HIP_SYMBOL(g_ray_stats), z, sizeof(z), 0, hipMemcpyHostToDevice, s) !=
                       hipSuccess ||
                   hipStreamSynchronize(s) != hipSuccess))
      return CDX_ELAUNCH;
    g_ray_count = enable != 0;
  }
  return CDX_OK;
}

}  // extern "C"
