// Farthest-point sampling for gfx950: the down-sampling in front of GPIS.fit (optimize_pregrasp.py:904,
// get_observable_pcd.py:40; open3d's farthest_point_down_sample in the reference).  The rule is csrc/cdx_fps.h; both
// paths below give its bits, for B clouds of P rows each that never interact.
//
//   fps_block_kernel   one workgroup (1024 lanes) per cloud, all K rounds in one launch.  A lane keeps up to
//                      FPS_MAX_PER_LANE rows and their dist in registers (row j lives in lane j % 1024, slot
//                      j / 1024).  A round: the update and the lane's own arg-max, a DPP reduction over the wave,
//                      one LDS exchange of the 16 wave winners (every wave reduces them again, so nobody waits for
//                      a broadcast), then the owner of the winner puts its coordinates in LDS for all.  Two barriers
//                      a round.  Serves P ≤ cdx_fps_capacity().
//   fps_round_kernel   one launch per round, ceil(P / 1024) workgroups per cloud.  A workgroup updates its slice of
//                      dist (in the workspace), writes its (dist, index) winner to its slot, fences and takes a ticket
//                      from the cloud's counter.  The workgroup that draws the last ticket reduces the slots, writes
//                      the next centre and resets the counter.  Nobody waits for anybody: no grid barrier, no
//                      cooperative launch, no spin, no residency requirement.  The launches follow each other on the
//                      caller's stream with no host synchronisation.
// The update of the last round changes no output, so neither path runs it: K − 1 per-round launches (one for K = 1).
#include <hip/hip_runtime.h>

#include "cdx_fps.h"

namespace {

constexpr int FPS_BLOCK = 1024;  // one-workgroup path: 16 waves, 4 a SIMD, 128 VGPRs each
constexpr int FPS_WAVES = FPS_BLOCK / 64;
constexpr int FPS_MAX_PER_LANE = 8;  // 8 rows × (3 coordinates + dist) × 2 = 64 VGPRs of state
constexpr int64_t FPS_CAPACITY = (int64_t)FPS_BLOCK * FPS_MAX_PER_LANE;

constexpr int FPS_RBLOCK = 256;  // per-round path
constexpr int FPS_RWAVES = FPS_RBLOCK / 64;
constexpr int FPS_RPER = 4;
constexpr int FPS_RPOINTS = FPS_RBLOCK * FPS_RPER;  // rows per workgroup

constexpr double FPS_PAD = -2.0;   // dist of a register slot past the cloud: below every row's, and it never moves
constexpr double FPS_NONE = -3.0;  // below every slot's: a lane's arg-max before its first row
constexpr int FPS_NO_INDEX = 0x7fffffff;

struct FpsSlot {
  double d;
  int64_t i;
};

int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// One step of the arg-max over lanes on the data-parallel path of the vector ALU (no LDS round trip): every lane
// meets the pair of the lane CTRL names.  A lane whose source does not exist meets its own pair, which changes nothing.
template <int CTRL>
__device__ __forceinline__ void fps_dpp_step(double& bd, int& bi) {
  const int lo = __double2loint(bd), hi = __double2hiint(bd);
  const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const int oi = __builtin_amdgcn_update_dpp(bi, bi, CTRL, 0xf, 0xf, false);
  const double od = __hiloint2double(ohi, olo);
  if (cdx::fps_beats(od, oi, bd, bi)) {
    bd = od;
    bi = oi;
  }
}

__device__ __forceinline__ void fps_read_lane(double& bd, int& bi, int lane) {
  bd = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(bd), lane),
                        __builtin_amdgcn_readlane(__double2loint(bd), lane));
  bi = __builtin_amdgcn_readlane(bi, lane);
}

constexpr int DPP_ROW_SHR = 0x110;     // row_shr:n is 0x110 + n: lane l of a 16-lane row reads lane l − n
constexpr int DPP_ROW_BCAST15 = 0x142; // lane 15 of each row to every lane of the next row
constexpr int DPP_ROW_BCAST31 = 0x143; // lane 31 to every lane of rows 2 and 3

// Lane 15 of each 16-lane row gets its row's winner.
__device__ __forceinline__ void fps_row_reduce(double& bd, int& bi) {
  fps_dpp_step<DPP_ROW_SHR + 1>(bd, bi);
  fps_dpp_step<DPP_ROW_SHR + 2>(bd, bi);
  fps_dpp_step<DPP_ROW_SHR + 4>(bd, bi);
  fps_dpp_step<DPP_ROW_SHR + 8>(bd, bi);
}

// Every lane gets the winner of the wave's 64 pairs.  All 64 lanes must be active.
__device__ __forceinline__ void fps_wave_reduce(double& bd, int& bi) {
  fps_row_reduce(bd, bi);
  fps_dpp_step<DPP_ROW_BCAST15>(bd, bi);  // lane 31: rows 0-1, lane 63: rows 2-3
  fps_dpp_step<DPP_ROW_BCAST31>(bd, bi);  // lane 63: the wave
  fps_read_lane(bd, bi, 63);
}

template <typename T, int NPL>
__global__ __launch_bounds__(FPS_BLOCK) void fps_block_kernel(const T* __restrict__ X, int P, int K, int start,
                                                              int64_t* __restrict__ sel, double* __restrict__ radius,
                                                              double* __restrict__ points) {
  __shared__ double s_d[FPS_WAVES];
  __shared__ int s_i[FPS_WAVES];
  __shared__ double s_c[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const T* Xb = X + b * (int64_t)P * 3;
  double px[NPL], py[NPL], pz[NPL], dist[NPL];
#pragma unroll
  for (int u = 0; u < NPL; ++u) {
    const int j = u * FPS_BLOCK + tid;
    if (j < P) {
      px[u] = (double)Xb[3 * (int64_t)j];
      py[u] = (double)Xb[3 * (int64_t)j + 1];
      pz[u] = (double)Xb[3 * (int64_t)j + 2];
      dist[u] = cdx::fps_init_dist(px[u], py[u], pz[u]);
    } else {
      px[u] = py[u] = pz[u] = 0.0;
      dist[u] = FPS_PAD;
    }
  }
  int s = start;
  double cx = (double)Xb[3 * (int64_t)s], cy = (double)Xb[3 * (int64_t)s + 1], cz = (double)Xb[3 * (int64_t)s + 2];
  double r = cdx::fps_init_dist(cx, cy, cz);
  for (int i = 0;; ++i) {
    if (tid == 0) {
      const int64_t o = b * K + i;
      if (sel) sel[o] = s;
      if (radius) radius[o] = r;
      if (points) {
        points[3 * o] = cx;
        points[3 * o + 1] = cy;
        points[3 * o + 2] = cz;
      }
    }
    if (i == K - 1) break;
    double bd = FPS_NONE;
    int bi = FPS_NO_INDEX;
#pragma unroll
    for (int u = 0; u < NPL; ++u) {  // rows in ascending index: a strict > keeps the lowest
      dist[u] = cdx::fps_update(dist[u], cdx::fps_sqdist(px[u], py[u], pz[u], cx, cy, cz));
      if (dist[u] > bd) {
        bd = dist[u];
        bi = u * FPS_BLOCK + tid;
      }
    }
    fps_wave_reduce(bd, bi);
    if (lane == 0) {
      s_d[wave] = bd;
      s_i[wave] = bi;
    }
    __syncthreads();
    static_assert(FPS_WAVES == 16, "one wave winner per lane of a 16-lane row");
    bd = s_d[lane & (FPS_WAVES - 1)];
    bi = s_i[lane & (FPS_WAVES - 1)];
    fps_row_reduce(bd, bi);
    fps_read_lane(bd, bi, 15);
    if ((bi & (FPS_BLOCK - 1)) == tid) {  // the winner's owner: its slot's coordinates, by selects on registers
      const int slot = bi / FPS_BLOCK;
      double ox = px[0], oy = py[0], oz = pz[0];
#pragma unroll
      for (int u = 1; u < NPL; ++u)
        if (slot == u) {
          ox = px[u];
          oy = py[u];
          oz = pz[u];
        }
      s_c[0] = ox;
      s_c[1] = oy;
      s_c[2] = oz;
    }
    __syncthreads();
    cx = s_c[0];
    cy = s_c[1];
    cz = s_c[2];
    s = bi;
    r = bd;
  }
}

template <typename T>
__global__ __launch_bounds__(FPS_RBLOCK) void fps_round_kernel(const T* __restrict__ X, int P, int K, int round,
                                                               int start, int G, double* __restrict__ dist,
                                                               FpsSlot* slots, int64_t* cur, unsigned* counter,
                                                               int64_t* __restrict__ sel, double* __restrict__ radius,
                                                               double* __restrict__ points) {
  __shared__ double s_d[FPS_RWAVES];
  __shared__ int s_i[FPS_RWAVES];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const T* Xb = X + b * (int64_t)P * 3;
  double* db = dist + b * (int64_t)P;
  FpsSlot* sb = slots + b * (int64_t)G;
  const bool first = round == 0;
  const int s = first ? start : (int)cur[b];
  const double cx = (double)Xb[3 * (int64_t)s], cy = (double)Xb[3 * (int64_t)s + 1],
               cz = (double)Xb[3 * (int64_t)s + 2];
  if (first && g == 0 && tid == 0) {
    const int64_t o = b * K;
    if (sel) sel[o] = s;
    if (radius) radius[o] = cdx::fps_init_dist(cx, cy, cz);
    if (points) {
      points[3 * o] = cx;
      points[3 * o + 1] = cy;
      points[3 * o + 2] = cz;
    }
  }
  double bd = FPS_NONE;
  int bi = FPS_NO_INDEX;
#pragma unroll
  for (int u = 0; u < FPS_RPER; ++u) {
    const int64_t j = (int64_t)g * FPS_RPOINTS + u * FPS_RBLOCK + tid;
    if (j < P) {
      const double x = (double)Xb[3 * j], y = (double)Xb[3 * j + 1], z = (double)Xb[3 * j + 2];
      double d = first ? cdx::fps_init_dist(x, y, z) : db[j];
      d = cdx::fps_update(d, cdx::fps_sqdist(x, y, z, cx, cy, cz));
      db[j] = d;
      if (d > bd) {
        bd = d;
        bi = (int)j;
      }
    }
  }
  fps_wave_reduce(bd, bi);
  if (lane == 0) {
    s_d[wave] = bd;
    s_i[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < FPS_RWAVES; ++w)
      if (cdx::fps_beats(s_d[w], s_i[w], bd, bi)) {
        bd = s_d[w];
        bi = s_i[w];
      }
    sb[g].d = bd;
    sb[g].i = bi;
    __threadfence();  // release: the slot is visible to the device before the ticket is
    const unsigned ticket = __hip_atomic_fetch_add(&counter[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = ticket == (unsigned)(G - 1);
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();  // acquire: every other workgroup's slot was written before its ticket
  bd = FPS_NONE;
  bi = FPS_NO_INDEX;
  for (int q = tid; q < G; q += FPS_RBLOCK) {
    const double od = __hip_atomic_load(&sb[q].d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int oi = (int)__hip_atomic_load(&sb[q].i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cdx::fps_beats(od, oi, bd, bi)) {
      bd = od;
      bi = oi;
    }
  }
  fps_wave_reduce(bd, bi);
  __syncthreads();  // s_d / s_i were read by thread 0 above
  if (lane == 0) {
    s_d[wave] = bd;
    s_i[wave] = bi;
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int w = 1; w < FPS_RWAVES; ++w)
    if (cdx::fps_beats(s_d[w], s_i[w], bd, bi)) {
      bd = s_d[w];
      bi = s_i[w];
    }
  __hip_atomic_store(&counter[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
  if (round + 1 >= K) return;
  cur[b] = bi;
  const int64_t o = b * K + round + 1;
  if (sel) sel[o] = bi;
  if (radius) radius[o] = bd;
  if (points) {
    points[3 * o] = (double)Xb[3 * (int64_t)bi];
    points[3 * o + 1] = (double)Xb[3 * (int64_t)bi + 1];
    points[3 * o + 2] = (double)Xb[3 * (int64_t)bi + 2];
  }
}

// Workspace of the per-round path: dist [B·P], slots [B·G], current centre [B], counters [B], each on 256 bytes.
struct FpsLayout {
  int64_t G;
  size_t dist, slots, cur, counter, bytes;
};

FpsLayout fps_layout(int64_t P, int64_t B) {
  FpsLayout l;
  l.G = (P + FPS_RPOINTS - 1) / FPS_RPOINTS;
  l.dist = 0;
  l.slots = l.dist + (size_t)round_up(B * P * (int64_t)sizeof(double), 256);
  l.cur = l.slots + (size_t)round_up(B * l.G * (int64_t)sizeof(FpsSlot), 256);
  l.counter = l.cur + (size_t)round_up(B * (int64_t)sizeof(int64_t), 256);
  l.bytes = l.counter + (size_t)round_up(B * (int64_t)sizeof(unsigned), 256);
  return l;
}

bool fps_shape_ok(int64_t P, int64_t B) {
  // B·ceil(P / 1024) workgroups in one grid dimension, and B·P·8 bytes far from overflow
  return P >= 1 && P < ((int64_t)1 << 31) && B >= 1 && B <= 0x7fffffff &&
         B * ((P + FPS_RPOINTS - 1) / FPS_RPOINTS) <= 0x7fffffff;
}

// 0: bad mode, or mode 1 beyond its capacity.
int fps_path(int64_t P, int32_t mode) {
  if (mode == 0) return P <= FPS_CAPACITY ? 1 : 2;
  if (mode == 1) return P <= FPS_CAPACITY ? 1 : 0;
  return mode == 2 ? 2 : 0;
}

template <typename T, int NPL>
void block_launch(const void* X, int P, int B, int K, int start, int64_t* sel, double* radius, double* points,
                  hipStream_t s) {
  hipLaunchKernelGGL((fps_block_kernel<T, NPL>), dim3((unsigned)B), dim3(FPS_BLOCK), 0, s, static_cast<const T*>(X),
                     P, K, start, sel, radius, points);
}

template <typename T>
void block_dispatch(const void* X, int P, int B, int K, int start, int64_t* sel, double* radius, double* points,
                    hipStream_t s) {
  const int per = (P + FPS_BLOCK - 1) / FPS_BLOCK;
  if (per <= 1) block_launch<T, 1>(X, P, B, K, start, sel, radius, points, s);
  else if (per <= 2) block_launch<T, 2>(X, P, B, K, start, sel, radius, points, s);
  else if (per <= 4) block_launch<T, 4>(X, P, B, K, start, sel, radius, points, s);
  else block_launch<T, FPS_MAX_PER_LANE>(X, P, B, K, start, sel, radius, points, s);
}

template <typename T>
int round_dispatch(const void* X, int P, int B, int K, int start, void* ws, int64_t* sel, double* radius,
                   double* points, hipStream_t s) {
  const FpsLayout l = fps_layout(P, B);
  char* w = static_cast<char*>(ws);
  double* dist = reinterpret_cast<double*>(w + l.dist);
  FpsSlot* slots = reinterpret_cast<FpsSlot*>(w + l.slots);
  int64_t* cur = reinterpret_cast<int64_t*>(w + l.cur);
  unsigned* counter = reinterpret_cast<unsigned*>(w + l.counter);
  // the counters of a workspace nobody has used yet; every launch leaves them at zero again
  if (hipMemsetAsync(counter, 0, (size_t)B * sizeof(unsigned), s) != hipSuccess) return CDX_ELAUNCH;
  const int rounds = K > 1 ? K - 1 : 1;
  for (int i = 0; i < rounds; ++i)
    hipLaunchKernelGGL(fps_round_kernel<T>, dim3((unsigned)(B * l.G)), dim3(FPS_RBLOCK), 0, s,
                       static_cast<const T*>(X), P, K, i, start, (int)l.G, dist, slots, cur, counter, sel, radius, points);
  return CDX_OK;
}

}  // namespace

extern "C" {

int64_t cdx_fps_capacity(void) { return FPS_CAPACITY; }

size_t cdx_fps_workspace(int64_t P, int64_t B, int32_t mode) {
  if (!fps_shape_ok(P, B)) return 0;
  const int path = fps_path(P, mode);
  if (path == 0) return 0;
  return path == 1 ? 256 : fps_layout(P, B).bytes;  // the one-workgroup path keeps everything on chip
}

int cdx_fps(const void* X, int32_t dtype, int64_t P, int64_t B, int64_t K, int64_t start, int32_t mode,
            void* workspace, int64_t* sel, double* radius, double* points, cdx_stream_t stream) {
  if (!X || !workspace || !fps_shape_ok(P, B) || K < 1 || K > P || start < 0 || start >= P) return CDX_EINVAL;
  if (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) return CDX_EINVAL;
  const int path = fps_path(P, mode);
  if (path == 0) return CDX_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (path == 1) {
    if (dtype == CDX_DTYPE_F32) block_dispatch<float>(X, (int)P, (int)B, (int)K, (int)start, sel, radius, points, s);
    else block_dispatch<double>(X, (int)P, (int)B, (int)K, (int)start, sel, radius, points, s);
  } else {
    const int rc = dtype == CDX_DTYPE_F32
                       ? round_dispatch<float>(X, (int)P, (int)B, (int)K, (int)start, workspace, sel, radius, points, s)
                       : round_dispatch<double>(X, (int)P, (int)B, (int)K, (int)start, workspace, sel, radius, points,
                                                s);
    if (rc) return rc;
  }
  return hipGetLastError() == hipSuccess ? CDX_OK : CDX_ELAUNCH;
}

}  // extern "C"
