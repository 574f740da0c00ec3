// Host (x86) build of the per-candidate device code in cdx_fk.h / cdx_cost.h / cdx_collision.h /
// cdx_sdf.h / cdx_gpis_mode.h / cdx_field.h / cdx_fps.h / cdx_mesh.h / cdx_sample.h / cdx_knn.h /
// cdx_wrench.h / cdx_hand.h / cdx_traj.h / cdx_equil.h.
//
// TEST-ONLY: libcdx_host.so lets the CPU test suite check the hand-derived backward
// (Kabsch/SVD, cost terms, FK) against the oracle's autograd without a GPU.  The
// product path never loads it; the Python package loads only the gfx950 libcdx.so.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "cdx_collision.h"
#include "cdx_cost.h"
#include "cdx_dyn.h"
#include "cdx_equil.h"
#include "cdx_field.h"
#include "cdx_fps.h"
#include "cdx_gpis_joint.h"
#include "cdx_gpis_mode.h"
#include "cdx_hand.h"
#include "cdx_ik.h"
#include "cdx_knn.h"
#include "cdx_mesh.h"
#include "cdx_ray.h"
#include "cdx_sample.h"
#include "cdx_sdf.h"
#include "cdx_traj.h"
#include "cdx_wrench.h"

namespace {

struct HostGpis {
  const double *mean, *gmean, *normal, *std_, *gstd;
  int64_t E, e;
  int T, Lq;
  cdx::GpisPoint operator()(int kind, int u, int f) const {
    cdx::GpisPoint p;
    int64_t qi;
    if (kind == 0) qi = cdx::q_alltip(u, e, f, E, T);
    else if (kind == 1) qi = cdx::q_target(Lq, e, f, E, T);
    else if (kind == 2) qi = cdx::q_pre(Lq, e, f, E, T);
    else qi = cdx::q_palm(Lq, e, E, T);
    memset(&p, 0, sizeof(p));
    p.mean = mean[qi];
    for (int i = 0; i < 3; ++i) p.gmean[i] = gmean[3 * qi + i];
    if (kind == 0) {
      p.std = std_[qi];
      for (int i = 0; i < 3; ++i) { p.gstd[i] = gstd[3 * qi + i]; p.normal[i] = normal[3 * qi + i]; }
    }
    return p;
  }
};

// GPIS.topcd (gpis.py:127-150) as a plain loop over the shared cell rule: the surface cells in C order of (i, j, k)
// (the order of numpy's boolean-mask indexing, :147-149), at most `capacity` rows written.
template <typename T>
int64_t surface_extract(const T* mean, const T* normal, int steps, int flip_k, const double* px, const double* py,
                        const double* pz, int64_t capacity, int64_t* cells, double* points, T* normals) {
  int64_t n = 0;
  for (int i = 1; i < steps - 1; ++i)
    for (int j = 1; j < steps - 1; ++j)
      for (int k = 1; k < steps - 1; ++k) {
        if (!cdx::field_surface_cell(mean, steps, i, j, k, flip_k)) continue;
        if (n < capacity) {
          if (cells) cells[n] = ((int64_t)i * steps + j) * steps + k;
          if (points) { points[3 * n] = px[j]; points[3 * n + 1] = py[i]; points[3 * n + 2] = pz[k]; }
          if (normal && normals) {
            const int64_t src = cdx::field_src(steps, i, j, k, flip_k);
            for (int d = 0; d < 3; ++d) normals[3 * n + d] = normal[3 * src + d];
          }
        }
        ++n;
      }
  return n;
}

// The rule of cdx_mesh.h as plain loops: the nodes in C order (vertices in ascending key order, each node's first
// vertex number kept), then the cubes in C order (their tetrahedra's triangles).  counts[0] = V, counts[1] = F; at most
// vcap / fcap rows are written.
template <typename T>
void mesh_extract(const T* mean, int steps, const double* px, const double* py, const double* pz, int64_t vcap,
                  int64_t fcap, double* vertices, int64_t* edges, int32_t* faces, int64_t* counts) {
  const int64_t total = (int64_t)steps * steps * steps;
  int64_t* base = new int64_t[total];
  int64_t V = 0, F = 0;
  for (int64_t c = 0; c < total; ++c) {
    int i, j, k;
    cdx::field_cell(c, steps, i, j, k);
    const int ex = cdx::mesh_exists(steps, i, j, k);
    const int cross = cdx::mesh_cross_mask(cdx::mesh_corner_bits(mean, steps, i, j, k, ex), ex);
    base[c] = V;
    for (int d = 0; d < 7; ++d) {
      if (!((cross >> d) & 1)) continue;
      if (V < vcap) {
        cdx::mesh_vertex(mean, steps, px, py, pz, i, j, k, d, vertices + 3 * V);
        if (edges) edges[V] = 7 * c + d;
      }
      ++V;
    }
  }
  const int gs = cdx::mesh_axes_sign(px[steps - 1] - px[0], py[steps - 1] - py[0], pz[steps - 1] - pz[0]);
  for (int i = 0; i < steps - 1; ++i)
    for (int j = 0; j < steps - 1; ++j)
      for (int k = 0; k < steps - 1; ++k) {
        const int bits = cdx::mesh_corner_bits(mean, steps, i, j, k, 0xff);
        for (int tet = 0; tet < 6; ++tet) {
          uint32_t tris;
          const int nt = cdx::mesh_tet_faces(cdx::mesh_tet_bits(tet, bits), cdx::mesh_tet_sign(tet) * gs, tris);
          for (int t = 0; t < nt; ++t, ++F) {
            if (F >= fcap) continue;
            for (int v = 0; v < 3; ++v) {
              int m, d;
              cdx::mesh_tet_edge_node(tet, (tris >> (4 * (3 * t + v))) & 15u, m, d);
              const int ni = i + (m & 1), nj = j + ((m >> 1) & 1), nk = k + ((m >> 2) & 1);
              faces[3 * F + v] = (int32_t)(base[cdx::field_src(steps, ni, nj, nk, 0)] +
                                           cdx::mesh_cross_below(mean, steps, ni, nj, nk, d));
            }
          }
        }
      }
  delete[] base;
  counts[0] = V;
  counts[1] = F;
}

// The sorted list of one query of cdx_knn.h: insertion of (d, i) into at most K pairs.
struct KnnHostList {
  double d[CDX_KNN_MAX_K];
  int64_t i[CDX_KNN_MAX_K];
  int n, K;
  double max_d2;
  void offer(double cd, int64_t ci) {
    if (cd > max_d2 || cd != cd) return;
    if (n == K && !cdx::knn_before(cd, ci, d[K - 1], i[K - 1])) return;
    int at = n < K ? n : K - 1;
    while (at > 0 && cdx::knn_before(cd, ci, d[at - 1], i[at - 1])) {
      d[at] = d[at - 1];
      i[at] = i[at - 1];
      --at;
    }
    d[at] = cd;
    i[at] = ci;
    if (n < K) ++n;
  }
};

// The grid of cdx_knn.h on the host: shape, cell of every row (−1 for a non-finite row) and the running extrema.
template <typename T>
void knn_grid_host(const T* X, int64_t P, cdx::KnnGrid& g, int32_t* cell, double* below, double* above) {
  const double inf = (double)INFINITY;
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  bool any = false;
  for (int64_t j = 0; j < P; ++j) {
    const double p[3] = {(double)X[3 * j], (double)X[3 * j + 1], (double)X[3 * j + 2]};
    if (!cdx::knn_finite3(p[0], p[1], p[2])) continue;
    any = true;
    for (int a = 0; a < 3; ++a) {
      lo[a] = p[a] < lo[a] ? p[a] : lo[a];
      hi[a] = p[a] > hi[a] ? p[a] : hi[a];
    }
  }
  const int n0 = cdx::knn_grid_n0(P);
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = any ? lo[a] : 0.0;
    hi[a] = any ? hi[a] : 0.0;
    const double e = hi[a] - g.lo[a];
    ext = e > ext ? e : ext;
  }
  g.inv = cdx::knn_grid_inv(ext, n0);
  for (int a = 0; a < 3; ++a) {
    const int n = cdx::knn_cell_raw(hi[a], g.lo[a], g.inv) + 1;
    g.n[a] = n < n0 ? n : n0;
  }
  g.pad = 0;
  for (int k = 0; k < 3 * CDX_KNN_MAX_DIM; ++k) {
    below[k] = -inf;
    above[k] = inf;
  }
  for (int64_t j = 0; j < P; ++j) {
    const double p[3] = {(double)X[3 * j], (double)X[3 * j + 1], (double)X[3 * j + 2]};
    const bool ok = cdx::knn_finite3(p[0], p[1], p[2]);
    for (int a = 0; a < 3; ++a) {
      if (!ok) {
        cell[3 * j + a] = -1;
        continue;
      }
      const int c = cdx::knn_cell(p[a], g.lo[a], g.inv, g.n[a]);
      cell[3 * j + a] = c;
      double& b = below[a * CDX_KNN_MAX_DIM + c];
      double& t = above[a * CDX_KNN_MAX_DIM + c];
      b = p[a] > b ? p[a] : b;
      t = p[a] < t ? p[a] : t;
    }
  }
  for (int a = 0; a < 3; ++a) {
    for (int c = 1; c < CDX_KNN_MAX_DIM; ++c) {
      double& b = below[a * CDX_KNN_MAX_DIM + c];
      const double pb = below[a * CDX_KNN_MAX_DIM + c - 1];
      b = pb > b ? pb : b;
    }
    for (int c = CDX_KNN_MAX_DIM - 2; c >= 0; --c) {
      double& t = above[a * CDX_KNN_MAX_DIM + c];
      const double pt = above[a * CDX_KNN_MAX_DIM + c + 1];
      t = pt < t ? pt : t;
    }
  }
}

template <typename T>
void knn_host(const T* X, int64_t P, const T* Q, int64_t M, int K, double max_d2, int mode, int64_t* idx, double* d2,
              int32_t* count) {
  cdx::KnnGrid g;
  std::vector<int32_t> cell;
  std::vector<double> below, above;
  std::vector<std::vector<int64_t>> rows;  // of every cell
  if (mode == CDX_KNN_GRID) {
    cell.resize(3 * P);
    below.resize(3 * CDX_KNN_MAX_DIM);
    above.resize(3 * CDX_KNN_MAX_DIM);
    knn_grid_host(X, P, g, cell.data(), below.data(), above.data());
    rows.resize((size_t)g.n[0] * g.n[1] * g.n[2]);
    for (int64_t j = 0; j < P; ++j)
      if (cell[3 * j] >= 0) rows[((size_t)cell[3 * j] * g.n[1] + cell[3 * j + 1]) * g.n[2] + cell[3 * j + 2]].push_back(j);
  }
  for (int64_t m = 0; m < M; ++m) {
    const double q[3] = {(double)Q[3 * m], (double)Q[3 * m + 1], (double)Q[3 * m + 2]};
    KnnHostList l;
    l.n = 0;
    l.K = K;
    l.max_d2 = max_d2;
    auto offer = [&](int64_t j) {
      const double x = (double)X[3 * j], y = (double)X[3 * j + 1], z = (double)X[3 * j + 2];
      if (cdx::knn_finite3(x, y, z)) l.offer(cdx::fps_sqdist(x, y, z, q[0], q[1], q[2]), j);
    };
    if (cdx::knn_finite3(q[0], q[1], q[2])) {
      if (mode != CDX_KNN_GRID) {
        for (int64_t j = 0; j < P; ++j) offer(j);
      } else {
        int cq[3];
        for (int a = 0; a < 3; ++a) cq[a] = cdx::knn_cell(q[a], g.lo[a], g.inv, g.n[a]);
        const int rings = std::max(g.n[0], std::max(g.n[1], g.n[2]));
        for (int r = 0; r < rings; ++r) {
          for (int x = std::max(cq[0] - r, 0); x <= std::min(cq[0] + r, g.n[0] - 1); ++x)
            for (int y = std::max(cq[1] - r, 0); y <= std::min(cq[1] + r, g.n[1] - 1); ++y)
              for (int z = std::max(cq[2] - r, 0); z <= std::min(cq[2] + r, g.n[2] - 1); ++z) {
                const int ch = std::max(std::abs(x - cq[0]), std::max(std::abs(y - cq[1]), std::abs(z - cq[2])));
                if (ch != r) continue;
                for (int64_t j : rows[((size_t)x * g.n[1] + y) * g.n[2] + z]) offer(j);
              }
          bool none;
          const double bound = cdx::knn_ring_bound(g, below.data(), above.data(), q, cq, r, &none);
          const double kth = l.n == K ? l.d[K - 1] : (double)INFINITY;
          if (none || bound > kth || bound > max_d2) break;
        }
      }
    }
    for (int t = 0; t < K; ++t) {
      idx[m * K + t] = t < l.n ? l.i[t] : -1;
      if (d2) d2[m * K + t] = t < l.n ? l.d[t] : (double)INFINITY;
    }
    if (count) count[m] = l.n;
  }
}

template <typename T>
void normals_host(const T* X, int64_t P, const int64_t* idx, const int32_t* count, int K, const double* eye,
                  double* normals, double* eigenvalues, double* cov) {
  for (int64_t row = 0; row < P; ++row) {
    int c = count[row];
    c = c < 0 ? 0 : (c > K ? K : c);
    const int64_t* list = idx + row * K;
    cdx::KnnMoments k;
    cdx::knn_moments_init(k);
    for (int t = 0; t < c; ++t) {
      const int64_t j = list[t];
      if (j < 0 || j >= P) {
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
    cdx::knn_normal_finish(k, c, p, eye != nullptr, eye, n, w, cov ? cov + 6 * row : nullptr);
    for (int a = 0; a < 3; ++a) {
      normals[3 * row + a] = n[a];
      if (eigenvalues) eigenvalues[3 * row + a] = w[a];
    }
  }
}

// The rule of cdx_fps.h as a plain single-threaded loop over one cloud.
template <typename T>
void fps_host(const T* X, int64_t P, int64_t K, int64_t start, int64_t* sel, double* radius, double* points) {
  double* dist = new double[P];
  for (int64_t j = 0; j < P; ++j) dist[j] = cdx::fps_init_dist(X[3 * j], X[3 * j + 1], X[3 * j + 2]);
  int64_t s = start;
  for (int64_t i = 0; i < K; ++i) {
    const double cx = X[3 * s], cy = X[3 * s + 1], cz = X[3 * s + 2];
    if (sel) sel[i] = s;
    if (radius) radius[i] = dist[s];
    if (points) { points[3 * i] = cx; points[3 * i + 1] = cy; points[3 * i + 2] = cz; }
    double bd = -3.0;  // below every dist
    int64_t bi = 0;
    for (int64_t j = 0; j < P; ++j) {
      dist[j] = cdx::fps_update(dist[j], cdx::fps_sqdist(X[3 * j], X[3 * j + 1], X[3 * j + 2], cx, cy, cz));
      if (cdx::fps_beats(dist[j], j, bd, bi)) { bd = dist[j]; bi = j; }
    }
    s = bi;
  }
  delete[] dist;
}

// cdxh_depth_unproject for one depth type D, z in Z: the full count; the first `capacity` points are written.
template <typename D, typename Z>
int64_t depth_unproject(const D* depth, int32_t W, int32_t H, int32_t stride, const double* intr, double scale,
                        double trunc, double z_max, const double* M, int64_t capacity, double* points) {
  int64_t n = 0;
  for (int i = 0; i < H; i += stride)
    for (int j = 0; j < W; j += stride) {
      double p[3];
      if (!cdx::depth_point<Z>((Z)depth[(int64_t)i * W + j], i, j, intr, scale, trunc, z_max, M, p)) continue;
      if (n < capacity) { points[3 * n] = p[0]; points[3 * n + 1] = p[1]; points[3 * n + 2] = p[2]; }
      ++n;
    }
  return n;
}

// The rows of an IK entry of variant V, one after the other in one row's storage: row(e, q0's row, storage) is the
// variant's solve of row e and returns its status.
template <class V, class ROW>
int ik_host_rows(const cdx_chain& c, int64_t E, const void* q0, int32_t q_dtype, uint32_t rot_mask, void* q,
                 int32_t* status, ROW&& row) {
  const int T = c.n_tips, D = c.n_dofs, f64 = q_dtype == CDX_DTYPE_F64;
  std::vector<double> mem((cdx::ik_mem_bytes<V>(T, D, rot_mask) + 7) / 8);
  const cdx::IkMem m = cdx::ik_mem_at<V>(mem.data(), T, D, rot_mask, 0, 1);
  for (int64_t e = 0; e < E; ++e) {
    const int st = row(e, cdx::ik_q0_row(q0, f64, e, D), m);
    cdx::ik_store_q(q, q0, f64, e, D, st, m);
    status[e] = st;
  }
  return CDX_OK;
}

}  // namespace

// Host build of cdx_gpis_joint (same arguments without the workspace and the stream; the descriptor's X1 and Linv_t are
// host pointers, Linv_t the caller's own factor): the rule of cdx_gpis_joint.h as plain loops, the columns in their
// order in one sum.  tests/test_joint_cpu.py checks it against a numpy statement of Σ.
template <int KT>
static void host_gpis_joint(const cdx_gpis& g, const double* X, int64_t M, double* cov) {
  const double R = g.R, inv_s2 = 1.0 / (g.sigma * g.sigma);
  std::vector<double> b((size_t)g.N * 4);
  for (int64_t m = 0; m < M; ++m) {
    const double* x = X + 3 * m;
    for (int j = 0; j < g.N; ++j) {
      const double* xj = g.X1 + 3 * (int64_t)j;
      for (int c = 0; c < 4; ++c)
        b[(size_t)j * 4 + c] = cdx::gpis_joint_entry<KT>(x[0] - xj[0], x[1] - xj[1], x[2] - xj[2], c, R, inv_s2);
    }
    double gram[cdx::JOINT_OUT] = {};
    for (int n = 0; n < g.N; ++n) {
      double w[4] = {0.0, 0.0, 0.0, 0.0};
      for (int j = 0; j <= n; ++j) {  // L⁻ᵀ is upper triangular
        const double l = g.Linv_t[(int64_t)j * g.N_pad + n];
        for (int c = 0; c < 4; ++c) w[c] = fma(l, b[(size_t)j * 4 + c], w[c]);
      }
      cdx::gpis_joint_gram(w, gram);
    }
    for (int e = 0; e < cdx::JOINT_OUT; ++e) cov[m * cdx::JOINT_OUT + e] = cdx::gpis_joint_prior<KT>(e, R, inv_s2) - gram[e];
  }
}

extern "C" {

// (the chain checks of the device entries: a malformed or over-deep chain → CDX_ECHAIN, nothing written)
int cdxh_fk_forward(const cdx_chain* c, const float* q, int64_t B, float* pos, float* quat) {
  if (!cdx::chain_ok(c)) return CDX_ECHAIN;
  for (int64_t b = 0; b < B; ++b)
    for (int k = 0; k < c->n_tips; ++k)
      cdx::fk_tip(*c, k, q + b * c->n_dofs, pos + (b * c->n_tips + k) * 3, quat ? quat + (b * c->n_tips + k) * 4 : nullptr);
  return CDX_OK;
}

int cdxh_fk_backward(const cdx_chain* c, const float* q, int64_t B, const float* gpos, float* gq) {
  if (!cdx::chain_ok(c)) return CDX_ECHAIN;
  for (int64_t b = 0; b < B; ++b) {
    float* g = gq + b * c->n_dofs;
    for (int i = 0; i < c->n_dofs; ++i) g[i] = 0.f;
    for (int k = 0; k < c->n_tips; ++k) cdx::fk_tip_bwd(*c, k, q + b * c->n_dofs, gpos + (b * c->n_tips + k) * 3, cdx::GqAdd{g});
  }
  return CDX_OK;
}

// Geometric fingertip Jacobians and the batched IK solve (cdx_ik.h), with the device entries' argument checks.
int cdxh_fk_jacobian(const cdx_chain* c, const float* q, int64_t B, float* lin, float* ang) {
  const int rc = cdx::chain_code(c);
  if (rc) return rc;
  if (B < 0) return CDX_EINVAL;
  if (B == 0) return CDX_OK;
  if (!q || !lin) return CDX_ECHAIN;
  const int T = c->n_tips, D = c->n_dofs;
  for (int64_t t = 0; t < B * T; ++t)
    cdx::fk_jacobian_tip(*c, (int)(t % T), q + (t / T) * D, lin + t * 3 * D, ang ? ang + t * 3 * D : nullptr);
  return CDX_OK;
}

int cdxh_ik_solve(const cdx_chain* c, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                  const double* target, const double* palm, const double* palm_offset, const double* w, void* q,
                  double* err, int32_t* iters, int32_t* status) {
  cdx_ik_params p;
  double po[3];
  int rc = cdx::ik_call_code(c, params, E, q_dtype, &p);
  if (rc || E == 0) return rc;
  if (!q0 || !target || !q || !err || !iters || !status) return CDX_ECHAIN;
  rc = cdx::ik_offset_code(palm_offset, po);
  if (rc) return rc;
  const int T = c->n_tips;
  return ik_host_rows<cdx::IkFixed>(*c, E, q0, q_dtype, 0, q, status,
                                    [&](int64_t e, const cdx::Q0Row& q0r, const cdx::IkMem& m) {
    return cdx::ik_row(*c, p, po, q0r, target + e * T * 3, palm ? palm + e * 6 : nullptr, w ? w + e * T : nullptr, m,
                       err + e * T, iters + e);
  });
}

// The free-wrist solve (ik_pose_row), with cdx_ik_solve_pose's argument checks.
int cdxh_ik_solve_pose(const cdx_chain* c, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                       const double* target, const double* palm0_pos, const double* palm0_rot, const double* palm_offset,
                       const double* w, void* q, double* palm_pos, double* palm_rot, double* err, int32_t* iters,
                       int32_t* status) {
  cdx_ik_params p;
  double po[3];
  int rc = cdx::ik_call_code(c, params, E, q_dtype, &p);
  if (rc || E == 0) return rc;
  if (!q0 || !target || !q || !palm_pos || !palm_rot || !err || !iters || !status) return CDX_ECHAIN;
  if (!palm0_pos != !palm0_rot) return CDX_ECHAIN;
  rc = cdx::ik_offset_code(palm_offset, po);
  if (rc) return rc;
  const int T = c->n_tips;
  return ik_host_rows<cdx::IkPose>(*c, E, q0, q_dtype, 0, q, status,
                                   [&](int64_t e, const cdx::Q0Row& q0r, const cdx::IkMem& m) {
    return cdx::ik_pose_row(*c, p, po, q0r, target + e * T * 3, palm0_pos ? palm0_pos + e * 3 : nullptr,
                            palm0_rot ? palm0_rot + e * 9 : nullptr, w ? w + e * T : nullptr, m, palm_pos + e * 3,
                            palm_rot + e * 9, err + e * T, iters + e);
  });
}

// The pose-target solve (frame_ik_row), with cdx_ik_solve_frames' argument checks.  device_trig = 0: the FK's sines
// are this build's (the row is cdxh_ik_solve's bit for bit without the additions); 1: the device's definition of them
// (cdx_hd.h), with which the kernel is held to this build bit for bit.
int cdxh_ik_solve_frames(const cdx_chain* c, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                         const double* target_pos, const double* target_rot, const double* palm,
                         const double* palm_offset, const double* w, const double* wr, uint64_t rot_mask64,
                         uint64_t dof_mask64, void* q, double* err, double* rot_err, int32_t* iters, int32_t* status,
                         int32_t device_trig) {
  const cdx::HostDeviceTrig trig(device_trig ? 1 : 0);
  cdx_ik_params p;
  double po[3];
  int rc = cdx::ik_call_code(c, params, E, q_dtype, &p);
  if (rc) return rc;
  const int T = c->n_tips, D = c->n_dofs;
  rc = cdx::ik_frames_mask_code(T, D, rot_mask64, dof_mask64);
  if (rc) return rc;
  const uint32_t rot_mask = (uint32_t)rot_mask64, dof_mask = (uint32_t)dof_mask64;
  if (cdx::ik_mem_bytes<cdx::IkFrames>(T, D, rot_mask) > 65536) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!q0 || !target_pos || !q || !err || !rot_err || !iters || !status || (rot_mask && !target_rot)) return CDX_ECHAIN;
  rc = cdx::ik_offset_code(palm_offset, po);
  if (rc) return rc;
  return ik_host_rows<cdx::IkFrames>(*c, E, q0, q_dtype, rot_mask, q, status,
                                     [&](int64_t e, const cdx::Q0Row& q0r, const cdx::IkMem& m) {
    return cdx::frame_ik_row(*c, p, po, q0r, target_pos + e * T * 3, target_rot ? target_rot + e * T * 9 : nullptr,
                             palm ? palm + e * 6 : nullptr, w ? w + e * T : nullptr, wr ? wr + e * T : nullptr, rot_mask,
                             dof_mask, m, err + e * T, rot_err + e * T, iters + e);
  });
}

// Rigid-body dynamics (cdx_dyn.h) row by row, with the device entries' argument checks; every pointer is host memory.
int cdxh_dyn_inverse(const cdx_chain* c, const cdx_dyn* dyn, int64_t B, const void* q, const void* qd, const void* qdd,
                     int32_t dtype, int32_t include_gravity, int32_t use_damping, const double* gravity,
                     int32_t gravity_per_row, const double* tip_forces, void* tau) {
  const int rc = cdx::dyn_chain_code(c, dyn);
  if (rc) return rc;
  if (B < 0 || (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64)) return CDX_EINVAL;
  if (B == 0) return CDX_OK;
  if (!q || !tau) return CDX_ECHAIN;
  const int n = c->n_bodies, D = c->n_dofs, T = c->n_tips, f64 = dtype == CDX_DTYPE_F64;
  std::vector<double> mem((cdx::dyn_mem_bytes(n, D, 0) + 7) / 8);
  const cdx::DynMem m = cdx::dyn_mem_at(mem.data(), n, D, 0, 0, 1);
  const size_t w = f64 ? 8 : 4;
  for (int64_t e = 0; e < B; ++e) {
    double g[3];
    cdx::dyn_gravity(include_gravity != 0, gravity ? gravity + (gravity_per_row ? e * 3 : 0) : nullptr, g);
    const size_t off = (size_t)e * D * w;
    cdx::dyn_inverse_row(*c, *dyn, m, cdx::DynVec{(const char*)q + off, f64},
                         cdx::DynVec{qd ? (const char*)qd + off : nullptr, f64},
                         cdx::DynVec{qdd ? (const char*)qdd + off : nullptr, f64}, g, use_damping != 0,
                         tip_forces && T > 0 ? tip_forces + e * T * 3 : nullptr, cdx::DynOut{(char*)tau + off, f64});
  }
  return CDX_OK;
}

int cdxh_dyn_inertia(const cdx_chain* c, const cdx_dyn* dyn, int64_t B, const void* q, int32_t dtype, void* H) {
  const int rc = cdx::dyn_chain_code(c, dyn);
  if (rc) return rc;
  if (B < 0 || (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64)) return CDX_EINVAL;
  if (B == 0) return CDX_OK;
  if (!q || !H) return CDX_ECHAIN;
  const int n = c->n_bodies, D = c->n_dofs, f64 = dtype == CDX_DTYPE_F64;
  std::vector<double> mem((cdx::dyn_mem_bytes(n, D, 0) + 7) / 8);
  const cdx::DynMem m = cdx::dyn_mem_at(mem.data(), n, D, 0, 0, 1);
  const size_t w = f64 ? 8 : 4;
  for (int64_t e = 0; e < B; ++e)
    cdx::dyn_inertia_row(*c, *dyn, m, cdx::DynVec{(const char*)q + (size_t)e * D * w, f64},
                         cdx::DynOut{(char*)H + (size_t)e * D * D * w, f64});
  return CDX_OK;
}

int cdxh_dyn_forward(const cdx_chain* c, const cdx_dyn* dyn, int64_t B, const void* q, const void* qd, const void* f,
                     int32_t dtype, int32_t include_gravity, int32_t use_damping, const double* gravity,
                     int32_t gravity_per_row, void* qdd) {
  const int rc = cdx::dyn_chain_code(c, dyn);
  if (rc) return rc;
  if (B < 0 || (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64)) return CDX_EINVAL;
  if (cdx::dyn_has_dead_joint(*c)) return CDX_EINVAL;
  if (B == 0) return CDX_OK;
  if (!q || !f || !qdd) return CDX_ECHAIN;
  const int n = c->n_bodies, D = c->n_dofs, f64 = dtype == CDX_DTYPE_F64;
  std::vector<double> mem((cdx::dyn_mem_bytes(n, D, 1) + 7) / 8);
  const cdx::DynMem m = cdx::dyn_mem_at(mem.data(), n, D, 1, 0, 1);
  const size_t w = f64 ? 8 : 4;
  for (int64_t e = 0; e < B; ++e) {
    double g[3];
    cdx::dyn_gravity(include_gravity != 0, gravity ? gravity + (gravity_per_row ? e * 3 : 0) : nullptr, g);
    const size_t off = (size_t)e * D * w;
    cdx::dyn_forward_row(*c, *dyn, m, cdx::DynVec{(const char*)q + off, f64},
                         cdx::DynVec{qd ? (const char*)qd + off : nullptr, f64}, cdx::DynVec{(const char*)f + off, f64}, g,
                         use_damping != 0, cdx::DynOut{(char*)qdd + off, f64});
  }
  return CDX_OK;
}

// The minimum-wrench solve (cdx_wrench.h) row by row, with the device entry's argument checks.
int cdxh_min_wrench(const cdx_wrench_params* params, int64_t E, const double* tips, const double* normals,
                    double* forces, double* wrench, double* margin, double* dual, double* gap, int32_t* iters,
                    int32_t* status, double* grad_tips) {
  const int rc = cdx::wr_params_code(params);
  if (rc) return rc;
  if (E < 0) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!tips || !normals || !forces || !wrench || !margin || !dual || !gap || !iters || !status) return CDX_EINVAL;
  const int T = params->n_tips;
  std::vector<double> mem(cdx::wr_mem_doubles(T));
  const cdx::WrMem m = cdx::wr_mem_at(mem.data(), T, 0, 1);
  for (int64_t e = 0; e < E; ++e)
    status[e] = cdx::mw_row(*params, tips + e * T * 3, normals + e * T * 3, m, forces + e * T * 3, wrench + e,
                            margin + e * T, dual + e * 6, gap + e, iters + e, grad_tips ? grad_tips + e * T * 3 : nullptr);
  return CDX_OK;
}

// The disturbance-load test (cdx_equil.h) item by item and its reduction row by row, with the device entries' argument
// checks.
int cdxh_grasp_equilibrium(const cdx_equil_params* params, int64_t E, int64_t W, const double* contact,
                           const double* target, const double* stiffness, const double* normal,
                           const double* load_force, const double* load_point, int32_t loads_shared, double* rot,
                           double* trans, double* force, double* normal_force, double* margin, double* shift,
                           double* chord, uint8_t* stable, int32_t* iters, int32_t* status) {
  const int rc = cdx::eq_params_code(params);
  if (rc) return rc;
  if (E < 0 || W < 0) return CDX_EINVAL;
  if (E == 0 || W == 0) return CDX_OK;
  if (!contact || !target || !stiffness || !normal || !load_force || !load_point || !normal_force || !margin ||
      !shift || !chord || !stable || !iters || !status)
    return CDX_EINVAL;
  if (E > 0x7fffffff / W || E * W > 0x7fffffff / params->n_tips) return CDX_EINVAL;
  const int T = params->n_tips;
  for (int64_t e = 0; e < E; ++e) {
    cdx::EqRow row;
    const bool ok = cdx::eq_row_prepare(T, contact + e * T * 3, target + e * T * 3, stiffness + e * T, normal + e * T * 3, &row);
    for (int64_t w = 0; w < W; ++w) {
      const int64_t item = e * W + w, l = loads_shared ? w : item;
      status[item] = cdx::equil_row(*params, row, ok, normal + e * T * 3, load_force + l * 3, load_point + l * 3,
                                    rot ? rot + item * 9 : nullptr, trans ? trans + item * 3 : nullptr,
                                    force ? force + item * T * 3 : nullptr, normal_force + item * T, margin + item * T,
                                    shift + item, chord + item, stable + item, iters + item);
    }
  }
  return CDX_OK;
}

int cdxh_equil_reduce(const cdx_equil_limits* limits, int64_t E, int64_t W, int32_t n_tips, const double* margin,
                      const double* normal_force, const double* shift, const double* chord, const uint8_t* stable,
                      const int32_t* status, double* worst_margin, int32_t* worst_load, int32_t* worst_tip,
                      double* max_shift, double* max_chord, int32_t* n_failed, uint8_t* holds) {
  if (!limits || E < 0 || W < 0 || W > 0x7fffffff || n_tips < 1 || n_tips > CDX_MAX_TIPS) return CDX_EINVAL;
  if (E == 0 || W == 0) return CDX_OK;
  if (!margin || !normal_force || !shift || !chord || !stable || !status || !worst_margin || !worst_load ||
      !worst_tip || !max_shift || !max_chord || !n_failed || !holds)
    return CDX_EINVAL;
  for (int64_t e = 0; e < E; ++e) {
    const int64_t at = e * W;
    cdx::equil_reduce_row(W, n_tips, margin + at * n_tips, normal_force + at * n_tips, shift + at, chord + at,
                          stable + at, status + at, *limits, worst_margin + e, worst_load + e, worst_tip + e,
                          max_shift + e, max_chord + e, n_failed + e, holds + e);
  }
  return CDX_OK;
}

// The whole-hand sphere model (cdx_hand.h) row by row, with the device entries' argument checks; the tables of
// cdxh_hand_prepare live in HOST memory (cdx::hand_bytes(S, P) bytes).
int cdxh_hand_prepare(int32_t n_bodies, int32_t S, const float* local, const double* radius, const int32_t* body,
                      int32_t P, const int32_t* pairs, void* tables, cdx_hand* out) {
  if (!cdx::hand_bytes(S, P) || !tables || !out) return CDX_EINVAL;
  return cdx::hand_fill(n_bodies, S, local, radius, body, P, pairs, static_cast<char*>(tables), out);
}

int cdxh_hand_spheres(const cdx_chain* c, const cdx_hand* h, int64_t E, const double* q, const double* pp,
                      const double* po, float* poses, double* centers) {
  int rc = cdx::hand_chain_code(c);
  if (rc) return rc;
  rc = cdx::hand_code(h);
  if (rc) return rc;
  if (h->n_bodies != c->n_bodies || E < 0) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if ((!q && c->n_dofs > 0) || !poses || !centers) return CDX_EINVAL;
  const int64_t nb = c->n_bodies, S = h->n_spheres;
  for (int64_t e = 0; e < E; ++e)
    cdx::hand_spheres_row(*c, *h, q + e * c->n_dofs, pp ? pp + 3 * e : nullptr, po ? po + 3 * e : nullptr,
                          poses + e * nb * 12, centers + e * S * 3);
  return CDX_OK;
}

int cdxh_hand_cost(const cdx_hand* h, const cdx_hand_params* p, int64_t E, const double* centers, const double* dist,
                   const double* gdist, double* cost, double* depth, int32_t* worst, double* g_centers) {
  int rc = cdx::hand_code(h);
  if (rc) return rc;
  rc = cdx::hand_params_code(p);
  if (rc) return rc;
  if (E < 0 || E > 0x7fffffff || (dist == nullptr) != (gdist == nullptr)) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!centers || !cost || !depth || !worst || !g_centers) return CDX_EINVAL;
  const int64_t S = h->n_spheres;
  for (int64_t e = 0; e < E; ++e)
    cdx::hand_cost_row(*h, *p, centers + e * S * 3, dist ? dist + e * S : nullptr, gdist ? gdist + e * S * 3 : nullptr,
                       cost + e, depth + 3 * e, worst + 3 * e, g_centers + e * S * 3);
  return CDX_OK;
}

int cdxh_hand_pullback(const cdx_chain* c, const cdx_hand* h, int64_t E, const float* poses, const double* g_centers,
                       const double* po, double* g_q, double* g_pp, double* g_po) {
  int rc = cdx::hand_chain_code(c);
  if (rc) return rc;
  rc = cdx::hand_code(h);
  if (rc) return rc;
  if (h->n_bodies != c->n_bodies || E < 0 || E > 0x7fffffff) return CDX_EINVAL;
  if (E == 0) return CDX_OK;
  if (!poses || !g_centers || (!g_q && c->n_dofs > 0) || !g_pp || !g_po) return CDX_EINVAL;
  const int64_t nb = c->n_bodies, S = h->n_spheres;
  for (int64_t e = 0; e < E; ++e)
    cdx::hand_pullback_row(*c, *h, poses + e * nb * 12, g_centers + e * S * 3, po ? po + 3 * e : nullptr,
                           g_q + e * c->n_dofs, g_pp + 3 * e, g_po + 3 * e);
  return CDX_OK;
}

int cdxh_hand_term(const cdx_chain* c, const cdx_hand* h, const cdx_hand_params* p, int64_t E, const float* poses,
                   const double* centers, const double* dist, const double* gdist, const double* po, double weight,
                   int32_t accumulate, double* loss, double* g_q, double* g_pp, double* g_po, double* depth,
                   int32_t* worst) {
  int rc = cdx::hand_chain_code(c);
  if (rc) return rc;
  rc = cdx::hand_code(h);
  if (rc) return rc;
  rc = cdx::hand_params_code(p);
  if (rc) return rc;
  rc = cdx::hand_term_code(c, h, E, poses, centers, dist, gdist, weight, accumulate, loss, g_q);
  if (rc || E == 0) return rc;
  const int64_t nb = c->n_bodies, S = h->n_spheres, D = c->n_dofs;
  for (int64_t e = 0; e < E; ++e)
    cdx::hand_term_row(*c, *h, *p, poses + e * nb * 12, centers + e * S * 3, dist ? dist + e * S : nullptr,
                       gdist ? gdist + e * S * 3 : nullptr, po ? po + 3 * e : nullptr, weight, accumulate != 0, loss + e,
                       g_q ? g_q + e * D : nullptr, g_pp ? g_pp + 3 * e : nullptr, g_po ? g_po + 3 * e : nullptr,
                       depth ? depth + 3 * e : nullptr, worst ? worst + 3 * e : nullptr);
  return CDX_OK;
}

size_t cdxh_hand_bytes(int32_t S, int32_t P) { return cdx::hand_bytes(S, P); }

// cdx::hand_sincos on n angles.
void cdxh_hand_sincos(const double* x, int64_t n, double* s, double* c) {
  for (int64_t i = 0; i < n; ++i) cdx::hand_sincos(x[i], s + i, c + i);
}

// The trajectory rule (cdx_traj.h) row by row, with the device entries' argument checks.
int cdxh_traj_seed(int64_t G, int32_t seeds, int32_t T, int32_t n_dofs, const double* q_start, const double* q_goal,
                   double amp, uint64_t seed, double* traj) {
  const int rc = cdx::traj_seed_code(G, seeds, T, n_dofs, q_start, q_goal, amp, traj);
  if (rc || G == 0) return rc;
  for (int64_t row = 0; row < G * seeds; ++row) {
    const int64_t g = row / seeds;
    cdx::traj_seed_row(row, (int32_t)(row - g * seeds), T, n_dofs, q_start + g * n_dofs, q_goal + g * n_dofs, amp, seed,
                       traj + row * T * n_dofs);
  }
  return CDX_OK;
}

int cdxh_traj_step(const cdx_traj_params* p, int64_t E, double* traj, const double* g_c, const double* cost_t,
                   int32_t iteration, double* cost, double* best_cost, int32_t* best_iter, double* best_traj) {
  const int rc = cdx::traj_step_code(p, E, traj, g_c, cost_t, cost, best_cost, best_iter, best_traj);
  if (rc || E == 0) return rc;
  cdx::TrajFactor F;
  cdx::traj_factor(p->T - 2, &F);
  const int64_t n = (int64_t)p->T * p->n_dofs;
  for (int64_t e = 0; e < E; ++e)
    cdx::traj_step_row(*p, F, traj + e * n, g_c ? g_c + e * n : nullptr, cost_t ? cost_t + e * p->T : nullptr, iteration,
                       cost + 3 * e, best_cost + e, best_iter + e, best_traj + e * n);
  return CDX_OK;
}

// The gradient g of cdx_traj.h alone (the step's first half): g [E*T*n_dofs], its two endpoint rows 0.
int cdxh_traj_gradient(const cdx_traj_params* p, int64_t E, const double* traj, const double* g_c, double* g) {
  if (cdx::traj_params_code(p) || E < 0 || !traj || !g) return CDX_EINVAL;
  const int T = p->T, D = p->n_dofs;
  for (int64_t e = 0; e < E; ++e) {
    double* x = g + e * T * D;
    for (int i = 0; i < T * D; ++i) x[i] = g_c ? g_c[e * T * D + i] : 0.0;
    double us, ul;
    for (int d = 0; d < D; ++d) {
      cdx::traj_gradient_column(*p, d, traj + e * T * D, x, &us, &ul);
      x[d] = x[(T - 1) * D + d] = 0.0;
    }
  }
  return CDX_OK;
}

int64_t cdxh_n_queries(const cdx_problem* P, int64_t E) { return cdx::n_queries(*P, E); }

int cdxh_closure_queries(const cdx_problem* P, int64_t E, const double* q, const double* target, const double* palm_pos,
                         const double* palm_ori, double* X) {
  if (!P || !cdx::chain_ok(&P->chain)) return CDX_ECHAIN;
  const int T = P->chain.n_tips, D = P->chain.n_dofs, Lq = P->n_query_levels;
  for (int64_t e = 0; e < E; ++e) {
    double tip[CDX_MAX_TIPS][3], Rp[9];
    float tl[CDX_MAX_TIPS][3];
    cdx::pregrasp_tips(*P, q + e * D, palm_pos + 3 * e, palm_ori + 3 * e, tip, tl, Rp);
    const double* tg = target + e * T * 3;
    for (int u = 0; u < Lq; ++u) {
      int k = 0;
      while (k < P->n_levels - 1 && P->level_query[k] != u) ++k;
      for (int f = 0; f < T; ++f) {
        const double c = (double)P->coeff[k][f];
        const int64_t qi = cdx::q_alltip(u, e, f, E, T);
        for (int i = 0; i < 3; ++i) X[3 * qi + i] = tg[3 * f + i] + c * (tip[f][i] - tg[3 * f + i]);
      }
    }
    for (int f = 0; f < T; ++f)
      for (int i = 0; i < 3; ++i) {
        X[3 * cdx::q_target(Lq, e, f, E, T) + i] = tg[3 * f + i];
        X[3 * cdx::q_pre(Lq, e, f, E, T) + i] = tip[f][i];
      }
    if (P->optimize_palm)
      for (int i = 0; i < 3; ++i) X[3 * cdx::q_palm(Lq, e, E, T) + i] = palm_pos[3 * e + i];
  }
  return CDX_OK;
}

int cdxh_closure_cost(const cdx_problem* P, int64_t E, const double* q, const double* comp, const double* target,
                      const double* palm_pos, const double* palm_ori, const double* noise, const double* mean,
                      const double* gmean, const double* normal, const double* std_, const double* gstd,
                      double* total_loss, double* total_margin, double* g_q, double* g_comp, double* g_target,
                      double* g_palm_pos, double* g_palm_ori, int32_t* flip) {
  if (!P || !cdx::chain_ok(&P->chain)) return CDX_ECHAIN;
  const int T = P->chain.n_tips, D = P->chain.n_dofs;
  HostGpis g{mean, gmean, normal, std_, gstd, E, 0, T, P->n_query_levels};
  for (int64_t e = 0; e < E; ++e) {
    cdx::CandidateIn in;
    in.q = q + e * D;
    in.comp = comp + e * T;
    in.target = target + e * T * 3;
    in.palm_pos = palm_pos + 3 * e;
    in.palm_ori = palm_ori + 3 * e;
    in.noise = noise + e * 9;
    in.noise_stride = E * 9;
    g.e = e;
    cdx::CandidateOut out;
    cdx::closure_candidate(*P, in, g, out);
    total_loss[e] = out.loss;
    for (int f = 0; f < T; ++f) {
      total_margin[e * T + f] = out.margin[f];
      g_comp[e * T + f] = out.g_comp[f];
      for (int i = 0; i < 3; ++i) g_target[(e * T + f) * 3 + i] = out.g_target[f][i];
    }
    for (int i = 0; i < D; ++i) g_q[e * D + i] = out.g_q[i];
    for (int i = 0; i < 3; ++i) { g_palm_pos[3 * e + i] = out.g_palm_pos[i]; g_palm_ori[3 * e + i] = out.g_palm_ori[i]; }
    for (int k = 0; k < P->n_levels; ++k) flip[k * E + e] = out.flip[k];
  }
  return CDX_OK;
}

int cdxh_collision(const cdx_collision* C, int64_t E, const double* q, const double* pp, const double* po,
                   double* cost, double* g_q, double* g_pp, double* g_po) {
  if (!C || !cdx::chain_ok(&C->chain)) return CDX_ECHAIN;
  const int D = C->chain.n_dofs;
  for (int64_t e = 0; e < E; ++e)
    cdx::collision_candidate(*C, q + e * D, pp + 3 * e, po + 3 * e, cost[e], g_q + e * D, g_pp + 3 * e, g_po + 3 * e);
  return CDX_OK;
}

void cdxh_force_eq(const cdx_force_eq* p, int64_t B, const double* tip, const double* target, const double* comp,
                   const double* normal, const double* noise, const double* g_reward, const double* g_fn,
                   double* reward, double* margin, double* fn, int32_t* flip, double* g_tip, double* g_target,
                   double* g_comp) {
  cdx::ForceEqParams fp;
  fp.cos_mu = (double)p->cos_mu;
  fp.gravity = p->gravity;
  for (int i = 0; i < 3; ++i) fp.com[i] = (double)p->com[i];
  fp.dummy_target_z = (double)p->dummy_target_z;
  fp.dummy_comp = (double)p->dummy_comp;
  const int T = p->n_tips;
  for (int64_t b = 0; b < B; ++b) {
    double tp[CDX_MAX_TIPS][3], nr[CDX_MAX_TIPS][3];
    for (int f = 0; f < T; ++f)
      for (int i = 0; i < 3; ++i) { tp[f][i] = tip[(b * T + f) * 3 + i]; nr[f][i] = normal[(b * T + f) * 3 + i]; }
    cdx::ForceEq<0> fe;
    fe.forward(fp, T, tp, target + b * T * 3, comp + b * T, nr, noise + b * 9);
    reward[b] = fe.reward;
    flip[b] = fe.flip;
    double gt[CDX_MAX_TIPS][3] = {}, gg[CDX_MAX_TIPS][3] = {}, gc[CDX_MAX_TIPS] = {};
    for (int f = 0; f < T; ++f) { margin[b * T + f] = fe.margin[f]; fn[b * T + f] = fe.fn[f]; }
    fe.backward(g_reward[b], g_fn + b * T, comp + b * T, gt, gg, gc);
    for (int f = 0; f < T; ++f) {
      for (int i = 0; i < 3; ++i) { g_tip[(b * T + f) * 3 + i] = gt[f][i]; g_target[(b * T + f) * 3 + i] = gg[f][i]; }
      g_comp[b * T + f] = gc[f];
    }
  }
}

// The GPIS-mode optimiser iteration (cdx_gpis_mode_cost / cdx_gpis_mode_step) over a batch of host arrays: the same
// per-candidate code, the same argument checks, the `any` flags kept as the device keeps them.
int cdxh_gpis_mode_cost(const cdx_chain* chain, const cdx_gpis_mode_params* p, const cdx_gpis_mode_buffers* buf,
                        int64_t E, int32_t n_tips, const double* noise, uint64_t seed, int32_t iteration) {
  if (cdx::gpis_mode_check(chain, p, E, n_tips) || iteration < 0) return CDX_EINVAL;
  if (cdx::gpis_mode_check_chain(chain, p)) return CDX_ECHAIN;
  if (E == 0) return CDX_OK;
  if (cdx::gpis_mode_check_cost(p, buf)) return CDX_EINVAL;
  const cdx_gpis_mode_buffers& b = *buf;
  const int slot = iteration & 1;
  const bool fk = p->mode == 1;
  const bool shallow = fk && cdx::chain_max_depth(*chain) <= 8;
  const cdx_chain none{};
  float fk_g[CDX_MAX_DOFS];
  for (int64_t e = 0; e < E; ++e) {
    if (fk && shallow)  // (the depth bound the device picks: it selects the FK backward's form)
      cdx::gpis_mode_cost_candidate<0, 8, true>(
          *chain, *p, n_tips, e, b.pose, b.tips, b.target, b.comp, noise, seed, b.mean, b.gmean, b.normal, b.std, b.gstd,
          b.tmean, b.tgmean, b.loss, b.margin[slot], b.normal_slot[slot], b.g_pose, b.g_target, b.g_comp, b.g_tip, fk_g, 1);
    else if (fk)
      cdx::gpis_mode_cost_candidate<0, CDX_MAX_DEPTH, true>(
          *chain, *p, n_tips, e, b.pose, b.tips, b.target, b.comp, noise, seed, b.mean, b.gmean, b.normal, b.std, b.gstd,
          b.tmean, b.tgmean, b.loss, b.margin[slot], b.normal_slot[slot], b.g_pose, b.g_target, b.g_comp, b.g_tip, fk_g, 1);
    else
      cdx::gpis_mode_cost_candidate<0, CDX_MAX_DEPTH, false>(
          none, *p, n_tips, e, nullptr, b.pose, b.target, b.comp, noise, seed, b.mean, b.gmean, b.normal, b.std, b.gstd,
          b.tmean, b.tgmean, b.loss, b.margin[slot], b.normal_slot[slot], nullptr, b.g_target, b.g_comp, b.g_pose, fk_g, 1);
  }
  return CDX_OK;
}

int cdxh_gpis_mode_step(const cdx_chain* chain, const cdx_gpis_mode_params* p, const cdx_gpis_mode_opt* opt,
                        const cdx_gpis_mode_buffers* buf, int64_t E, int32_t n_tips, int32_t iteration,
                        int32_t finalize) {
  if (cdx::gpis_mode_check(chain, p, E, n_tips) || !opt) return CDX_EINVAL;
  if (cdx::gpis_mode_check_chain(chain, p)) return CDX_ECHAIN;
  if (E == 0) return CDX_OK;
  if (cdx::gpis_mode_check_step(opt, buf, iteration, finalize)) return CDX_EINVAL;
  const cdx_gpis_mode_buffers& b = *buf;
  const int s = iteration;
  const cdx_chain none{};
  if (s > 0 && b.any[(s - 1) % 3])
    for (int64_t e = 0; e < E; ++e) cdx::gpis_mode_commit(b, n_tips, e, (s - 1) & 1);
  if (finalize) return CDX_OK;
  b.any[(s + 1) % 3] = 0u;
  for (int64_t e = 0; e < E; ++e) {
    const bool flag = p->mode == 1 ? cdx::gpis_mode_step_candidate<true>(*chain, *p, *opt, b, n_tips, e)
                                   : cdx::gpis_mode_step_candidate<false>(none, *p, *opt, b, n_tips, e);
    if (flag) b.any[s % 3] |= 1u;
  }
  return CDX_OK;
}

void cdxh_svd3(const double* H, double* U, double* S, double* V) { cdx::svd3(H, U, S, V); }

void cdxh_sdf_forward(const float* points, int64_t P, const float* faces, int64_t F, float* dist, int32_t* sign,
                      float* nrm, float* clst, int32_t* face) {
  for (int64_t i = 0; i < P; ++i) {
    const cdx::F3 p = cdx::f3(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
    float best = 0;
    int bs = 0, bf = -1;
    cdx::F3 bn = cdx::f3(0, 0, 0), bc = bn;
    for (int64_t f0 = 0; f0 < F; f0 += CDX_SDF_REF_TILE) {
      const int64_t nt = F - f0 < CDX_SDF_REF_TILE ? F - f0 : CDX_SDF_REF_TILE;
      float tb = 0;
      int ts = 0, tf = -1;
      cdx::F3 tn = bn, tc = bn;
      for (int64_t s = 0; s < nt; ++s) {
        const float* v = faces + 9 * (f0 + s);
        cdx::F3 c, n;
        int sg;
        const float d = cdx::point_face(p, cdx::f3(v[0], v[1], v[2]), cdx::f3(v[3], v[4], v[5]), cdx::f3(v[6], v[7], v[8]), c, n, sg);
        if (s == 0 || tb > d) { tb = d; ts = sg; tn = n; tc = c; tf = (int)(f0 + s); }
      }
      if (f0 == 0 || best > tb) { best = tb; bs = ts; bn = tn; bc = tc; bf = tf; }
    }
    dist[i] = best;
    sign[i] = bs;
    nrm[3 * i] = bn.x; nrm[3 * i + 1] = bn.y; nrm[3 * i + 2] = bn.z;
    clst[3 * i] = bc.x; clst[3 * i + 1] = bc.y; clst[3 * i + 2] = bc.z;
    if (face) face[i] = bf;
  }
}

// Test-only: face_dist2 (the culled kernels' evaluation from a face record) and point_face's squared
// distance for n (point, face) pairs — tests/test_sdf_cpu.py checks them bit-identical.
void cdxh_face_dist2(const float* points, const float* faces, int64_t n, float* d_rec, float* d_ref) {
  for (int64_t i = 0; i < n; ++i) {
    const cdx::F3 p = cdx::f3(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
    const float* v = faces + 9 * i;
    const cdx::F3 v1 = cdx::f3(v[0], v[1], v[2]), v2 = cdx::f3(v[3], v[4], v[5]), v3 = cdx::f3(v[6], v[7], v[8]);
    d_rec[i] = cdx::face_dist2(p, cdx::face_rec(v1, v2, v3, (int)i));
    cdx::F3 c, nrm;
    int sg;
    d_ref[i] = cdx::point_face(p, v1, v2, v3, c, nrm, sg);
  }
}

// Host build of cdx_gpis_surface_count + cdx_gpis_surface_place (same arguments, host pointers): returns the full
// count of surface cells, or CDX_EINVAL.  tests/test_field_cpu.py checks it against the reference's topcd outputs.
int64_t cdxh_surface_extract(const void* mean, const void* normal, int32_t dtype, int32_t steps, int32_t flip_k,
                             const double* px, const double* py, const double* pz, int64_t capacity, int64_t* cells,
                             double* points, void* normals) {
  if (!mean || steps < 1 || steps > CDX_FIELD_MAX_STEPS || capacity < 0 || (points && (!px || !py || !pz)))
    return CDX_EINVAL;
  if (dtype == CDX_DTYPE_F32)
    return surface_extract(static_cast<const float*>(mean), static_cast<const float*>(normal), steps, flip_k, px, py,
                           pz, capacity, cells, points, static_cast<float*>(normals));
  if (dtype == CDX_DTYPE_F64)
    return surface_extract(static_cast<const double*>(mean), static_cast<const double*>(normal), steps, flip_k, px, py,
                           pz, capacity, cells, points, static_cast<double*>(normals));
  return CDX_EINVAL;
}

// Host build of cdx_gpis_mesh_count + cdx_gpis_mesh_place (host pointers, no workspace): counts [2] = (V, F) in full,
// at most vcap vertices (and keys, nullable) and fcap faces written.  tests/test_mesh_cpu.py checks it against a numpy
// statement of the rule; the device passes are checked against it.
int cdxh_mesh_extract(const void* mean, int32_t dtype, int32_t steps, const double* px, const double* py,
                      const double* pz, int64_t vcap, int64_t fcap, double* vertices, int64_t* edges, int32_t* faces,
                      int64_t* counts) {
  if (!mean || !counts || steps < 1 || steps > CDX_FIELD_MAX_STEPS || vcap < 0 || fcap < 0 || !px || !py || !pz ||
      (vcap > 0 && !vertices) || (fcap > 0 && !faces))
    return CDX_EINVAL;
  counts[0] = counts[1] = 0;
  if (steps < 2) return CDX_OK;
  if (dtype == CDX_DTYPE_F32)
    mesh_extract(static_cast<const float*>(mean), steps, px, py, pz, vcap, fcap, vertices, edges, faces, counts);
  else if (dtype == CDX_DTYPE_F64)
    mesh_extract(static_cast<const double*>(mean), steps, px, py, pz, vcap, fcap, vertices, edges, faces, counts);
  else
    return CDX_EINVAL;
  return counts[0] >= ((int64_t)1 << 31) || counts[1] >= ((int64_t)1 << 31) ? CDX_EINVAL : CDX_OK;
}

// Host build of cdx_gpis_mesh_refine_init (fv null) / _step (host pointers): cdx::mesh_refine_vertex over the vertices.
int cdxh_mesh_refine(const void* mean, int32_t dtype, const double* fv, int32_t steps, const double* px,
                     const double* py, const double* pz, const int64_t* edges, int64_t V, double* state,
                     double* vertices) {
  if (steps < 1 || steps > CDX_FIELD_MAX_STEPS || !px || !py || !pz || V < 0 || (!fv && !mean)) return CDX_EINVAL;
  if (V > 0 && (!edges || !state || !vertices)) return CDX_EINVAL;
  if (!fv && dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) return CDX_EINVAL;
  for (int64_t r = 0; r < V; ++r) {
    if (!fv && dtype == CDX_DTYPE_F32)
      cdx::mesh_refine_vertex(static_cast<const float*>(mean), fv, steps, px, py, pz, edges, V, r, state, vertices);
    else
      cdx::mesh_refine_vertex(static_cast<const double*>(mean), fv, steps, px, py, pz, edges, V, r, state, vertices);
  }
  return CDX_OK;
}

// Host build of cdx_fps (same arguments without the workspace, the mode and the stream; host pointers): the rule of
// cdx_fps.h as a plain single-threaded loop.  tests/test_fps_cpu.py checks it against a numpy statement of the rule.
int cdxh_fps(const void* X, int32_t dtype, int64_t P, int64_t B, int64_t K, int64_t start, int64_t* sel,
             double* radius, double* points) {
  if (!X || P < 1 || P >= ((int64_t)1 << 31) || B < 1 || K < 1 || K > P || start < 0 || start >= P) return CDX_EINVAL;
  if (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) return CDX_EINVAL;
  for (int64_t b = 0; b < B; ++b) {
    int64_t* sb = sel ? sel + b * K : nullptr;
    double* rb = radius ? radius + b * K : nullptr;
    double* pb = points ? points + b * K * 3 : nullptr;
    if (dtype == CDX_DTYPE_F32) fps_host(static_cast<const float*>(X) + b * P * 3, P, K, start, sb, rb, pb);
    else fps_host(static_cast<const double*>(X) + b * P * 3, P, K, start, sb, rb, pb);
  }
  return CDX_OK;
}

// Host build of cdx_knn (same arguments without the grid, the workspace and the stream; host pointers).  mode
// CDX_KNN_SCAN (or AUTO): brute force over the rule of cdx_knn.h.  CDX_KNN_GRID: the ring walk over a grid built here
// with the rule's own cell assignment and bound.  tests/test_knn_cpu.py checks both against a numpy statement.
int cdxh_knn(const void* X, int32_t dtype, int64_t P, const void* Q, int64_t M, int64_t K, double max_d2, int32_t mode,
             int64_t* idx, double* d2, int32_t* count) {
  if (!X || P < 1 || P >= ((int64_t)1 << 31) - 1024 || M < 0 || K < 1 || K > CDX_KNN_MAX_K) return CDX_EINVAL;
  if ((dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) || mode < CDX_KNN_AUTO || mode > CDX_KNN_GRID)
    return CDX_EINVAL;
  if (!Q) {
    Q = X;
    M = P;
  }
  if (M == 0) return CDX_OK;
  if (!idx) return CDX_EINVAL;
  if (dtype == CDX_DTYPE_F32)
    knn_host(static_cast<const float*>(X), P, static_cast<const float*>(Q), M, (int)K, max_d2, mode, idx, d2, count);
  else
    knn_host(static_cast<const double*>(X), P, static_cast<const double*>(Q), M, (int)K, max_d2, mode, idx, d2, count);
  return CDX_OK;
}

// Host build of cdx_cloud_normals (no stream; host pointers); cov [P·6], nullable, receives each row's covariance.
int cdxh_cloud_normals(const void* X, int32_t dtype, int64_t P, const int64_t* idx, const int32_t* count, int64_t K,
                       const double* eye, double* normals, double* eigenvalues, double* cov) {
  if (!X || !idx || !count || !normals || P < 1 || K < 1 || K > CDX_KNN_MAX_K) return CDX_EINVAL;
  if (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) return CDX_EINVAL;
  if (dtype == CDX_DTYPE_F32)
    normals_host(static_cast<const float*>(X), P, idx, count, (int)K, eye, normals, eigenvalues, cov);
  else
    normals_host(static_cast<const double*>(X), P, idx, count, (int)K, eye, normals, eigenvalues, cov);
  return CDX_OK;
}

// cdx::sym3_eig on n symmetric matrices A [n·6] = (a00, a01, a02, a11, a12, a22): w [n·3] ascending, V [n·9] row-major
// with the eigenvectors in columns.
void cdxh_sym3_eig(const double* A, int64_t n, double* w, double* V) {
  for (int64_t k = 0; k < n; ++k) {
    const double* a = A + 6 * k;
    cdx::sym3_eig(a[0], a[1], a[2], a[3], a[4], a[5], w + 3 * k, V + 9 * k);
  }
}

// The grid of cdx_knn.h for a float64 cloud: info = (lo[3], inv) doubles and dims = n[3]; cell [P·3] the cell of every
// row (−1 for a non-finite one); below / above [3·CDX_KNN_MAX_DIM].
int cdxh_knn_grid(const double* X, int64_t P, double* info, int32_t* dims, int32_t* cell, double* below,
                  double* above) {
  if (!X || P < 1 || !info || !dims || !cell || !below || !above) return CDX_EINVAL;
  cdx::KnnGrid g;
  knn_grid_host(X, P, g, cell, below, above);
  for (int a = 0; a < 3; ++a) {
    info[a] = g.lo[a];
    dims[a] = g.n[a];
  }
  info[3] = g.inv;
  return CDX_OK;
}

// Cell cq [3] of the queries Q [M·3] in that grid and, for ring r, cdx::knn_ring_bound of each: bound [M], none [M].
int cdxh_knn_ring_bound(const double* info, const int32_t* dims, const double* below, const double* above,
                        const double* Q, int64_t M, int32_t r, int32_t* cq, double* bound, int32_t* none) {
  cdx::KnnGrid g;
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = info[a];
    g.n[a] = dims[a];
  }
  g.inv = info[3];
  g.pad = 0;
  for (int64_t m = 0; m < M; ++m) {
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = cq[3 * m + a] = cdx::knn_cell(Q[3 * m + a], g.lo[a], g.inv, g.n[a]);
    bool nn;
    bound[m] = cdx::knn_ring_bound(g, below, above, Q + 3 * m, c, r, &nn);
    none[m] = nn;
  }
  return CDX_OK;
}

// Host build of cdx_ray_cast's rule (same arguments without the meshes, the mode and the stream; host pointers): a plain
// double loop over cdx_ray.h.  tests/test_ray_cpu.py checks it against a numpy statement of the rule; the device scan
// and walk are checked against it.
int cdxh_ray_cast(const float* faces, int64_t F, const double* origins, const double* dirs, int64_t R, double tmin,
                  double tmax, double* t, int32_t* face, double* uv) {
  if (R < 0 || F <= 0 || !faces) return CDX_EINVAL;
  if (R == 0) return CDX_OK;
  if (!origins || !dirs || !t || !face) return CDX_EINVAL;
  for (int64_t r = 0; r < R; ++r) {
    const double* o = origins + 3 * r;
    const double* d = dirs + 3 * r;
    cdx::RayHit best = cdx::ray_miss();
    if (cdx::ray_valid(o, d))
      for (int64_t f = 0; f < F; ++f) cdx::ray_update(o, d, faces + 9 * f, (int32_t)f, tmin, tmax, best);
    double u, v;
    cdx::ray_result(best, t[r], face[r], u, v);
    if (uv) { uv[2 * r] = u; uv[2 * r + 1] = v; }
  }
  return CDX_OK;
}

// The rays cdx_depth_render generates: origins, dirs [H·W·3] in row-major pixel order.
int cdxh_pixel_rays(int32_t W, int32_t H, const double* intr, const double* cam_to_world, double* origins,
                    double* dirs) {
  if (W < 1 || H < 1 || !intr || !cam_to_world || !origins || !dirs) return CDX_EINVAL;
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < W; ++j) {
      const int64_t q = (int64_t)i * W + j;
      cdx::pixel_ray(i, j, intr, cam_to_world, origins + 3 * q, dirs + 3 * q);
    }
  return CDX_OK;
}

// Test hook of the walk's node skip: cdx::ray_ball_miss for n (ray, ball) pairs, balls [n·4] = (centre, radius);
// cdx::ray_in_domain into dom when given.
void cdxh_ray_ball_miss(const double* origins, const double* dirs, const double* s0, const double* s1,
                        const float* balls, int64_t n, int32_t* miss, int32_t* dom) {
  for (int64_t i = 0; i < n; ++i) {
    const float* b = balls + 4 * i;
    miss[i] = cdx::ray_ball_miss(origins + 3 * i, dirs + 3 * i, s0[i], s1[i], b[0], b[1], b[2], b[3]) ? 1 : 0;
    if (dom) dom[i] = cdx::ray_in_domain(origins + 3 * i, dirs + 3 * i) ? 1 : 0;
  }
}

// Host build of cdx_depth_count + cdx_depth_place (host pointers): returns the full count of points, or CDX_EINVAL.
int64_t cdxh_depth_unproject(const void* depth, int32_t dtype, int32_t W, int32_t H, int32_t stride, const double* intr,
                             double depth_scale, double depth_trunc, double z_max, const double* transform,
                             int64_t capacity, double* points) {
  if (!depth || !intr || W < 1 || H < 1 || stride < 1 || capacity < 0 || (capacity > 0 && !points)) return CDX_EINVAL;
  if (dtype == CDX_DTYPE_F32)
    return depth_unproject<float, float>(static_cast<const float*>(depth), W, H, stride, intr, depth_scale, depth_trunc,
                                         z_max, transform, capacity, points);
  if (dtype == CDX_DTYPE_F64)
    return depth_unproject<double, double>(static_cast<const double*>(depth), W, H, stride, intr, depth_scale,
                                           depth_trunc, z_max, transform, capacity, points);
  if (dtype == CDX_DEPTH_U16)
    return depth_unproject<uint16_t, float>(static_cast<const uint16_t*>(depth), W, H, stride, intr, depth_scale,
                                            depth_trunc, z_max, transform, capacity, points);
  return CDX_EINVAL;
}

// Host build of cdx_sample_prepare (same arguments without the workspace and the stream; host pointers): the rule of
// cdx_sample.h as plain loops.  tests/test_sample_cpu.py checks it against a numpy statement of the rule.
int cdxh_sample_prepare(const void* faces, int32_t dtype, int64_t F, uint64_t* cdf, int32_t* info) {
  if (!faces || !cdf || !info || F < 1 || F > 0x7fffffff / 9) return CDX_EINVAL;
  if (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) return CDX_EINVAL;
  auto area = [&](int64_t f) {
    return dtype == CDX_DTYPE_F32 ? cdx::sample_area(cdx::sample_face(static_cast<const float*>(faces) + 9 * f))
                                  : cdx::sample_area(cdx::sample_face(static_cast<const double*>(faces) + 9 * f));
  };
  double A = 0.0;
  for (int64_t f = 0; f < F; ++f) A = fmax(A, area(f));
  uint64_t c = 0;
  for (int64_t f = 0; f < F; ++f) cdf[f] = c += cdx::sample_weight(area(f), A);
  *info = A > 0.0 ? 0 : 1;
  return CDX_OK;
}

// Host build of cdx_sample_draw (same arguments without the mode and the stream; host pointers).
int cdxh_sample_draw(const void* faces, int32_t dtype, int64_t F, const uint64_t* cdf, uint64_t seed, uint64_t first,
                     int64_t K, double* points, int64_t* face, double* bary, double* normal) {
  if (!faces || !cdf || F < 1 || F > 0x7fffffff / 9 || K < 0) return CDX_EINVAL;
  if (dtype != CDX_DTYPE_F32 && dtype != CDX_DTYPE_F64) return CDX_EINVAL;
  const uint64_t total = cdf[F - 1];
  for (int64_t row = 0; row < K; ++row) {
    uint64_t t;
    double u, v, p[3], n[3];
    cdx::sample_uniforms(seed, first + (uint64_t)row, total, t, u, v);
    const int64_t f = total != 0 ? cdx::sample_upper(cdf, 0, F, t) : -1;
    if (f >= 0 && f < F) {
      const cdx::SampleFace s = dtype == CDX_DTYPE_F32 ? cdx::sample_face(static_cast<const float*>(faces) + 9 * f)
                                                       : cdx::sample_face(static_cast<const double*>(faces) + 9 * f);
      cdx::sample_point(s, u, v, p);
      cdx::sample_normal(s, n);
    } else {
      u = v = p[0] = p[1] = p[2] = n[0] = n[1] = n[2] = (double)NAN;
    }
    if (face) face[row] = f >= 0 && f < F ? f : -1;
    for (int k = 0; k < 3; ++k) {
      if (points) points[3 * row + k] = p[k];
      if (normal) normal[3 * row + k] = n[k];
    }
    if (bary) { bary[2 * row] = u; bary[2 * row + 1] = v; }
  }
  return CDX_OK;
}

int cdxh_gpis_joint(const cdx_gpis* g, const double* X, int64_t M, double* cov) {
  if (!g || !g->X1 || !g->Linv_t || g->N <= 0 || g->N_pad < g->N) return CDX_EINVAL;
  if (g->kernel < 0 || g->kernel > 2) return CDX_EKERNEL;
  if (M < 0 || (M > 0 && (!X || !cov))) return CDX_EINVAL;
  switch (g->kernel) {
    case CDX_KERNEL_TPS: host_gpis_joint<CDX_KERNEL_TPS>(*g, X, M, cov); break;
    case CDX_KERNEL_RBF: host_gpis_joint<CDX_KERNEL_RBF>(*g, X, M, cov); break;
    default: host_gpis_joint<CDX_KERNEL_JOINT>(*g, X, M, cov); break;
  }
  return CDX_OK;
}

// gpis_kappa / gpis_k0 / gpis_k of csrc/cdx_gpis.h for one kernel id: out4 = (k, kd, k0, κ) at squared distance r2.
int cdxh_gpis_kernel_values(int32_t kernel, double r2, double R, double sigma, double* out4) {
  if (!out4) return CDX_EINVAL;
  const double inv_s2 = 1.0 / (sigma * sigma);
  switch (kernel) {
    case CDX_KERNEL_TPS:
      cdx::gpis_k<CDX_KERNEL_TPS>(r2, R, inv_s2, out4[0], out4[1]);
      out4[2] = cdx::gpis_k0<CDX_KERNEL_TPS>(R); out4[3] = cdx::gpis_kappa<CDX_KERNEL_TPS>(R, inv_s2);
      return CDX_OK;
    case CDX_KERNEL_RBF:
      cdx::gpis_k<CDX_KERNEL_RBF>(r2, R, inv_s2, out4[0], out4[1]);
      out4[2] = cdx::gpis_k0<CDX_KERNEL_RBF>(R); out4[3] = cdx::gpis_kappa<CDX_KERNEL_RBF>(R, inv_s2);
      return CDX_OK;
    case CDX_KERNEL_JOINT:
      cdx::gpis_k<CDX_KERNEL_JOINT>(r2, R, inv_s2, out4[0], out4[1]);
      out4[2] = cdx::gpis_k0<CDX_KERNEL_JOINT>(R); out4[3] = cdx::gpis_kappa<CDX_KERNEL_JOINT>(R, inv_s2);
      return CDX_OK;
  }
  return CDX_EKERNEL;
}

// cdx::philox4x32_10 for the known-answer vectors: counter [4], key [2] → out [4].
void cdxh_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  cdx::philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], out);
}

}  // extern "C"
