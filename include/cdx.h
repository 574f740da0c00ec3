/* compliancedex_amd — C ABI of the MI355X (gfx950) probabilistic-pregrasp hot path.
 *
 * Conventions:
 *   - every array argument is a DEVICE pointer owned by the caller, row-major, dense;
 *   - work is stream-ordered on the given hipStream_t (0 = null stream); nothing is
 *     allocated and nothing synchronises inside these calls;
 *   - return 0 on success, a negative CDX_E* code on a bad argument (checked before any
 *     launch), or CDX_ELAUNCH if the HIP launch itself failed.
 *
 * The reference has no FFI on this path except TorchSDF's pybind module; the entry
 * points below replace the Python/torch operators the reference calls, as cited on
 * each declaration.  Descriptor structs are plain data passed by host pointer; they
 * hold device pointers and scalars only.
 */
#ifndef CDX_H
#define CDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* cdx_stream_t; /* == hipStream_t */

enum {
  CDX_OK = 0,
  CDX_EINVAL = -1,     /* null pointer / bad size */
  CDX_EKERNEL = -2,    /* unsupported GPIS kernel id */
  CDX_ECHAIN = -3,     /* chain too large for the fixed-capacity descriptor */
  CDX_ELAUNCH = -10    /* hipLaunch / hipGetLastError failure */
};

/* ------------------------------------------------------------------ GPIS --------
 * Replaces the GPIS object of gpis.py:4-168 (pred :43-59, compute_normal :63-87).
 * State precomputed once per object (gpis.py:33-40 fit / :162-168 load):
 *   X1     [N_pad*3]  inducing points (N_pad: multiple of CDX_NPAD_ALIGN), AoS xyz, rows >= N padded with any finite point
 *   alpha  [N_pad]    E11^{-1} y1 (zero-padded); mean = Σ alpha_j k(x, x_j) + bias
 *   Ainv   [N_pad*N_pad] E11^{-1}, symmetric, zero-padded; ∇std path
 *   Linv_t [N_pad*N_pad] (L^{-1})^T for E11 = L L^T (upper triangular), zero-padded; std path:
 *          std² = |k0 - ‖L^{-1} k‖²| (the whitened form: N² flops per query, and 1e-12 from the
 *          reference's per-call solve where k^T E11^{-1} k with an explicit inverse is 1e-7)
 *   Linv   [N_pad*N_pad] L^{-1} (lower triangular, row-major), zero-padded; closure ∇std path:
 *          E11^{-1} k = L^{-T} v from the stored whitened vector v = L^{-1} k (N² flops per query)
 * kernel: 0 = thin-plate spline 2r³-3Rr²+R³ (gpis.py:21-26, the default),
 *         1 = RBF exp(-r²/2σ²) (:16-19), 2 = 0.3·RBF + 0.7·TPS (:28-29). */
enum { CDX_KERNEL_TPS = 0, CDX_KERNEL_RBF = 1, CDX_KERNEL_JOINT = 2 };
#define CDX_NPAD_ALIGN 256   /* column width of one std-GEMM workgroup tile */

typedef struct {
  const double* X1;
  const double* alpha;
  const double* Ainv;
  const double* Linv_t;
  const double* Linv;
  int32_t N;
  int32_t N_pad;      /* multiple of CDX_NPAD_ALIGN (256), >= N */
  int32_t kernel;
  int32_t _pad;
  double R;           /* TPS radius = max pairwise training distance */
  double sigma;       /* RBF length scale */
  double bias;
  const void* screen; /* nullable: split-precision variance screen (cdx_gpis_screen_prepare) */
  double screen_delta;/* absolute bound on the screen's |Δstd²| (calibrated per state); the closure
                         screens only when screen != NULL and screen_delta > 0 */
} cdx_gpis;

/* Posterior mean and its spatial gradient at M query points (gpis.py:43-55 mean part,
 * and the autograd gradient the reference takes through it).  normal (optional) is
 * ∇mean / (‖∇mean‖ + 1e-8) — compute_normal (gpis.py:63-87), detached.
 * X [M*3]; mean [M]; grad_mean [M*3] (nullable); normal [M*3] (nullable). */
int cdx_gpis_mean(const cdx_gpis* g, const double* X, int64_t M, double* mean,
                  double* grad_mean, double* normal, cdx_stream_t stream);

/* Workspace bytes cdx_gpis_std needs for M queries. */
size_t cdx_gpis_std_workspace(const cdx_gpis* g, int64_t M);

/* Posterior standard deviation sqrt|k(0) - kᵀ E11^{-1} k| (gpis.py:56-59, the value the
 * reference returns as "var") and its gradient -sign·(E11^{-1}k)ᵀ(∂k/∂x)/std, in the whitened
 * form: v = L^{-1}k (triangular fp64 MFMA GEMM, K* generated on chip), std² = |k0 − ‖v‖²|, and
 * for the gradient E11^{-1}k = L^{-T}v (second triangular GEMM on the kept v; needs Linv, else
 * the explicit Ainv).  std [M]; grad_std [M*3] (nullable).  Workspace holds v: M·N_pad·8 bytes
 * plus partial sums (cdx_gpis_std_workspace). */
int cdx_gpis_std(const cdx_gpis* g, const double* X, int64_t M, double* std, double* grad_std,
                 void* workspace, cdx_stream_t stream);

/* Workspace bytes cdx_gpis_joint needs for M queries (the partial sums of its column splits). */
size_t cdx_gpis_joint_workspace(const cdx_gpis* g, int64_t M);

/* Posterior covariance of (f, ∂f/∂x, ∂f/∂y, ∂f/∂z) at M query points, the 4-vector Gaussian whose mean
 * cdx_gpis_mean gives (the reference has no such function; its compute_multinormals, gpis.py:89-111, samples normals
 * from nested subsets of the inducing points instead): Σ = P0 − WᵀW with W = L^{-1}·[k, ∂ₓk, ∂ᵧk, ∂_z k] (fp64 MFMA,
 * the four columns generated on chip) and the prior P0 = diag(k0, κ, κ, κ), κ = −k″(0).  Reads Linv_t, X1, N, N_pad,
 * kernel, R, sigma.  X [M*3]; cov [M*10]: the upper triangle of Σ row-major — ff, fx, fy, fz, xx, xy, xz, yy, yz, zz —
 * signed (Σ00 = the signed variance of cdx_gpis_std; far from the data the TPS form is indefinite).  A row's entries
 * have the same bits whatever M and its neighbours; a query with a non-finite coordinate gives NaN in its own row.
 * Return codes as cdx_gpis_std; M = 0 is a no-op; nothing is written on a refusal. */
int cdx_gpis_joint(const cdx_gpis* g, const double* X, int64_t M, double* cov, void* workspace,
                   cdx_stream_t stream);

/* On-device fit.  Replaces GPIS.fit (gpis.py:33-40):
 *   R   = max_ij ‖X1_i − X1_j‖ for the TPS / joint kernels (device scalar; 0 for RBF),
 *   E11 = K(X1, X1) + diag(noise²)   [N*N] row-major; noise [N] per point (nullable = 0).
 * N ≤ 65535. */
int cdx_gpis_fit(const double* X1, int32_t N, const double* noise, int32_t kernel, double sigma,
                 double* E11, double* R, cdx_stream_t stream);

/* Workspace bytes of cdx_gpis_factor (2·N_pad²·8). */
size_t cdx_gpis_factor_workspace(int32_t N_pad);

/* Query state from a fitted E11 (the solve gpis.py:53 repeats on every pred, done once):
 * E11 = L Lᵀ by blocked Cholesky + triangular inverse in f64, then Ainv = E11⁻¹ = L⁻ᵀL⁻¹,
 * Linv_t = L⁻ᵀ and Linv = L⁻¹ [N_pad*N_pad] zero-padded, alpha = L⁻ᵀ(L⁻¹ y1) [N_pad] zero-padded.
 * *info (device int32) = 0, or the 1-based row of the first non-positive pivot (E11 not
 * positive definite; outputs are then undefined). */
int cdx_gpis_factor(const double* E11, const double* y1, int32_t N, int32_t N_pad, void* workspace,
                    double* Ainv, double* Linv_t, double* Linv, double* alpha, int32_t* info,
                    cdx_stream_t stream);

/* Split-precision variance screen (fp16 matrix cores).  Estimates std² = k0 − ‖L⁻¹k‖² (gpis.py:56-59)
 * as k0 − ‖Ã·L⁻ᵀ + k0·colsum(L⁻ᵀ)‖² with Ã = K* − k0 generated in fp32, both operands scaled by
 * powers of two and split into two fp16 slices (three slice products, fp32 accumulation):
 * fp32-level accuracy at 32× the fp64 MFMA rate per product.  The closure uses it to skip the fp64
 * pass for fingertips that cannot be the variance cost's maximum; alone it is a throughput estimate
 * with no parity claim.  A query farther than 3.5R − max_n |x_n − centre| from the inducing points'
 * centre (TPS / joint kernels) estimates NaN.
 * cdx_gpis_screen_bytes: size of the per-state screen buffer (≈ 4·N_pad² bytes);
 * cdx_gpis_screen_prepare: fills it from g->Linv_t, g->X1, g->kernel and g->R (the descriptor's own
 *   screen field is ignored; point it at the buffer afterwards);
 * cdx_gpis_screen_var: var [M] = the estimate of k0 − ‖L⁻¹k‖² (signed), workspace
 *   cdx_gpis_screen_workspace bytes. */
size_t cdx_gpis_screen_bytes(int32_t N_pad);
int cdx_gpis_screen_prepare(const cdx_gpis* g, void* screen, cdx_stream_t stream);
/* Closure margin of a screened row at query x: screen_delta · w[b] · max(1, ‖Ṽ‖²/k0) with the distance
 * band b = ⌊4·|x − c|/ρ⌋ (last band beyond), c the inducing points' centre and ρ their largest distance
 * from it; w[CDX_SCREEN_BANDS] (host array, each in (0, 1]) is the calibrated error envelope of bands
 * ≤ b relative to the largest; cdx_gpis_screen_prepare sets them all to 1.
 * cdx_gpis_screen_info: out8 = [cx, cy, cz, SA, rq², 4/ρ, 0, 0] (host). */
#define CDX_SCREEN_BANDS 24
int cdx_gpis_screen_set_bands(const cdx_gpis* g, const double* w, cdx_stream_t stream);
int cdx_gpis_screen_info(const cdx_gpis* g, double* out8, cdx_stream_t stream);
size_t cdx_gpis_screen_workspace(const cdx_gpis* g, int64_t M);
int cdx_gpis_screen_var(const cdx_gpis* g, const double* X, int64_t M, double* var, void* workspace,
                        cdx_stream_t stream);

/* GPIS field on a lattice and its surface cells: get_visualization_data (gpis.py:113-125) and topcd (:127-150)
 * on the device.  The lattice is steps³ cells in C order; cell (i, j, k) sits at (ax[j], ay[i], az[k]) — the
 * reference's meshgrid(..., indexing="xy") — with ax, ay, az device arrays of `steps` doubles, 1 ≤ steps ≤
 * CDX_FIELD_MAX_STEPS.
 *
 * cdx_gpis_field: mean [steps³], std [steps³] (nullable; needs g->Linv_t), normal [steps³·3] (nullable), f64.  The
 *   cells go through the cdx_gpis_mean launch (mean and normal from one pass) and the whitened std pass without a
 *   stored V, `chunk` cells at a time (chunk > 0: any size, a test can force a ragged last chunk; 0: the largest
 *   multiple of 128 whose workspace stays under 1 GiB, at most the lattice).  Every chunk is enqueued on the
 *   stream; a cell's mean and normal do not depend on the chunking (bit-identical).  Workspace:
 *   cdx_gpis_field_workspace(g, steps, chunk) bytes for the same (steps, chunk).
 * cdx_gpis_field_points: X [n·3] = the coordinates of the cells cells[0 .. n) (cells null: cells 0 .. n in
 *   order); an index outside the lattice gives NaN.
 *
 * Surface cells (the cell rule is csrc/cdx_field.h): interior cells with mean < 0 that have a face neighbour
 * with !(mean < 0).  mean [steps³] and normal [steps³·3] are float or double (dtype = CDX_DTYPE_*).  flip_k != 0
 * reads mean and normal at k' = steps − 1 − k, as the reference does for tensor inputs (:130-133); the points do
 * not flip.  Ordered stream compaction without atomics: the output is in C order of (i, j, k) — numpy's
 * boolean-mask order — and deterministic.
 * cdx_gpis_surface_count: per-workgroup counts and their exclusive scan into the workspace
 *   (cdx_gpis_surface_workspace(steps) bytes), *total (device int64) = the number of surface cells.  steps < 3
 *   has no interior cell: total = 0 at once.
 * cdx_gpis_surface_place: after a count on the same inputs and workspace.  Row r < capacity of the outputs is the
 *   r-th surface cell: cells [capacity] its C-ordered index (nullable), points [capacity·3] = (px[j], py[i], pz[k])
 *   from three device arrays of `steps` doubles (nullable, then px, py, pz are not read), normals [capacity·3] =
 *   its normal in the input's dtype (nullable; needs normal).  Rows ≥ capacity are not written. */
#define CDX_FIELD_MAX_STEPS 1024
enum { CDX_DTYPE_F32 = 0, CDX_DTYPE_F64 = 1 };
size_t cdx_gpis_field_workspace(const cdx_gpis* g, int32_t steps, int64_t chunk);
int cdx_gpis_field(const cdx_gpis* g, const double* ax, const double* ay, const double* az, int32_t steps,
                   int64_t chunk, double* mean, double* std, double* normal, void* workspace, cdx_stream_t stream);
int cdx_gpis_field_points(const double* ax, const double* ay, const double* az, int32_t steps, const int64_t* cells,
                          int64_t n, double* X, cdx_stream_t stream);
size_t cdx_gpis_surface_workspace(int32_t steps);
int cdx_gpis_surface_count(const void* mean, int32_t dtype, int32_t steps, int32_t flip_k, void* workspace,
                           int64_t* total, cdx_stream_t stream);
int cdx_gpis_surface_place(const void* mean, const void* normal, int32_t dtype, int32_t steps, int32_t flip_k,
                           const double* px, const double* py, const double* pz, const void* workspace,
                           int64_t capacity, int64_t* cells, double* points, void* normals, cdx_stream_t stream);

/* Iso-surface mesh of a lattice field: GPIS.tomesh / surface_mesh, marching tetrahedra on the field lattice (the
 * rule is csrc/cdx_mesh.h; the reference meshes its completed shape with open3d's Poisson reconstruction,
 * train_gpis_completion.py:67-76 — a different, global algorithm whose output is not pinned here).  mean [steps³] is
 * float or double (dtype = CDX_DTYPE_*), read unflipped; node c = (i·steps + j)·steps + k sits at (px[j], py[i], pz[k]);
 * inside = mean < 0.  A vertex sits on every lattice edge (seven types per node, key 7c + d) whose ends differ in
 * `inside`, at the linear zero of the two end values (the midpoint when that is not in [0, 1]: never non-finite);
 * vertices are in ascending key order.  Every cube's six Kuhn tetrahedra give 0, 1 or 2 triangles each, in the order
 * (cube, tetrahedron, triangle), wound so that cross(v1 − v0, v2 − v0) points from inside to outside; away from the
 * lattice's border the faces are a closed oriented 2-manifold.  Two ordered stream compactions without atomics.
 * cdx_gpis_mesh_count: per-workgroup vertex and face counts and their exclusive scans into the workspace
 *   (cdx_gpis_mesh_workspace(steps) bytes), totals (device int64[2]) = (V, F).  steps < 2 has no edge: V = F = 0 at
 *   once.
 * cdx_gpis_mesh_place: after a count on the same inputs and workspace.  vertices [vcap·3] f64, edges [vcap] the
 *   vertices' keys (nullable), faces [fcap·3] int32 vertex numbers; px, py, pz device arrays of `steps` doubles.  A
 *   capacity cuts the rows written, never the totals (a face may then name a vertex past vcap).  CDX_EINVAL if V or
 *   F ≥ 2³¹ (only lattices above 564 steps can reach that; for those the call reads the totals back and so waits for
 *   the stream).
 *
 * Refinement of the vertices along their own lattice edges (bracketed regula falsi; the faces never change): edges [V]
 * are the keys a place wrote, state [5·V] doubles = ta, fa, tb, fb, t (the bracket's ends as parameters of the edge,
 * the field there, and the vertex), vertices [V·3].  cdx_gpis_mesh_refine_init starts the state at the edges' ends
 * with the lattice's values and writes the rule's own vertices; cdx_gpis_mesh_refine_step takes fv [V], the field at
 * the current vertices (the caller's cdx_gpis_mean between two steps), replaces the bracket end whose `inside` is
 * the vertex's, sets t = ta + (tb − ta)·fa/(fa − fb) — the midpoint unless that lies in [ta, tb] — and writes the new
 * vertices; a non-finite fv leaves its vertex alone.  A key that is no edge of the lattice gives a NaN vertex. */
size_t cdx_gpis_mesh_workspace(int32_t steps);
int cdx_gpis_mesh_count(const void* mean, int32_t dtype, int32_t steps, void* workspace, int64_t* totals,
                        cdx_stream_t stream);
int cdx_gpis_mesh_place(const void* mean, int32_t dtype, int32_t steps, const double* px, const double* py,
                        const double* pz, void* workspace, int64_t vcap, int64_t fcap, double* vertices,
                        int64_t* edges, int32_t* faces, cdx_stream_t stream);
int cdx_gpis_mesh_refine_init(const void* mean, int32_t dtype, int32_t steps, const double* px, const double* py,
                              const double* pz, const int64_t* edges, int64_t V, double* state, double* vertices,
                              cdx_stream_t stream);
int cdx_gpis_mesh_refine_step(const double* fv, int32_t steps, const double* px, const double* py, const double* pz,
                              const int64_t* edges, int64_t V, double* state, double* vertices, cdx_stream_t stream);

/* Farthest-point sampling: the down-sampling in front of GPIS.fit (optimize_pregrasp.py:904 and
 * get_observable_pcd.py:40, open3d's farthest_point_down_sample in the reference).  The rule is csrc/cdx_fps.h:
 * float64 squared distances, a running minimum, the SMALLEST index among the rows with the largest distance, rows
 * with a non-finite coordinate held at −1 (chosen only as `start`).  X [B·P·3] float or double (dtype = CDX_DTYPE_*):
 * B clouds of P rows that never interact; `start` is the first index of every cloud.  Outputs, each nullable:
 * sel [B·K] the chosen rows in selection order, radius [B·K] the squared distance of each to the ones before it
 * (+inf for the first, −1 for a non-finite start), points [B·K·3] = X[sel] as doubles.
 * mode 1: one workgroup per cloud, all rounds in one launch, P ≤ cdx_fps_capacity();  mode 2: one launch per round,
 * several workgroups per cloud joined by a ticket counter (no grid barrier, no waiting), any P < 2³¹;  mode 0 picks.
 * Both give the same bits.  Workspace: cdx_fps_workspace(P, B, mode) bytes (0 for a bad argument), never read before
 * it is written and left ready for the next call.
 * CDX_EINVAL: null X or workspace, K < 1, K > P, start outside 0 … P−1, B < 1, P ≥ 2³¹, an unknown dtype or mode,
 * mode 1 beyond its capacity. */
int64_t cdx_fps_capacity(void);
size_t cdx_fps_workspace(int64_t P, int64_t B, int32_t mode);
int cdx_fps(const void* X, int32_t dtype, int64_t P, int64_t B, int64_t K, int64_t start, int32_t mode,
            void* workspace, int64_t* sel, double* radius, double* points, cdx_stream_t stream);

/* Area-weighted surface sampling: a cloud of a mesh's whole surface (optimize_pregrasp.py:887 and gpis.py:199-263,
 * open3d's sample_points_poisson_disk in the reference, whose first step is a uniform sample).  The rule is
 * csrc/cdx_sample.h: float64 face areas, integer weights floor(area/max area · 2³²) and their running sums C [F]
 * uint64, Philox4x32-10 keyed by `seed` at counter first + row, the face by a search of C, a uniform point of it.
 * faces [F·9] float or double (dtype = CDX_DTYPE_*), 1 ≤ F ≤ INT32_MAX/9.  A face with a non-finite coordinate, no
 * area, or less than 2⁻³² of the largest area is never drawn.
 * cdx_sample_prepare, once per mesh: C into cdf [F], and *info (device) = 1 when no face has area, else 0.
 *   Workspace: cdx_sample_prepare_workspace(F) bytes (0 for a bad F), never read before it is written.
 * cdx_sample_draw: samples first … first + K − 1 of the stream `seed`.  Outputs, each nullable: points [K·3], face [K],
 *   bary [K·2] = (u, v) with point = v0 + u·(v1 − v0) + v·(v2 − v0), normal [K·3] = the face's unit normal.  From a
 *   table whose info is 1 every face is −1 and every other output NaN.  A sample depends on (seed, first + row) only.
 *   mode 1: C whole in LDS, F ≤ cdx_sample_table_capacity();  mode 2: splitters of C in LDS, the search ends in global
 *   memory, any F;  mode 0 picks.  Both give the same bits.  K = 0 is a no-op.
 * CDX_EINVAL: null faces, workspace, cdf or info, F out of range, K < 0, an unknown dtype or mode, mode 1 beyond its
 * capacity.  cdx_sample_scan_faces(): faces per workgroup of prepare's scan (for tests of its seams). */
int64_t cdx_sample_scan_faces(void);
int64_t cdx_sample_table_capacity(void);
size_t cdx_sample_prepare_workspace(int64_t F);
int cdx_sample_prepare(const void* faces, int32_t dtype, int64_t F, void* workspace, uint64_t* cdf, int32_t* info,
                       cdx_stream_t stream);
int cdx_sample_draw(const void* faces, int32_t dtype, int64_t F, const uint64_t* cdf, uint64_t seed, uint64_t first,
                    int64_t K, int32_t mode, double* points, int64_t* face, double* bary, double* normal,
                    cdx_stream_t stream);

/* k-nearest-neighbour search in a cloud, and the normals of a cloud from its neighbour lists (concatenate_pcd.py:35-36:
 * open3d's estimate_normals and orient_normals_towards_camera_location in the reference; open3d's
 * remove_statistical_outlier and compute_point_cloud_distance are the same query).  The rule is csrc/cdx_knn.h.
 * X [P·3] and Q [M·3] float or double (one dtype = CDX_DTYPE_* for both), 1 ≤ P < 2³¹ − 1024, 1 ≤ K ≤ CDX_KNN_MAX_K.
 * cdx_knn: row m of idx [M·K] / d2 [M·K] (nullable) holds the K smallest (d2, index) pairs of query m in ascending
 *   order, d2 = (dx·dx + dy·dy) + dz·dz in float64, ties to the smaller index; pairs with d2 > max_d2 are left out
 *   (+inf: none); count [M] (nullable) = pairs found, the slots past it hold −1 and +inf.  A cloud row with a
 *   non-finite coordinate is never a neighbour, a query with one gets count 0.  Q null: the queries are X's rows (M
 *   is then P whatever was passed).  M = 0 is a no-op.
 *   mode CDX_KNN_SCAN: every row against every query, `grid` may be NULL;  CDX_KNN_GRID: the uniform grid of
 *   cdx_knn_prepare on these X and P;  CDX_KNN_AUTO: the grid when one is given and P is above the measured threshold
 *   (DESIGN §5i), else the scan.  All give the same bits.
 *   Workspace: cdx_knn_workspace(P, M, K, mode) bytes (0 for a bad argument); reserved — both paths keep their lists in
 *   registers and neither reads nor writes it, so NULL is accepted.
 * cdx_knn_prepare: the grid of X into `grid`, caller-owned cdx_knn_grid_bytes(P) bytes (0 for a bad P), which need no
 *   clearing and may be prepared again for any cloud whose cdx_knn_grid_bytes fits.  No host synchronisation.
 * cdx_cloud_normals: normals [P·3] and eigenvalues [P·3] (nullable, ascending) of X's rows from their lists idx [P·K],
 *   count [P]; eye: 3 host doubles to orient the normals towards, or NULL for the largest-component-positive sign.
 *   Fewer than 3 neighbours: (0, 0, 1) and NaN eigenvalues; a non-finite row: NaN.
 * CDX_EINVAL: K outside 1 … CDX_KNN_MAX_K, P out of range, M < 0, null X (idx with M > 0; idx, count or normals for the
 *   normals), CDX_KNN_GRID without a grid, an unknown dtype or mode. */
#define CDX_KNN_AUTO 0
#define CDX_KNN_SCAN 1
#define CDX_KNN_GRID 2
#define CDX_KNN_MAX_K 64
int64_t cdx_knn_auto_rows(void); /* CDX_KNN_AUTO scans clouds of up to this many rows */
size_t cdx_knn_grid_bytes(int64_t P);
int cdx_knn_prepare(const void* X, int32_t dtype, int64_t P, void* grid, cdx_stream_t stream);
size_t cdx_knn_workspace(int64_t P, int64_t M, int64_t K, int32_t mode);
int cdx_knn(const void* X, int32_t dtype, int64_t P, const void* grid, const void* Q, int64_t M, int64_t K,
            double max_d2, int32_t mode, void* workspace, int64_t* idx, double* d2, int32_t* count,
            cdx_stream_t stream);
int cdx_cloud_normals(const void* X, int32_t dtype, int64_t P, const int64_t* idx, const int32_t* count, int64_t K,
                      const double* eye, double* normals, double* eigenvalues, cdx_stream_t stream);

/* ------------------------------------------------------------------ FK ----------
 * Replaces DifferentiableRobotModel.compute_forward_kinematics(q, link_names,
 * recursive=False, offsets) (robot_model.py:224-264 with update_kinematic_state
 * :140-196, rigid_body.py:130-157, spatial_vector_algebra.py:14-136,
 * se3_so3_util.py:240-250).  Computes in float32 like the reference. */
#define CDX_MAX_BODIES 32
#define CDX_MAX_TIPS 8
#define CDX_MAX_DOFS 32
#define CDX_MAX_DEPTH 16 /* longest root→tip path: bodies from the root's child down to a tip's body */

typedef struct {
  float F[9];        /* fixed rotation (Rz(yaw)·Ry(pitch))·Rx(roll), row-major */
  float t[3];        /* joint origin translation */
  float sign;        /* sign of the recognised joint axis component (0 ⇒ identity) */
  int8_t axis;       /* 0 = x, 1 = y, 2 = z */
  int8_t parent;     /* parent body index, -1 for the root */
  int8_t dof;        /* DOF index, -1 for fixed joints */
  int8_t _pad;
} cdx_body;

typedef struct {
  int32_t n_bodies;
  int32_t n_dofs;
  int32_t n_tips;
  int32_t has_offsets;
  int32_t tip_body[CDX_MAX_TIPS];
  float tip_offset[CDX_MAX_TIPS][3];
  cdx_body bodies[CDX_MAX_BODIES];
} cdx_chain;
/* A chain is valid when its sizes fit the capacities above, every body's parent precedes it (body 0 is the root),
 * every dof is below n_dofs, every tip_body is a body, and no tip lies more than CDX_MAX_DEPTH levels below the root
 * (the FK keeps one pose per level in registers).  Every entry that takes a chain checks this on the host before it
 * launches: a malformed or over-deep chain returns CDX_ECHAIN and writes nothing (cdx_closure_workspace: 0 bytes). */

/* q [B*n_dofs] f32 → pos [B*3*n_tips] f32, quat [B*4*n_tips] f32 (xyzw, nullable). */
int cdx_fk_forward(const cdx_chain* chain, const float* q, int64_t B, float* pos, float* quat,
                   cdx_stream_t stream);
/* Vector-Jacobian product of pos with the reference's gradient semantics (detached
 * quaternion scale, spatial_vector_algebra.py:135).  grad_pos [B*3*n_tips] → grad_q [B*n_dofs]. */
int cdx_fk_backward(const cdx_chain* chain, const float* q, int64_t B, const float* grad_pos,
                    float* grad_q, cdx_stream_t stream);

/* Geometric fingertip Jacobians (compute_endeffector_jacobian, robot_model.py:643-683; the rule is csrc/cdx_ik.h):
 * q [B*n_dofs] f32 → lin [B*n_tips*3*n_dofs] f32, the derivative of cdx_fk_forward's pos (tip offsets included) with
 * respect to q, and ang [B*n_tips*3*n_dofs] f32 (nullable), the joint axes; columns of joints off a tip's path are 0.
 * This is the true derivative, not cdx_fk_backward's (which keeps the reference autograd's detached quaternion scale).
 * Return codes of this entry and of cdx_ik_solve: a null required pointer → CDX_ECHAIN (−3), as a null chain gives
 * everywhere; n_tips / n_dofs / n_bodies outside the descriptor's capacity, B < 0 → CDX_EINVAL; B = 0 is a no-op. */
int cdx_fk_jacobian(const cdx_chain* chain, const float* q, int64_t B, float* lin, float* ang, cdx_stream_t stream);

/* Batched inverse kinematics: joint angles whose fingertips reach `target`, E independent rows, the WHOLE solve in one
 * launch (what the reference leaves to PyBullet's calculateInverseKinematics, verify_pregrasp.py:50-53).  The rule is
 * csrc/cdx_ik.h: Levenberg–Marquardt on ½‖w·(target − tip)‖² + ½·rho·‖q − ref_q‖² with the joints projected onto
 * [lower, upper], float32 FK (the fingertips are cdx_fk_forward's, bit for bit) and float64 algebra.
 *   q0 [E*D] of q_dtype (CDX_DTYPE_F32 / CDX_DTYPE_F64; a double is rounded to float32 like the FK's input);
 *   target [E*T*3] f64;  palm [E*6] f64 (nullable: identity) = position + XYZ Euler angles, held fixed;
 *   palm_offset: 3 HOST doubles added to every fingertip (nullable: 0);  w [E*T] f64 ≥ 0 (nullable: 1), 0 drops a tip.
 * Outputs: q [E*D] of q_dtype (float32 values), err [E*T] f64 the unweighted fingertip distances at q, iters [E],
 *   status [E]: 0 = largest weighted fingertip error ≤ tol (tested before each iteration), 1 = max_iters used,
 *   2 = a non-finite input in this row (q = q0 as given, err = NaN, iters = 0).
 * No workspace is needed (per-row state lives in LDS): cdx_ik_workspace returns 0 and `workspace` may be NULL.
 * CDX_EINVAL besides the above: E < 0, an unknown q_dtype, max_iters < 0, tol / mu0 / mu_min / mu_max / nu not finite
 * and positive, rho negative or not finite, a non-finite ref_q, lower > upper or a NaN bound (±inf: unbounded). */
typedef struct {
  double lower[CDX_MAX_DOFS];
  double upper[CDX_MAX_DOFS];
  double ref_q[CDX_MAX_DOFS]; /* rest pose of the rho term */
  double rho;                 /* rest-pose weight, ≥ 0 */
  double tol;                 /* metres */
  double mu0, mu_min, mu_max, nu;
  int32_t max_iters;
  int32_t _pad;
} cdx_ik_params;
size_t cdx_ik_workspace(int64_t E, int32_t n_tips, int32_t n_dofs);
int cdx_ik_solve(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                 const double* target, const double* palm, const double* palm_offset, const double* w,
                 void* workspace, void* q, double* err, int32_t* iters, int32_t* status, cdx_stream_t stream);
/* Rows per workgroup of cdx_ik_solve for a chain of these sizes (for tests of its seams), and sizeof(cdx_ik_params). */
int32_t cdx_ik_rows_per_block(int32_t n_tips, int32_t n_dofs);
size_t cdx_ik_abi_size(void);

/* Free-wrist inverse kinematics: cdx_ik_solve with the palm's rigid pose an unknown next to the joint angles (the rule is
 * ik_pose_row in csrc/cdx_ik.h; one launch, no workspace, `workspace` may be NULL).  Arguments as cdx_ik_solve, but:
 *   palm0_pos [E*3] / palm0_rot [E*9] f64 (row-major rotation, orthogonal by the caller's contract): the start pose,
 *   both or neither — both NULL starts every row at the weighted Kabsch fit of its start's fingertips onto its targets.
 * Outputs besides q / err / iters / status: palm_pos [E*3], palm_rot [E*9] f64, the pose at the returned q (the
 *   fingertips are palm_rot·FK(q) + palm_pos + palm_offset).  A status-2 row (a non-finite q0, target, w, palm0_pos or
 *   palm0_rot) has q = q0 and NaN in palm_pos / palm_rot / err.
 * Return codes as cdx_ik_solve; exactly one of palm0_pos / palm0_rot NULL → CDX_ECHAIN. */
int cdx_ik_solve_pose(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                      const double* target, const double* palm0_pos, const double* palm0_rot,
                      const double* palm_offset, const double* w, void* workspace, void* q, double* palm_pos,
                      double* palm_rot, double* err, int32_t* iters, int32_t* status, cdx_stream_t stream);
/* Rows per workgroup of cdx_ik_solve_pose for a chain of these sizes (for tests of its seams). */
int32_t cdx_ik_pose_rows_per_block(int32_t n_tips, int32_t n_dofs);

/* Pose-target inverse kinematics: cdx_ik_solve with orientation targets on chosen tips and chosen joints held at their
 * start (the rule is frame_ik_row in csrc/cdx_ik.h; one launch, no workspace, `workspace` may be NULL).  Arguments as
 * cdx_ik_solve (`palm` is the pose of the chain's root: for an arm its base), but:
 *   rot_mask: bit k set — tip k also has to reach the orientation target_rot [E*T*9] f64 (row-major, world frame,
 *     orthogonal by the caller's contract; may be NULL where rot_mask is 0);
 *   wr [E*T] f64 ≥ 0 in metres per radian (nullable: 0.1): the weight of a tip's orientation error, so that the one
 *     `tol` (metres) stops both errors — 1e-5 m at 0.1 m/rad is 1e-4 rad;
 *   dof_mask: bit d set — joint d is solved; the others keep clamp(float(q0)) and take no part in the rho term.
 * Outputs besides q / err / iters / status: rot_err [E*T] f64, the chord 2·sin(θ/2) of the angle left between a tip's
 *   frame and its target (0 for a tip outside rot_mask).  Status 2 also for a non-finite target_rot or wr; rot_err is
 *   then NaN like err.  With rot_mask = 0 and every joint in dof_mask the results are cdx_ik_solve's bit for bit.
 * Return codes as cdx_ik_solve; besides: a rot_mask bit at or above n_tips, a dof_mask bit at or above n_dofs or no
 * bit at all, or a row whose storage exceeds 64 KB of LDS → CDX_EINVAL; target_rot NULL with rot_mask ≠ 0 → CDX_ECHAIN. */
int cdx_ik_solve_frames(const cdx_chain* chain, const cdx_ik_params* params, int64_t E, const void* q0, int32_t q_dtype,
                        const double* target_pos, const double* target_rot, const double* palm,
                        const double* palm_offset, const double* w, const double* wr, uint64_t rot_mask,
                        uint64_t dof_mask, void* workspace, void* q, double* err, double* rot_err, int32_t* iters,
                        int32_t* status, cdx_stream_t stream);
/* Rows per workgroup of cdx_ik_solve_frames for a chain of these sizes and this rot_mask (for tests of its seams);
 * 0 for sizes or a mask the entry refuses. */
int32_t cdx_ik_frames_rows_per_block(int32_t n_tips, int32_t n_dofs, uint64_t rot_mask);

/* Rigid-body dynamics of a chain (compute_inverse_dynamics, compute_lagrangian_inertia_matrix and
 * compute_forward_dynamics, robot_model.py:266-640; the rule is csrc/cdx_dyn.h): recursive Newton–Euler in body
 * coordinates, B independent rows, one launch each, per-row state in LDS.  The inertial constants travel in a descriptor
 * of their own, next to the chain (bodies and DOFs in the chain's order):
 *   mass; mcom = mass·(centre of mass, body frame); inertia = xx, xy, xz, yy, yz, zz of I + mass·[c]ₓ[c]ₓᵀ, the rotational
 *   inertia about the body frame's ORIGIN (spatial_vector_algebra.py:321-372); damping per DOF (N·m·s/rad). */
typedef struct {
  double mass[CDX_MAX_BODIES];
  double mcom[CDX_MAX_BODIES][3];
  double inertia[CDX_MAX_BODIES][6];
  double damping[CDX_MAX_DOFS];
} cdx_dyn;
/* Unlike the other descriptors, `dyn` is a DEVICE pointer: a copy of the struct in device memory, made once per robot
 * by the caller and read by the kernels (chain and constants together exceed a kernel's argument block); the chain stays
 * a host pointer.  q rounds to float32 and its sine / cosine are float32 like the FK's; everything after that is
 * float64.  q, qd, qdd, f [B*D] and the outputs are float32 or float64 (dtype = CDX_DTYPE_*); gravity and tip_forces are
 * float64.
 *   gravity: the gravity vector in the BASE frame, [3] (gravity_per_row = 0) or [B*3] (1), a device array; NULL:
 *     (0, 0, −9.81), the reference's base acceleration of +9.81 z (:360-366).  include_gravity = 0: none.
 *   use_damping: cdx_dyn_inverse adds damping·qd to tau (:383-389); cdx_dyn_forward takes it from a copy of f (:532-537
 *     without the reference's write into the caller's f).
 * cdx_dyn_inverse: tau [B*D], the torques that give qdd at (q, qd); qd / qdd NULL: zero.  tip_forces [B*n_tips*3]
 *   (nullable): external forces in the base frame acting at the chain's tips (with their offsets); tau is then what the
 *   joints must supply, τ_RNEA − Σ_t J_tᵀ·F_t, the forces entering the backward sweep (no Jacobian is formed).
 * cdx_dyn_inertia: H [B*D*D], symmetric bit for bit (one triangle computed, then mirrored).
 * cdx_dyn_forward: qdd [B*D] = H⁻¹·(f − damping·qd − nle), H factored by Cholesky in LDS; qd NULL: zero.
 * A moving joint whose sign is 0 (it never moves): its tau is damping·qd alone, its row and column of H are 0, and
 *   cdx_dyn_forward returns CDX_EINVAL.  A chain needs no tip here, and no depth limit applies (state is per body).
 * Return codes: NULL chain, dyn or required array → CDX_ECHAIN; sizes outside the descriptor's capacity, B < 0, an
 *   unknown dtype → CDX_EINVAL; a malformed tree → CDX_ECHAIN; nothing is launched or written on any of them.  B = 0 is
 *   a no-op.
 * cdx_dyn_rows_per_block: rows per workgroup of entry 0 (inverse), 1 (inertia), 2 (forward) for a chain of these sizes
 *   (for tests of its seams; 0 for sizes out of range);  cdx_dyn_abi_size: sizeof(cdx_dyn). */
int cdx_dyn_inverse(const cdx_chain* chain, const cdx_dyn* dyn, int64_t B, const void* q, const void* qd,
                    const void* qdd, int32_t dtype, int32_t include_gravity, int32_t use_damping, const double* gravity,
                    int32_t gravity_per_row, const double* tip_forces, void* tau, cdx_stream_t stream);
int cdx_dyn_inertia(const cdx_chain* chain, const cdx_dyn* dyn, int64_t B, const void* q, int32_t dtype, void* H,
                    cdx_stream_t stream);
int cdx_dyn_forward(const cdx_chain* chain, const cdx_dyn* dyn, int64_t B, const void* q, const void* qd, const void* f,
                    int32_t dtype, int32_t include_gravity, int32_t use_damping, const double* gravity,
                    int32_t gravity_per_row, void* qdd, cdx_stream_t stream);
int32_t cdx_dyn_rows_per_block(int32_t n_bodies, int32_t n_dofs, int32_t entry);
size_t cdx_dyn_abi_size(void);

/* Batched minimum-wrench contact forces (what the reference asks of cvxpy in math_utils.py:6-57; the rule is
 * csrc/cdx_wrench.h): per candidate row, the forces F [T][3] inside their friction cones (n̂·F ≤ −‖F‖/sqrt(1 + mu²))
 * that press at least min_force along the normal (n̂·F ≤ −min_force) and minimise
 * ½‖ΣF‖ + ½‖Σ r×F‖ + (reg/2)·Σ‖F‖², r = tip − mean of the row's tips.  E independent rows, the WHOLE solve (ADMM with
 * penalty rho, a duality-gap certificate every check_every iterations) in one launch, float64, no workspace.
 *   tips, normals [E*T*3] f64 (normals need not be unit).
 * Outputs (f64 unless noted): forces [E*T*3]; wrench [E] = ‖ΣF‖ + ‖Σ r×F‖; margin [E*T] = (−F/‖F‖)·n̂ − 1/sqrt(1 + mu²);
 *   dual [E*6] = (y_f, y_τ), each of norm ≤ ½; gap [E] = P(F) − D(y) ≥ ‖F − F*‖²·reg/2; iters [E] i32; status [E] i32:
 *   0 = gap ≤ tol·max(1, |P|), 1 = max_iters used (the best pair checked is returned, finite and feasible), 2 = a
 *   non-finite input or a zero normal in this row (every float output NaN, iters 0);
 *   grad_tips [E*T*3] (nullable) = ∂wrench/∂tips with F held constant.
 * CDX_EINVAL, with nothing launched: a null params or required pointer, E < 0, n_tips outside 1 … CDX_MAX_TIPS,
 *   mu / reg / rho / tol not finite and positive, min_force negative or not finite, max_iters < 0, check_every < 1.
 *   E = 0 is a no-op. */
typedef struct {
  int32_t n_tips;
  int32_t max_iters;
  int32_t check_every;
  int32_t _pad;
  double mu;
  double min_force;
  double reg;
  double rho;
  double tol;
} cdx_wrench_params;
int cdx_min_wrench(const cdx_wrench_params* params, int64_t E, const double* tips, const double* normals,
                   double* forces, double* wrench, double* margin, double* dual, double* gap, int32_t* iters,
                   int32_t* status, double* grad_tips, cdx_stream_t stream);
/* Rows per workgroup of cdx_min_wrench (for tests of its seams; 0 for n_tips out of range), and
 * sizeof(cdx_wrench_params). */
int32_t cdx_wrench_rows_per_block(int32_t n_tips);
size_t cdx_wrench_abi_size(void);

/* Batched disturbance-load test (the rule is csrc/cdx_equil.h): the spring equilibrium of E grasps under W dead loads
 * each, the reference's quasi-static model of a compliant grasp (force_eq_reward, optimize_pregrasp.py:73-118: sticking
 * contacts, every fingertip a spring of its own stiffness towards its target) solved exactly for any load, every
 * (grasp, load) item its own Levenberg–Marquardt solve on the exact Hessian, all E·W items in one launch, float64, no
 * workspace.  Item index e·W + w.
 *   contact, target, normal [E*T*3], stiffness [E*T] f64 (normals outward, need not be unit);
 *   load_force, load_point: [W*3] used by every row if loads_shared != 0, else [E*W*3]; the force is constant in the
 *   world frame and acts at the body-fixed point load_point (world coordinates at the nominal pose).
 * Outputs per item (f64 unless noted; rot, trans and force may be NULL and are then skipped):
 *   rot [9] row-major, trans [3]: the object's displacement, x = rot·p + trans;  force [T*3] of each spring on the object;
 *   normal_force [T], margin [T] = (−F/‖F‖)·(rot·n̂) − 1/sqrt(1 + mu²);  shift: displacement of the stiffness centre;
 *   chord = 2·sin(θ/2) of rot;  stable u8: the energy's Hessian at the returned pose is positive definite;  iters i32;
 *   status i32: 0 = net force ≤ tol·Fs and net torque ≤ tol·Fs·ℓ, 1 = max_iters used (finite outputs), 2 = a
 *   non-finite input, a stiffness ≤ 0 or a zero normal in the row (all its W items), or a non-finite load (that item):
 *   float outputs NaN, stable 0, iters 0.
 * CDX_EINVAL, with nothing launched: a null params or required pointer, E < 0, W < 0, E·W·T beyond 2^31 − 1, n_tips
 *   outside 1 … CDX_MAX_TIPS, max_iters < 0, mu / tol / mu0 / mu_min / mu_max / nu not finite and positive.  E = 0 or
 *   W = 0 is a no-op. */
typedef struct {
  int32_t n_tips;
  int32_t max_iters;
  double mu;       /* friction coefficient */
  double tol;
  double mu0;      /* Levenberg–Marquardt damping: start, floor, ceiling, factor */
  double mu_min;
  double mu_max;
  double nu;
} cdx_equil_params;
int cdx_grasp_equilibrium(const cdx_equil_params* params, int64_t E, int64_t W, const double* contact,
                          const double* target, const double* stiffness, const double* normal,
                          const double* load_force, const double* load_point, int32_t loads_shared, double* rot,
                          double* trans, double* force, double* normal_force, double* margin, double* shift,
                          double* chord, uint8_t* stable, int32_t* iters, int32_t* status, cdx_stream_t stream);
/* The verdict per grasp row from those outputs, one launch, no atomics.  An item holds when status = 0 and stable, every
 * margin > margin_min, every normal_force ≥ min_normal_force, shift ≤ max_shift and chord ≤ max_chord.
 *   worst_margin [E] f64: the least margin over the row's items with status ≠ 2 (NaN if none); worst_load, worst_tip [E]
 *   i32: where (the first in the order w, tip on a tie; −1 if none); max_shift, max_chord [E] f64 over the same items;
 *   n_failed [E] i32: items that do not hold; holds [E] u8: n_failed = 0.
 * CDX_EINVAL: a null pointer, E < 0, W < 0 or beyond 2^31 − 1, n_tips outside 1 … CDX_MAX_TIPS.  E = 0 or W = 0 is a
 *   no-op. */
typedef struct {
  double margin_min;
  double min_normal_force;
  double max_shift;
  double max_chord;
} cdx_equil_limits;
int cdx_equil_reduce(const cdx_equil_limits* limits, int64_t E, int64_t W, int32_t n_tips, const double* margin,
                     const double* normal_force, const double* shift, const double* chord, const uint8_t* stable,
                     const int32_t* status, double* worst_margin, int32_t* worst_load, int32_t* worst_tip,
                     double* max_shift, double* max_chord, int32_t* n_failed, uint8_t* holds, cdx_stream_t stream);
/* sizeof(cdx_equil_params), sizeof(cdx_equil_limits) into out[2]. */
void cdx_equil_abi_sizes(size_t* out);

/* ------------------------------------------------------ prob-mode closure -------
 * Replaces ProbabilisticGraspOptimizer.closure (optimize_pregrasp.py:741-769) —
 * forward AND backward for E candidates — plus its callees compute_loss (:713-739),
 * force_eq_reward (:73-118), optimal_transformation_batch (:49-69),
 * compute_contact_margin (:703-710), forward_kinematics (:657-669). */
#define CDX_MAX_LEVELS 4

/* Device-resident loop counters (optional).  When cdx_problem.loop is set, every cdx_closure
 * first advances seed and step by one on the device, keys its on-device Kabsch noise by
 * (seed argument ^ loop->seed), and cdx_optimizer_step with cdx_opt_buffers.loop set takes its
 * iteration from loop->step — so a whole optimise loop can be captured once in a hipGraph and
 * replayed (fresh noise and Adam bias correction per replayed iteration). */
typedef struct {
  uint64_t seed;
  int32_t step;     /* set to -1 before the first iteration */
  int32_t _pad;
} cdx_loop;

typedef struct {
  cdx_chain chain;
  cdx_gpis gpis;
  int32_t n_levels;                     /* pregrasp levels K (3 in the reference) */
  int32_t n_query_levels;               /* distinct coefficient rows (1 if all equal) */
  int32_t level_query[CDX_MAX_LEVELS];  /* level → distinct row */
  float coeff[CDX_MAX_LEVELS][CDX_MAX_TIPS]; /* pregrasp coefficients, f32 (:644) */
  double weight[CDX_MAX_LEVELS];        /* pregrasp weights, f64 (:645) */
  float ref_q[CDX_MAX_DOFS];            /* f32 (:634) */
  float cos_mu;                         /* sqrt(1/(1+mu²)) in f32 (:111, :707) */
  int32_t gravity;                      /* dummy gravity spring on (:87-97) */
  int32_t optimize_palm;                /* palm-distance term (:760-763) */
  int32_t _pad;
  float com[3];                         /* dummy tip = COM (f32 tensor, :90-91) */
  float dummy_target_z;                 /* -M (:93) */
  float dummy_comp;                     /* gravity·mass/M (f32, :94) */
  float _pad2;
  double uncertainty;                   /* variance-cost weight (:733) */
  cdx_loop* loop;                       /* device loop counters (nullable) */
} cdx_problem;

/* Workspace bytes for E candidates. */
size_t cdx_closure_workspace(const cdx_problem* p, int64_t E);

/* One cost+grad eval for E candidates.
 * q [E*n_dofs] f64, comp [E*n_tips], target [E*n_tips*3], palm_pos [E*3], palm_ori [E*3];
 * kabsch_noise [n_levels*E*9] f64, the reference's rand_like(H) draw (:61); when NULL the
 *   noise is drawn on device from a counter-based generator keyed by (seed, row, entry).
 * Outputs: total_loss [E], total_margin [E*n_tips], pregrasp_tip [E*n_tips*3] (nullable),
 *   gradients of Σ total_loss: g_q [E*n_dofs], g_comp [E*n_tips], g_target [E*n_tips*3],
 *   g_palm_pos [E*3], g_palm_ori [E*3]; flip [n_levels*E] int32 Kabsch det<0 mask (nullable).
 * All work is ordered on `stream`; a screened call also runs the GPIS mean on a per-device side
 * stream forked from and joined back into `stream` by events, so concurrent calls from several
 * host threads on one device are not supported. */
int cdx_closure(const cdx_problem* p, int64_t E, const double* q, const double* comp,
                const double* target, const double* palm_pos, const double* palm_ori,
                const double* kabsch_noise, uint64_t seed, void* workspace,
                double* total_loss, double* total_margin, double* pregrasp_tip,
                double* g_q, double* g_comp, double* g_target, double* g_palm_pos,
                double* g_palm_ori, int32_t* flip, cdx_stream_t stream);

/* Screening statistics of the last cdx_closure on this workspace (one device→host copy on the null
 * stream; prefer cdx_closure_screen_report): out[0] = all-tip rows that ran the exact fp64 whitened
 * pass, out[1] = kept rows whose split-precision estimate missed the exact value by more than its
 * margin, out[2] = all-tip rows screened; all −1 when the closure did not screen. */
int cdx_closure_screen_stats(const cdx_problem* p, int64_t E, const void* workspace, int32_t* out3);

/* The screened closure's verification record.  Every screened closure runs the exact fp64 pass for
 * each group's leader, every fingertip the selection keeps, and an AUDIT of the fingertips it discards
 * nearest the keep threshold — smallest normalised gap z = (lo − a_f)/Δ_f, lo = max_g (a_g − Δ_g), the
 * margins by which the row's estimate sits below its group's keep floor (64 rows:
 * the lowest 1/8-octave z bins within that budget) — and checks each of those estimates against its
 * margin Δ_f.  The maximum of each group is taken over exact values.  If any check fails (a kept or
 * audited estimate off by more than Δ_f, an audited row that is its group's exact maximum, a maximum on
 * a row the exact pass did not run) the same closure REPAIRS itself: every all-tip row runs the exact
 * pass and the groups select as the unscreened closure does (repaired = 1), so no entry point returns a
 * screened result that failed a check.  A discarded row left unaudited (z ≥ min_gap) can hold its
 * group's true maximum only if its estimate is off by more than z·Δ_f; the checked rows' largest error
 * is max_ratio·Δ_f.  Fields cum_* accumulate over closures since the last cdx_closure_screen_reset (call
 * it once after allocating the workspace). */
typedef struct {
  int32_t screened;        /* 1 if the last closure on this workspace screened (else all fields 0) */
  int32_t screened_rows;   /* all-tip rows estimated by the screen */
  int32_t exact_rows;      /* rows of the exact fp64 pass: leaders + kept + audited */
  int32_t audited_rows;    /* screen-discarded rows re-checked by the exact pass */
  int32_t bound_misses;    /* kept rows whose estimate missed the exact value by more than Δ_f */
  int32_t audit_misses;    /* audited rows whose estimate missed by more than Δ_f */
  int32_t audit_flips;     /* groups whose exact maximum was an audited (screen-discarded) row */
  int32_t faults;          /* groups whose maximum fell on a row the exact pass did not run */
  double max_ratio;        /* max |estimate − exact| / Δ_f over kept rows (finite estimates) */
  double max_ratio_audit;  /* the same over audited rows */
  int64_t cum_closures;
  int64_t cum_audited_rows;
  int64_t cum_bound_misses;
  int64_t cum_audit_misses;
  int64_t cum_audit_flips;
  int64_t cum_faults;
  double cum_max_ratio;
  double cum_max_ratio_audit;
  int32_t repaired;        /* 1 if a check failed and the closure re-ran every row exactly */
  int32_t discarded_rows;  /* rows the screen discarded (audited or not) */
  double min_gap;          /* smallest z among discarded rows left unaudited (+inf: none) */
  double audit_cut;        /* every discarded row with z below this was audited */
  int64_t cum_repairs;
  int64_t cum_discarded_rows;
  double cum_min_gap;      /* smallest min_gap over the closures (+inf: none) */
} cdx_screen_report;

/* Reads the record (an async copy on `stream`, then a wait on that stream). */
int cdx_closure_screen_report(const cdx_problem* p, int64_t E, const void* workspace, cdx_screen_report* out,
                              cdx_stream_t stream);
/* Zeroes the cumulative fields and the exact pass's arrival counters (stream-ordered; REQUIRED once
 * after allocating a workspace for a screened closure); a no-op when the closure does not screen. */
int cdx_closure_screen_reset(const cdx_problem* p, int64_t E, void* workspace, cdx_stream_t stream);
/* Test hook: the next screened cdx_closure returns CDX_ELAUNCH at injection point `stage` (1: after the
 * screen / selection and the side-stream fork, 2: after the exact pass, 3: after the ∇std pass; 0 clears),
 * through the error path of a failed launch — which joins the side stream before returning. */
int cdx_debug_fail_next_closure(int32_t stage);

/* ------------------------------------------------------------ survivor exchange ------
 * Multi-GPU record pack (no reference counterpart — the reference is single-GPU):
 * candidates whose margins are all > 0 (the success test `opt_margin > 0`, optimize_pregrasp.py:226)
 * go to buf [(capacity + 1) * W] f64, W = 5 + n_tips + n_dofs + n_tips + 3·n_tips + 6: row 0 the header
 * [stored, survived, capacity, 0, …], rows 1.. the first `capacity` survivors in candidate order as
 * [object_id, rank, cand_offset + e, best_loss, 1, margin[T], q[D], comp[T], target[3T], palm[6]],
 * the remaining rows zero.  Two launches over 64-candidate tiles (counts, then rows), no host
 * synchronisation; the buffer feeds one all_gather.  The tile counts use a per-device scratch array: packs on
 * one device run one at a time in stream order (not concurrently on several streams). */
int cdx_pack_survivors(int64_t E, int32_t n_tips, int32_t n_dofs, const double* margin, const double* best_loss,
                       const double* q, const double* comp, const double* target, const double* palm,
                       double object_id, double rank, int64_t cand_offset, int64_t capacity, double* buf,
                       cdx_stream_t stream);

/* ------------------------------------------------------------ force_eq_reward ------
 * Replaces force_eq_reward (optimize_pregrasp.py:73-118) with optimal_transformation_batch
 * (:49-69) where the SDF / Kin / GPIS / KinGPIS optimisers (:121-513) call it directly, in f64.
 * Rows are independent: tip, target, normal [B*n_tips*3], comp [B*n_tips]; noise [B*9] is the
 * rand_like(H) draw (:61), or NULL for the on-device counter-based draw keyed by (seed, row) —
 * backward must get the same noise / seed as forward.  normal is detached (every caller passes
 * GPIS/SDF normals without a graph). */
typedef struct {
  float cos_mu;          /* sqrt(1/(1+mu²)) in f32 (:111) */
  int32_t gravity;       /* dummy gravity spring (gravity is not None, :87-97) */
  float com[3];          /* dummy tip = COM (f32 tensor, :90-91) */
  float dummy_target_z;  /* -M (:93) */
  float dummy_comp;      /* gravity·mass/M (f32, :94) */
  int32_t n_tips;
} cdx_force_eq;

/* → reward [B], margin [B*n_tips] (clamped, :112), force_norm [B*n_tips], flip [B] (nullable). */
int cdx_force_eq_forward(const cdx_force_eq* p, int64_t B, const double* tip, const double* target,
                         const double* comp, const double* normal, const double* noise, uint64_t seed,
                         double* reward, double* margin, double* force_norm, int32_t* flip,
                         cdx_stream_t stream);
/* Vector-Jacobian product: g_reward [B], g_force_norm [B*n_tips] (either nullable = 0) →
 * g_tip, g_target [B*n_tips*3], g_comp [B*n_tips] (overwritten). */
int cdx_force_eq_backward(const cdx_force_eq* p, int64_t B, const double* tip, const double* target,
                          const double* comp, const double* normal, const double* noise, uint64_t seed,
                          const double* g_reward, const double* g_force_norm, double* g_tip,
                          double* g_target, double* g_comp, cdx_stream_t stream);

/* ------------------------------------------------------------ Kin-mode iteration ------
 * KinGraspOptimizer's per-iteration cost and its backward (optimize_pregrasp.py:183-208) for E
 * candidates, one lane each, after the iteration's FK (tip = FK(q) + palm offset, float32 [E*T*3]) and
 * its three TorchSDF queries: tips vs the deflated mesh (sign1, n1), tips vs the mesh (sqdist, sign2,
 * n2, clst), targets vs the mesh (tsqdist, tsign, tclst; tsign read as [E, T]).  Returns loss [E] and
 * the force-closure margins [E*T] (f64), the blended normals [E*T*3] (nullable) and the gradients of the
 * loss w.r.t. q [E*D], target [E*T*3] and compliance [E*T] (float32, the parameters' dtype) — through
 * force_eq_reward (noise [E*9] = its rand_like draw, or NULL: drawn on device from seed), the TorchSDF
 * backward and the FK chain (float32, like the reference's autograd).  g_tip [E*T*3] (nullable) receives
 * the gradient w.r.t. the fingertips.  chain NULL: SDFGraspOptimizer's iteration (:229-320) — the tips are
 * the parameters, no ref_cost, no FK backward (q, g_q unused; g_tip required). */
typedef struct {
  cdx_force_eq fe;            /* force_eq_reward constants (mass, COM, gravity spring, friction) */
  float ref_q[CDX_MAX_DOFS];  /* ref_cost = 10·|q − ref_q| */
} cdx_kin_params;
int cdx_kin_cost(const cdx_chain* chain, const cdx_kin_params* p, int64_t E, const float* q, const float* tip,
                 const float* target, const float* comp, const int32_t* sign1, const float* n1,
                 const float* sqdist, const int32_t* sign2, const float* n2, const float* clst,
                 const float* tsqdist, const int32_t* tsign, const float* tclst, const double* noise,
                 uint64_t seed, double* loss, double* margin, float* normal, float* g_q, float* g_target,
                 float* g_comp, float* g_tip, cdx_stream_t stream);

/* ------------------------------------------------------- Kin / SDF optimiser step ------
 * One launch per iteration of KinGraspOptimizer / SDFGraspOptimizer after cdx_kin_cost (float32 like the
 * reference's parameters):
 *   1. the best-iterate update (optimize_pregrasp.py:212-222 / :299-309): per candidate, loss < opt_value
 *      (compared in double, stored as float) copies the pose, target and compliance the loss was computed on;
 *      opt_margin / opt_normal are the WHOLE batch's margin / normal of the last iteration in which ANY
 *      candidate improved (:215-217) — committed one launch late from the alternating kin_cost output slots
 *      margin[s & 1] / normal[s & 1] through the device flags any[3] (zero them before iteration 0), and by a
 *      `finalize` call after the last iteration (iteration = the iteration count; only commits);
 *   2. the optimiser step (torch's single-tensor update order in float32): rule 0 Adam (Kin, :171-176; step
 *      count iteration + 1), rule 1 RMSprop (SDF, :253-259; alpha, eps); lr 0 freezes a group;
 *   3. clamp_box: target (and, for rule 1, the tips) into [box_lb, box_ub] per fingertip (:312-314);
 *   4. rule 0 with `tips` set: the next iteration's fingertips FK(q) + palm_offset (:148), so the loop needs
 *      no separate FK launch.
 * pose is q [E*n_dofs] (rule 0) or the tips [E*n_tips*3] (rule 1); m_* are unused by RMSprop (v_* hold its
 * square averages).  chain is required for rule 0 and ignored for rule 1. */
typedef struct {
  int32_t rule;                           /* 0 Adam (Kin), 1 RMSprop (SDF) */
  int32_t clamp_box;
  double lr[3];                           /* pose, target, compliance */
  double beta1, beta2, eps;               /* Adam (eps also RMSprop's) */
  double alpha;                           /* RMSprop */
  float palm_offset[3];                   /* rule 0: tips = FK(q) + palm_offset */
  float box_lb[CDX_MAX_TIPS * 3];
  float box_ub[CDX_MAX_TIPS * 3];
  int32_t _pad;
} cdx_kin_opt;

typedef struct {                          /* device pointers, candidate-major */
  float *pose, *target, *comp;            /* parameters, in place */
  const float *g_pose, *g_target, *g_comp;
  float *m_pose, *v_pose, *m_target, *v_target, *m_comp, *v_comp;
  const double* loss;                     /* [E] this iteration's cdx_kin_cost loss */
  double* margin[2];                      /* [E*n_tips] cdx_kin_cost margin slots (iteration s wrote s & 1) */
  float* normal[2];                       /* [E*n_tips*3] cdx_kin_cost normal slots */
  float* opt_value;                       /* [E], +inf before iteration 0 */
  double* opt_margin;                     /* [E*n_tips] */
  float* opt_normal;                      /* [E*n_tips*3] */
  float *opt_pose, *opt_target, *opt_comp;
  uint32_t* any;                          /* [3] */
  float* tips;                            /* rule 0: next fingertips [E*n_tips*3] (nullable) */
  float* fk_state;                        /* rule 0, one-launch iterations with tips: the FK-walk cache, */
                                          /* cdx_kin_fk_state_bytes(E, n_tips) bytes (nullable; see below) */
} cdx_kin_opt_buffers;

/* Bytes of the FK-walk cache cdx_kin_iteration's one-launch Kin iteration uses (0: the case does not use one).  The
 * step's next-fingertip FK walk leaves each fingertip chain's joint axes / origins and final pose there, with the joint
 * angles it read, and the next iteration's FK backward takes them instead of walking the chain again when the
 * candidate's joint row still has exactly those bits and the previous iteration wrote it (else it walks): the same
 * gradient bits either way.  Any initial contents work (0xFF bytes in the Python layer); one cache per loop state and
 * chain. */
int64_t cdx_kin_fk_state_bytes(int64_t E, int32_t n_tips);

int cdx_kin_step(const cdx_chain* chain, const cdx_kin_opt* cfg, const cdx_kin_opt_buffers* buf, int64_t E,
                 int32_t n_tips, int32_t iteration, int32_t finalize, cdx_stream_t stream);
/* One whole optimiser iteration on the loop state in `buf`: cdx_kin_cost (q = pose, tip = tips for rule 0 / tip = pose
 * for rule 1; loss, margin[iteration & 1], normal[iteration & 1] and the g_* gradients into buf's buffers) followed by
 * cdx_kin_step(iteration, finalize = 0).  Two cases run as ONE launch with the same results as the two: the Kin
 * optimiser's (rule 0 = Adam, a chain, four fingertips, no clamp_box) and the SDF optimiser's (rule 1 = RMSprop, no
 * chain, four fingertips, box clamps allowed); other cases run the two launches.  chain: rule 0 only. */
int cdx_kin_iteration(const cdx_chain* chain, const cdx_kin_params* p, const cdx_kin_opt* cfg,
                      const cdx_kin_opt_buffers* buf, int64_t E, int32_t n_tips, const int32_t* sign1, const float* n1,
                      const float* sqdist, const int32_t* sign2, const float* n2, const float* clst,
                      const float* tsqdist, const int32_t* tsign, const float* tclst, const double* noise,
                      uint64_t seed, int32_t iteration, cdx_stream_t stream);

/* ------------------------------------------------- GPIS / KinGPIS optimiser iteration ------
 * The fused loop of GPISGraspOptimizer (optimize_pregrasp.py:322-406, mode 0: the fingertips are the parameters)
 * and KinGPISGraspOptimizer (:408-511, mode 1: the joint angles are, tips = FK(q) + palm_offset), one lane per
 * candidate, after the iteration's GPIS queries: cdx_gpis_mean over [tips; targets] (mean, ∇mean, normal) and
 * cdx_gpis_std over the tips (std, ∇std; the reference's variance of the targets, :364 / :465, is never used).
 *
 * Dtypes: every array is f64 — the reference runs both modes in double.  Mode 1's FK is the float32 chain of
 * cdx_fk_forward / cdx_fk_backward: tips = double(FK_f32(float(q))) + palm_offset, and the fingertip gradient is
 * rounded to float32, walked back through the chain in float32 and widened again (robot_model._FK).
 *
 * cdx_gpis_mode_cost: loss [E], the force-closure margins into margin[iteration & 1], the fingertip normals copied
 *   into normal_slot[iteration & 1] (when set), and the gradients of the loss
 *     mode 0 (:374-383)  −25·reward + 1000·Σ|mean| + 10·Σ tmean + 10·‖mean tip − mean target‖
 *                        − Σ min(fn·softmin(fn), 1) + uncertainty·Σ std
 *     mode 1 (:473-486)  −5·reward + (the same four terms) + 20·‖q − ref_q‖ + max_t uncertainty·log(100·std_t)
 *   into g_pose (tips / q), g_target, g_comp and (mode 1, nullable) g_tip, with torch autograd's rules: sign(0) = 0,
 *   a zero norm gives a zero gradient, clamp(max = 1) passes the gradient where it does not clamp, the max feeds its
 *   first maximal fingertip, normals are detached.  noise [E*9] is force_eq_reward's rand_like draw, or NULL for the
 *   on-device draw keyed by (seed, row) of cdx_force_eq_*.
 * cdx_gpis_mode_step: in this order
 *   1. the best-iterate update (:389-397 / :495-503): per candidate, loss < opt_value in f64 copies the pose, target
 *      and compliance the loss was computed on (a non-finite loss never does); opt_margin / opt_normal are the WHOLE
 *      batch's margin / normal of the last iteration in which ANY candidate improved, committed one launch late from
 *      the alternating slots through any[3] (zeroed before iteration 0) and by a `finalize` call after the last
 *      iteration (iteration = the iteration count; only commits) — the protocol of cdx_kin_step;
 *   2. RMSprop in f64, torch's single-tensor order (:348-355 / :454-460): sq = α·sq + (1 − α)·g², p −= lr·g/(√sq + eps);
 *      one lr per group (pose, target, compliance), lr 0 freezes a group;
 *   3. the clamps — mode 0: tips into [box_lb, box_ub] per fingertip, comp ≥ comp_min (:399-401); mode 1:
 *      comp ≥ comp_min and the TARGETS into the box, optimised or not (:505-507);
 *   4. mode 1 with `tips` set: the next iteration's fingertips, so that the loop needs no FK launch (iteration 0's
 *      come from one cdx_fk_forward).
 * cdx_gpis_mode_iteration: cost then step on the state in `buf`, in ONE launch for four fingertips (bit-identical
 *   to the two calls), else the two launches.
 * One cdx_gpis_mode_buffers (its slots, moments, best iterate and any[3]) belongs to one loop: two loops never share
 * one, and the caller zeroes v_* / any and sets opt_value to +inf before iteration 0.  chain: mode 1 only (NULL for
 * mode 0).  Runtime n_tips ≤ CDX_MAX_TIPS, n_dofs ≤ CDX_MAX_DOFS.  E = 0 is a no-op. */
typedef struct {
  int32_t mode;                  /* 0 GPIS (fingertip space), 1 KinGPIS (joint space) */
  int32_t _pad;
  cdx_force_eq fe;               /* force_eq_reward constants */
  double uncertainty;            /* variance-cost weight (:383 / :480) */
  double ref_q[CDX_MAX_DOFS];    /* mode 1: ref_cost = 20·‖q − ref_q‖ */
  double palm_offset[3];         /* mode 1: tips = FK(q) + palm_offset */
} cdx_gpis_mode_params;

typedef struct {
  double lr[3];                  /* pose, target, compliance */
  double alpha, eps;             /* RMSprop */
  double box_lb[CDX_MAX_TIPS * 3];
  double box_ub[CDX_MAX_TIPS * 3];
  double comp_min;
} cdx_gpis_mode_opt;

typedef struct {                 /* device pointers, candidate-major, all f64 */
  double *pose, *target, *comp;  /* parameters, in place: pose = tips [E*T*3] (mode 0) or q [E*D] (mode 1) */
  double* tips;                  /* mode 1: this iteration's fingertips [E*T*3]; the step writes the next ones */
  const double *mean, *gmean, *normal, *std, *gstd; /* GPIS at the fingertips: [E*T], [E*T*3], … */
  const double *tmean, *tgmean;  /* GPIS mean / ∇mean at the targets */
  double *g_pose, *g_target, *g_comp;
  double* g_tip;                 /* mode 1: gradient w.r.t. the fingertips (nullable) */
  double *v_pose, *v_target, *v_comp; /* RMSprop square averages */
  double* loss;                  /* [E] */
  double* margin[2];             /* [E*T] slots (iteration s writes s & 1) */
  double* normal_slot[2];        /* [E*T*3] slots */
  double* opt_value;             /* [E], +inf before iteration 0 */
  double *opt_margin, *opt_normal;
  double *opt_pose, *opt_target, *opt_comp;
  uint32_t* any;                 /* [3] */
} cdx_gpis_mode_buffers;

int cdx_gpis_mode_cost(const cdx_chain* chain, const cdx_gpis_mode_params* p, const cdx_gpis_mode_buffers* buf,
                       int64_t E, int32_t n_tips, const double* noise, uint64_t seed, int32_t iteration,
                       cdx_stream_t stream);
int cdx_gpis_mode_step(const cdx_chain* chain, const cdx_gpis_mode_params* p, const cdx_gpis_mode_opt* opt,
                       const cdx_gpis_mode_buffers* buf, int64_t E, int32_t n_tips, int32_t iteration,
                       int32_t finalize, cdx_stream_t stream);
int cdx_gpis_mode_iteration(const cdx_chain* chain, const cdx_gpis_mode_params* p, const cdx_gpis_mode_opt* opt,
                            const cdx_gpis_mode_buffers* buf, int64_t E, int32_t n_tips, const double* noise,
                            uint64_t seed, int32_t iteration, cdx_stream_t stream);
/* sizeof of the three structs above (cdx_abi_sizes keeps its thirteen). */
void cdx_gpis_mode_abi_sizes(size_t* out3);

/* ------------------------------------------------------------ collision loss -------
 * Replaces ProbabilisticGraspOptimizer.compute_collision_loss (optimize_pregrasp.py:671-701):
 * anchor links by f32 FK (:674-676), palm transform R(euler XYZ)·a + palm_pos (:677-678), then
 *   Σ_pairs 1/‖a_l − a_r‖ where < pair_threshold (:679-686)
 * + Σ_anchors (1/z)·0.1 where z < floor_z (:688-691)
 * + 1/palm_z where palm_z < floor_z, if palm_term (:693-698),
 * and its gradient w.r.t. q and the palm pose.  The reference's closure leaves the call
 * commented out (:765); config 4 ("self-collision enabled") turns it on. */
#define CDX_MAX_PAIRS 28

typedef struct {
  cdx_chain chain;                      /* anchor links (collision_links + offsets) as tips */
  int32_t n_pairs;
  int32_t palm_term;                    /* optimize_palm */
  int8_t pairs[CDX_MAX_PAIRS][2];       /* anchor indices (collision_pairs) */
  double pair_threshold;                /* collision_pair_threshold (0.02) */
  double floor_z;                       /* 0.02 (:688, :694) */
} cdx_collision;

/* q [E*n_dofs] f64, palm_pos [E*3], palm_ori [E*3] → cost [E], g_q [E*n_dofs], g_palm_pos [E*3],
 * g_palm_ori [E*3] (gradients of Σ cost).  accumulate = 1 adds into the outputs (fusing the term
 * into a closure's total_loss and gradients) instead of overwriting them. */
int cdx_collision_loss(const cdx_collision* c, int64_t E, const double* q, const double* palm_pos,
                       const double* palm_ori, double* cost, double* g_q, double* g_palm_pos,
                       double* g_palm_ori, int32_t accumulate, cdx_stream_t stream);

/* ------------------------------------------------------ whole-hand spheres -------
 * The hand's volume as spheres fixed to its links, and the three kernels that turn it into a penetration cost, its
 * gradient in joint space and a report (the reference leaves whole-hand checks to PyBullet, verify_pregrasp.py, and
 * cuRobo's collision spheres, traj_gen.py).  The rule — every formula and the order of every sum — is csrc/cdx_hand.h.
 *
 * cdx_hand_prepare, once per model: checks the caller's HOST tables and copies them, with the per-sphere partner
 *   lists, into `tables` (device, cdx_hand_bytes(S, P) caller-owned bytes; waits on `stream`), and fills *out, the
 *   descriptor the other entries take (host struct of device pointers; valid while `tables` is).  local [S*3] f32 the
 *   centres in their bodies' frames, radius [S] f64 finite and > 0, body [S] ascending in 0 … n_bodies − 1, pairs
 *   [P*2] sphere indices with 0 ≤ a < b < S, no sphere in more than min(S − 1, P) of them.  1 ≤ S ≤ CDX_MAX_SPHERES, 0 ≤ P ≤ CDX_HAND_MAX_PAIRS.
 * cdx_hand_spheres: q [E*n_dofs] f64 (rounded to float32 like every FK input), palm_pos, palm_ori [E*3] f64 (each
 *   nullable: zero) → poses [E*n_bodies*12] f32 (R row-major, then t, in the hand frame; a body's pose has the bits of
 *   cdx_fk_forward's walk to it) and centers [E*S*3] f64 in the world frame: Rp·(double)(R_b·c_local + t_b) + palm_pos.
 *   h->n_bodies must be the chain's.
 * cdx_hand_cost: centers [E*S*3]; dist [E*S], gdist [E*S*3] the object's signed distance (positive outside) and its
 *   gradient at the centres (both or neither: NULL turns the object class off) → cost [E], depth [E*3] the largest
 *   penetration at zero margin per class (object r − d, self r_a + r_b − ρ, floor r − (z − floor_z); positive =
 *   intersecting; −inf for a class that is off or empty), worst [E*3] i32 the sphere (object, floor) or pair (self)
 *   that attains it (first on ties, −1 for −inf), g_centers [E*S*3] = ∂cost/∂centers.  No atomics: the bits do not
 *   depend on E, on the row's position or on the run.
 * cdx_hand_pullback: poses (cdx_hand_spheres' own), g_centers [E*S*3], palm_ori [E*3] (nullable: zero; the palm
 *   position does not enter) → g_q [E*n_dofs], g_palm_pos [E*3], g_palm_ori [E*3] f64: the true derivative of Σ
 *   g_centers·centers (a sign-0 joint gets 0).
 * cdx_hand_term: cdx_hand_cost then cdx_hand_pullback in one launch, as a weighted term of a caller's loss (one wave
 *   per candidate, g_centers stays in LDS): poses and centers as cdx_hand_spheres wrote them, dist / gdist (both or
 *   neither), palm_ori (nullable: zero) → loss [E], g_q [E*n_dofs], g_palm_pos [E*3], g_palm_ori [E*3] (each of the two
 *   nullable: not wanted), every element weight·x with accumulate = 0 and old + weight·x with accumulate = 1, x being
 *   the bits the two entries give (the product and the sum round separately; one lane owns each element, no atomics);
 *   depth [E*3], worst [E*3] (each nullable) as cdx_hand_cost's, neither weighted nor accumulated.  weight finite,
 *   accumulate 0 or 1.  Nothing is allocated or read back.
 * A row with a non-finite input is NaN in its own float outputs (worst −1) and touches no other row.
 * Return codes: a null or malformed chain, or a body more than CDX_MAX_DEPTH levels deep → CDX_ECHAIN; sizes over the
 *   limits, a null required pointer, a model whose n_bodies is not the chain's, non-finite parameters, E < 0 →
 *   CDX_EINVAL, with nothing launched; E = 0 is a no-op. */
#define CDX_MAX_SPHERES 256
#define CDX_HAND_MAX_PAIRS 32768
#define CDX_HAND_LANES 64 /* lanes per candidate of the cost and pull-back kernels (fixes the order of their sums) */

typedef struct {
  int32_t n_spheres;
  int32_t n_pairs;
  int32_t n_bodies;
  int32_t _pad;
  const double* radius;    /* [S] */
  const float* local;      /* [S*3] */
  const int32_t* body;     /* [S] ascending */
  const int32_t* len;      /* [S] length of every sphere's partner list */
  const int32_t* pairs;    /* [P*2] */
  const int32_t* entry;    /* partner lists: entry k of sphere s at group_base[s/64] + 64k + s%64 = partner | pair << 8, */
                           /* in ascending pair index (a group of 64 spheres is as long as its longest list) */
  int32_t group_base[4];
} cdx_hand;

typedef struct {
  double m_obj, m_self, m_floor; /* margins, metres */
  double w_obj, w_self, w_floor; /* weights */
  double floor_z;
  int32_t floor_on;
  int32_t _pad;
} cdx_hand_params;

size_t cdx_hand_bytes(int32_t S, int32_t P);
int cdx_hand_prepare(int32_t n_bodies, int32_t S, const float* local, const double* radius, const int32_t* body,
                     int32_t P, const int32_t* pairs, void* tables, cdx_hand* out, cdx_stream_t stream);
int cdx_hand_spheres(const cdx_chain* chain, const cdx_hand* h, int64_t E, const double* q, const double* palm_pos,
                     const double* palm_ori, float* poses, double* centers, cdx_stream_t stream);
int cdx_hand_cost(const cdx_hand* h, const cdx_hand_params* p, int64_t E, const double* centers, const double* dist,
                  const double* gdist, double* cost, double* depth, int32_t* worst, double* g_centers,
                  cdx_stream_t stream);
int cdx_hand_pullback(const cdx_chain* chain, const cdx_hand* h, int64_t E, const float* poses, const double* g_centers,
                      const double* palm_ori, double* g_q, double* g_palm_pos, double* g_palm_ori, cdx_stream_t stream);
int cdx_hand_term(const cdx_chain* chain, const cdx_hand* h, const cdx_hand_params* p, int64_t E, const float* poses,
                  const double* centers, const double* dist, const double* gdist, const double* palm_ori, double weight,
                  int32_t accumulate, double* loss, double* g_q, double* g_palm_pos, double* g_palm_ori, double* depth,
                  int32_t* worst, cdx_stream_t stream);
/* sizeof(cdx_hand), sizeof(cdx_hand_params). */
void cdx_hand_abi_sizes(size_t* out2);

/* ------------------------------------------------------ approach trajectories -------
 * Batched CHOMP (Ratliff et al., ICRA 2009) on joint-space trajectories: what the reference asks of cuRobo's MotionGen
 * (traj_gen.py); parity with cuRobo is unpinned and not attempted.  The rule — every formula and the order of every
 * sum — is csrc/cdx_traj.h.  A trajectory row is q [T*n_dofs] f64, waypoint-major; q[0] and q[T−1] are given and no
 * entry writes them; 3 ≤ T ≤ CDX_TRAJ_MAX_T, 1 ≤ n_dofs ≤ CDX_MAX_DOFS.
 *
 * cdx_traj_seed: q_start, q_goal [G*n_dofs] → traj [G*seeds*T*n_dofs]: row g·seeds + s is the straight line plus
 *   a_d·16u²(1−u)² per joint d, u = t/(T−1), a_d = amp·(2·U01 − 1) from Philox4x32-10 keyed by `seed` and counted by
 *   (g·seeds + s)·n_dofs + d; a_d = 0 for s = 0.  A row depends on (seed, g, s) alone.  A non-finite start or goal makes
 *   the whole row NaN.
 * cdx_traj_step: one covariant step on E rows, in place.  g_c [E*T*n_dofs] and cost_t [E*T] are the collision term per
 *   waypoint (cdx_hand_term at weight 1, accumulate 0, over E·T rows; both NULL: no collision term; the two endpoint
 *   rows of g_c do not enter the gradient).  cost [E*3] = (U_s, U_c, U_l) unweighted at the iterate the step starts
 *   from; U = w_smooth·U_s + w_col·U_c + w_lim·U_l replaces the row's best when U < best_cost (strict; a NaN never
 *   wins): then best_cost [E] = U, best_iter [E] = iteration and best_traj [E*T*n_dofs] = the whole row before the
 *   step.  The caller presets best_cost to +inf.  Then the interior becomes ξ − step·A_T⁻¹g per joint.  One workgroup
 *   per row, no atomics: a row's bits depend neither on E nor on its position nor on the run.  A row with a non-finite
 *   value in traj, g_c or cost_t gets NaN in its interior and in cost, and its best_* entries stay as they are.
 * CDX_EINVAL, with nothing written: T or n_dofs out of range, lower > upper or a NaN bound (±inf: unbounded), a
 *   non-finite weight, margin, step or amp, seeds < 1, a NULL required pointer, only one of g_c / cost_t, G or E < 0.
 *   G = 0 or E = 0 is a no-op. */
#define CDX_TRAJ_MAX_T 64
#define CDX_TRAJ_LANES 32 /* width of the tree that joins the per-joint sums (fixes their order) */

typedef struct {
  double lower[CDX_MAX_DOFS];
  double upper[CDX_MAX_DOFS];
  double w_smooth, w_col, w_lim; /* weights of U_s, U_c, U_l */
  double m_lim;                  /* the limit hinge starts m_lim inside the bounds */
  double step;                   /* ξ ← ξ − step·A_T⁻¹g */
  int32_t T;
  int32_t n_dofs;
} cdx_traj_params;

int cdx_traj_seed(int64_t G, int32_t seeds, int32_t T, int32_t n_dofs, const double* q_start, const double* q_goal,
                  double amp, uint64_t seed, double* traj, cdx_stream_t stream);
int cdx_traj_step(const cdx_traj_params* p, int64_t E, double* traj, const double* g_c, const double* cost_t,
                  int32_t iteration, double* cost, double* best_cost, int32_t* best_iter, double* best_traj,
                  cdx_stream_t stream);
/* sizeof(cdx_traj_params). */
void cdx_traj_abi_sizes(size_t* out1);

/* ------------------------------------------------------- fused optimizer step ------
 * One launch per iteration of ProbabilisticGraspOptimizer.optimize (optimize_pregrasp.py:805-836)
 * after the closure: best-iterate update (:821-829, before the step, only when s > best_after),
 * torch.optim.Adam for the five parameter groups (:782-796; the single-tensor / foreach update
 * order: m.lerp_(g, 1-β1), v·β2 + (1-β2)·g·g, p += -lr/(1-β1^t) · m / (sqrt(v)/sqrt(1-β2^t) + eps)),
 * then the clamps compliance ≥ comp_min and target ∈ [lb, ub] (:833-834).  No host sync. */
typedef struct {
  double lr[5];                        /* q, compliance, target, palm_pos, palm_ori; 0 = frozen */
  double beta1, beta2, eps;
  double comp_min;
  double target_lb[CDX_MAX_TIPS * 3];
  double target_ub[CDX_MAX_TIPS * 3];
  int32_t clamp_target;
  int32_t best_after;                  /* best-iterate tracking from iteration best_after+1 */
} cdx_adam;

typedef struct {                       /* all device pointers, candidate-major */
  double *q, *comp, *target, *palm_pos, *palm_ori;                 /* parameters (in place) */
  const double *g_q, *g_comp, *g_target, *g_palm_pos, *g_palm_ori; /* closure gradients */
  double *m_q, *v_q, *m_comp, *v_comp, *m_target, *v_target;       /* Adam moments */
  double *m_palm_pos, *v_palm_pos, *m_palm_ori, *v_palm_ori;
  const double *total_loss, *total_margin;                         /* closure outputs */
  double *opt_value, *opt_margin, *opt_q, *opt_comp, *opt_target, *opt_palm;  /* best iterate */
  const cdx_loop* loop;                                            /* nullable: iteration from loop->step */
} cdx_opt_buffers;

/* iteration = 0-based loop index s (ignored when buf->loop is set); Adam's step count is s + 1. */
int cdx_optimizer_step(const cdx_adam* cfg, const cdx_opt_buffers* buf, int64_t E, int32_t n_dofs,
                       int32_t n_tips, int32_t iteration, cdx_stream_t stream);

/* --------------------------------------------------------------- TorchSDF -------
 * Replaces torchsdf._C.unbatched_triangle_distance_forward_cuda / _backward_cuda
 * (thirdparty/TorchSDF/torchsdf/csrc/bindings.cpp:22-27, kernels
 * unbatched_triangle_distance_cuda.cu:176-270).  float32 (the dtype the reference path uses,
 * optimize_pregrasp.py:165-168) and, through the _f64 entry points, float64 (the reference's
 * double dispatch, .cu:32-41 / :282).  Outputs are caller-allocated.
 * points [P*3], faces [F*9] → sqdist [P], sign [P] (±1), normals [P*3], clst [P*3],
 * face_idx [P] (argmin face, first minimum; nullable). */
int cdx_sdf_forward(const float* points, int64_t P, const float* faces, int64_t F,
                    float* sqdist, int32_t* sign, float* normals, float* clst,
                    int32_t* face_idx, cdx_stream_t stream);
/* grad_points = 2·grad_dist·(p − clst) (unbatched_triangle_distance_cuda.cu:256-270). */
int cdx_sdf_backward(const float* grad_dist, const float* points, const float* clst, int64_t P,
                     float* grad_points, cdx_stream_t stream);
/* float64 points / faces: the reference's double instantiation — double arithmetic except the
 * float edge parameter of point_at (.cu:171-173) and the float squared distance (.cu:237), so
 * sqdist holds float values; brute force with the reference's 512-face tile rule. */
int cdx_sdf_forward_f64(const double* points, int64_t P, const double* faces, int64_t F,
                        double* sqdist, int32_t* sign, double* normals, double* clst,
                        int32_t* face_idx, cdx_stream_t stream);
int cdx_sdf_backward_f64(const double* grad_dist, const double* points, const double* clst, int64_t P,
                         double* grad_points, cdx_stream_t stream);

/* A prepared mesh for repeated float32 queries (the SDF optimisers query the same two meshes every
 * iteration): the face records in the order of a median-split k-d tree on the face centroids (built on
 * the host: cdx_sdf_mesh_prepare copies the faces to the host and WAITS on `stream`), their disk slabs,
 * the 32-face chunks' and 512-face top nodes' bounding cylinders and balls, and the may-NaN flag of the
 * culled path.  cdx_sdf_query is cdx_sdf_forward on it — identical outputs (the face order only steers the
 * culling; ties resolve by face index).  faces must stay the ones prepared (the exact path of a NaN-capable
 * mesh scans them, and every output is recomputed from them).  mesh: cdx_sdf_mesh_bytes(F) caller-owned
 * device bytes.  cdx_sdf_query's scratch (the points' Morton sort) is `workspace` (device, at least
 * cdx_sdf_query_workspace(P) bytes — no allocation in the call), or stream-ordered scratch allocated by the
 * call when workspace is NULL. */
size_t cdx_sdf_mesh_bytes(int64_t F);
int cdx_sdf_mesh_prepare(const float* faces, int64_t F, void* mesh, cdx_stream_t stream);
size_t cdx_sdf_query_workspace(int64_t P);
/* flags of cdx_sdf_query: CDX_SDF_REUSE_ORDER — walk the points in the order the last sort on `workspace` left,
 * which must have been of P points (the same fingertips against a second mesh, or the same points a few optimiser
 * iterations earlier): the points are not sorted again.  The results do not depend on the order, only the
 * culling's speed does;
 * CDX_SDF_MESH_CULLED / CDX_SDF_MESH_EXACT — the mesh's kind as cdx_sdf_mesh_flags read it once (no NaN-capable
 * face: the culled kernel only; else the brute-force tile rule only); without either, both kernels are launched
 * and the device picks. */
/* The points' Morton order alone, into `workspace` (what cdx_sdf_query does first without CDX_SDF_REUSE_ORDER):
 * several queries of these points may then run with CDX_SDF_REUSE_ORDER concurrently on other streams, each
 * ordered after this call. */
int cdx_sdf_query_order(const float* points, int64_t P, void* workspace, size_t workspace_bytes, cdx_stream_t stream);
#define CDX_SDF_REUSE_ORDER 1
#define CDX_SDF_MESH_CULLED 2
#define CDX_SDF_MESH_EXACT 4
#define CDX_SDF_SCHED_KEEP 8 /* cdx_sdf_query_batch, first query's flags: keep the schedule's order (durations still
                                recorded; the order is recomputed on the next launch without it) */
int cdx_sdf_mesh_flags(const void* mesh, int32_t* flags, cdx_stream_t stream);  /* waits on stream */
/* Up to four cdx_sdf_query calls in one launch (the SDF / Kin optimisers' three queries per iteration): each with
 * flags CDX_SDF_REUSE_ORDER | CDX_SDF_MESH_CULLED (its workspace already holds its points' order —
 * cdx_sdf_query_order — and its mesh has no NaN-capable face); outputs identical to the separate calls. */
typedef struct cdx_sdf_batch_query {
  const void* mesh;
  const float* faces;
  int64_t F;
  const float* points;
  int64_t P;
  float* sqdist;
  int32_t* sign;
  float* normals;
  float* clst;
  int32_t* face_idx; /* nullable */
  void* workspace;
  size_t workspace_bytes;
  int32_t flags;
  int32_t _pad;
} cdx_sdf_batch_query;
/* schedule (nullable): device bytes, all zero before their first use (at least
 * cdx_sdf_batch_schedule_bytes(n, P) for the queries' point counts P[n]) that carry each point group's walk time from
 * one launch to the next — the next launch of a batch with as many groups starts the heaviest groups first (the
 * optimiser loops' same points, an iteration apart); used in stream order only, by this function only.  The outputs do
 * not depend on it. */
size_t cdx_sdf_batch_schedule_bytes(int32_t n, const int64_t* P);
int cdx_sdf_query_batch(int32_t n, const cdx_sdf_batch_query* queries, void* schedule, size_t schedule_bytes,
                        cdx_stream_t stream);
int cdx_sdf_query(const void* mesh, const float* faces, int64_t F, const float* points, int64_t P, float* sqdist,
                  int32_t* sign, float* normals, float* clst, int32_t* face_idx, void* workspace,
                  size_t workspace_bytes, int32_t flags, cdx_stream_t stream);
/* Diagnostic work counters of cdx_sdf_forward / cdx_sdf_query (float path): out3 (nullable, host) =
 * [(point, face) pairs the culled kernel evaluated exactly — each lane's greedy seed face plus the pairs
 * its slab bounds could not rule out —, pairs of brute-force scans (the exact path), points queried]; read before `enable` applies.
 * enable 1: zero the counters and count from now on (one atomic per wave); 0: stop counting; −1: only
 * read.  Against P·F per call this is the culling's work saving. */
int cdx_sdf_stats(int32_t enable, uint64_t* out3, cdx_stream_t stream);
/* Diagnostic companion of cdx_sdf_stats: chunks (32 faces) the culled kernel's waves evaluated pairs in
 * since counting was enabled, summed over waves. */
int cdx_sdf_chunk_visits(uint64_t* out, cdx_stream_t stream);

/* ------------------------------------------------------------- ray casting ----------
 * First hit of R rays on a float32 triangle mesh, and the depth camera built on it: what the reference takes
 * from PyBullet's depth image, open3d's create_from_depth_image (get_observable_pcd.py:26-40) and open3d's
 * RaycastingScene.cast_rays (concatenate_pcd.py:41-49).  The rule is csrc/cdx_ray.h: the float64 Möller–Trumbore test
 * on the widened float32 vertices with a relative determinant threshold of 2⁻²⁰, tmin ≤ t ≤ tmax inclusive, d not
 * normalised (t in units of |d|), the smallest t wins and equal t goes to the smallest ORIGINAL face index.  Parity
 * with open3d, Embree and PyBullet is unpinned (none is a dependency).
 * cdx_ray_cast: origins, dirs [R·3] doubles.  Outputs t [R] (+inf on a miss), face [R] (−1 on a miss), uv [R·2]
 *   (nullable; the hit's barycentric u, v: the point is (1 − u − v)·v0 + u·v1 + v·v2; 0 on a miss).  A ray with a
 *   non-finite component or d = 0 is a miss.  mode CDX_RAY_SCAN: every face against every ray, on `faces` alone
 *   (mesh and ray_mesh may be NULL); CDX_RAY_WALK: the hierarchy of a prepared mesh — `mesh` from
 *   cdx_sdf_mesh_prepare and `ray_mesh` from cdx_ray_mesh_prepare, both of these `faces`; CDX_RAY_AUTO: the walk
 *   when both are given.  Both modes give the same bits on every mesh; on a mesh with a NaN-capable face
 *   (CDX_SDF_MESH_EXACT) the walk skips nothing, so the scan is the one to ask for.
 *   CDX_EINVAL: R < 0, F ≤ 0, F > INT32_MAX/9, null faces, origins, dirs, t or face (R > 0), an unknown mode, the
 *   walk without mesh or ray_mesh.  Nothing is written then.
 * cdx_ray_mesh_prepare: the walk's records (node balls, face vertices with their original index, in the mesh's
 *   order) from a prepared mesh of F faces into ray_mesh, cdx_ray_mesh_bytes(F) caller-owned device bytes
 *   (0 for a bad F).  One launch, no sync.
 * cdx_depth_render: the cast with the rays of a W×H pinhole camera generated in the kernel: pixel (i, j) — row i,
 *   column j — has the camera-frame direction ((j − cx)/fx, (i − cy)/fy, 1), x right, y down, z forward; intr =
 *   (fx, fy, cx, cy) and cam_to_world (row-major 4×4) are HOST doubles, read during the call.  depth [H·W] doubles =
 *   t, the z-depth (0 on a miss); face [H·W] (nullable).
 * Depth unprojection (create_from_depth_image, stated in csrc/cdx_ray.h): depth [H·W] of dtype CDX_DTYPE_F32,
 *   CDX_DTYPE_F64 or CDX_DEPTH_U16; pixels i, j = 0, stride, … in row-major order; z = depth/depth_scale in the depth's
 *   precision (float for uint16); dropped if depth == 0, z ≥ depth_trunc or — z_max not NaN — !(z < z_max); x, y in
 *   float64; `transform` (HOST, row-major 4×4, nullable) applied last.  Ordered compaction without atomics.
 *   cdx_depth_count: counts and their scan into workspace (cdx_depth_workspace(W, H, stride) bytes), *total (device
 *   int64) = the number of points.  cdx_depth_place: after a count on the same inputs and workspace; rows
 *   < capacity of points [capacity·3] are written. */
#define CDX_RAY_AUTO 0
#define CDX_RAY_SCAN 1
#define CDX_RAY_WALK 2
#define CDX_DEPTH_U16 2 /* depth dtype next to CDX_DTYPE_F32 / CDX_DTYPE_F64 */
size_t cdx_ray_mesh_bytes(int64_t F);
int cdx_ray_mesh_prepare(const void* mesh, int64_t F, void* ray_mesh, cdx_stream_t stream);
int cdx_ray_cast(const void* mesh, const void* ray_mesh, const float* faces, int64_t F, const double* origins,
                 const double* dirs, int64_t R, double tmin, double tmax, int32_t mode, double* t, int32_t* face,
                 double* uv, cdx_stream_t stream);
int cdx_depth_render(const void* mesh, const void* ray_mesh, const float* faces, int64_t F, int32_t W, int32_t H,
                     const double* intr, const double* cam_to_world, double tmin, double tmax, int32_t mode,
                     double* depth, int32_t* face, cdx_stream_t stream);
size_t cdx_depth_workspace(int32_t W, int32_t H, int32_t stride);
int cdx_depth_count(const void* depth, int32_t dtype, int32_t W, int32_t H, int32_t stride, double depth_scale,
                    double depth_trunc, double z_max, void* workspace, int64_t* total, cdx_stream_t stream);
int cdx_depth_place(const void* depth, int32_t dtype, int32_t W, int32_t H, int32_t stride, const double* intr,
                    double depth_scale, double depth_trunc, double z_max, const double* transform,
                    const void* workspace, int64_t capacity, double* points, cdx_stream_t stream);
/* Diagnostic counters of the walk: out2 (nullable, host) = [(ray, face) pairs evaluated, rays cast]; enable as
 * cdx_sdf_stats. */
int cdx_ray_stats(int32_t enable, uint64_t* out2, cdx_stream_t stream);

/* Library identification (gfx arch string compiled in). */
const char* cdx_version(void);

/* Per-stage kernel timing with HIP events recorded on the launch stream (off by default).
 * Stages: 0 closure query generation, 1 GPIS mean, 2 GPIS std (whitened K*·L⁻ᵀ fp64 GEMM only; in a
 * screened closure the refine pass and its merge), 3 closure cost+backward, 4 GPIS ∇std GEMM only,
 * 5 the closure's split-precision screen (fp16 GEMM + selection).  cdx_profile_read syncs on the
 * recorded events, returns the summed milliseconds and launch counts per stage (arrays of 6),
 * and clears the pool (4096 launches per stage).  `stages` is a bit mask (bit s = stage s; 0x3f
 * all, 0 off): each event record costs ≈ 5 µs of stream time, so a throughput run times only
 * the stages it reports. */
int cdx_profile_enable(int stages);
int cdx_profile_read(double* ms6, int64_t* count6);

/* sizeof(cdx_gpis), sizeof(cdx_body), sizeof(cdx_chain), sizeof(cdx_problem),
 * sizeof(cdx_collision), sizeof(cdx_adam), sizeof(cdx_opt_buffers), sizeof(cdx_force_eq),
 * sizeof(cdx_screen_report), sizeof(cdx_kin_params), sizeof(cdx_kin_opt), sizeof(cdx_kin_opt_buffers)
 * — lets a binding verify its struct layouts before the first call. */
void cdx_abi_sizes(size_t* out13);

/* Test hook: D[16×16] = A[16×4]·B[4×16] through one v_mfma_f64_16x16x4_f64 (checks the
 * fragment layout the GPIS std kernel relies on). */
int cdx_selftest_mfma_f64(const double* A, const double* B, double* D, cdx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CDX_H */
