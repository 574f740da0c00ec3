"""k-nearest-neighbour search on an MI355X (cdx_knn: the scan and the grid walk) against the numpy statement of
csrc/cdx_knn.h, bit for bit; cdx_cloud_normals against the host build and numpy; and the entry points on top:
knn / KnnGrid / estimate_normals / orient_normals_towards_camera_location / statistical_outlier_mask /
remove_statistical_outlier / point_cloud_distance / GPIS.fit_pointcloud(outlier=...)."""
import numpy as np
import pytest
import torch

from tests import _fps, _knn
from tests._knn import AUTO, GRID, INF, SCAN, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4  # output rows past the last, preset and found untouched
TILE = 1024  # KNN_TILE of csrc/cdx_knn.hip: cloud rows per LDS tile of the scan
QPB = 4  # queries per workgroup of both paths
CASES = _knn.shared_cases()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def device_grid(x, buffer=None):
    from compliancedex_amd import _native as N
    lib = N.load()
    need = lib.cdx_knn_grid_bytes(x.shape[0])
    assert need > 0
    if buffer is None:
        buffer = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert buffer.numel() >= need
    dtype = N.DTYPE_F32 if x.dtype == torch.float32 else N.DTYPE_F64
    N.check(lib.cdx_knn_prepare(N.ptr(x), dtype, x.shape[0], N.ptr(buffer), N.stream_ptr()), "cdx_knn_prepare")
    return buffer


def device_knn(X, K, Q=None, max_d2=INF, mode=SCAN, grid=None, x=None):
    """cdx_knn through the C ABI on host arrays uploaded in X's dtype: (idx, d2, count) as numpy arrays; GUARD rows
    past each output are checked to be untouched.  The grid is prepared here for mode GRID / AUTO unless given."""
    from compliancedex_amd import _native as N
    lib = N.load()
    X = np.ascontiguousarray(X)
    x = torch.from_numpy(X).to(DEV) if x is None else x
    q = None if Q is None else torch.from_numpy(np.ascontiguousarray(Q, dtype=X.dtype)).to(DEV)
    P, M = len(X), len(X) if Q is None else len(Q)
    if grid is None and mode != SCAN:
        grid = device_grid(x)
    idx = torch.full((M + GUARD, K), -5, dtype=torch.int64, device=DEV)
    d2 = torch.full((M + GUARD, K), -7.0, dtype=torch.float64, device=DEV)
    count = torch.full((M + GUARD,), -9, dtype=torch.int32, device=DEV)
    dtype = N.DTYPE_F32 if X.dtype == np.float32 else N.DTYPE_F64
    assert lib.cdx_knn_workspace(P, M, K, mode) > 0
    N.check(lib.cdx_knn(N.ptr(x), dtype, P, N.ptr(grid), N.ptr(q), M, K, max_d2, mode, None, N.ptr(idx), N.ptr(d2),
                        N.ptr(count), N.stream_ptr()), "cdx_knn")
    idx, d2, count = idx.cpu().numpy(), d2.cpu().numpy(), count.cpu().numpy()
    assert np.all(idx[M:] == -5) and np.all(d2[M:] == -7.0) and np.all(count[M:] == -9)
    return idx[:M], d2[:M], count[:M]


def equal(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_cases_both_paths(name):
    """Every case of the host build in modes 1 and 2 against numpy, bit for bit; mode 0 equals both; a float32 cloud
    equals the same cloud widened to float64."""
    c = CASES[name]
    ref = _knn.reference(name)
    for mode in (SCAN, GRID, AUTO):
        assert equal(device_knn(c["X"], c["K"], c["Q"], c["max_d2"], mode), ref), (name, mode)
    if c["X"].dtype == np.float32:
        wide = c["X"].astype(np.float64)
        for mode in (SCAN, GRID):
            assert equal(device_knn(wide, c["K"], None, c["max_d2"], mode), ref), (name, mode)


@pytest.mark.parametrize("P", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_seams(P):
    """P around the scan's LDS tile, M not a multiple of the queries per workgroup, K = 1, 63 and 64."""
    X = _fps.normal_cloud(P, seed=P)
    for K, M in ((1, QPB + 1), (63, 2 * QPB - 1), (64, 1), (64, 3 * QPB + 2)):
        Q = np.concatenate([X[-(M // 2 + 1):], _fps.normal_cloud(M, seed=K)])[:M]  # rows of the cloud, then others
        ref = _knn.numpy_knn(X, K, Q)
        for mode in (SCAN, GRID):
            assert equal(device_knn(X, K, Q, INF, mode), ref), (P, K, M, mode)


def test_ragged_70001():
    """All 70001 rows query their own cloud, K = 30: the scan equals the walk on every row, and both equal numpy on a
    1024-row slice."""
    X = _fps.large_cases()["ragged_70001"][0]
    x = torch.from_numpy(X).to(DEV)
    scan = device_knn(X, 30, None, INF, SCAN, x=x)
    walk = device_knn(X, 30, None, INF, GRID, x=x)
    assert equal(scan, walk)
    rows = slice(34000, 35024)
    ref = _knn.numpy_knn(X, 30, X[rows])
    assert equal([a[rows] for a in scan], ref)


def test_radius_above_the_automatic_threshold():
    """Hybrid search on 20 000 rows, where automatic mode prepares and walks a grid: many lists are cut short by the
    radius, so the walk must stop on max_d2 and not on a full list.  The scan equals the walk on every row, both equal
    numpy on a 512-row slice, and far queries find nothing."""
    from compliancedex_amd import knn
    from compliancedex_amd.pointcloud import AUTO_PREPARE_ROWS
    rng = np.random.default_rng(20000)
    base = _fps.banana()
    X = base[rng.integers(0, len(base), 20000)] + 0.002 * rng.standard_normal((20000, 3))
    assert len(X) > AUTO_PREPARE_ROWS
    x = torch.from_numpy(X).to(DEV)
    radius = 0.003  # about 0.46 of the lists come out short
    scan = device_knn(X, 30, None, radius * radius, SCAN, x=x)
    walk = device_knn(X, 30, None, radius * radius, GRID, x=x)
    assert equal(scan, walk)
    assert 0.3 < (scan[2] < 30).mean() < 0.7
    rows = slice(9000, 9512)
    assert equal([a[rows] for a in walk], _knn.numpy_knn(X, 30, X[rows], radius * radius))
    auto = knn(x, 30, max_distance=radius)
    assert equal([a.cpu().numpy() for a in auto], scan)
    Q = np.concatenate([X[:5] + 0.5, _knn.outside_queries(), X[5:8]])
    ref = _knn.numpy_knn(X, 30, Q, radius * radius)
    assert (ref[2][:-3] == 0).all() and (ref[2][-3:] > 0).all()
    assert equal(device_knn(X, 30, Q, radius * radius, GRID, x=x), ref)
    assert equal(device_knn(X, 30, Q, 0.0, GRID, x=x), _knn.numpy_knn(X, 30, Q, 0.0))


def grid_shape_cases():
    rng = np.random.default_rng(17)
    one = np.tile(np.array([[0.5, -1.25, 3.0]]), (200, 1))
    few = _fps.normal_cloud(90, seed=19)
    few[5:] = np.nan  # K greater than the finite rows
    far = np.array([[1e3, 1e3, 1e3], [-1e6, 0.0, 0.0], [0.0, 1e12, -1e12], [1e200, 0.0, 0.0], [0.3, 0.1, 1e-3]])
    return {
        "one_cell": (one, 30, np.concatenate([one[:3], far])),
        "two_clusters": (_knn.two_clusters(), 64, None),
        "two_clusters_between": (_knn.two_clusters(), 30, rng.uniform(-1e3, 1e3, (37, 3))),
        "planar": (_knn.planar_cloud(), 30, None),
        "planar_off_plane": (_knn.planar_cloud(), 30, rng.uniform(-2, 2, (41, 3))),
        "far_outside": (_fps.normal_cloud(3000, seed=23), 30, np.concatenate([far, _knn.outside_queries()])),
        "K_above_finite_rows": (few, 30, None),
        "line": (np.stack([np.linspace(0, 1, 700), np.zeros(700), np.zeros(700)], axis=1), 20, None),
    }


@pytest.mark.parametrize("name", sorted(grid_shape_cases()))
def test_grid_shapes_end_and_equal_the_scan(name):
    X, K, Q = grid_shape_cases()[name]
    ref = _knn.numpy_knn(X, K, Q)
    assert equal(device_knn(X, K, Q, INF, SCAN), ref)
    assert equal(device_knn(X, K, Q, INF, GRID), ref)


@pytest.mark.parametrize("mode", [SCAN, GRID], ids=["scan", "grid"])
def test_row_independence(mode):
    """Poisoned query rows get count 0 and the other rows keep their bits; poisoned cloud rows leave every list equal
    to that of the cloud with those rows deleted, indices mapped back; the same for cdx_cloud_normals."""
    X = _fps.normal_cloud(1500, seed=31)
    Q = _fps.normal_cloud(203, seed=32)
    K = 30
    clean = device_knn(X, K, Q, INF, mode)
    bad = np.array([0, 5, 64, 101, 202])
    Qp = Q.copy()
    Qp[bad, np.arange(5) % 3] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    idx, d2, count = device_knn(X, K, Qp, INF, mode)
    assert (count[bad] == 0).all() and (idx[bad] == -1).all() and (d2[bad] == INF).all()
    keep = np.setdiff1d(np.arange(len(Q)), bad)
    assert equal([idx[keep], d2[keep], count[keep]], [a[keep] for a in clean])
    rows = np.array([3, 63, 64, 700, 1023, 1024, 1499])
    Xp = X.copy()
    Xp[rows, np.arange(7) % 3] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]
    left = np.setdiff1d(np.arange(len(X)), rows)
    i2, dd2, c2 = device_knn(X[left], K, Q, INF, mode)
    poisoned = device_knn(Xp, K, Q, INF, mode)
    assert equal(poisoned, [np.where(i2 >= 0, left[np.maximum(i2, 0)], -1), dd2, c2])
    # normals: the lists of the poisoned cloud querying itself
    from compliancedex_amd.pointcloud import normals_from_neighbours
    xp = torch.from_numpy(Xp).to(DEV)
    li, _, lc = device_knn(Xp, K, None, INF, mode)
    n, w = normals_from_neighbours(xp, torch.from_numpy(li).to(DEV), torch.from_numpy(lc).to(DEV),
                                   return_eigenvalues=True)
    n, w = n.cpu().numpy(), w.cpu().numpy()
    assert np.isnan(n[rows]).all() and np.isnan(w[rows]).all()
    xl = torch.from_numpy(X[left]).to(DEV)
    li2, _, lc2 = device_knn(X[left], K, None, INF, mode)
    n2, w2 = normals_from_neighbours(xl, torch.from_numpy(li2).to(DEV), torch.from_numpy(lc2).to(DEV),
                                     return_eigenvalues=True)
    assert same_bits(n[left], n2.cpu().numpy()) and same_bits(w[left], w2.cpu().numpy())


def test_grid_and_workspace_reuse():
    """Two different clouds through one grid buffer without clearing: the results equal fresh-buffer results."""
    from compliancedex_amd import _native as N
    A, B = _fps.normal_cloud(5000, seed=51), 3.0 * _fps.normal_cloud(1300, seed=52) + 7.0
    a, b = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    buffer = torch.full((N.load().cdx_knn_grid_bytes(5000),), 0xA5, dtype=torch.uint8, device=DEV)
    fresh_a = device_knn(A, 20, None, INF, GRID, x=a)
    fresh_b = device_knn(B, 20, None, INF, GRID, x=b)
    for _ in range(2):
        assert equal(device_knn(A, 20, None, INF, GRID, grid=device_grid(a, buffer), x=a), fresh_a)
        assert equal(device_knn(B, 20, None, INF, GRID, grid=device_grid(b, buffer), x=b), fresh_b)
    assert equal([v[:256] for v in fresh_a], _knn.numpy_knn(A, 20, A[:256]))


def test_python_knn_and_grid_handle():
    from compliancedex_amd import KnnGrid, knn
    X = _fps.banana()
    x = torch.from_numpy(X).to(DEV)
    ref = _knn.reference("banana_f64")
    grid = KnnGrid(x)
    for kw in (dict(mode="scan"), dict(mode="grid"), dict(mode="grid", grid=grid), dict(mode="auto", grid=grid), {}):
        idx, d2, count = knn(x, 30, **kw)
        assert equal([idx.cpu().numpy(), d2.cpu().numpy(), count.cpu().numpy()], ref), kw
    Q = _fps.normal_cloud(50, seed=3) * 0.05
    out = knn(x, 7, queries=torch.from_numpy(Q).to(DEV), max_distance=0.03, grid=grid)
    assert equal([o.cpu().numpy() for o in out], _knn.numpy_knn(X, 7, Q, 0.03 * 0.03))
    out = knn(x.float(), 7, queries=torch.from_numpy(Q).to(DEV))  # mixed dtypes: both widened
    assert equal([o.cpu().numpy() for o in out], _knn.numpy_knn(X.astype(np.float32), 7, Q))
    grid.prepare(x[:500])
    out = knn(x[:500], 3, grid=grid)
    assert equal([o.cpu().numpy() for o in out], _knn.numpy_knn(X[:500], 3))
    # a strided cloud is served by its own grid; a cloud written to after prepare is refused until prepared again
    y = torch.from_numpy(np.concatenate([X, X], axis=1)).to(DEV)[:, 3:]
    assert not y.is_contiguous()
    gy = KnnGrid(y)
    assert equal([o.cpu().numpy() for o in knn(y, 5, grid=gy)], _knn.numpy_knn(X, 5))
    z = x.clone()
    gz = KnnGrid(z)
    z[0, 0] += 1.0
    with pytest.raises(ValueError, match="written to"):
        knn(z, 5, grid=gz)
    assert equal([o.cpu().numpy() for o in knn(z, 5, grid=gz.prepare(z))], _knn.numpy_knn(z.cpu().numpy(), 5))


def test_estimate_normals_on_the_banana_cloud():
    from compliancedex_amd import estimate_normals, knn, orient_normals_towards_camera_location
    from compliancedex_amd.pointcloud import normals_from_neighbours
    X = _fps.banana()
    x = torch.from_numpy(X).to(DEV)
    idx, _, count = _knn.reference("banana_f64")
    eye = np.array([0.1, -0.4, 0.6])
    for e in (None, eye):
        n, w = estimate_normals(x, knn=30, camera_location=None if e is None else e.tolist(), return_eigenvalues=True)
        n, w = n.cpu().numpy(), w.cpu().numpy()
        hn, hw, _ = _knn.host_normals(X, idx, count, e)
        rn, rw, _ = _knn.numpy_normals(X, idx, count, e)
        assert same_bits(n, hn) and same_bits(w, hw) and same_bits(n, rn) and same_bits(w, rw)
        if e is None:
            lead = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], axis=1)
            assert (lead > 0).all()
        else:
            d = eye[None, :] - X
            assert ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] >= 0).all()
    plain = estimate_normals(x)
    turned = orient_normals_towards_camera_location(x, plain, eye.tolist())
    assert same_bits(turned.cpu().numpy(), n)
    assert same_bits(estimate_normals(x.float()).cpu().numpy(),
                     _knn.numpy_normals(X.astype(np.float32), *_knn.numpy_knn(X.astype(np.float32), 30)[::2])[0])
    # radius = knn with max_distance
    li, _, lc = knn(x, 30, max_distance=0.006)
    assert int(lc.min()) < 30
    assert torch.equal(estimate_normals(x, knn=30, radius=0.006), normals_from_neighbours(x, li, lc))
    rn, _, _ = _knn.numpy_normals(X, *_knn.numpy_knn(X, 30, None, 0.006 * 0.006)[::2])
    assert same_bits(estimate_normals(x, knn=30, radius=0.006).cpu().numpy(), rn)


def _icosphere(level=3):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1),
         (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    tri = np.array(v, np.float64)[np.array(f)]
    tri /= np.linalg.norm(tri, axis=2, keepdims=True)
    for _ in range(level):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = [m / np.linalg.norm(m, axis=1, keepdims=True) for m in (a + b, b + c, c + a)]
        tri = np.concatenate([np.stack(t3, axis=1) for t3 in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return tri


def test_sphere_normals():
    """An accuracy sanity check, not parity: a 4096-point Poisson-disk cloud of a unit sphere mesh (1280 faces), normals
    oriented to an eye at the centre.  The largest angle to the inward radial direction is printed and bounded by what
    the numpy restatement gives on the same cloud, plus nothing."""
    from compliancedex_amd import estimate_normals, sample_points_poisson_disk
    mesh = torch.from_numpy(_icosphere()).to(DEV)
    cloud = sample_points_poisson_disk(mesh, 4096, init_factor=5, seed=1)
    X = cloud.cpu().numpy().astype(np.float64)
    n = estimate_normals(cloud, knn=30, camera_location=(0.0, 0.0, 0.0)).cpu().numpy()
    rn, _, _ = _knn.numpy_normals(X, *_knn.numpy_knn(X, 30)[::2], eye=np.zeros(3))
    inward = -X / np.linalg.norm(X, axis=1, keepdims=True)

    def worst(v):
        return float(np.degrees(np.arccos(np.clip((v * inward).sum(axis=1), -1.0, 1.0))).max())

    print(f"sphere: largest angle to the radial direction {worst(n):.4f}° (numpy restatement {worst(rn):.4f}°)")
    assert worst(n) <= worst(rn)
    assert worst(rn) < 10.0  # the cloud lies on facets at most 0.6 % inside the sphere, ~0.08 apart: a few degrees


def test_outlier_entry_points():
    from compliancedex_amd import point_cloud_distance, remove_statistical_outlier, statistical_outlier_mask
    X, rows = _knn.salted_banana()
    x = torch.from_numpy(X).to(DEV)
    keep = statistical_outlier_mask(x, 20, 2.0)
    assert keep.dtype == torch.bool and np.flatnonzero(~keep.cpu().numpy()).tolist() == rows.tolist()
    assert np.array_equal(keep.cpu().numpy(), _knn.numpy_outlier_mask(X, 20, 2.0)[0])
    kept, index = remove_statistical_outlier(x, 20, 2.0)
    left = np.setdiff1d(np.arange(len(X)), rows)
    assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), left)
    assert same_bits(kept.cpu().numpy(), X[left])
    Y = x.clone()
    Y[7, 1] = float("nan")
    assert not bool(statistical_outlier_mask(Y, 20, 2.0)[7])
    # cloud-to-cloud distance
    S = _fps.normal_cloud(333, seed=61) * 0.05
    s = torch.from_numpy(S).to(DEV)
    d = point_cloud_distance(s, x)
    assert d.dtype == torch.float64 and same_bits(d.cpu().numpy(), np.sqrt(_knn.numpy_knn(X, 1, S)[1][:, 0]))
    nothing = torch.full((9, 3), float("nan"), dtype=torch.float64, device=DEV)
    assert bool((point_cloud_distance(s, nothing) == INF).all())


def test_fit_pointcloud_with_outlier_removal():
    from compliancedex_amd import GPIS, completion_arrays
    from compliancedex_amd.pointcloud import bbox_center, fps
    X, rows = _knn.salted_banana()
    x = torch.from_numpy(X).to(DEV)
    weights = torch.rand(50, 200, generator=torch.Generator().manual_seed(9)).to(DEV)
    g = GPIS(0.08, 1.0).fit_pointcloud(x, weights=weights, outlier=(20, 2.0))
    masked = np.where(_knn.numpy_outlier_mask(X, 20, 2.0)[0][:, None], X, np.nan)
    chosen = g.sample_index.cpu().numpy()
    assert np.array_equal(chosen, _fps.numpy_fps(masked, 200)[0])
    assert not set(rows.tolist()) & set(chosen.tolist())
    assert bool(torch.isfinite(g.E11).all())
    left = np.setdiff1d(np.arange(len(X)), rows)
    # without `outlier`: the tensors of a direct fps + completion_arrays + fit, and the outliers are sampled
    h = GPIS(0.08, 1.0).fit_pointcloud(x, weights=weights)
    sel, _, surface = fps(x, 200, 0, gather=True)
    X1, y, nz = completion_arrays(surface, 0.15, 50, 30.0, (0.2, 0.005, 0.1), center=bbox_center(x), weights=weights)
    d = GPIS(0.08, 1.0)
    d.fit(X1, y, noise=nz)
    assert torch.equal(h.sample_index, sel) and set(rows.tolist()) <= set(sel.cpu().numpy().tolist())
    for name in ("X1", "y1", "R", "E11"):
        assert torch.equal(getattr(h, name), getattr(d, name)), name
    # the exterior points sit around the box of the kept rows
    centre = torch.from_numpy(0.5 * (X[left].min(0) + X[left].max(0))).to(DEV)
    from compliancedex_amd.pointcloud import exterior_points
    assert torch.equal(g.X1[:14], exterior_points(0.15, DEV) + centre)


def test_bad_arguments():
    from compliancedex_amd import KnnGrid, _native as N, estimate_normals, knn, point_cloud_distance
    from compliancedex_amd import statistical_outlier_mask
    lib = N.load()
    x = torch.zeros(10, 3, dtype=torch.float64, device=DEV)
    idx = torch.zeros(10, 3, dtype=torch.int64, device=DEV)
    count = torch.zeros(10, dtype=torch.int32, device=DEV)
    out = torch.zeros(10, 3, dtype=torch.float64, device=DEV)
    s = N.stream_ptr()

    def call(X=N.ptr(x), dtype=N.DTYPE_F64, P=10, grid=None, M=10, K=3, mode=SCAN):
        return lib.cdx_knn(X, dtype, P, grid, None, M, K, INF, mode, None, N.ptr(idx), None, None, s)

    assert call() == 0
    for kw in (dict(K=0), dict(K=65), dict(P=0), dict(P=-1), dict(P=1 << 31), dict(M=-1), dict(X=None),
               dict(mode=GRID), dict(mode=3), dict(mode=-1), dict(dtype=2)):
        assert call(**kw) == -1, kw
    assert lib.cdx_knn_grid_bytes(0) == 0 and lib.cdx_knn_workspace(10, 10, 65, 0) == 0
    assert lib.cdx_knn_prepare(None, N.DTYPE_F64, 10, N.ptr(out), s) == -1
    assert lib.cdx_knn_prepare(N.ptr(x), N.DTYPE_F64, 10, None, s) == -1
    assert lib.cdx_cloud_normals(N.ptr(x), N.DTYPE_F64, 10, N.ptr(idx), N.ptr(count), 65, None, N.ptr(out), None, s) == -1
    assert lib.cdx_cloud_normals(N.ptr(x), 5, 10, N.ptr(idx), N.ptr(count), 3, None, N.ptr(out), None, s) == -1
    assert lib.cdx_cloud_normals(N.ptr(x), N.DTYPE_F64, 10, None, N.ptr(count), 3, None, N.ptr(out), None, s) == -1
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn(x.cpu(), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        estimate_normals(x.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        statistical_outlier_mask(x.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        point_cloud_distance(x.cpu(), x)
    with pytest.raises(ValueError):
        knn(x, 0)
    with pytest.raises(ValueError):
        knn(x, 65)
    with pytest.raises(ValueError):
        knn(x, 3, mode="tree")
    with pytest.raises(ValueError):
        knn(x, 3, max_distance=-1.0)
    with pytest.raises(ValueError):
        knn(x[:, :2], 3)
    with pytest.raises(TypeError):
        knn(x.to(torch.float16), 3)
    with pytest.raises(TypeError):
        knn(x, 3, grid=out)
    with pytest.raises(ValueError):
        knn(x, 3, grid=KnnGrid(out))
