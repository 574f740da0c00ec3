"""Helpers shared by test_knn_cpu.py and test_gpu_knn.py: the rule of csrc/cdx_knn.h stated in numpy (neighbours,
covariance, Jacobi, normals, the outlier mask), the host build's bindings and the cases both files run."""

import numpy as np

from tests import _fps
from tests._host import host, p

F32, F64 = 0, 1  # CDX_DTYPE_*
AUTO, SCAN, GRID = 0, 1, 2  # CDX_KNN_*
MAX_K = 64
MAX_DIM = 256  # CDX_KNN_MAX_DIM
SWEEPS = 10  # CDX_KNN_SWEEPS
INF = float("inf")

same_bits = _fps.same_bits


# ---------------------------------------------------------------- numpy statements

def numpy_knn(X, K, Q=None, max_d2=INF, chunk=64):
    """(idx int64 [M, K], d2 f64 [M, K], count int32 [M]): brute force, np.lexsort on (index, d2) per query, chunked
    over query rows so that no P × M × 3 array is ever whole in memory."""
    X = np.asarray(X).astype(np.float64)
    Q = X if Q is None else np.asarray(Q).astype(np.float64)
    P, M = len(X), len(Q)
    idx = np.full((M, K), -1, np.int64)
    d2 = np.full((M, K), INF)
    count = np.zeros(M, np.int32)
    row_ok = np.isfinite(X).all(axis=1)
    rows = np.arange(P)
    take = min(K, P)
    with np.errstate(invalid="ignore", over="ignore"):
        for m0 in range(0, M, chunk):
            q = Q[m0:m0 + chunk]
            dx = X[None, :, 0] - q[:, None, 0]
            dy = X[None, :, 1] - q[:, None, 1]
            dz = X[None, :, 2] - q[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            ok = row_ok[None, :] & np.isfinite(q).all(axis=1)[:, None] & ~(d > max_d2)
            order = np.lexsort((np.broadcast_to(rows, d.shape), d, ~ok), axis=-1)[:, :take]
            got = np.take_along_axis(ok, order, axis=1)
            idx[m0:m0 + chunk, :take] = np.where(got, order, -1)
            d2[m0:m0 + chunk, :take] = np.where(got, np.take_along_axis(d, order, axis=1), INF)
            count[m0:m0 + chunk] = got.sum(axis=1)
    return idx, d2, count


def numpy_covariance(X, idx, count):
    """cov f64 [P, 6] = (00, 01, 02, 11, 12, 22): sequential sums in list order, as the rule states them."""
    X = np.asarray(X).astype(np.float64)
    P, K = idx.shape
    c = count.astype(np.int64)
    s = np.zeros((P, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(K):
            use = t < c
            x = X[np.where(use, idx[:, t], 0)]
            s = np.where(use[:, None], s + x, s)
        mean = s / np.maximum(c, 1)[:, None].astype(np.float64)
        mean = np.where((c > 0)[:, None], mean, 0.0)
        acc = np.zeros((P, 6))
        for t in range(K):
            use = t < c
            d = X[np.where(use, idx[:, t], 0)] - mean
            prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1],
                             d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], axis=1)
            acc = np.where(use[:, None], acc + prod, acc)
        return acc / np.maximum(c, 1)[:, None].astype(np.float64)


def _rotate(A, V, act, pp, qq, pq, rp, rq, colp, colq):
    """One Jacobi rotation of the rule on every matrix where `act`; A is a dict of the six entries, V [n, 3, 3]."""
    app, aqq, apq = A[pp], A[qq], A[pq]
    g = np.abs(apq)
    tiny = (np.abs(app) + g == np.abs(app)) & (np.abs(aqq) + g == np.abs(aqq))
    live = act & (g != 0.0)
    zero = live & tiny
    rot = live & ~tiny
    theta = (aqq - app) / (2.0 * apq)
    den = np.abs(theta) + np.sqrt(theta * theta + 1.0)
    t = np.where(theta < 0.0, -1.0, 1.0) / den
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    A[pp] = np.where(rot, app - h, app)
    A[qq] = np.where(rot, aqq + h, aqq)
    A[pq] = np.where(rot | zero, 0.0, apq)
    x, y = A[rp], A[rq]
    A[rp] = np.where(rot, c * x - s * y, x)
    A[rq] = np.where(rot, s * x + c * y, y)
    x, y = V[:, :, colp].copy(), V[:, :, colq].copy()
    V[:, :, colp] = np.where(rot[:, None], c[:, None] * x - s[:, None] * y, x)
    V[:, :, colq] = np.where(rot[:, None], s[:, None] * x + c[:, None] * y, y)


def numpy_sym3_eig(cov):
    """(w [n, 3] ascending, V [n, 3, 3] eigenvectors in columns) of cov [n, 6]: the Jacobi rule operation by
    operation, all matrices at once; a matrix that has stopped (off == 0 or NaN) stays stopped."""
    cov = np.asarray(cov, np.float64)
    n = len(cov)
    A = {k: cov[:, i].copy() for i, k in enumerate(("00", "01", "02", "11", "12", "22"))}
    V = np.tile(np.eye(3), (n, 1, 1))
    act = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            off = (A["01"] * A["01"] + A["02"] * A["02"]) + A["12"] * A["12"]
            act = act & (off != 0.0) & ~np.isnan(off)
            if not act.any():
                break
            _rotate(A, V, act, "00", "11", "01", "02", "12", 0, 1)
            _rotate(A, V, act, "00", "22", "02", "01", "12", 0, 2)
            _rotate(A, V, act, "11", "22", "12", "01", "02", 1, 2)
    w = np.stack([A["00"], A["11"], A["22"]], axis=1)
    for a, b in ((0, 1), (1, 2), (0, 1)):
        swap = w[:, a] > w[:, b]
        wa, wb = w[:, a].copy(), w[:, b].copy()
        w[:, a], w[:, b] = np.where(swap, wb, wa), np.where(swap, wa, wb)
        va, vb = V[:, :, a].copy(), V[:, :, b].copy()
        V[:, :, a] = np.where(swap[:, None], vb, va)
        V[:, :, b] = np.where(swap[:, None], va, vb)
    return w, V


def numpy_normals(X, idx, count, eye=None):
    """(normals [P, 3], eigenvalues [P, 3], cov [P, 6]) of the rule."""
    X = np.asarray(X).astype(np.float64)
    cov = numpy_covariance(X, idx, count)
    w, V = numpy_sym3_eig(cov)
    n = V[:, :, 0].copy()
    fallback = (count < 3) | ~np.isfinite(cov).all(axis=1)
    n[fallback] = (0.0, 0.0, 1.0)
    w[fallback] = np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        if eye is not None:
            e = np.asarray(eye, np.float64)[None, :] - X
            flip = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2] < 0.0
        else:
            a = np.abs(n)
            lead = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), n[:, 0],
                            np.where(a[:, 1] >= a[:, 2], n[:, 1], n[:, 2]))
            flip = lead < 0.0
    n = np.where(flip[:, None], -n, n)
    bad = ~np.isfinite(X).all(axis=1)
    n[bad] = np.nan
    w[bad] = np.nan
    return n, w, cov


def numpy_outlier_mask(X, nb_neighbors=20, std_ratio=2.0):
    """(keep bool [P], avg f64 [P], threshold): the statement of pointcloud.statistical_outlier_mask."""
    _, d2, count = numpy_knn(X, nb_neighbors)
    slot = np.arange(nb_neighbors)[None, :] < count[:, None]
    avg = np.where(slot, np.sqrt(np.where(slot, d2, 0.0)), 0.0).sum(axis=1) / np.maximum(count, 1)
    found = count > 0
    mean = avg[found].mean()
    std = avg[found].std(ddof=1) if found.sum() > 1 else 0.0
    thr = mean + std_ratio * std
    return found & (avg <= thr), avg, thr


# ---------------------------------------------------------------- the host build

def _dtype(X):
    return {np.dtype(np.float32): F32, np.dtype(np.float64): F64}[X.dtype]


def host_knn(X, K, Q=None, max_d2=INF, mode=SCAN, dtype=None):
    """cdxh_knn on host arrays in their own dtype: (rc, idx, d2, count)."""
    lib = host()
    X = np.ascontiguousarray(X)
    Qc = None if Q is None else np.ascontiguousarray(Q, dtype=X.dtype)
    M = len(X) if Q is None else len(Qc)
    rows = max(K, 0)
    idx = np.full((M, rows), -7, np.int64)
    d2 = np.full((M, rows), -7.0)
    count = np.full(M, -7, np.int32)
    rc = lib.cdxh_knn(p(X), _dtype(X) if dtype is None else dtype, len(X), None if Qc is None else p(Qc), M, K,
                      max_d2, mode, p(idx), p(d2), p(count))
    return rc, idx, d2, count


def host_normals(X, idx, count, eye=None):
    """cdxh_cloud_normals: (normals, eigenvalues, cov)."""
    lib = host()
    X = np.ascontiguousarray(X)
    idx, count = np.ascontiguousarray(idx, np.int64), np.ascontiguousarray(count, np.int32)
    P, K = idx.shape
    n, w, cov = np.full((P, 3), -7.0), np.full((P, 3), -7.0), np.full((P, 6), -7.0)
    e = None if eye is None else np.ascontiguousarray(eye, np.float64)
    rc = lib.cdxh_cloud_normals(p(X), _dtype(X), P, p(idx), p(count), K, None if e is None else p(e), p(n), p(w),
                                p(cov))
    assert rc == 0
    return n, w, cov


def host_sym3_eig(cov):
    lib = host()
    cov = np.ascontiguousarray(cov, np.float64)
    w, V = np.zeros((len(cov), 3)), np.zeros((len(cov), 3, 3))
    lib.cdxh_sym3_eig(p(cov), len(cov), p(w), p(V))
    return w, V


def host_grid(X):
    """cdxh_knn_grid of a float64 cloud: dict(info [4] = lo, inv; dims [3]; cell [P, 3]; below, above [3, MAX_DIM])."""
    lib = host()
    X = np.ascontiguousarray(X, np.float64)
    g = dict(info=np.zeros(4), dims=np.zeros(3, np.int32), cell=np.zeros((len(X), 3), np.int32),
             below=np.zeros((3, MAX_DIM)), above=np.zeros((3, MAX_DIM)))
    assert lib.cdxh_knn_grid(p(X), len(X), p(g["info"]), p(g["dims"]), p(g["cell"]), p(g["below"]), p(g["above"])) == 0
    return g


def host_ring_bound(g, Q, r):
    """(cq int32 [M, 3], bound f64 [M], none bool [M]) of cdx::knn_ring_bound at ring r, in the kernel's arithmetic."""
    lib = host()
    Q = np.ascontiguousarray(Q, np.float64)
    cq, bound, none = np.zeros((len(Q), 3), np.int32), np.zeros(len(Q)), np.zeros(len(Q), np.int32)
    assert lib.cdxh_knn_ring_bound(p(g["info"]), p(g["dims"]), p(g["below"]), p(g["above"]), p(Q), len(Q), r, p(cq),
                                   p(bound), p(none)) == 0
    return cq, bound, none.astype(bool)


# ---------------------------------------------------------------- clouds and cases

def lattice_queries(n=512):
    """Rows of the 35 × 35 × 33 lattice: every K-th distance there is shared by several rows."""
    X = _fps.lattice(35, 35, 33)
    return X[np.random.default_rng(512).choice(len(X), n, replace=False)]


def two_clusters():
    """Two clusters of width ~10⁻³ whose centres are 10³ apart: a million cluster widths of empty space.  (The grid
    spans the box with at most 256 cells an axis, so a gap cannot be stated in cell widths beyond that.)"""
    rng = np.random.default_rng(22)
    a = 1e-3 * rng.standard_normal((200, 3))
    b = 1e-3 * rng.standard_normal((150, 3)) + np.array([1e3, -2e2, 5e2])
    return np.concatenate([a, b])[rng.permutation(350)]


def outside_queries():
    """Queries beyond every side of a standard normal cloud's box, near and far, and at huge magnitudes."""
    q = []
    for s in (6.0, 50.0, 1e6, 1e150):
        for a in range(3):
            for sign in (-1.0, 1.0):
                v = np.zeros(3)
                v[a] = sign * s
                q.append(v)
        q.append(np.array([s, -s, s]))
    return np.array(q)


def planar_cloud(P=900):
    x = np.random.default_rng(9).uniform(-1, 1, (P, 3))
    x[:, 2] = 0.25
    return x


def salted_banana():
    """(cloud, the 12 outlier rows): the banana cloud with 12 rows moved 0.15–0.25 m off the bounding-box centre."""
    X = _fps.banana().copy()
    rng = np.random.default_rng(7)
    d = rng.standard_normal((12, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    radius = rng.uniform(0.15, 0.25, 12)
    rows = 1 + rng.choice(len(X) - 1, 12, replace=False)
    centre = 0.5 * (X.min(axis=0) + X.max(axis=0))
    X[rows] = centre + radius[:, None] * d
    return X, np.sort(rows)


def shared_cases():
    """name → dict(X, K, Q (None: the cloud itself), max_d2): what the host build and both device paths are checked on."""
    cases = {}
    for P in (1, 2, 63, 64, 65, 1025):
        for K in (1, 30, 64):
            cases[f"P{P}_K{K}"] = dict(X=_fps.normal_cloud(P), K=K)
    cases["banana_f64"] = dict(X=_fps.banana(), K=30)
    cases["banana_f32"] = dict(X=_fps.banana().astype(np.float32), K=30)
    cases["lattice"] = dict(X=_fps.lattice(35, 35, 33), K=30, Q=lattice_queries())
    cases["duplicates"] = dict(X=_fps.duplicates(), K=5)
    cases["salted"] = dict(X=_fps.salted_cloud(), K=30)
    cases["all_nonfinite"] = dict(X=_fps.all_nonfinite(), K=3)
    cases["outside"] = dict(X=_fps.normal_cloud(500, seed=5), K=30, Q=outside_queries())
    cases["two_clusters"] = dict(X=two_clusters(), K=30)
    cases["max_d2"] = dict(X=_fps.normal_cloud(300, seed=8), K=30, max_d2=0.05)
    cases["max_d2_zero"] = dict(X=np.concatenate([_fps.duplicates(), _fps.normal_cloud(40, seed=4)]), K=4, max_d2=0.0)
    for c in cases.values():
        c.setdefault("Q", None)
        c.setdefault("max_d2", INF)
    return cases


_REFERENCE = {}


def reference(name):
    """numpy_knn of a shared case, computed once."""
    if name not in _REFERENCE:
        c = shared_cases()[name]
        _REFERENCE[name] = numpy_knn(c["X"], c["K"], c["Q"], c["max_d2"])
    return _REFERENCE[name]
