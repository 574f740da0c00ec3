"""From a sensed point cloud to the arrays GPIS.fit takes, on MI355X.

The reference down-samples its clouds with open3d's ``farthest_point_down_sample`` (optimize_pregrasp.py:904,
get_observable_pcd.py:40) and then adds exterior and interior points (optimize_pregrasp.py:905-922,
train_gpis_completion.py:25-58).  Here the sampling is cdx_fps (csrc/cdx_fps.hip, the rule in csrc/cdx_fps.h) and
the recipe is a handful of tensor operators on the same device; nothing synchronises with the host.

Parity with open3d's implementation is unpinned (open3d is not a dependency): its published loop also starts at
index 0, keeps float64 squared distances with a running minimum and takes the first maximum, and returns the chosen
rows in ascending index order, which is what ``farthest_point_down_sample`` returns.
"""
from __future__ import annotations

import torch

from . import _native as N


def _require_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what} must be a CUDA (ROCm) tensor: compliancedex_amd has no CPU path")


def capacity():
    """Largest cloud the one-workgroup path of cdx_fps takes."""
    return int(N.load().cdx_fps_capacity())


def fps(points, k, start=0, mode="auto", radius=False, gather=False, workspace=None):
    """cdx_fps on a [P, 3] or [B, P, 3] device tensor: (sel int64, radius f64 or None, points[sel] f64 or None), with
    the batch dimension of the input.  ``workspace`` (uint8, at least cdx_fps_workspace bytes) is reused when given."""
    _require_cuda(points, "point cloud")
    if points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise ValueError(f"point cloud must be [P, 3] or [B, P, 3], got {tuple(points.shape)}")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"point cloud must be float32 or float64, got {points.dtype}")
    if mode not in N.FPS_MODES:
        raise ValueError(f"mode must be one of {sorted(N.FPS_MODES)}, got {mode!r}")
    batched = points.dim() == 3
    X = points.detach().contiguous()
    B, P = (X.shape[0], X.shape[1]) if batched else (1, X.shape[0])
    k, start = int(k), int(start)
    if not 1 <= k <= P:
        raise ValueError(f"k must be in 1..{P}, got {k}")
    if not 0 <= start < P:
        raise ValueError(f"start must be in 0..{P - 1}, got {start}")
    if B < 1:
        raise ValueError("empty batch")
    lib = N.load()
    m = N.FPS_MODES[mode]
    need = lib.cdx_fps_workspace(P, B, m)
    if need == 0:
        raise ValueError(f"cdx_fps takes no cloud of {P} rows in mode {mode!r} (one workgroup: up to {capacity()})")
    dev = X.device
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"workspace of {workspace.numel() * workspace.element_size()} bytes, {need} needed")
    shape = (B, k) if batched else (k,)
    sel = torch.empty(shape, dtype=torch.int64, device=dev)
    rad = torch.empty(shape, dtype=torch.float64, device=dev) if radius else None
    pts = torch.empty(shape + (3,), dtype=torch.float64, device=dev) if gather else None
    dtype = N.DTYPE_F32 if X.dtype == torch.float32 else N.DTYPE_F64
    N.check(lib.cdx_fps(N.ptr(X), dtype, P, B, k, start, m, N.ptr(workspace), N.ptr(sel), N.ptr(rad), N.ptr(pts),
                        N.stream_ptr(dev)), "cdx_fps")
    return sel, rad, pts


def farthest_point_sample(points, k, start=0, return_radius=False, mode="auto"):
    """Indices of a farthest-point sample of ``points`` ([P, 3] or [B, P, 3], float32 or float64, on the device):
    int64 [k] or [B, k] in selection order, beginning with ``start``; with ``return_radius`` also the float64 squared
    distance of each chosen row to the rows chosen before it (+inf for the first).  Distances are float64, ties go to
    the smallest index, rows with a non-finite coordinate are never chosen (except as ``start``); the first j entries
    of a k-sample are the j-sample.  ``mode``: "block" (one workgroup per cloud, up to ``capacity()`` rows), "rounds"
    (one launch per round) or "auto"; all give the same indices.  No host synchronisation."""
    sel, rad, _ = fps(points, k, start, mode, radius=return_radius)
    return (sel, rad) if return_radius else sel


def farthest_point_down_sample(points, k):
    """open3d's ``PointCloud.farthest_point_down_sample(k)`` on a [P, 3] device tensor: the k chosen rows of
    ``points`` in ascending index order, in the input's dtype."""
    if torch.is_tensor(points) and points.dim() != 2:
        raise ValueError(f"point cloud must be [P, 3], got {tuple(points.shape)}")
    sel = farthest_point_sample(points, k)
    return points[torch.sort(sel).values]


def exterior_points(bound, device):
    """The 14 exterior points of the reference's recipe (train_gpis_completion.py:25-38): the 8 corners and the 6
    face centres of the cube of half-width ``bound``, built in float32 and widened as the reference does."""
    b = float(bound)
    ext = torch.tensor([[-b, -b, -b], [b, -b, -b], [-b, b, -b], [b, b, -b], [-b, -b, b], [b, -b, b], [-b, b, b],
                        [b, b, b], [-b, 0., 0.], [0., -b, 0.], [b, 0., 0.], [0., b, 0], [0., 0., b], [0., 0., -b]],
                       dtype=torch.float32)
    return ext.double().to(device)


def completion_arrays(surface, bound, n_internal, sharpness, noise, center=None, weights=None, generator=None):
    """(X1 [14 + n + n_internal, 3], y [., 1], noise [.]) float64 on the device of ``surface`` [n, 3]: the reference's
    fit recipe (optimize_pregrasp.py:905-922, train_gpis_completion.py:25-58).

      exterior  14 points at ±``bound`` (``exterior_points``), shifted by ``center`` in float64;  y = +bound
      surface   the given points;                                                                   y = 0
      interior  softmax(weights · sharpness, dim=1) @ surface, weights [n_internal, n];            y = −bound

    ``weights`` not given: ``torch.rand`` in float32 from ``generator`` (on the generator's device), widened.
    ``noise`` = (exterior, surface, interior) levels, each repeated over its group; like the reference's
    ``torch.tensor([...]).double()`` they are float32 values widened."""
    _require_cuda(surface, "surface points")
    if surface.dim() != 2 or surface.shape[1] != 3:
        raise ValueError(f"surface points must be [n, 3], got {tuple(surface.shape)}")
    dev = surface.device
    surf = surface.detach().double()
    n, n_internal = surf.shape[0], int(n_internal)
    ext = exterior_points(bound, dev)
    if center is not None:
        ext = ext + torch.as_tensor(center, dtype=torch.float64, device=dev)
    if weights is None:
        gdev = generator.device if generator is not None else dev
        weights = torch.rand(n_internal, n, generator=generator, device=gdev)
    weights = weights.to(dev).double()
    if tuple(weights.shape) != (n_internal, n):
        raise ValueError(f"weights must be [{n_internal}, {n}], got {tuple(weights.shape)}")
    interior = torch.softmax(weights * sharpness, dim=1) @ surf
    X1 = torch.vstack([ext, surf, interior])
    b = float(bound)
    y = torch.cat([torch.full((len(ext),), b, dtype=torch.float64), torch.zeros(n, dtype=torch.float64),
                   torch.full((n_internal,), -b, dtype=torch.float64)]).view(-1, 1).to(dev)
    lv = [float(v) for v in noise]
    if len(lv) != 3:
        raise ValueError("noise must be (exterior, surface, interior)")
    nz = torch.tensor([lv[0]] * len(ext) + [lv[1]] * n + [lv[2]] * n_internal, dtype=torch.float32).double().to(dev)
    return X1, y, nz


def bbox_center(points):
    """Centre of the axis-aligned bounding box of the finite rows of ``points`` [P, 3] (open3d's
    ``get_axis_aligned_bounding_box().get_center()``), float64 [3] on the device."""
    p = points.detach().double()
    ok = torch.isfinite(p).all(dim=1, keepdim=True)
    lo = torch.where(ok, p, torch.full_like(p, float("inf"))).min(dim=0).values
    hi = torch.where(ok, p, torch.full_like(p, float("-inf"))).max(dim=0).values
    return 0.5 * (lo + hi)


# ---------------------------------------------------------------- neighbours, normals, outliers (csrc/cdx_knn.h)
#
# open3d's KDTreeFlann searches, estimate_normals / orient_normals_towards_camera_location (concatenate_pcd.py:35-36),
# remove_statistical_outlier and compute_point_cloud_distance, all on cdx_knn (csrc/cdx_knn.hip).  Parity with open3d's
# own covariance (raw moments) and closed-form eigen-solver is unpinned and not attempted.

def _cloud(points, what):
    _require_cuda(points, what)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what} must be [P, 3], got {tuple(points.shape)}")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what} must be float32 or float64, got {points.dtype}")
    return points.detach().contiguous()


def _dtype(t):
    return N.DTYPE_F32 if t.dtype == torch.float32 else N.DTYPE_F64


def auto_grid_rows():
    """Cloud rows above which the automatic mode of cdx_knn walks a grid it is given instead of scanning."""
    return int(N.load().cdx_knn_auto_rows())


# ``knn(mode="auto")`` without a grid prepares one above this many rows: measured with every row a query,
# prepare + walk is level with the scan at 10⁴ rows (0.22 against 0.25 ms at K = 30, 0.17 against 0.13 ms at K = 1) and
# 1.6–1.8× faster at 2·10⁴.
AUTO_PREPARE_ROWS = 10000


class KnnGrid:
    """The uniform grid of a cloud [P, 3] for ``knn(..., grid=...)``: prepared once on the device (cdx_knn_prepare, no
    host synchronisation) and reusable for any number of queries.  ``prepare(points)`` rebuilds it in the same bytes
    for another cloud when they suffice.  The grid holds a copy of the rows in cell order, so it serves the tensor it
    was prepared from only as long as that tensor is not written to: ``knn`` compares the tensor's version counter
    and raises on a cloud changed in place since ``prepare`` (writes through raw pointers escape the counter)."""

    def __init__(self, points):
        self.buffer = None
        self.prepare(points)

    def prepare(self, points):
        X = _cloud(points, "point cloud")
        P = X.shape[0]
        lib = N.load()
        need = lib.cdx_knn_grid_bytes(P)
        if need == 0:
            raise ValueError(f"cdx_knn takes no cloud of {P} rows")
        if self.buffer is None or self.buffer.numel() < need or self.buffer.device != X.device:
            self.buffer = torch.empty(need, dtype=torch.uint8, device=X.device)
        N.check(lib.cdx_knn_prepare(N.ptr(X), _dtype(X), P, N.ptr(self.buffer), N.stream_ptr(X.device)),
                "cdx_knn_prepare")
        self.points = X  # the contiguous rows the grid indexes: the tensor itself, or its copy if it was strided
        self.source = (points.data_ptr(), tuple(points.shape), tuple(points.stride()), points.dtype)
        self.version = points._version
        return self

    def check(self, points):
        """Raises unless ``points`` is the tensor (or a view of the same memory and layout) this grid was prepared
        from, unchanged since."""
        if not torch.is_tensor(points) or \
                (points.data_ptr(), tuple(points.shape), tuple(points.stride()), points.dtype) != self.source:
            raise ValueError("grid was prepared for another cloud")
        if points._version != self.version:
            raise ValueError("the cloud was written to after its grid was prepared: call grid.prepare(points) again")


def knn(points, k, queries=None, max_distance=None, mode="auto", grid=None):
    """The ``k`` nearest rows of ``points`` [P, 3] to every row of ``queries`` [M, 3] (default: the points themselves,
    each then its own first neighbour), both float32 or float64 on the device: (idx int64 [M, k], d2 float64 [M, k],
    count int32 [M]).  Rows are ascending in (d2, index); d2 is the float64 squared distance, ties go to the smaller
    index.  With ``max_distance`` pairs farther than that are left out (open3d's hybrid search; compared as
    d2 > max_distance²).  Slots past ``count`` hold −1 and +inf.  Rows of ``points`` with a non-finite coordinate are
    never neighbours; such a query finds nothing.  1 ≤ k ≤ 64; k may exceed P.  ``mode``: "scan" (every row against
    every query), "grid" (a uniform grid, ``grid`` = a ``KnnGrid`` of these points or built here) or "auto" (a given grid
    above ``auto_grid_rows()`` rows, one built here above ``AUTO_PREPARE_ROWS``, else the scan); all give the same bits.
    No host synchronisation."""
    X = _cloud(points, "point cloud")
    if mode not in N.KNN_MODES:
        raise ValueError(f"mode must be one of {sorted(N.KNN_MODES)}, got {mode!r}")
    k = int(k)
    if not 1 <= k <= N.KNN_MAX_K:
        raise ValueError(f"k must be in 1..{N.KNN_MAX_K}, got {k}")
    P = X.shape[0]
    if P < 1:
        raise ValueError("empty point cloud")
    Q = None
    if queries is not None:
        Q = _cloud(queries, "queries")
        if Q.device != X.device:
            raise ValueError("queries and points must be on one device")
        if Q.dtype != X.dtype:  # widening is exact
            X, Q = X.double(), Q.double()
            if grid is not None:
                raise TypeError("a grid serves queries of its cloud's dtype only")
    max_d2 = float("inf")
    if max_distance is not None:
        r = float(max_distance)
        if not r >= 0.0:
            raise ValueError(f"max_distance must be ≥ 0, got {max_distance}")
        max_d2 = r * r
    if grid is not None:
        if not isinstance(grid, KnnGrid):
            raise TypeError("grid must be a KnnGrid")
        grid.check(points)
        X = grid.points
    elif mode == "grid" or (mode == "auto" and P > AUTO_PREPARE_ROWS):
        grid = KnnGrid(X)
    lib = N.load()
    M = P if Q is None else Q.shape[0]
    dev = X.device
    idx = torch.empty((M, k), dtype=torch.int64, device=dev)
    d2 = torch.empty((M, k), dtype=torch.float64, device=dev)
    count = torch.empty((M,), dtype=torch.int32, device=dev)
    N.check(lib.cdx_knn(N.ptr(X), _dtype(X), P, N.ptr(grid.buffer) if grid is not None else None, N.ptr(Q), M, k,
                        max_d2, N.KNN_MODES[mode], None, N.ptr(idx), N.ptr(d2), N.ptr(count), N.stream_ptr(dev)),
            "cdx_knn")
    return idx, d2, count


_knn_search = knn


def _eye(camera_location):
    import ctypes
    e = torch.as_tensor(camera_location, dtype=torch.float64).reshape(-1).tolist()
    if len(e) != 3:
        raise ValueError("camera_location must be a point")
    return (ctypes.c_double * 3)(*e)


def normals_from_neighbours(points, idx, count, camera_location=None, return_eigenvalues=False):
    """cdx_cloud_normals: the normals [P, 3] float64 of ``points`` from their neighbour lists (``knn``'s idx and
    count), and with ``return_eigenvalues`` the covariance's eigenvalues [P, 3] in ascending order."""
    X = _cloud(points, "point cloud")
    P = X.shape[0]
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != P or not 1 <= idx.shape[1] <= N.KNN_MAX_K:
        raise ValueError(f"idx must be int64 [{P}, 1..{N.KNN_MAX_K}]")
    if count.dtype != torch.int32 or tuple(count.shape) != (P,):
        raise ValueError(f"count must be int32 [{P}]")
    _require_cuda(idx, "idx")
    _require_cuda(count, "count")
    dev = X.device
    normals = torch.empty((P, 3), dtype=torch.float64, device=dev)
    eig = torch.empty((P, 3), dtype=torch.float64, device=dev) if return_eigenvalues else None
    eye = _eye(camera_location) if camera_location is not None else None
    N.check(N.load().cdx_cloud_normals(N.ptr(X), _dtype(X), P, N.ptr(idx.contiguous()), N.ptr(count.contiguous()),
                                       idx.shape[1], eye, N.ptr(normals), N.ptr(eig), N.stream_ptr(dev)),
            "cdx_cloud_normals")
    return (normals, eig) if return_eigenvalues else normals


def estimate_normals(points, knn=30, radius=None, camera_location=None, return_eigenvalues=False):
    """open3d's ``estimate_normals`` on a [P, 3] device tensor: float64 [P, 3], the eigenvector of the smallest
    eigenvalue of the covariance of each point's ``knn`` nearest neighbours (the point included; within ``radius``
    when given: open3d's hybrid search).  ``camera_location`` (a host point) orients them towards it as
    ``orient_normals_towards_camera_location`` does; without it the component of largest magnitude is positive.  Fewer
    than 3 neighbours give (0, 0, 1); a non-finite point gives NaN.  ``return_eigenvalues``: also [P, 3], ascending.
    The rule is csrc/cdx_knn.h; parity with open3d's covariance and eigen-solver is unpinned.  No host
    synchronisation."""
    idx, _, count = _knn_search(points, knn, max_distance=radius)
    return normals_from_neighbours(points, idx, count, camera_location, return_eigenvalues)


def orient_normals_towards_camera_location(points, normals, camera_location=(0.0, 0.0, 0.0)):
    """open3d's function of that name: ``normals`` [P, 3] flipped where n · (camera_location − p) < 0, in float64 with
    the dot product summed as (x + y) + z like the kernel."""
    _require_cuda(points, "point cloud")
    _require_cuda(normals, "normals")
    if tuple(points.shape) != tuple(normals.shape) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points and normals must both be [P, 3]")
    n = normals.detach().double()
    e = torch.as_tensor(camera_location, dtype=torch.float64).reshape(3).to(n.device) - points.detach().double()
    dot = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
    return torch.where((dot < 0).unsqueeze(1), -n, n)


def statistical_outlier_mask(points, nb_neighbors=20, std_ratio=2.0):
    """open3d's ``remove_statistical_outlier`` as a mask, bool [P], True = keep: per row the mean of sqrt(d2) over
    the ``nb_neighbors`` nearest neighbours found (the point itself included, as open3d averages); a row is kept when
    that mean is ≤ the cloud's mean + ``std_ratio`` × its standard deviation (n − 1 divisor), both over the rows that
    found a neighbour.  Non-finite rows are False.  No host synchronisation."""
    _, d2, count = _knn_search(points, nb_neighbors)
    k = d2.shape[1]
    slot = torch.arange(k, device=d2.device).unsqueeze(0) < count.unsqueeze(1)
    dist = torch.where(slot, torch.sqrt(d2), torch.zeros_like(d2))
    found = count > 0
    avg = dist.sum(dim=1) / count.clamp(min=1).double()
    n = found.sum().double()
    zero = torch.zeros_like(avg)
    mean = torch.where(found, avg, zero).sum() / n
    dev2 = torch.where(found, (avg - mean) ** 2, zero).sum()
    std = torch.sqrt(torch.where(n > 1, dev2 / (n - 1), torch.zeros_like(dev2)))
    return found & (avg <= mean + float(std_ratio) * std)


def remove_statistical_outlier(points, nb_neighbors=20, std_ratio=2.0):
    """open3d's contract: (the kept rows of ``points`` in their order, their int64 indices).  Synchronises once, since
    the result's shape depends on the data."""
    keep = statistical_outlier_mask(points, nb_neighbors, std_ratio)
    index = torch.nonzero(keep).reshape(-1)
    return points[index], index


def point_cloud_distance(source, target):
    """open3d's ``compute_point_cloud_distance``: float64 [S], the distance of every row of ``source`` [S, 3] to the
    nearest row of ``target`` [T, 3]; +inf where the target has no finite row (NaN-free: a non-finite source row gives
    +inf too).  No host synchronisation."""
    _, d2, _ = _knn_search(target, 1, queries=source)
    return torch.sqrt(d2[:, 0])
