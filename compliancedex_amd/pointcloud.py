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
