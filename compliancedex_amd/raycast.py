"""Ray casting on triangle meshes and the depth camera in front of ``GPIS.fit_pointcloud``, on MI355X.

The reference makes its partial clouds outside the optimiser (get_observable_pcd.py: a PyBullet depth camera, open3d's
``create_from_depth_image``, a flip, a z mask, the inverse extrinsic, ``farthest_point_down_sample``) and filters
completed points with open3d's ``RaycastingScene.cast_rays`` (concatenate_pcd.py:41-49).  Here both are cdx_ray.hip on
the device that holds the mesh: ``cast_rays`` / ``occluded`` are cdx_ray_cast, ``render_depth`` is cdx_depth_render,
``depth_to_pointcloud`` is cdx_depth_count / cdx_depth_place, and ``observable_pointcloud`` chains them with cdx_fps.
The rule they compute is stated in csrc/cdx_ray.h.

Parity with open3d, Embree and PyBullet is unpinned (none of them is a dependency): the ray–triangle test here is the
float64 Möller–Trumbore test with a relative determinant threshold, ``t_min ≤ t ≤ t_max`` inclusive; the unprojection
follows open3d's published ``create_from_depth_image`` (float32 z, float64 x and y, row-major pixel order).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from .pointcloud import farthest_point_down_sample
from .torchsdf import PreparedMesh

REF_DEPTH_TRUNC = 9.9  # get_observable_pcd.py:35


def _require_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what} must be a CUDA (ROCm) tensor: compliancedex_amd has no CPU path")


def _mesh_args(mesh, mode):
    """(mesh pointer, ray-record pointer, faces, mode) of a cast.  ``auto``: the walk for a prepared mesh without
    NaN-capable faces, the scan otherwise."""
    if mode not in N.RAY_MODES:
        raise ValueError(f"mode must be one of {sorted(N.RAY_MODES)}, got {mode!r}")
    if isinstance(mesh, PreparedMesh):
        if mode == "auto":
            mode = "walk" if mesh.kind == N.SDF_MESH_CULLED else "scan"
        if mode == "walk":
            return N.ptr(mesh.buf), N.ptr(mesh.ray_records()), mesh.faces, N.RAY_MODES["walk"]
        return None, None, mesh.faces, N.RAY_MODES["scan"]
    _require_cuda(mesh, "mesh")
    if mesh.dtype != torch.float32 or mesh.dim() != 3 or mesh.shape[1:] != (3, 3) or mesh.shape[0] == 0:
        raise ValueError("mesh must be a PreparedMesh or a non-empty float32 [F, 3, 3] tensor")
    if mode == "walk":
        raise ValueError("mode 'walk' needs a PreparedMesh")
    return None, None, mesh.detach().contiguous(), N.RAY_MODES["scan"]


def cast_rays(mesh, origins, directions, tmin=0.0, tmax=math.inf, mode="auto", want_uv=False):
    """First hit of the rays ``origins + t·directions`` ([R, 3] each, on the device; float32 rays are widened) on
    ``mesh`` (a PreparedMesh or a float32 [F, 3, 3] tensor): ``(t [R] float64, face [R] int32)`` and with ``want_uv``
    the hit's barycentric ``uv [R, 2]``.  ``directions`` are not normalised: t is in units of their length.  A miss —
    also a ray with a non-finite component or a zero direction — gives t = +inf, face = −1, uv = 0.  Hits have
    ``tmin ≤ t ≤ tmax``; the smallest t wins, equal t goes to the smallest face index.  ``mode``: "scan" (every face),
    "walk" (the prepared mesh's hierarchy) or "auto" (the walk for a PreparedMesh without NaN-capable faces); all give
    the same bits.  No host synchronisation."""
    mp, rp, faces, m = _mesh_args(mesh, mode)
    _require_cuda(origins, "origins")
    _require_cuda(directions, "directions")
    if origins.dim() != 2 or origins.shape[1] != 3 or origins.shape != directions.shape:
        raise ValueError(f"origins and directions must both be [R, 3], got {tuple(origins.shape)} and "
                         f"{tuple(directions.shape)}")
    for x in (origins, directions):
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"rays must be float32 or float64, got {x.dtype}")
    dev = faces.device
    o = origins.detach().to(torch.float64).contiguous()
    d = directions.detach().to(torch.float64).contiguous()
    R = o.shape[0]
    t = torch.empty(R, dtype=torch.float64, device=dev)
    face = torch.empty(R, dtype=torch.int32, device=dev)
    uv = torch.empty(R, 2, dtype=torch.float64, device=dev) if want_uv else None
    if R:
        N.check(N.load().cdx_ray_cast(mp, rp, N.ptr(faces), faces.shape[0], N.ptr(o), N.ptr(d), R, float(tmin),
                                      float(tmax), m, N.ptr(t), N.ptr(face), N.ptr(uv), N.stream_ptr(dev)),
                "cdx_ray_cast")
    return (t, face, uv) if want_uv else (t, face)


def _as_f64(x, shape, what):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    a = np.array(x, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{what} must have shape {shape}, got {a.shape}")
    return a


class Camera:
    """A pinhole camera: ``width`` × ``height`` pixels, intrinsics ``fx, fy, cx, cy`` and the float64 4×4
    ``world_to_camera`` extrinsic.  Convention (open3d's, and what ``create_from_depth_image`` unprojects into): in
    the camera frame x points right, y DOWN and z FORWARD; pixel (i, j) — row i, column j — looks along
    ((j − cx)/fx, (i − cy)/fy, 1), so a depth image holds z, not the distance along the ray."""

    def __init__(self, width, height, fx, fy, cx, cy, world_to_camera):
        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1:
            raise ValueError("camera needs at least one pixel")
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.world_to_camera = _as_f64(world_to_camera, (4, 4), "world_to_camera")
        self.camera_to_world = np.linalg.inv(self.world_to_camera)

    @classmethod
    def look_at(cls, eye, target, up, fov_deg, width, height, aspect=1.0):
        """The reference's camera (get_observable_pcd.py:50-55): PyBullet's ``computeViewMatrix(eye, target, up)``
        and ``computeProjectionMatrixFOV(fov_deg, aspect, near, far)`` — ``fov_deg`` is the VERTICAL field of view,
        ``aspect`` is 1 as in the reference, whatever the image's shape (pass width/height for square pixels) — turned
        into intrinsics as its ``getIntrinsicParams`` does: fx = (1/tan(fov/2)/aspect)·width/2,
        fy = (1/tan(fov/2))·height/2, cx = width/2, cy = height/2.  The view matrix is OpenGL's (x right, y up,
        z backward); the reference flips its unprojected points by [1, −1, −1] before applying the inverse view matrix, which is the same as unprojecting into this
        class's frame (x right, y down, z forward) with world_to_camera = diag(1, −1, −1, 1)·view: the world points
        are the same.  Near and far planes do not enter (the depth here is metric, not a z-buffer)."""
        eye, target, up = (_as_f64(v, (3,), n) for v, n in ((eye, "eye"), (target, "target"), (up, "up")))
        f = target - eye
        f = f / np.linalg.norm(f)
        s = np.cross(f, up)
        s = s / np.linalg.norm(s)
        u = np.cross(s, f)
        w2c = np.eye(4)
        w2c[0, :3], w2c[1, :3], w2c[2, :3] = s, -u, f
        w2c[:3, 3] = -(w2c[:3, :3] @ eye)
        yscale = 1.0 / math.tan(math.radians(float(fov_deg)) / 2.0)
        aspect = float(aspect)
        return cls(width, height, yscale / aspect * width / 2.0, yscale * height / 2.0, width / 2.0, height / 2.0, w2c)

    @property
    def eye(self):
        """The camera centre in the world."""
        return self.camera_to_world[:3, 3].copy()

    def _intr(self):
        return (C.c_double * 4)(self.fx, self.fy, self.cx, self.cy)

    def rays(self, device=None):
        """(origins, directions) [H·W, 3] float64 of the pixels in row-major order, as ``render_depth`` casts them
        (csrc/cdx_ray.h, pixel rays) — computed on the host."""
        M = self.camera_to_world
        i, j = np.meshgrid(np.arange(self.height, dtype=np.float64), np.arange(self.width, dtype=np.float64),
                           indexing="ij")
        dx, dy = ((j - self.cx) / self.fx).reshape(-1), ((i - self.cy) / self.fy).reshape(-1)
        d = np.stack([(M[k, 0] * dx + M[k, 1] * dy) + M[k, 2] for k in range(3)], axis=1)
        o = np.broadcast_to(M[:3, 3], d.shape).copy()
        o, d = torch.from_numpy(o), torch.from_numpy(d)
        return (o.to(device), d.to(device)) if device is not None else (o, d)


def _mat16(M):
    return (C.c_double * 16)(*np.ascontiguousarray(M, dtype=np.float64).reshape(-1))


def render_depth(mesh, camera, want_face=False, mode="auto", tmin=0.0, tmax=math.inf):
    """Depth image of ``mesh`` from ``camera``: float64 [H, W] z-depth on the mesh's device, 0 where the pixel's ray
    hits nothing; with ``want_face`` also the int32 [H, W] image of hit faces (−1: none).  The rays are generated in
    the kernel (``Camera.rays`` states them); each is cast as ``cast_rays`` does.  No host synchronisation."""
    mp, rp, faces, m = _mesh_args(mesh, mode)
    dev = faces.device
    H, W = camera.height, camera.width
    depth = torch.empty(H, W, dtype=torch.float64, device=dev)
    face = torch.empty(H, W, dtype=torch.int32, device=dev) if want_face else None
    N.check(N.load().cdx_depth_render(mp, rp, N.ptr(faces), faces.shape[0], W, H, camera._intr(),
                                      _mat16(camera.camera_to_world), float(tmin), float(tmax), m, N.ptr(depth),
                                      N.ptr(face), N.stream_ptr(dev)), "cdx_depth_render")
    return (depth, face) if want_face else depth


_DEPTH_DTYPES = {torch.float32: N.DTYPE_F32, torch.float64: N.DTYPE_F64, torch.uint16: N.DEPTH_U16}


def depth_to_pointcloud(depth, camera, depth_scale=1000.0, depth_trunc=1000.0, z_max=None, world=True, stride=1):
    """open3d's ``PointCloud.create_from_depth_image`` on a device depth image [H, W] (uint16, float32 or float64):
    float64 [n, 3] points in row-major pixel order.  z = depth/depth_scale in the image's precision (float32 for
    uint16); a pixel is dropped where depth == 0 or z ≥ depth_trunc, and — with ``z_max`` — unless z < z_max (the
    reference's mask, get_observable_pcd.py:37); x = (j − cx)·z/fx, y = (i − cy)·z/fy in float64; ``world``: the
    points go through ``camera.camera_to_world`` (else they stay in the camera frame: x right, y down, z forward);
    ``stride``: every stride-th row and column.  One host read (the count).  Parity with open3d is unpinned."""
    _require_cuda(depth, "depth")
    if depth.dim() != 2 or tuple(depth.shape) != (camera.height, camera.width):
        raise ValueError(f"depth must be [{camera.height}, {camera.width}], got {tuple(depth.shape)}")
    if depth.dtype not in _DEPTH_DTYPES:
        raise TypeError(f"depth must be uint16, float32 or float64, got {depth.dtype}")
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be at least 1")
    lib = N.load()
    dev = depth.device
    img = depth.detach().contiguous()
    H, W = camera.height, camera.width
    dt = _DEPTH_DTYPES[img.dtype]
    zm = float("nan") if z_max is None else float(z_max)
    ws = torch.empty(lib.cdx_depth_workspace(W, H, stride), dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    stream = N.stream_ptr(dev)
    N.check(lib.cdx_depth_count(N.ptr(img), dt, W, H, stride, float(depth_scale), float(depth_trunc), zm, N.ptr(ws),
                                N.ptr(total), stream), "cdx_depth_count")
    n = int(total.item())
    points = torch.empty(n, 3, dtype=torch.float64, device=dev)
    if n:
        N.check(lib.cdx_depth_place(N.ptr(img), dt, W, H, stride, camera._intr(), float(depth_scale),
                                    float(depth_trunc), zm, _mat16(camera.camera_to_world) if world else None,
                                    N.ptr(ws), n, N.ptr(points), stream), "cdx_depth_place")
    return points


def observable_pointcloud(mesh, camera, num_points=2048, depth_scale=1000.0, z_max=0.9, noise=0.0, generator=None,
                          shuffle=False):
    """The reference's partial cloud of ``mesh`` seen from ``camera`` (get_observable_pcd.py:26-46), on the device:
    render the depth; quantise it to uint16 units of 1/depth_scale (millimetres) by truncation, as
    ``(depth·1000).astype(np.uint16)`` does; unproject (``depth_to_pointcloud``, depth_trunc 9.9); add Gaussian
    ``noise`` (standard deviation, metres) when asked; keep z < ``z_max`` in the camera frame (the reference's
    ``points[:, 2] > −0.9`` after its flip); go to the world; ``farthest_point_down_sample(num_points)``; ``shuffle``
    the rows like the reference.  float64 [num_points, 3], the input ``GPIS.fit_pointcloud`` takes.  ``generator``
    drives the noise and the shuffle.  Fewer visible points than ``num_points`` is an error."""
    depth = render_depth(mesh, camera)
    q = torch.clamp(depth * float(depth_scale), max=65535.0).to(torch.int32).to(torch.uint16)
    if noise:
        pts = depth_to_pointcloud(q, camera, depth_scale, REF_DEPTH_TRUNC, None, world=False)
        gdev = generator.device if generator is not None else pts.device
        pts = pts + (float(noise) * torch.randn(pts.shape, dtype=torch.float64, generator=generator, device=gdev)).to(
            pts.device)
        if z_max is not None:
            pts = pts[pts[:, 2] < float(z_max)]
        M = torch.from_numpy(camera.camera_to_world).to(pts.device)
        pts = pts @ M[:3, :3].T + M[:3, 3]
    else:
        pts = depth_to_pointcloud(q, camera, depth_scale, REF_DEPTH_TRUNC, z_max, world=True)
    num_points = int(num_points)
    if pts.shape[0] < num_points:
        raise ValueError(f"only {pts.shape[0]} points are visible, {num_points} asked for")
    cloud = farthest_point_down_sample(pts, num_points)
    if shuffle:
        gdev = generator.device if generator is not None else cloud.device
        cloud = cloud[torch.randperm(num_points, generator=generator, device=gdev).to(cloud.device)]
    return cloud


def occluded(mesh, eye, points):
    """bool [P]: whether ``mesh`` hides each of ``points`` [P, 3] from ``eye`` (concatenate_pcd.py:43-48: a ray from
    the eye with direction point − eye, occluded iff it hits at t < 1)."""
    _require_cuda(points, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [P, 3], got {tuple(points.shape)}")
    p = points.detach().to(torch.float64)
    e = torch.as_tensor(_as_f64(eye, (3,), "eye"), device=p.device)
    t, _ = cast_rays(mesh, e.expand_as(p).contiguous(), p - e)
    return t < 1.0
