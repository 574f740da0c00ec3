"""Helpers shared by test_ray_cpu.py and test_gpu_ray.py: the ray casting and depth unprojection rules of csrc/cdx_ray.h
stated in numpy, the host build (cdxh_ray_cast, cdxh_pixel_rays, cdxh_depth_unproject, cdxh_ray_ball_miss) and the
meshes and rays both files cast."""
import os

import numpy as np

from tests._host import host, p

F32, F64, U16 = 0, 1, 2  # CDX_DTYPE_F32, CDX_DTYPE_F64, CDX_DEPTH_U16
TAU2 = 2.0 ** -40        # cdx::RAY_DET_TAU2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the rule in numpy

def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def numpy_cast(faces, origins, dirs, tmin=0.0, tmax=np.inf):
    """(t f64 [R], face i32 [R], uv f64 [R, 2]) of the rule, vectorised over the faces of one ray at a time, in the
    header's order of operations."""
    f = np.asarray(faces, np.float32).astype(np.float64)
    v0 = f[:, 0]
    e1, e2 = f[:, 1] - v0, f[:, 2] - v0
    n12 = _dot(e1, e1) * _dot(e2, e2)
    R = len(origins)
    t_out = np.full(R, np.inf)
    f_out = np.full(R, -1, np.int32)
    uv = np.zeros((R, 2))
    with np.errstate(all="ignore"):
        for r in range(R):
            o, d = np.asarray(origins[r], np.float64), np.asarray(dirs[r], np.float64)
            if not (np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any()):
                continue
            db = np.broadcast_to(d, e2.shape)
            pv = _cross(db, e2)
            det = _dot(e1, pv)
            lim = (n12 * _dot(d, d)) * TAU2
            ok = np.isfinite(det) & (det * det > lim)
            T = o - v0
            u = _dot(T, pv) / det
            q = _cross(T, e1)
            v = _dot(db, q) / det
            t = _dot(e2, q) / det
            hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tmin) & (t <= tmax)
            if hit.any():
                tm = t[hit].min()
                k = int(np.flatnonzero(hit & (t == tm))[0])
                t_out[r], f_out[r], uv[r] = t[k], k, (u[k], v[k])
    return t_out, f_out, uv


def numpy_hits(faces, o, d, tmin=0.0, tmax=np.inf):
    """Indices of every face the rule accepts for one ray, and their t."""
    f = np.asarray(faces, np.float32).astype(np.float64)
    out = []
    for k in range(len(f)):
        t, fi, _ = numpy_cast(f[k:k + 1].astype(np.float32), [o], [d], tmin, tmax)
        if fi[0] == 0:
            out.append((k, t[0]))
    return out


def numpy_pixel_rays(W, H, intr, M):
    fx, fy, cx, cy = intr
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx, dy = ((j - cx) / fx).reshape(-1), ((i - cy) / fy).reshape(-1)
    d = np.stack([(M[k, 0] * dx + M[k, 1] * dy) + M[k, 2] for k in range(3)], axis=1)
    return np.broadcast_to(M[:3, 3], d.shape).copy(), d


def numpy_unproject(depth, intr, scale, trunc, z_max=None, M=None, stride=1):
    """The unprojection rule, vectorised: float64 [n, 3] in row-major order of the visited pixels."""
    fx, fy, cx, cy = intr
    Z = np.float64 if depth.dtype == np.float64 else np.float32
    H, W = depth.shape
    ii, jj = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    raw = depth[ii, jj].astype(Z)
    with np.errstate(all="ignore"):
        z = raw / Z(scale)
        keep = ~((raw == 0) | (z >= Z(trunc)))
        zz = z.astype(np.float64)
        if z_max is not None:
            keep &= zz < z_max
        x = ((jj.astype(np.float64) - cx) * zz) / fx
        y = ((ii.astype(np.float64) - cy) * zz) / fy
        if M is not None:
            pts = np.stack([((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * zz) + M[k, 3] for k in range(3)], axis=-1)
        else:
            pts = np.stack([x, y, zz], axis=-1)
    return pts[keep]


# ---- the host build

def host_cast(faces, origins, dirs, tmin=0.0, tmax=np.inf):
    lib = host()
    faces = np.ascontiguousarray(faces, np.float32)
    o, d = np.ascontiguousarray(origins, np.float64), np.ascontiguousarray(dirs, np.float64)
    R = len(o)
    t, face, uv = np.full(R, -7.0), np.full(R, -7, np.int32), np.full((R, 2), -7.0)
    rc = lib.cdxh_ray_cast(p(faces), len(faces), p(o), p(d), R, tmin, tmax, p(t), p(face), p(uv))
    assert rc == 0, rc
    return t, face, uv


def host_pixel_rays(W, H, intr, M):
    lib = host()
    intr, M = np.ascontiguousarray(intr, np.float64), np.ascontiguousarray(M, np.float64)
    o, d = np.zeros((H * W, 3)), np.zeros((H * W, 3))
    assert lib.cdxh_pixel_rays(W, H, p(intr), p(M), p(o), p(d)) == 0
    return o, d


def host_unproject(depth, intr, scale, trunc, z_max=None, M=None, stride=1):
    lib = host()
    depth = np.ascontiguousarray(depth)
    dt = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.uint16): U16}[depth.dtype]
    H, W = depth.shape
    intr = np.ascontiguousarray(intr, np.float64)
    Mp = None if M is None else p(np.ascontiguousarray(M, np.float64))
    zm = np.nan if z_max is None else z_max
    cap = H * W
    pts = np.full((cap, 3), -7.0)
    n = lib.cdxh_depth_unproject(p(depth), dt, W, H, stride, p(intr), scale, trunc, zm, Mp, cap, p(pts))
    assert n >= 0, n
    return pts[:n].copy()


def host_ball_miss(origins, dirs, s0, s1, balls):
    lib = host()
    o, d = np.ascontiguousarray(origins, np.float64), np.ascontiguousarray(dirs, np.float64)
    s0, s1 = np.ascontiguousarray(s0, np.float64), np.ascontiguousarray(s1, np.float64)
    balls = np.ascontiguousarray(balls, np.float32)
    n = len(o)
    miss, dom = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.cdxh_ray_ball_miss(p(o), p(d), p(s0), p(s1), p(balls), n, p(miss), p(dom))
    return miss.astype(bool), dom.astype(bool)


# ---- meshes

def grid_plane(n=4):
    """The square [0, n]² at z = 0 as 2·n² faces on integer coordinates, every cell split along the same diagonal:
    the face test's arithmetic is exact on it, so rays through shared vertices and edges really tie."""
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = (i, j, 0), (i + 1, j, 0), (i + 1, j + 1, 0), (i, j + 1, 0)
            faces += [(a, b, c), (a, c, d)]
    return np.array(faces, np.float32)


def icosphere(level, radius=1.0):
    """20·4^level faces on the sphere of `radius`, outward orientation."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1),
         (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    tri = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
           (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
           (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache, out = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in tri:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tri = out
    v = np.array(v) * radius
    return v[np.array(tri)].astype(np.float32)


TRUNCATIONS = (1, 7, 8, 9, 31, 32, 33, 511, 512, 513, 1280)  # one below, at and one above every node size


def truncated(F):
    """The first F faces of the 1280-face icosphere."""
    return np.ascontiguousarray(icosphere(3)[:F])


def banana():
    """The packaged banana mesh as the optimisers upload it: float32 [16384, 3, 3]."""
    d = np.load(os.path.join(REPO, "compliancedex_amd", "data", "meshes", "banana_mesh.npz"))
    v, tri = np.asarray(d["vertices"], np.float64), np.asarray(d["triangles"], np.int64)
    return v[tri.flatten()].reshape(len(tri), 3, 3).astype(np.float32)


def degenerate():
    """A 320-face icosphere with one zero-area face and one NaN vertex: a prepared handle of it is SDF_MESH_EXACT."""
    f = icosphere(2).copy()
    f[5, 2] = f[5, 1]
    f[17, 0, 1] = np.nan
    return f


# ---- rays

RAY_COUNTS = (1, 63, 64, 65, 255, 256, 257)


def _vertices(faces):
    """The finite vertices, float64 [n, 3]."""
    v = np.asarray(faces).astype(np.float64).reshape(-1, 3)
    return v[np.isfinite(v).all(axis=1)]


def rays_inside(faces, R, seed):
    """From the vertex mean, random directions."""
    rng = np.random.default_rng(seed)
    c = _vertices(faces).mean(axis=0)
    return np.tile(c, (R, 1)), rng.standard_normal((R, 3))


def rays_outside(faces, R, seed, away=False):
    """From a shell around the mesh, aimed at points near it (or away from them)."""
    rng = np.random.default_rng(seed)
    v = _vertices(faces)
    c, ext = v.mean(axis=0), np.linalg.norm(v.max(axis=0) - v.min(axis=0))
    u = rng.standard_normal((R, 3))
    o = c + 2.0 * ext * u / np.linalg.norm(u, axis=1, keepdims=True)
    target = v[rng.integers(0, len(v), R)] + 0.02 * ext * rng.standard_normal((R, 3))
    d = target - o
    return o, (-d if away else d)


def mixed_rays(faces, R, seed):
    """A batch of every geometry: inside, outside aimed at and away, scaled directions."""
    k = max(1, R // 4)
    parts = [rays_inside(faces, k, seed), rays_outside(faces, k, seed + 1), rays_outside(faces, k, seed + 2, away=True)]
    o3, d3 = rays_outside(faces, R - 3 * k, seed + 3) if R > 3 * k else (np.zeros((0, 3)), np.zeros((0, 3)))
    scale = np.where(np.arange(len(o3)) % 2 == 0, 1e-3, 1e3)[:, None]
    parts.append((o3, d3 * scale))
    o = np.concatenate([q[0] for q in parts])[:R]
    d = np.concatenate([q[1] for q in parts])[:R]
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def lattice_rays():
    """Vertical rays down onto grid_plane(4) at its 81 half-integer lattice points, from z = 1: every hit is at t = 1
    exactly, on 1, 2, 3 or 6 faces."""
    x, y = np.meshgrid(np.arange(9) * 0.5, np.arange(9) * 0.5, indexing="ij")
    o = np.stack([x.reshape(-1), y.reshape(-1), np.ones(81)], axis=1)
    return o, np.tile([0.0, 0.0, -1.0], (81, 1))


def look_at_reference(eye, target, up, fov_deg, W, H):
    """(intrinsics [w, h, fx, fy, cx, cy], view matrix 4×4) from the reference's closed forms: PyBullet's
    computeViewMatrix / computeProjectionMatrixFOV (OpenGL conventions, column-major lists) and
    get_observable_pcd.py:19-24 (getIntrinsicParams), :55 (the transposed reshape)."""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, up / np.linalg.norm(up))
    s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    view = [s[0], u[0], -f[0], 0.0, s[1], u[1], -f[1], 0.0, s[2], u[2], -f[2], 0.0,
            -np.dot(s, eye), -np.dot(u, eye), np.dot(f, eye), 1.0]
    aspect = 1.0  # get_observable_pcd.py:53
    ys = 1.0 / np.tan(np.pi / 180.0 * fov_deg / 2.0)
    proj = np.zeros(16)
    proj[0], proj[5] = ys / aspect, ys
    intr = np.array([W, H, proj[0] * W / 2, proj[5] * H / 2, (-proj[2] * W + W) / 2, (proj[6] * H + H) / 2])
    return intr, np.asarray(view).reshape(4, 4).T


def banana_camera(faces, W, H):
    """The depth tests' camera: 12 cm from the banana's bounding-box centre along −x, 60° field of view."""
    from compliancedex_amd.raycast import Camera
    v = faces.astype(np.float64).reshape(-1, 3)
    c = 0.5 * (v.min(axis=0) + v.max(axis=0))
    return Camera.look_at(c + np.array([-0.12, 0.0, 0.0]), c, (0.0, 0.0, 1.0), 60.0, W, H)
