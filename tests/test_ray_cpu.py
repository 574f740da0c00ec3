"""The ray casting and depth unprojection rules of csrc/cdx_ray.h without a GPU: the numpy statement against the host
build (cdxh_ray_cast, cdxh_pixel_rays, cdxh_depth_unproject) bit for bit on small meshes, the tie rule on the exact
lattice, the walk's node-skip margin (cdxh_ray_ball_miss), and Camera.look_at against the reference's closed forms.
The device kernels are held to the host build in test_gpu_ray.py."""
import numpy as np
import pytest

from tests import _ray
from tests._ray import host_cast, numpy_cast, same_bits


def agree(faces, o, d, tmin=0.0, tmax=np.inf):
    """numpy == host on (t, face, u, v), bit for bit; returns them."""
    nt, nf, nuv = numpy_cast(faces, o, d, tmin, tmax)
    ht, hf, huv = host_cast(faces, o, d, tmin, tmax)
    assert np.array_equal(nf, hf)
    assert same_bits(nt, ht) and same_bits(nuv, huv)
    return ht, hf, huv


def test_lattice_ties_go_to_the_smallest_face_index():
    """Vertical rays at the 81 half-integer lattice points of grid_plane(4): exact arithmetic, t == 1 on 1, 2, 3 or 6
    faces (18 / 42 / 12 / 9 rays), and the winner is the smallest index among them — also with the faces reversed,
    where the same geometric faces carry other indices."""
    faces = _ray.grid_plane(4)
    assert faces.shape == (32, 3, 3)
    o, d = _ray.lattice_rays()
    t, f, uv = agree(faces, o, d)
    assert np.all(t == 1.0)
    counts = []
    for r in range(81):
        hits = _ray.numpy_hits(faces, o[r], d[r])
        assert all(tt == 1.0 for _, tt in hits)
        counts.append(len(hits))
        assert f[r] == min(k for k, _ in hits)
    assert sorted(np.unique(counts, return_counts=True)[1].tolist()) == [9, 12, 18, 42]
    assert dict(zip(*np.unique(counts, return_counts=True))) == {1: 18, 2: 42, 3: 12, 6: 9}
    rt, rf, _ = agree(faces[::-1].copy(), o, d)
    assert np.all(rt == 1.0)
    for r in range(81):
        assert rf[r] == min(31 - k for k, _ in _ray.numpy_hits(faces, o[r], d[r]))


@pytest.mark.parametrize("F", [1, 7, 8, 9, 31, 32, 33, 320])
def test_numpy_equals_host_on_truncated_spheres(F):
    faces = _ray.truncated(F) if F != 320 else _ray.icosphere(2)
    o, d = _ray.mixed_rays(faces, 65, seed=F)
    t, f, _ = agree(faces, o, d)
    if F == 320:
        assert (f >= 0).sum() >= 16  # the inside rays all hit a closed sphere


def test_inside_a_closed_mesh_every_ray_hits():
    faces = _ray.icosphere(2)
    o, d = _ray.rays_inside(faces, 200, seed=5)
    t, f, uv = agree(faces, o, d)
    assert np.all(f >= 0) and np.all(np.isfinite(t)) and np.all(t > 0)
    # the hit point from (u, v) is the hit point from t
    fv = faces.astype(np.float64)[f]
    pb = fv[:, 0] * (1 - uv[:, :1] - uv[:, 1:]) + fv[:, 1] * uv[:, :1] + fv[:, 2] * uv[:, 1:]
    assert np.abs(pb - (o + t[:, None] * d)).max() < 1e-12


def test_aimed_away_is_a_miss():
    faces = _ray.icosphere(2)
    o, d = _ray.rays_outside(faces, 64, seed=2, away=True)
    t, f, uv = agree(faces, o, d)
    assert np.all(f == -1) and np.all(np.isinf(t)) and np.all(uv == 0)


def test_parallel_on_face_tmax_and_scaling():
    faces = _ray.grid_plane(4)
    # in the plane z = 0 and above it, along x: det == 0 on every face
    o = np.array([[-1.0, 1.25, 0.0], [-1.0, 1.25, 0.5]])
    d = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    t, f, _ = agree(faces, o, d)
    assert np.all(f == -1)
    # origin exactly on a face: t == 0 is a hit (tmin inclusive), from either side
    o = np.array([[1.25, 2.5, 0.0], [1.25, 2.5, 0.0]])
    d = np.array([[0.0, 0.0, -1.0], [0.3, 0.1, 1.0]])
    t, f, _ = agree(faces, o, d)
    assert np.all(t == 0.0) and np.all(f >= 0)
    t, f, _ = agree(faces, o, d, tmin=np.nextafter(0.0, 1.0))
    assert np.all(f == -1)
    # two stacked planes: tmax between the first and the second hit, and below the first
    two = np.concatenate([faces, faces + np.array([0, 0, -1], np.float32)])
    o, d = np.array([[1.25, 2.5, 1.0]]), np.array([[0.0, 0.0, -1.0]])
    assert agree(two, o, d)[0][0] == 1.0
    assert agree(two, o, d, tmax=1.5)[0][0] == 1.0
    assert agree(two, o, d, tmin=1.5)[0][0] == 2.0
    assert agree(two, o, d, tmax=0.5)[1][0] == -1
    assert agree(two, o, d, tmax=1.0)[0][0] == 1.0  # tmax inclusive
    # t scales with 1/|d|
    for s in (1e-3, 1e3):
        ts, fs, _ = agree(two, o, d * s)
        assert fs[0] >= 0 and abs(ts[0] * s - 1.0) < 1e-12


def test_nonfinite_rays_miss_and_leave_the_others_alone():
    faces = _ray.icosphere(2)
    o, d = _ray.mixed_rays(faces, 65, seed=9)
    t0, f0, uv0 = agree(faces, o, d)
    o2, d2 = o.copy(), d.copy()
    o2[0, 1] = np.nan
    d2[5, 2] = np.inf
    d2[63] = 0.0
    t, f, uv = agree(faces, o2, d2)
    bad = np.zeros(65, bool)
    bad[[0, 5, 63]] = True
    assert np.all(f[bad] == -1) and np.all(np.isinf(t[bad])) and np.all(uv[bad] == 0)
    assert np.array_equal(f[~bad], f0[~bad]) and same_bits(t[~bad], t0[~bad]) and same_bits(uv[~bad], uv0[~bad])


def test_degenerate_mesh():
    """A zero-area face and a NaN vertex: never hit, never in the way."""
    faces = _ray.degenerate()
    o, d = _ray.mixed_rays(faces, 64, seed=3)
    t, f, _ = agree(faces, o, d)
    assert not np.isin(f, [5, 17]).any()
    assert (f >= 0).sum() >= 16


def test_node_skip_is_conservative():
    """The walk's skip (cdx::ray_ball_miss) on faces the rule accepts: for a ball that holds the face's vertices —
    centre rounded to float32, radius padded by 1e-6 as the mesh's nodes are — no accepted hit with tmin ≤ t ≤ s1 is
    skipped, down to grazing angles at the determinant threshold, for near and far origins and scaled directions."""
    rng = np.random.default_rng(0)
    n = 20000
    v = rng.standard_normal((n, 3, 3)) * (10.0 ** rng.uniform(-4, 0, (n, 1, 1)))
    v[::3, 2] = v[::3, 1] + (v[::3, 1] - v[::3, 0]) * 0.5 + rng.standard_normal((len(v[::3]), 3)) * 1e-6  # slivers
    v += rng.standard_normal((n, 1, 3)) * rng.choice([0.0, 1.0, 100.0], (n, 1, 1))
    faces = v.astype(np.float32)
    fv = faces.astype(np.float64)
    w = rng.dirichlet([1, 1, 1], n)
    target = (fv * w[:, :, None]).sum(axis=1)
    nrm = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    edge = fv[:, 1] - fv[:, 0]
    edge /= np.maximum(np.linalg.norm(edge, axis=1, keepdims=True), 1e-300)
    graze = 10.0 ** rng.uniform(-7, 0, (n, 1))  # sine of the angle to the plane: across the 2^-20 threshold
    dirn = edge * np.sqrt(np.maximum(1 - graze ** 2, 0)) + nrm * graze
    dist = 10.0 ** rng.uniform(-3, 3, (n, 1))
    o = target - dirn * dist
    d = dirn * dist * 10.0 ** rng.uniform(-3, 3, (n, 1))
    c = (0.5 * (fv.min(axis=1) + fv.max(axis=1))).astype(np.float32)
    R = (np.sqrt(((fv - c[:, None, :].astype(np.float64)) ** 2).sum(axis=2).max(axis=1)) * (1 + 1e-6)).astype(np.float32)
    balls = np.concatenate([c, R[:, None]], axis=1)
    t = np.full(n, np.inf)
    hit = np.zeros(n, bool)
    for k in range(n):  # one face each: the host build, a ray at a time
        tt, ff, _ = host_cast(faces[k:k + 1], o[k:k + 1], d[k:k + 1], -np.inf, np.inf)
        t[k], hit[k] = tt[0], ff[0] == 0
    assert hit.sum() > n // 4 and (~hit).sum() > n // 100
    for s0, s1 in ((np.full(n, -np.inf), np.full(n, np.inf)), (t, t), (np.full(n, -np.inf), t), (t, np.full(n, np.inf))):
        miss, dom = _ray.host_ball_miss(o, d, s0, s1, balls)
        assert dom.sum() > n // 2
        assert not (miss & hit & dom).any()
    # and the skip does skip: a ball far off the ray
    far = balls.copy()
    far[:, :3] += (np.cross(dirn, nrm) * (100.0 * (R[:, None] + dist))).astype(np.float32)
    miss, _ = _ray.host_ball_miss(o, d, np.full(n, -np.inf), np.full(n, np.inf), far)
    assert miss.mean() > 0.99


def camera_setup(W, H):
    eye, target, up = np.array([-0.3, 0.02, 0.05]), np.array([0.01, 0.0, 0.02]), np.array([0.0, 0.0, 1.0])
    from compliancedex_amd.raycast import Camera
    return Camera.look_at(eye, target, up, 70.0, W, H), _ray.look_at_reference(eye, target, up, 70.0, W, H), eye


@pytest.mark.parametrize("W,H", [(1000, 1000), (65, 33)])
def test_look_at_matches_the_reference_formulas(W, H):
    cam, (intr, view), eye = camera_setup(W, H)
    assert np.allclose([cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy], intr, rtol=1e-14, atol=0)
    # the reference's world points: flip the unprojected point by [1, −1, −1], then the inverse view matrix
    pc = np.array([0.013, -0.021, 0.31, 1.0])  # a point in this camera's frame (x right, y down, z forward)
    ref_world = np.linalg.inv(view) @ (pc * np.array([1.0, -1.0, -1.0, 1.0]))
    assert np.abs(cam.camera_to_world @ pc - ref_world).max() < 1e-15
    assert np.abs(cam.eye - eye).max() < 1e-15
    # a known world point lands on the expected pixel: along the optical axis → (cy, cx); offset right and down
    axis = cam.camera_to_world @ np.array([0.0, 0.0, 0.25, 1.0])
    q = cam.world_to_camera @ axis
    assert abs(q[0] / q[2] * cam.fx + cam.cx - W / 2) < 1e-9 and abs(q[1] / q[2] * cam.fy + cam.cy - H / 2) < 1e-9
    i, j = H // 4, (3 * W) // 4
    o, d = (x.numpy() for x in cam.rays())
    pw = o[i * W + j] + 0.3 * d[i * W + j]
    q = cam.world_to_camera @ np.append(pw, 1.0)
    assert abs(q[2] - 0.3) < 1e-12
    assert abs(q[0] / q[2] * cam.fx + cam.cx - j) < 1e-9 and abs(q[1] / q[2] * cam.fy + cam.cy - i) < 1e-9
    # up in the world is up in the image: a point above the target has a smaller row
    above = cam.world_to_camera @ np.array([0.01, 0.0, 0.07, 1.0])
    assert above[1] / above[2] * cam.fy + cam.cy < cam.cy


def test_pixel_rays_numpy_equals_host():
    cam, _, _ = camera_setup(9, 7)
    intr = [cam.fx, cam.fy, cam.cx, cam.cy]
    ho, hd = _ray.host_pixel_rays(9, 7, intr, cam.camera_to_world)
    no, nd = _ray.numpy_pixel_rays(9, 7, intr, cam.camera_to_world)
    co, cd = (x.numpy() for x in cam.rays())
    assert same_bits(ho, no) and same_bits(hd, nd) and same_bits(ho, co) and same_bits(hd, cd)
    assert np.abs((cam.world_to_camera[:3, :3] @ hd.T)[2] - 1.0).max() < 1e-14  # the camera-frame z component is 1


def depth_images(W, H, seed=0):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.05, 1.2, (H, W))
    z[rng.random((H, W)) < 0.3] = 0.0
    return {"u16": (z * 1000.0).astype(np.uint16), "f32": z.astype(np.float32), "f64": z}


@pytest.mark.parametrize("kind,scale", [("u16", 1000.0), ("f32", 1.0), ("f64", 1.0)])
def test_unproject_numpy_equals_host(kind, scale):
    cam, _, _ = camera_setup(9, 7)
    intr = [cam.fx, cam.fy, cam.cx, cam.cy]
    depth = depth_images(9, 7)[kind]
    for stride in (1, 2):
        for trunc in (9.9, 0.8):
            for z_max in (None, 0.6):
                for M in (None, cam.camera_to_world):
                    hp = _ray.host_unproject(depth, intr, scale, trunc, z_max, M, stride)
                    npts = _ray.numpy_unproject(depth, intr, scale, trunc, z_max, M, stride)
                    assert same_bits(hp, npts), (kind, stride, trunc, z_max, M is not None)
    full = _ray.host_unproject(depth, intr, scale, 9.9)
    assert 0 < len(_ray.host_unproject(depth, intr, scale, 0.8)) < len(full) < 63
    assert len(_ray.host_unproject(np.zeros_like(depth), intr, scale, 9.9)) == 0


def test_python_entry_points_need_a_device():
    import torch

    from compliancedex_amd import Camera, cast_rays, depth_to_pointcloud, occluded, render_depth  # noqa: F401
    from compliancedex_amd.torchsdf import PreparedMesh
    assert hasattr(PreparedMesh, "cast_rays")
    faces = torch.from_numpy(_ray.grid_plane(2))
    with pytest.raises(RuntimeError):
        cast_rays(faces, torch.zeros(1, 3), torch.ones(1, 3))
    with pytest.raises(ValueError):
        cast_rays(faces, torch.zeros(1, 3), torch.ones(1, 3), mode="fast")
