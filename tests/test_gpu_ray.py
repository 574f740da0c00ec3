"""Ray casting and the depth camera on an MI355X (cdx_ray.hip) against the host build of the same rule (cdxh_ray_cast,
cdxh_depth_unproject — themselves held to the numpy statement in test_ray_cpu.py), bit for bit on t, face, u and v:
the scan and the walk through the C ABI and through cast_rays, render against explicit rays, unprojection against the
host, and the chain render → cloud → GPIS.fit_pointcloud."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import _ray
from tests._ray import host_cast, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4  # output rows past R, preset and found untouched
SCAN, WALK = 1, 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


_MESH, _PREP, _REF = {}, {}, {}


def mesh(name):
    """name → float32 [F, 3, 3] numpy faces, built once."""
    if name not in _MESH:
        if name == "grid":
            _MESH[name] = _ray.grid_plane(4)
        elif name == "banana":
            _MESH[name] = _ray.banana()
        elif name == "degenerate":
            _MESH[name] = _ray.degenerate()
        elif name == "stacked":
            g = _ray.grid_plane(4)
            _MESH[name] = np.concatenate([g, g + np.array([0, 0, -1], np.float32)])
        else:
            _MESH[name] = _ray.truncated(int(name[1:]))
    return _MESH[name]


def prepared(name):
    from compliancedex_amd import PreparedMesh
    if name not in _PREP:
        _PREP[name] = PreparedMesh(torch.from_numpy(mesh(name)).to(DEV))
    return _PREP[name]


def reference(key, name, o, d, tmin=0.0, tmax=np.inf):
    """The host build's answer for a named case, computed once for the module."""
    if key not in _REF:
        _REF[key] = host_cast(mesh(name), o, d, tmin, tmax)
    return _REF[key]


def device_cast(name, o, d, mode, tmin=0.0, tmax=np.inf):
    """cdx_ray_cast through the C ABI: (t, face, uv) as numpy; GUARD rows past the end of each output are checked
    to be untouched."""
    from compliancedex_amd import _native as N
    lib = N.load()
    pm = prepared(name)
    R = len(o)
    od, dd = torch.from_numpy(np.ascontiguousarray(o)).to(DEV), torch.from_numpy(np.ascontiguousarray(d)).to(DEV)
    t = torch.full((R + GUARD,), -7.0, dtype=torch.float64, device=DEV)
    face = torch.full((R + GUARD,), -7, dtype=torch.int32, device=DEV)
    uv = torch.full((R + GUARD, 2), -7.0, dtype=torch.float64, device=DEV)
    walk = mode == WALK
    N.check(lib.cdx_ray_cast(N.ptr(pm.buf) if walk else None, N.ptr(pm.ray_records()) if walk else None,
                             N.ptr(pm.faces), pm.faces.shape[0], N.ptr(od), N.ptr(dd), R, tmin, tmax, mode, N.ptr(t),
                             N.ptr(face), N.ptr(uv), N.stream_ptr()), "cdx_ray_cast")
    t, face, uv = t.cpu().numpy(), face.cpu().numpy(), uv.cpu().numpy()
    assert np.all(t[R:] == -7.0) and np.all(face[R:] == -7) and np.all(uv[R:] == -7.0)
    return t[:R], face[:R], uv[:R]


def check(key, name, o, d, tmin=0.0, tmax=np.inf):
    """Host == scan == walk through the C ABI, and == cast_rays on the raw tensor and on the prepared mesh."""
    from compliancedex_amd import cast_rays
    rt, rf, ruv = reference(key, name, o, d, tmin, tmax)
    for mode in (SCAN, WALK):
        t, f, uv = device_cast(name, o, d, mode, tmin, tmax)
        assert np.array_equal(f, rf), (key, mode, np.flatnonzero(f != rf)[:8])
        assert same_bits(t, rt) and same_bits(uv, ruv), (key, mode)
    od, dd = torch.from_numpy(np.ascontiguousarray(o)).to(DEV), torch.from_numpy(np.ascontiguousarray(d)).to(DEV)
    raw = torch.from_numpy(mesh(name)).to(DEV)
    for m, mode in ((raw, "auto"), (raw, "scan"), (prepared(name), "auto"), (prepared(name), "scan"),
                    (prepared(name), "walk")):
        t, f, uv = cast_rays(m, od, dd, tmin, tmax, mode=mode, want_uv=True)
        assert np.array_equal(f.cpu().numpy(), rf) and same_bits(t.cpu().numpy(), rt), (key, mode)
        assert same_bits(uv.cpu().numpy(), ruv), (key, mode)
    t, f = prepared(name).cast_rays(od, dd, tmin, tmax)
    assert np.array_equal(f.cpu().numpy(), rf) and same_bits(t.cpu().numpy(), rt)
    return rt, rf, ruv


MESHES = ["grid"] + [f"F{F}" for F in _ray.TRUNCATIONS] + ["banana", "degenerate"]


@pytest.mark.parametrize("name", MESHES)
def test_scan_walk_and_host_agree(name):
    """Every mesh — the node-size truncations, the exact lattice, the banana, the NaN-capable mesh — with every ray
    count around the wave and the workgroup, on a batch of all geometries (inside, aimed at, aimed away, directions
    scaled by 1e-3 and 1e3)."""
    hit_any = False
    for R in _ray.RAY_COUNTS:
        o, d = _ray.mixed_rays(mesh(name), R, seed=1000 + R)
        _, f, _ = check((name, R), name, o, d)
        hit_any |= bool((f >= 0).any())
    assert hit_any or name in ("F1", "F7", "F8", "F9")


def test_mesh_kinds_and_auto():
    from compliancedex_amd import _native as N
    assert prepared("banana").kind == N.SDF_MESH_CULLED and prepared("banana").num_faces == 16384
    assert prepared("degenerate").kind == N.SDF_MESH_EXACT  # auto takes the scan for it (_mesh_args)
    from compliancedex_amd.raycast import _mesh_args
    assert _mesh_args(prepared("degenerate"), "auto")[3] == N.RAY_MODES["scan"]
    assert _mesh_args(prepared("banana"), "auto")[3] == N.RAY_MODES["walk"]
    with pytest.raises(ValueError):
        _mesh_args(torch.from_numpy(mesh("grid")).to(DEV), "walk")


def test_lattice_ties():
    """81 vertical rays through the vertices, edges and diagonals of the integer lattice: t == 1 exactly on up to six
    faces; the smallest original index wins in the k-d ordered walk as in the scan."""
    o, d = _ray.lattice_rays()
    t, f, _ = check("lattice", "grid", o, d)
    assert np.all(t == 1.0) and np.all(f >= 0)
    # origin exactly on a face: t == 0, tmin inclusive
    o = np.array([[1.25, 2.5, 0.0], [2.0, 2.0, 0.0]])
    d = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]])
    t, f, _ = check("on_face", "grid", o, d)
    assert np.all(t == 0.0) and f[1] == min(k for k, _ in _ray.numpy_hits(mesh("grid"), o[1], d[1]))
    # parallel to the plane: det == 0
    o, d = np.array([[-1.0, 1.25, 0.0], [-1.0, 1.25, 0.5]]), np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    assert np.all(check("parallel", "grid", o, d)[1] == -1)


def test_inside_the_banana_every_ray_hits():
    o, d = _ray.rays_inside(mesh("banana"), 2000, seed=1)
    t, f, _ = check("inside", "banana", o, d)
    assert np.all(f >= 0) and np.all(np.isfinite(t))
    o, d = _ray.rays_outside(mesh("banana"), 257, seed=2, away=True)
    assert np.all(check("away", "banana", o, d)[1] == -1)


def test_tmin_tmax():
    o, d = np.array([[1.25, 2.5, 1.0]] * 3), np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1e-3], [0.0, 0.0, -1e3]])
    assert np.allclose(check("st0", "stacked", o, d)[0], [1.0, 1000.0, 0.001], rtol=1e-12, atol=0)  # t scales with 1/|d|
    assert check("st1", "stacked", o[:1], d[:1], 0.0, 1.5)[0][0] == 1.0   # between the first and the second hit
    assert check("st2", "stacked", o[:1], d[:1], 1.5, np.inf)[0][0] == 2.0
    assert check("st3", "stacked", o[:1], d[:1], 0.0, 0.5)[1][0] == -1    # below the first
    assert check("st4", "stacked", o[:1], d[:1], 0.0, 1.0)[0][0] == 1.0   # inclusive
    # on the banana: tmax between a ray's first hit and beyond, and below it
    ob, db = _ray.rays_outside(mesh("banana"), 65, seed=4)
    t, f, _ = check("b0", "banana", ob, db)
    k = int(np.flatnonzero(f >= 0)[0])
    assert check("b1", "banana", ob, db, 0.0, float(t[k]))[0][k] == t[k]
    assert check("b2", "banana", ob, db, 0.0, float(np.nextafter(t[k], 0.0)))[1][k] == -1
    t2 = check("b3", "banana", ob, db, float(np.nextafter(t[k], np.inf)), np.inf)[0][k]
    assert t2 > t[k]


def test_nonfinite_rays_stay_in_their_lane():
    for name in ("banana", "F513"):
        o, d = _ray.mixed_rays(mesh(name), 65, seed=77)
        t0, f0, uv0 = check((name, "nf0"), name, o, d)
        o2, d2 = o.copy(), d.copy()
        o2[0, 1] = np.nan
        d2[5, 2] = np.inf
        d2[63] = 0.0
        t, f, uv = check((name, "nf1"), name, o2, d2)
        bad = np.zeros(65, bool)
        bad[[0, 5, 63]] = True
        assert np.all(f[bad] == -1) and np.all(np.isinf(t[bad])) and np.all(uv[bad] == 0)
        assert np.array_equal(f[~bad], f0[~bad]) and same_bits(t[~bad], t0[~bad]) and same_bits(uv[~bad], uv0[~bad])


def test_out_of_domain_rays_walk_without_skipping():
    """Origins and directions outside the walk's proven domain (|o| > 1e6, |d| beyond 2^±64) still equal the scan."""
    o, d = _ray.mixed_rays(mesh("F1280"), 64, seed=5)
    d[::4] *= 2.0 ** 70
    d[1::4] *= 2.0 ** -70
    o[2::4] += 3e6
    check("domain", "F1280", o, d, -np.inf, np.inf)


def test_float32_rays_are_widened():
    from compliancedex_amd import cast_rays
    o, d = _ray.mixed_rays(mesh("banana"), 257, seed=8)
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    rt, rf, _ = reference("f32", "banana", o32.astype(np.float64), d32.astype(np.float64))
    for mode in ("scan", "walk"):
        t, f = cast_rays(prepared("banana"), torch.from_numpy(o32).to(DEV), torch.from_numpy(d32).to(DEV), mode=mode)
        assert np.array_equal(f.cpu().numpy(), rf) and same_bits(t.cpu().numpy(), rt)
    t, f = cast_rays(prepared("banana"), torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV))
    assert t.shape == (0,) and f.shape == (0,)


def test_abi_rejections_write_nothing():
    from compliancedex_amd import _native as N
    lib = N.load()
    pm = prepared("F33")
    o, d = (torch.from_numpy(x).to(DEV) for x in _ray.mixed_rays(mesh("F33"), 8, seed=1))
    t = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    face = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    mp, rp, fp, F, s = N.ptr(pm.buf), N.ptr(pm.ray_records()), N.ptr(pm.faces), 33, N.stream_ptr()
    cast = lib.cdx_ray_cast
    args = dict(mesh=mp, ray=rp, faces=fp, F=F, o=N.ptr(o), d=N.ptr(d), R=8, mode=WALK, t=N.ptr(t), face=N.ptr(face))

    def call(**kw):
        a = dict(args, **kw)
        return cast(a["mesh"], a["ray"], a["faces"], a["F"], a["o"], a["d"], a["R"], 0.0, math.inf, a["mode"], a["t"],
                    a["face"], None, s)
    for bad in (dict(R=-1), dict(F=0), dict(F=-3), dict(faces=None), dict(o=None), dict(d=None), dict(t=None),
                dict(face=None), dict(mode=3), dict(mode=-1), dict(mesh=None), dict(ray=None),
                dict(F=2 ** 31)):
        assert call(**bad) < 0, bad
    assert call(R=0) == 0
    torch.cuda.synchronize()
    assert torch.all(t == -7.0) and torch.all(face == -7)
    assert lib.cdx_ray_mesh_bytes(0) == 0 and lib.cdx_ray_mesh_bytes(-1) == 0
    assert lib.cdx_ray_mesh_prepare(None, 33, rp, s) < 0 and lib.cdx_ray_mesh_prepare(mp, 0, rp, s) < 0
    intr = (C.c_double * 4)(1, 1, 0, 0)
    M = (C.c_double * 16)(*np.eye(4).reshape(-1))
    depth = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    render = lib.cdx_depth_render
    assert render(None, None, fp, F, 0, 2, intr, M, 0.0, math.inf, SCAN, N.ptr(depth), None, s) < 0
    assert render(None, None, fp, F, 2, 2, None, M, 0.0, math.inf, SCAN, N.ptr(depth), None, s) < 0
    assert render(None, None, fp, F, 2, 2, intr, M, 0.0, math.inf, SCAN, None, None, s) < 0
    assert render(None, None, fp, F, 2, 2, intr, M, 0.0, math.inf, WALK, N.ptr(depth), None, s) < 0
    ws = torch.empty(lib.cdx_depth_workspace(2, 2, 1), dtype=torch.uint8, device=DEV)
    total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    assert lib.cdx_depth_workspace(0, 2, 1) == 0 and lib.cdx_depth_workspace(2, 2, 0) == 0
    assert lib.cdx_depth_count(N.ptr(depth), 5, 2, 2, 1, 1.0, 9.9, math.nan, N.ptr(ws), N.ptr(total), s) < 0
    assert lib.cdx_depth_count(None, 1, 2, 2, 1, 1.0, 9.9, math.nan, N.ptr(ws), N.ptr(total), s) < 0
    assert lib.cdx_depth_place(N.ptr(depth), 1, 2, 2, 1, None, 1.0, 9.9, math.nan, None, N.ptr(ws), 4, N.ptr(depth),
                               s) < 0
    assert lib.cdx_depth_place(N.ptr(depth), 1, 2, 2, 1, intr, 1.0, 9.9, math.nan, None, N.ptr(ws), -1, N.ptr(depth),
                               s) < 0
    torch.cuda.synchronize()
    assert torch.all(depth == -7.0) and int(total.item()) == -7


# ---- depth

SIZES = [(1, 1), (8, 8), (9, 7), (65, 33)]
_RENDER = {}


def camera(W, H):
    return _ray.banana_camera(mesh("banana"), W, H)


def rendered(W, H):
    """(depth, face) of the banana at W×H by the walk, as numpy, rendered once for the module."""
    from compliancedex_amd import render_depth
    if (W, H) not in _RENDER:
        depth, face = render_depth(prepared("banana"), camera(W, H), want_face=True)
        _RENDER[(W, H)] = (depth.cpu().numpy(), face.cpu().numpy())
    return _RENDER[(W, H)]


@pytest.mark.parametrize("W,H", SIZES)
def test_render_equals_explicit_rays(W, H):
    from compliancedex_amd import cast_rays, render_depth
    cam = camera(W, H)
    o, d = cam.rays()
    ho, hd = _ray.host_pixel_rays(W, H, [cam.fx, cam.fy, cam.cx, cam.cy], cam.camera_to_world)
    assert same_bits(o.numpy(), ho) and same_bits(d.numpy(), hd)
    rt, rf, _ = reference(("px", W, H), "banana", ho, hd)
    depth, face = rendered(W, H)
    assert depth.shape == (H, W) and face.shape == (H, W)
    assert np.array_equal(face.reshape(-1), rf)
    assert same_bits(depth.reshape(-1), np.where(rf >= 0, rt, 0.0))
    t, f = cast_rays(prepared("banana"), o.to(DEV), d.to(DEV))
    assert np.array_equal(f.cpu().numpy(), rf) and same_bits(t.cpu().numpy(), rt)
    for m, mode in ((prepared("banana"), "scan"), (torch.from_numpy(mesh("banana")).to(DEV), "auto")):
        d2, f2 = render_depth(m, cam, want_face=True, mode=mode)
        assert same_bits(d2.cpu().numpy(), depth) and np.array_equal(f2.cpu().numpy(), face)
    assert same_bits(render_depth(prepared("banana"), cam).cpu().numpy(), depth)
    if W * H >= 63:
        share = (rf >= 0).mean()
        print(f"{W}x{H}: {(rf >= 0).sum()} of {W * H} pixels hit")
        assert 0.10 <= share <= 0.90


def unproject_cases(cam, depth):
    """Strides 1 and 2, a depth_trunc above every pixel and one at the third quartile of the hit depths, the z mask off
    and at their median, the transform off and on."""
    q50, q75 = np.quantile(depth[depth > 0], [0.5, 0.75])
    return [dict(stride=s, trunc=tr, z_max=zm, M=M) for s in (1, 2) for tr in (9.9, float(q75))
            for zm in (None, float(q50)) for M in (None, cam.camera_to_world)]


@pytest.mark.parametrize("kind", ["u16", "f32", "f64"])
def test_unproject_equals_host(kind):
    from compliancedex_amd import depth_to_pointcloud
    W, H = 65, 33
    cam = camera(W, H)
    depth, _ = rendered(W, H)
    img = {"u16": (depth * 1000.0).astype(np.uint16), "f32": depth.astype(np.float32), "f64": depth}[kind]
    scale = 1000.0 if kind == "u16" else 1.0
    intr = [cam.fx, cam.fy, cam.cx, cam.cy]
    dimg = torch.from_numpy(img).to(DEV)
    counts = set()
    for c in unproject_cases(cam, depth):
        ref = _ray.host_unproject(img, intr, scale, c["trunc"], c["z_max"], c["M"], c["stride"])
        if c["M"] is None:
            got = depth_to_pointcloud(dimg, cam, scale, c["trunc"], c["z_max"], world=False, stride=c["stride"])
        else:
            got = depth_to_pointcloud(dimg, cam, scale, c["trunc"], c["z_max"], world=True, stride=c["stride"])
        assert got.dtype == torch.float64 and got.is_cuda
        assert same_bits(got.cpu().numpy(), ref), (kind, c["stride"], c["trunc"], c["z_max"], c["M"] is not None)
        counts.add(len(ref))
    assert len(counts) >= 4 and min(counts) > 0  # the truncation, the mask and the stride each cut some pixels
    empty = depth_to_pointcloud(torch.zeros_like(dimg), cam, scale)
    assert tuple(empty.shape) == (0, 3) and empty.dtype == torch.float64


def test_unproject_small_images():
    from compliancedex_amd import depth_to_pointcloud
    for W, H in ((1, 1), (8, 8), (9, 7)):
        cam = camera(W, H)
        depth, _ = rendered(W, H)
        ref = _ray.host_unproject(depth, [cam.fx, cam.fy, cam.cx, cam.cy], 1.0, 9.9, None, cam.camera_to_world, 1)
        got = depth_to_pointcloud(torch.from_numpy(depth).to(DEV), cam, 1.0, 9.9)
        assert same_bits(got.cpu().numpy(), ref)


def test_round_trip():
    """render → unproject to the world against o + t·d.  float64 depth: 1e-12 m (float64 rounding through about ten
    operations at about 0.3 m, with a wide margin).  uint16 millimetres: within 1 mm·|d| along the ray, the truncation."""
    from compliancedex_amd import depth_to_pointcloud
    W, H = 65, 33
    cam = camera(W, H)
    depth, face = rendered(W, H)
    o, d = (x.numpy() for x in cam.rays())
    hit = face.reshape(-1) >= 0
    pts = o[hit] + depth.reshape(-1)[hit, None] * d[hit]
    got = depth_to_pointcloud(torch.from_numpy(depth).to(DEV), cam, 1.0, 9.9).cpu().numpy()
    assert got.shape == pts.shape
    err = np.abs(got - pts).max()
    print(f"float64 round trip: {err:.3e} m")
    assert err < 1e-12
    q = (depth * 1000.0).astype(np.uint16)
    got = depth_to_pointcloud(torch.from_numpy(q).to(DEV), cam, 1000.0, 9.9).cpu().numpy()
    assert got.shape == pts.shape
    dn = np.linalg.norm(d[hit], axis=1)
    along = ((pts - got) * d[hit]).sum(axis=1) / dn   # the truncation moves a point toward the camera, along its ray
    off = np.linalg.norm((pts - got) - along[:, None] * d[hit] / dn[:, None], axis=1)
    print(f"uint16 round trip: along {along.min():.3e} .. {along.max():.3e} m, off the ray {off.max():.3e} m")
    assert np.all(np.abs(along) <= 1e-3 * dn) and off.max() < 1e-12


# ---- end to end

def test_observable_pointcloud_feeds_fit_pointcloud():
    from compliancedex_amd import GPIS, compute_sdf, observable_pointcloud
    cam = camera(64, 64)
    cloud = observable_pointcloud(prepared("banana"), cam, num_points=200)
    assert tuple(cloud.shape) == (200, 3) and cloud.is_cuda and cloud.dtype == torch.float64
    assert torch.isfinite(cloud).all()
    sq, _, _, _ = compute_sdf(cloud.float(), prepared("banana"))
    dist = sq.sqrt().max().item()
    print(f"observable cloud: max distance to the mesh {dist * 1e3:.3f} mm")
    # 1 mm quantisation along the ray times |d| ≤ sqrt(1 + 2·tan²30°) ≈ 1.29 at this 60° field of view
    assert dist < 1.5e-3
    same = observable_pointcloud(torch.from_numpy(mesh("banana")).to(DEV), cam, num_points=200)
    assert same_bits(same.cpu().numpy(), cloud.cpu().numpy())
    g = torch.Generator(device="cpu").manual_seed(0)
    noisy = observable_pointcloud(prepared("banana"), cam, num_points=200, noise=1e-4, generator=g, shuffle=True)
    assert tuple(noisy.shape) == (200, 3) and torch.isfinite(noisy).all()
    with pytest.raises(ValueError):
        observable_pointcloud(prepared("banana"), cam, num_points=100000)
    gp = GPIS().fit_pointcloud(cloud, num_points=64)
    assert torch.isfinite(gp.E11).all()
    assert tuple(gp.X1.shape) == (14 + 64 + 50, 3) and tuple(gp.E11.shape) == (128, 128)  # exterior, surface, interior


def test_occluded():
    """An icosphere seen from outside: its far-side vertices are hidden; near-side vertices pulled 1 % toward the eye
    are not.  Exact expectations."""
    from compliancedex_amd import occluded
    faces = _ray.icosphere(3)
    eye = np.array([3.0, 0.4, -0.2])
    v = np.unique(faces.astype(np.float64).reshape(-1, 3), axis=0)
    side = v @ eye / np.linalg.norm(eye)
    far, near = v[side < -0.2], v[side > 0.5]
    assert len(far) > 50 and len(near) > 50
    near = near + 0.01 * (eye - near)
    m = torch.from_numpy(faces).to(DEV)
    from compliancedex_amd import PreparedMesh
    for msh in (m, PreparedMesh(m)):
        assert occluded(msh, eye, torch.from_numpy(far).to(DEV)).all()
        assert not occluded(msh, torch.from_numpy(eye), torch.from_numpy(near).to(DEV)).any()
        out = occluded(msh, eye, torch.from_numpy(near).float().to(DEV))
        assert out.dtype == torch.bool and tuple(out.shape) == (len(near),)
