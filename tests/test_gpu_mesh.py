"""GPIS.tomesh / surface_mesh on an MI355X: the two compaction passes (cdx_gpis_mesh_count / _place) against their host
build (cdxh_mesh_extract) bit for bit, the public methods on the reference's field fixtures and on the mug state, and
the mesh's way into the triangle-mesh half (PreparedMesh, compute_sdf, occluded, render_depth)."""
import numpy as np
import pytest
import torch

from tests._field import F32, F64, point_axes
from tests._helpers import golden
from tests._mesh import host_mesh, key_ends, same_bits, salted_inf_mean

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIXTURES = {"banana": "field_banana_s13.npz", "mug": "field_mug_s9.npz"}
AXES_LB, AXES_UB = [-1.0, 0.5, 2.0], [1.0, 3.5, 2.5]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


@pytest.fixture(scope="module")
def mug():
    from compliancedex_amd.workloads import stored_gpis
    return stored_gpis("mug", DEV)


@pytest.fixture(scope="module")
def mug_mesh(mug):
    """tomesh of the field_mug_s9 fixture mean (a closed mesh), shared."""
    d = golden(FIXTURES["mug"])
    return d, mug.tomesh(d["mean"], d["lb"], d["ub"], steps=int(d["steps"]))


def device_mesh(mean, axes, vcap, fcap, vrows, frows):
    """cdx_gpis_mesh_count + _place on a host lattice uploaded in its own dtype: ((V, F), vertices, keys, faces) with
    vrows ≥ vcap and frows ≥ fcap rows preset to guard values."""
    from compliancedex_amd import _native as N
    lib = N.load()
    steps = mean.shape[0]
    dtype = F32 if mean.dtype == np.float32 else F64
    m = torch.from_numpy(np.ascontiguousarray(mean)).to(DEV)
    ax = torch.from_numpy(np.stack(axes)).to(DEV)
    ws = torch.empty(lib.cdx_gpis_mesh_workspace(steps), dtype=torch.uint8, device=DEV)
    totals = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    v = torch.full((vrows, 3), -7.0, dtype=torch.float64, device=DEV)
    keys = torch.full((vrows,), -1, dtype=torch.int64, device=DEV)
    faces = torch.full((frows, 3), -1, dtype=torch.int32, device=DEV)
    s = N.stream_ptr()
    N.check(lib.cdx_gpis_mesh_count(N.ptr(m), dtype, steps, N.ptr(ws), N.ptr(totals), s), "count")
    N.check(lib.cdx_gpis_mesh_place(N.ptr(m), dtype, steps, N.ptr(ax[0]), N.ptr(ax[1]), N.ptr(ax[2]), N.ptr(ws), vcap,
                                    fcap, N.ptr(v), N.ptr(keys), N.ptr(faces), s), "place")
    V, F = (int(x) for x in totals.cpu())
    return (V, F), v.cpu().numpy(), keys.cpu().numpy(), faces.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("steps", [2, 3, 23, 41])
def test_device_vs_host(steps, dtype):
    """4. Salted lattices (NaN, ±0, ±inf): totals, vertices, keys and faces equal the host build's exactly; guard rows
    past V and F untouched.  Steps 23: 48 workgroups of 256 nodes with a ragged last one and runs of rows that cross
    workgroup ends; steps 41: 270 workgroups, more than one count per thread of the scan."""
    rng = np.random.default_rng(31 * steps + (dtype is np.float64))
    mean = salted_inf_mean(rng, steps, dtype)
    axes = point_axes(AXES_LB, AXES_UB, steps)
    (V, F), hv, hk, hf = host_mesh(mean, axes)
    assert V > 0 and F > 0
    (dV, dF), v, keys, faces = device_mesh(mean, axes, V + 3, F + 3, V + 3, F + 3)
    assert (dV, dF) == (V, F)
    assert same_bits(v[:V], hv) and same_bits(keys[:V], hk) and same_bits(faces[:F], hf)
    assert np.all(v[V:] == -7.0) and np.all(keys[V:] == -1) and np.all(faces[F:] == -1)


def test_capacity_cut():
    """5. Vertex and face capacities below the totals, both inside a workgroup's run of rows: the first rows as without
    a cut, the totals in full, guard values past the capacities untouched."""
    steps = 23
    rng = np.random.default_rng(17)
    mean = salted_inf_mean(rng, steps, np.float64)
    axes = point_axes(AXES_LB, AXES_UB, steps)
    (V, F), hv, hk, hf = host_mesh(mean, axes)
    vcap, fcap = 5003, 10007  # several workgroups in, not at a workgroup's first row
    assert V > vcap + 100 and F > fcap + 100
    (dV, dF), v, keys, faces = device_mesh(mean, axes, vcap, fcap, V, F)
    assert (dV, dF) == (V, F)
    assert same_bits(v[:vcap], hv[:vcap]) and same_bits(keys[:vcap], hk[:vcap]) and same_bits(faces[:fcap], hf[:fcap])
    assert np.all(v[vcap:] == -7.0) and np.all(keys[vcap:] == -1) and np.all(faces[fcap:] == -1)


@pytest.mark.parametrize("state", list(FIXTURES))
def test_tomesh_fixtures(mug, state):
    """6. tomesh on the fixture means, as numpy and as tensors (host and device, read unflipped), equals the host
    build; steps < 2 gives empty arrays."""
    d = golden(FIXTURES[state])
    steps = int(d["steps"])
    _, hv, _, hf = host_mesh(d["mean"], point_axes(d["lb"], d["ub"], steps))
    for mean in (d["mean"], torch.from_numpy(d["mean"]), torch.from_numpy(d["mean"]).to(DEV)):
        v, f = mug.tomesh(mean, d["lb"], d["ub"], steps=steps)
        assert v.dtype == np.float64 and f.dtype == np.int32
        assert same_bits(v, hv) and same_bits(f, hf)
    v, f = mug.tomesh(d["mean"][:1, :1, :1], d["lb"], d["ub"], steps=1)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float64 and f.dtype == np.int32


def test_surface_mesh_from_state(mug):
    """7. surface_mesh on the mug state in the field_mug_s9 box at 9 steps: bit for bit tomesh of its own lattice mean;
    normals = compute_normal at the vertices; refine=3 keeps the faces, keeps every vertex between its edge's end
    points, lowers max |pred_mean(vertices)|, and gives the bits of the rule's torch statement (EdgeRefiner with
    pred_mean as the callable: the same IEEE float64 operations, none contracted)."""
    from compliancedex_amd import refine_vertices
    d = golden(FIXTURES["mug"])
    lb, ub, steps = d["lb"], d["ub"], 9
    axes = point_axes(lb, ub, steps)
    grid = torch.from_numpy(np.stack(np.meshgrid(*axes, indexing="xy"), axis=3)).to(DEV)
    lattice = mug.pred_mean(grid)
    v, f, n = mug.surface_mesh(lb, ub, steps=steps)
    assert v.is_cuda and f.is_cuda and n.is_cuda
    assert v.dtype == torch.float64 and f.dtype == torch.int32 and n.dtype == torch.float64
    tv, tf = mug.tomesh(lattice, lb, ub, steps=steps)
    assert len(tv) > 100 and same_bits(v.cpu().numpy(), tv) and same_bits(f.cpu().numpy(), tf)
    assert torch.equal(n, mug.compute_normal(v))
    assert mug.surface_mesh(lb, ub, steps=steps, normals=False)[2] is None

    rv, rf, rn = mug.surface_mesh(lb, ub, steps=steps, refine=3)
    assert torch.equal(rf, f) and rv.shape == v.shape
    assert torch.equal(rn, mug.compute_normal(rv))
    _, _, hk, _ = host_mesh(lattice.cpu().numpy(), axes)
    a, b = key_ends(hk, steps)
    pa = np.stack([axes[0][a[:, 1]], axes[1][a[:, 0]], axes[2][a[:, 2]]], axis=1)
    pb = np.stack([axes[0][b[:, 1]], axes[1][b[:, 0]], axes[2][b[:, 2]]], axis=1)
    want = refine_vertices(mug.pred_mean, torch.from_numpy(hk).to(DEV), lattice,
                           torch.from_numpy(np.stack(axes)).to(DEV), 3)
    assert torch.equal(rv, want)
    r = rv.cpu().numpy()
    assert np.all(r >= np.minimum(pa, pb)) and np.all(r <= np.maximum(pa, pb))
    e0, e3 = float(mug.pred_mean(v).abs().max()), float(mug.pred_mean(rv).abs().max())
    print("max |mean| at the vertices: refine=0", e0, "refine=3", e3, "ratio", e3 / e0)
    assert e3 < e0


def test_mesh_into_the_mesh_half(mug_mesh):
    """8. The closed mesh of the field_mug_s9 mean as float32 face_vertices and a PreparedMesh: compute_sdf's sign at
    all 729 lattice nodes is −1 exactly where mean < 0; occluded hides all 94 inside nodes from each of six eyes at
    centre ± 2·extent along one axis plus (0.013, 0.007, 0.003)·extent; render_depth from one of them has a finite
    depth at the image centre."""
    from compliancedex_amd import (Camera, PreparedMesh, compute_sdf, mesh_face_vertices, occluded, render_depth,
                                   to_triangle_mesh)
    d, (v, f) = mug_mesh
    steps = int(d["steps"])
    fv = mesh_face_vertices(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    assert fv.is_cuda and fv.dtype == torch.float32 and tuple(fv.shape) == (len(f), 3, 3)
    assert to_triangle_mesh(v, f).triangles.shape == f.shape
    mesh = PreparedMesh(fv)
    axes = point_axes(d["lb"], d["ub"], steps)
    nodes = torch.from_numpy(np.stack(np.meshgrid(*axes, indexing="xy"), axis=3).reshape(-1, 3)).to(DEV)
    inside = torch.from_numpy(d["mean"] < 0).reshape(-1).to(DEV)
    assert int(inside.sum()) == 94
    _, sign, _, _ = compute_sdf(nodes.float(), mesh)
    assert torch.equal(sign == -1, inside)
    lb, ub = np.asarray(d["lb"], np.float64), np.asarray(d["ub"], np.float64)
    extent, centre = ub - lb, (lb + ub) / 2
    eyes = []
    for axis in range(3):
        for side in (1.0, -1.0):
            eye = centre + np.array([0.013, 0.007, 0.003]) * extent
            eye[axis] += side * 2 * extent[axis]
            eyes.append(eye)
            assert int(occluded(mesh, eye, nodes[inside]).sum()) == 94
    cam = Camera.look_at(eyes[0], centre, [0.0, 0.0, 1.0], 40.0, 33, 33)
    depth = render_depth(mesh, cam)
    mid = float(depth[16, 16])
    assert np.isfinite(mid) and mid > 0  # (0 is a miss)
