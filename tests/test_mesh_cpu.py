"""The marching-tetrahedra rule of GPIS.tomesh without a GPU: the host build (cdxh_mesh_extract, the same header the
kernels compile) against a numpy statement of the rule, the topology the rule promises, and the refinement of the
vertices along their lattice edges on CPU tensors."""
import numpy as np
import pytest
import torch

from tests._field import point_axes
from tests._helpers import golden
from tests._mesh import (SPHERE_AXES, edge_counts, euler, host_mesh, host_refine, key_ends, numpy_mesh, same_bits,
                         salted_inf_mean, signed_volume, sphere_field)

AXES_LB, AXES_UB = [-1.0, 0.5, 2.0], [1.0, 3.5, 2.5]


def check_host_equals_numpy(mean, axes):
    v, keys, faces = numpy_mesh(mean, axes)
    (V, F), hv, hk, hf = host_mesh(mean, axes)
    assert (V, F) == (len(v), len(faces))
    assert same_bits(hv, v) and same_bits(hk, keys) and same_bits(hf, faces)
    return V, F


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("steps", [1, 2, 3, 7])
def test_host_vs_numpy_salted(steps, dtype):
    """1. Lattices with NaN, ±0 and ±inf nodes: identical vertex bits, edge keys and faces."""
    rng = np.random.default_rng(100 * steps + (dtype is np.float64))
    mean = salted_inf_mean(rng, steps, dtype)
    V, F = check_host_equals_numpy(mean, point_axes(AXES_LB, AXES_UB, steps))
    if steps == 1:
        assert (V, F) == (0, 0)
    else:
        assert V > 0 and F > 0


def test_host_vs_numpy_sphere():
    """1. The analytic sphere at steps 12, and the numpy statement's own counts against the rule's prototype."""
    assert check_host_equals_numpy(sphere_field(SPHERE_AXES), SPHERE_AXES) == (786, 1568)


def test_host_vs_numpy_descending_axis():
    """1. A descending y axis (a reflection: every winding flips) on a salted lattice and on the sphere, which keeps
    its outward normals."""
    rng = np.random.default_rng(5)
    axes = [np.linspace(-1, 1, 7), np.linspace(3.5, 0.5, 7), np.linspace(2, 2.5, 7)]
    check_host_equals_numpy(salted_inf_mean(rng, 7, np.float64), axes)
    axes = (SPHERE_AXES[0], SPHERE_AXES[1][::-1].copy(), SPHERE_AXES[2])
    mean = sphere_field(axes)
    check_host_equals_numpy(mean, axes)
    _, v, _, f = host_mesh(mean, axes)
    assert signed_volume(v, f) > 0


def test_topology_salted_closed_border():
    """2. A salted lattice at steps 7 whose border nodes are +1 (the surface cannot reach the border): every undirected
    edge in exactly 2 faces, every directed edge once, every vertex referenced, all vertices finite."""
    rng = np.random.default_rng(21)
    mean = salted_inf_mean(rng, 7, np.float64)
    border = np.ones_like(mean, bool)
    border[1:-1, 1:-1, 1:-1] = False
    mean[border] = 1.0
    (V, F), v, _, f = host_mesh(mean, point_axes(AXES_LB, AXES_UB, 7))
    assert V > 100 and F > 100
    _, dc, _, uc = edge_counts(f)
    assert np.all(uc == 2) and np.all(dc == 1)
    assert np.array_equal(np.unique(f), np.arange(V))
    assert np.isfinite(v).all()


def test_topology_sphere():
    """2. The sphere: V − E + F = 2, every face normal points away from the centre, positive signed volume."""
    (V, F), v, _, f = host_mesh(sphere_field(SPHERE_AXES), SPHERE_AXES)
    assert (V, F) == (786, 1568)
    assert euler(V, f) == 2
    tri = v[f.astype(np.int64)]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert np.all(np.einsum("ij,ij->i", normal, tri.mean(axis=1)) > 0)
    assert signed_volume(v, f) > 0


def fixture_mesh(name):
    d = golden(name)
    steps = int(d["steps"])
    axes = point_axes(d["lb"], d["ub"], steps)
    check_host_equals_numpy(d["mean"], axes)
    return steps, host_mesh(d["mean"], axes)


def test_topology_mug_fixture():
    """2. field_mug_s9's mean: a closed surface of one piece."""
    _, ((V, F), v, _, f) = fixture_mesh("field_mug_s9.npz")
    assert (V, F) == (470, 936)
    _, dc, _, uc = edge_counts(f)
    assert np.all(uc == 2) and np.all(dc == 1)
    assert euler(V, f) == 2


def test_topology_banana_fixture_open_at_border():
    """2. field_banana_s13's mean has an inside node on the lattice's border: the surface is open there and nowhere
    else — every edge with a single face joins two vertices on one border face of the lattice."""
    steps, ((V, F), v, keys, f) = fixture_mesh("field_banana_s13.npz")
    assert (V, F) == (556, 1070)
    _, dc, u, uc = edge_counts(f)
    assert np.all(dc == 1) and np.all(uc <= 2)
    open_edges = u[uc == 1]
    assert len(open_edges) > 0
    a, b = key_ends(keys, steps)
    for lo, hi in open_edges:
        shared = False
        for ax in range(3):
            for side in (0, steps - 1):
                on = [a[x][ax] == side and b[x][ax] == side for x in (lo, hi)]
                shared |= all(on)
        assert shared, (lo, hi)


def test_refinement_on_cpu_tensors():
    """3. EdgeRefiner with the analytic sphere field as the callable, on CPU tensors: after each of 4 steps every vertex
    is inside the previous bracket (so on its edge), the bracket ends keep opposite `inside`, faces are what they
    were, and max |f(vertex)| after 4 steps is below its value before the first."""
    from compliancedex_amd.mesh import EdgeRefiner, refine_vertices
    axes = np.stack(SPHERE_AXES)
    mean = sphere_field(SPHERE_AXES)
    _, v, keys, faces = host_mesh(mean, SPHERE_AXES)
    faces0 = faces.copy()

    def field(X):
        return X.norm(dim=1) - 0.7

    r = EdgeRefiner(torch.from_numpy(keys), torch.from_numpy(mean), torch.from_numpy(axes))
    assert same_bits(r.vertices().numpy(), v)  # step 0 is the rule's own vertex
    err0 = float(field(r.vertices()).abs().max())
    for _ in range(4):
        ta, tb = r.ta.clone(), r.tb.clone()
        r.step(field)
        assert bool(((r.t >= ta) & (r.t <= tb)).all())
        assert bool(((r.ta >= 0) & (r.tb <= 1) & (r.ta <= r.tb)).all())
        assert bool(((r.fa < 0) != (r.fb < 0)).all())
    err4 = float(field(r.vertices()).abs().max())
    print("sphere refinement max |f|:", err0, "->", err4)
    assert err4 < err0
    assert np.array_equal(faces, faces0)
    out = refine_vertices(field, torch.from_numpy(keys), torch.from_numpy(mean), torch.from_numpy(axes), 4)
    assert torch.equal(out, r.vertices())
    # a non-finite value leaves its vertex alone
    r2 = EdgeRefiner(torch.from_numpy(keys), torch.from_numpy(mean), torch.from_numpy(axes))
    before = r2.t.clone()
    r2.step(lambda X: torch.where(torch.arange(len(X)) % 2 == 0, torch.full((len(X),), float("nan"), dtype=X.dtype),
                                  field(X)))
    assert torch.equal(r2.t[::2], before[::2]) and not torch.equal(r2.t[1::2], before[1::2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refinement_host_build_equals_torch_statement(dtype):
    """3. The refinement rule the kernel compiles (cdxh_mesh_refine) against EdgeRefiner on CPU tensors, bit for bit:
    both are the same IEEE float64 operations without contraction.  The sphere's lattice, and a salted lattice with a
    field that returns NaN and ±inf for some vertices."""
    from compliancedex_amd.mesh import EdgeRefiner
    rng = np.random.default_rng(9)
    cases = [(sphere_field(SPHERE_AXES).astype(dtype), SPHERE_AXES, lambda X: X.norm(dim=1) - 0.7)]
    axes = point_axes(AXES_LB, AXES_UB, 7)
    noise = torch.from_numpy(salted_inf_mean(rng, 20, np.float64).reshape(-1))
    cases.append((salted_inf_mean(rng, 7, dtype), axes, lambda X: noise[:len(X)] * 0.1 + torch.sin(40 * X.sum(dim=1))))
    for mean, ax, field in cases:
        _, v, keys, _ = host_mesh(mean, ax)
        r = EdgeRefiner(torch.from_numpy(keys), torch.from_numpy(mean), torch.from_numpy(np.stack(ax)))
        state, hv = host_refine(mean, None, ax, keys)
        assert same_bits(hv, v) and same_bits(hv, r.vertices().numpy())
        for _ in range(4):
            fv = field(torch.from_numpy(hv))
            r.step(lambda X: fv)
            state, hv = host_refine(mean, fv.numpy(), ax, keys, state)
            want = torch.stack([r.ta, r.fa, r.tb, r.fb, r.t]).numpy()
            assert same_bits(state, want) and same_bits(hv, r.vertices().numpy())
    bad = np.array([-1, 7 * 7 ** 3, 7 * (7 ** 3 - 1) + 6], np.int64)  # no edges of a 7³ lattice
    assert np.isnan(host_refine(mean, None, axes, bad)[1]).all()


def test_conveniences():
    """face_vertices and TriangleMesh of a mesh."""
    from compliancedex_amd import TriangleMesh, mesh_face_vertices, to_triangle_mesh
    _, v, _, f = host_mesh(sphere_field(SPHERE_AXES), SPHERE_AXES)
    fv = mesh_face_vertices(v, f)
    assert fv.dtype == torch.float32 and tuple(fv.shape) == (len(f), 3, 3)
    assert np.array_equal(fv.numpy(), v.astype(np.float32)[f.astype(np.int64)])
    m = to_triangle_mesh(torch.from_numpy(v), torch.from_numpy(f))
    assert isinstance(m, TriangleMesh) and m.vertices.shape == v.shape and m.triangles.dtype == np.int64
    assert np.array_equal(m.triangles, f)
