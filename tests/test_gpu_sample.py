"""Area-weighted surface sampling on an MI355X (cdx_sample_prepare / cdx_sample_draw, both draw paths) against the
numpy statement of the rule, bit for bit, and the entry points on top of it: SurfaceSampler / sample_points_uniformly /
sample_points_poisson_disk / TriangleMesh.sample_points_* / GPIS.fit_mesh."""
import itertools

import numpy as np
import pytest
import torch

from tests import _sample as S
from tests._sample import numpy_draw, numpy_prepare, same_bits, same_draw

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4  # output rows past K, preset and found untouched
AUTO, TABLE, SPLIT = 0, 1, 2
ALL = (True, True, True, True)  # points, face, bary, normal


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


@pytest.fixture(scope="module")
def table_cap():
    from compliancedex_amd import _native as N
    return int(N.load().cdx_sample_table_capacity())


@pytest.fixture(scope="module")
def scan_faces():
    from compliancedex_amd import _native as N
    return int(N.load().cdx_sample_scan_faces())


_CDF = {}


def reference_cdf(name, faces):
    """numpy's (C, info) for a named mesh, computed once for the module."""
    if name not in _CDF:
        _CDF[name] = numpy_prepare(faces)
    return _CDF[name]


_DRAW = {}


def reference_draw(name, faces, seed, first, K):
    """numpy's draw of a named mesh; one per (mesh, seed, first), grown to the largest K asked for (the first k of a
    K-sample are the k-sample: tests/test_sample_cpu.py)."""
    key = (name, seed, first)
    if key not in _DRAW or len(_DRAW[key][1]) < K:
        _DRAW[key] = numpy_draw(faces, reference_cdf(name, faces)[0], seed, first, K)
    return tuple(x[:K] for x in _DRAW[key])


def dtype_of(faces):
    from compliancedex_amd import _native as N
    return N.DTYPE_F32 if faces.dtype in (np.float32, torch.float32) else N.DTYPE_F64


def device_prepare(faces):
    """cdx_sample_prepare through the C ABI on a host array uploaded in its own dtype: (faces tensor, C tensor (int64
    holding the uint64 bits), C as numpy uint64, info)."""
    from compliancedex_amd import _native as N
    lib = N.load()
    f = torch.from_numpy(np.ascontiguousarray(faces)).to(DEV)
    F = len(faces)
    ws = torch.empty(lib.cdx_sample_prepare_workspace(F), dtype=torch.uint8, device=DEV)
    cdf = torch.full((F + GUARD,), -5, dtype=torch.int64, device=DEV)
    info = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    N.check(lib.cdx_sample_prepare(N.ptr(f), dtype_of(faces), F, N.ptr(ws), N.ptr(cdf), N.ptr(info), N.stream_ptr()),
            "cdx_sample_prepare")
    host = cdf.cpu().numpy()
    assert np.all(host[F:] == -5)
    return f, cdf[:F].contiguous(), host[:F].view(np.uint64), int(info.item())


def device_draw(f, cdf, seed, first, K, mode, want=ALL):
    """cdx_sample_draw through the C ABI: (points, face, bary, normal) as numpy arrays, None where ``want`` is False;
    GUARD rows past the end of each output are checked to be untouched."""
    from compliancedex_amd import _native as N
    shapes = ((K + GUARD, 3), (K + GUARD,), (K + GUARD, 2), (K + GUARD, 3))
    outs = [None if not w else
            (torch.full(s, -9, dtype=torch.int64, device=DEV) if len(s) == 1 else
             torch.full(s, -7.0, dtype=torch.float64, device=DEV)) for w, s in zip(want, shapes)]
    N.check(N.load().cdx_sample_draw(N.ptr(f), dtype_of(f), f.shape[0], N.ptr(cdf), seed, first, K, mode,
                                     *[N.ptr(o) for o in outs], N.stream_ptr()), "cdx_sample_draw")
    res = []
    for o in outs:
        if o is None:
            res.append(None)
            continue
        h = o.cpu().numpy()
        assert np.all(h[K:] == (-9 if h.dtype == np.int64 else -7.0))
        res.append(h[:K])
    return tuple(res)


def modes_for(F, table_cap):
    return (TABLE, SPLIT) if F <= table_cap else (SPLIT,)


def test_cdf_against_numpy(scan_faces, table_cap):
    """C [F] and info in both dtypes at the seams of the scan: the wave, the workgroup, its faces, the table path's
    capacity, more workgroups than the offsets kernel has threads, and a ragged size."""
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, scan_faces - 1, scan_faces, scan_faces + 1, table_cap - 1, table_cap,
             table_cap + 1, 70001, 256 * scan_faces + 7]
    for F in sizes:
        for dt in (np.float64, np.float32):
            faces = S.random_faces(F, dtype=dt)
            ref, rinfo = reference_cdf(f"random_F{F}_{np.dtype(dt).name}", faces)
            _, _, cdf, info = device_prepare(faces)
            assert info == rinfo == 0 and same_bits(cdf, ref), (F, dt)
    for name in ("banana", "cube", "sphere42"):
        faces = S.mesh(name)
        assert same_bits(device_prepare(faces)[2], reference_cdf(name, faces)[0]), name


def test_workspace_reuse_without_clearing():
    """Prepare writes every word it reads: a workspace that held another mesh's sums gives the same table."""
    from compliancedex_amd import _native as N
    lib = N.load()
    a, b = S.random_faces(5000, seed=41) * 100.0, S.random_faces(3000, seed=42)
    ws = torch.empty(lib.cdx_sample_prepare_workspace(5000), dtype=torch.uint8, device=DEV)
    for faces in (a, b):
        f = torch.from_numpy(faces).to(DEV)
        cdf = torch.empty(len(faces), dtype=torch.int64, device=DEV)
        info = torch.empty(1, dtype=torch.int32, device=DEV)
        N.check(lib.cdx_sample_prepare(N.ptr(f), N.DTYPE_F64, len(faces), N.ptr(ws), N.ptr(cdf), N.ptr(info),
                                       N.stream_ptr()), "cdx_sample_prepare")
        assert same_bits(cdf.cpu().numpy().view(np.uint64), numpy_prepare(faces)[0])


def test_draw_against_numpy_every_k_first_and_seed(table_cap):
    """One mesh whose splitter path ends in global memory (5000 faces: runs of 4), both paths, the whole grid of
    K × first × seed."""
    faces = S.random_faces(5000)
    f, cdf, _, _ = device_prepare(faces)
    for seed, first in itertools.product((0, 1, 0xDEADBEEF12345678), (0, 7, 2 ** 32 - 3, 2 ** 40)):
        for K in (1, 63, 64, 65, 255, 256, 257, 5000):
            ref = reference_draw("random_F5000", faces, seed, first, K)
            for mode in (TABLE, SPLIT, AUTO):
                assert same_draw(device_draw(f, cdf, seed, first, K, mode), ref), (seed, first, K, mode)


def test_draw_against_numpy_across_mesh_sizes(table_cap):
    """Both dtypes, from one face to beyond the table path's capacity; K spans several tiles of either path."""
    sizes = (1, 2, 257, 2048, 2049, table_cap - 1, table_cap, table_cap + 1, 70001)
    for F, dt in itertools.product(sizes, (np.float64, np.float32)):
        name = f"random_F{F}_{np.dtype(dt).name}"
        faces = S.random_faces(F, dtype=dt)
        f, cdf, _, _ = device_prepare(faces)
        for seed, first, K in ((0, 0, 3000), (0xDEADBEEF12345678, 2 ** 40, 257)):
            ref = reference_draw(name, faces, seed, first, K)
            for mode in modes_for(F, table_cap):
                assert same_draw(device_draw(f, cdf, seed, first, K, mode), ref), (F, dt, seed, mode)
    f, cdf, _, _ = device_prepare(S.random_faces(table_cap + 1))
    from compliancedex_amd import _native as N
    assert N.load().cdx_sample_draw(N.ptr(f), N.DTYPE_F64, table_cap + 1, N.ptr(cdf), 0, 0, 4, TABLE,
                                    None, None, None, None, None) == -1


def test_every_combination_of_null_outputs(table_cap):
    faces = S.random_faces(5000)
    f, cdf, _, _ = device_prepare(faces)
    ref = reference_draw("random_F5000", faces, 1, 7, 257)
    for want in itertools.product((False, True), repeat=4):
        for mode in (TABLE, SPLIT):
            got = device_draw(f, cdf, 1, 7, 257, mode, want)
            for g, r, w in zip(got, ref, want):
                assert (g is None) if not w else same_bits(g, r), (want, mode)


def test_two_hundred_thousand_samples_on_the_banana(table_cap):
    """The packaged banana has exactly the table path's capacity of faces; every workgroup strides over many tiles."""
    faces = S.mesh("banana")
    assert len(faces) == table_cap
    f, cdf, _, _ = device_prepare(faces)
    ref = reference_draw("banana", faces, 0, 0, 200_000)
    for mode in (TABLE, SPLIT):
        assert same_draw(device_draw(f, cdf, 0, 0, 200_000, mode), ref), mode
    w = S.weights_of(reference_cdf("banana", faces)[0])
    z = S.binomial_z(np.bincount(ref[1], minlength=len(w)).reshape(16, -1).sum(1),
                     w.reshape(16, -1).sum(1, dtype=np.uint64), 200_000)
    assert z.max() <= 5.0


def test_faces_the_rule_never_draws():
    for name, faces, dead in (("salted", S.salted_faces(), S.DEAD_ROWS), ("tiny", S.tiny_beside_unit(), (0, 2))):
        f, cdf, hcdf, info = device_prepare(faces)
        assert info == 0 and same_bits(hcdf, reference_cdf(name, faces)[0])
        assert not S.weights_of(hcdf)[list(dead)].any()
        for mode in (TABLE, SPLIT):
            got = device_draw(f, cdf, 0, 0, 20000, mode)
            assert same_draw(got, reference_draw(name, faces, 0, 0, 20000))
            assert not set(got[1].tolist()) & set(dead) and np.isfinite(got[0]).all()


def test_a_mesh_with_no_area():
    for faces in (S.all_degenerate(), S.all_degenerate(1), S.all_degenerate(3000).astype(np.float32)):
        f, cdf, hcdf, info = device_prepare(faces)
        assert info == 1 and not hcdf.any()
        for mode in (TABLE, SPLIT):
            points, face, bary, normal = device_draw(f, cdf, 4, 11, 300, mode)
            assert np.all(face == -1)
            assert np.isnan(points).all() and np.isnan(bary).all() and np.isnan(normal).all()
    from compliancedex_amd import SurfaceSampler
    with pytest.raises(ValueError, match="no face"):
        SurfaceSampler(torch.from_numpy(S.all_degenerate()).to(DEV))


def test_bad_arguments_are_rejected_through_the_abi(table_cap):
    from compliancedex_amd import _native as N
    lib = N.load()
    faces = S.mesh("cube")
    f, cdf, _, _ = device_prepare(faces)
    F, big = len(faces), 0x7fffffff // 9 + 1
    ws = torch.empty(lib.cdx_sample_prepare_workspace(F), dtype=torch.uint8, device=DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((8, 3), -7.0, dtype=torch.float64, device=DEV)
    s = N.stream_ptr()
    assert lib.cdx_sample_prepare_workspace(0) == 0 and lib.cdx_sample_prepare_workspace(big) == 0
    assert lib.cdx_sample_prepare_workspace(big - 1) > 0
    good = (N.ptr(f), N.DTYPE_F32, F, N.ptr(ws), N.ptr(cdf), N.ptr(info), s)
    for i, bad in ((0, None), (1, 2), (1, -1), (2, 0), (2, -4), (2, big), (3, None), (4, None), (5, None)):
        args = list(good)
        args[i] = bad
        assert lib.cdx_sample_prepare(*args) == -1, (i, bad)
    good = (N.ptr(f), N.DTYPE_F32, F, N.ptr(cdf), 0, 0, 8, AUTO, N.ptr(out), None, None, None, s)
    for i, bad in ((0, None), (1, 2), (2, 0), (2, big), (3, None), (6, -1), (7, 3), (7, -1)):
        args = list(good)
        args[i] = bad
        assert lib.cdx_sample_draw(*args) == -1, (i, bad)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing was launched
    args = list(good)
    args[6] = 0
    assert lib.cdx_sample_draw(*args) == 0  # K = 0: a no-op
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_draws_lie_on_the_mesh():
    """compute_sdf of the draws, rounded to float32, against the mesh: float32 rounding moves a coordinate by at most
    6e-8 of its size, the bound is 1e-6 of the bounding box's diagonal."""
    from compliancedex_amd import PreparedMesh, compute_sdf, sample_points_uniformly
    faces = torch.from_numpy(S.mesh("banana")).to(DEV)
    mesh = PreparedMesh(faces)
    points = sample_points_uniformly(mesh, 20000, seed=2)
    assert same_bits(points.cpu().numpy(), reference_draw("banana", S.mesh("banana"), 2, 0, 20000)[0])
    corners = faces.reshape(-1, 3).double()
    diagonal = float((corners.max(0).values - corners.min(0).values).norm())
    sq = compute_sdf(points.float(), mesh)[0]
    worst = float(sq.double().sqrt().max())
    print("largest distance to the mesh", worst, "bound", 1e-6 * diagonal)
    assert worst < 1e-6 * diagonal


def test_python_entry_points(table_cap):
    from compliancedex_amd import (PreparedMesh, SurfaceSampler, TriangleMesh, sample_points_uniformly,
                                   surface_sampler)
    faces = S.mesh("banana")
    ref = reference_draw("banana", faces, 3, 0, 1000)
    t = torch.from_numpy(faces).to(DEV)
    sampler = SurfaceSampler(t)
    t.zero_()  # the handle owns its copy
    assert sampler.num_faces == len(faces)
    for mode in ("auto", "table", "splitters"):
        points, face, normal, bary = sampler.draw(1000, seed=3, want_face=True, want_normal=True, want_bary=True,
                                                  mode=mode)
        assert points.dtype == normal.dtype == bary.dtype == torch.float64 and face.dtype == torch.int64
        assert same_draw([x.cpu().numpy() for x in (points, face, bary, normal)], ref)
    only = sampler.draw(100, seed=3)
    assert torch.is_tensor(only) and tuple(only.shape) == (100, 3) and same_bits(only.cpu().numpy(), ref[0][:100])
    shard = sampler.draw(400, seed=3, first=600, want_face=True)
    assert len(shard) == 2 and np.array_equal(shard[1].cpu().numpy(), ref[1][600:])
    assert tuple(sampler.draw(0).shape) == (0, 3)
    big = SurfaceSampler(torch.from_numpy(S.random_faces(table_cap + 1)).to(DEV))
    with pytest.raises(ValueError, match="table"):
        big.draw(4, mode="table")
    with pytest.raises(ValueError):
        sampler.draw(-1)
    with pytest.raises(ValueError):
        sampler.draw(1, seed=2 ** 64)
    with pytest.raises(ValueError):
        SurfaceSampler(torch.zeros(0, 3, 3, device=DEV))
    # a PreparedMesh keeps its sampler; a TriangleMesh samples its float64 vertices
    prepared = PreparedMesh(torch.from_numpy(faces).to(DEV))
    assert surface_sampler(prepared) is surface_sampler(prepared)
    assert same_bits(sample_points_uniformly(prepared, 1000, seed=3).cpu().numpy(), ref[0])
    d = np.load(S.MESHES + "/banana_mesh.npz")
    tm = TriangleMesh(d["vertices"], d["triangles"])
    fv = d["vertices"][d["triangles"].reshape(-1)].reshape(-1, 3, 3)
    cdf64, _ = numpy_prepare(fv)
    got = tm.sample_points_uniformly(500, seed=8)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (500, 3)
    assert same_bits(got.cpu().numpy(), numpy_draw(fv, cdf64, 8, 0, 500)[0])
    assert same_bits(tm.sample_points_poisson_disk(64, seed=8).cpu().numpy(), S.numpy_poisson(fv, 64, 5, 8)[0])


def test_poisson_disk_equals_the_host_composition():
    from compliancedex_amd import sample_points_poisson_disk
    from tests._fps import host_fps
    K = 256
    faces = S.mesh("banana")
    rc, cdf, _ = S.host_prepare(faces)
    _, hp, hf, _, hn = S.host_draw(faces, cdf, 0, 0, 5 * K)
    rc, sel, _, chosen = host_fps(hp, K, 0)
    assert rc == 0
    points, face, normal = sample_points_poisson_disk(torch.from_numpy(faces).to(DEV), K, want_face=True,
                                                      want_normal=True)
    assert same_bits(points.cpu().numpy(), chosen) and np.array_equal(face.cpu().numpy(), hf[sel])
    assert same_bits(normal.cpu().numpy(), hn[sel])
    assert len(np.unique(chosen, axis=0)) == K
    # another seed and another init_factor give other clouds; every prefix of a cloud is the smaller cloud
    t = torch.from_numpy(faces).to(DEV)
    assert torch.equal(sample_points_poisson_disk(t, 100, init_factor=3, seed=4),
                       torch.from_numpy(S.numpy_poisson(faces, 100, 3, 4)[0]).to(DEV))


def test_fit_mesh_on_the_banana():
    """GPIS.fit_mesh against the manual route, and the fitted field's signs.  Checked on the CPU with the numpy
    statement's draw and FPS rounds feeding the reference's own gpis.py fit and pred for this recipe: the smallest
    exterior mean 0.035, the largest interior mean −0.0012, the largest |mean| at the fresh samples 0.0016 — with the
    weights of torch.Generator().manual_seed(0), which this test therefore uses.  The interior points are soft-max
    mixtures of surface points and some land within the surface noise of the surface: with other weights (seed 9,
    say) the reference's own fit has +0.0003 at one of them, so the interior sign is a property of these weights."""
    from compliancedex_amd import GPIS, SurfaceSampler, sample_points_poisson_disk
    faces = torch.from_numpy(S.mesh("banana")).to(DEV)
    weights = torch.rand(50, 200, generator=torch.Generator().manual_seed(0)).to(DEV)
    sampler = SurfaceSampler(faces)
    g = GPIS(0.08, 1.0)
    assert g.fit_mesh(sampler, weights=weights) is g
    cloud = sample_points_poisson_disk(sampler, 4096, init_factor=5, seed=0)
    assert tuple(g.sample_cloud.shape) == (4096, 3) and torch.equal(g.sample_cloud, cloud)
    h = GPIS(0.08, 1.0).fit_pointcloud(cloud, weights=weights)
    assert torch.equal(g.E11, h.E11) and torch.equal(g.X1, h.X1) and torch.equal(g.sample_index, h.sample_index)
    assert tuple(g.X1.shape) == (264, 3)
    bound = 0.15
    exterior, _ = g.pred(g.X1[:14])
    interior, _ = g.pred(g.X1[214:])
    fresh, _ = g.pred(sampler.draw(1000, seed=1))
    print("exterior min", float(exterior.min()), "interior max", float(interior.max()), "fresh max |mean|",
          float(fresh.abs().max()))
    assert float(exterior.min()) > 0 and float(interior.max()) < 0
    assert float(fresh.abs().max()) < bound / 10
