"""Farthest-point sampling on an MI355X (cdx_fps, both paths) against the numpy statement of the rule, bit for bit, and
the entry points on top of it: farthest_point_sample / farthest_point_down_sample / completion_arrays /
GPIS.fit_pointcloud."""
import numpy as np
import pytest
import torch

from tests import _fps
from tests._fps import numpy_fps, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4  # output rows past K, preset and found untouched
BLOCK, ROUNDS = 1, 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


@pytest.fixture(scope="module")
def capacity():
    from compliancedex_amd import _native as N
    return int(N.load().cdx_fps_capacity())


_REF = {}


def reference(name, X, K, start):
    """numpy's result for a named case, computed once for the module."""
    if name not in _REF:
        _REF[name] = numpy_fps(X, K, start)
    return _REF[name]


def device_fps(X, K, start, mode, workspace=None):
    """cdx_fps through the C ABI on a [P, 3] or [B, P, 3] host array uploaded in its own dtype: (sel, radius, points)
    as [B, K, …] numpy arrays; GUARD rows past the end of each output are checked to be untouched."""
    from compliancedex_amd import _native as N
    lib = N.load()
    X = np.ascontiguousarray(X)
    B, P = (X.shape[0], X.shape[1]) if X.ndim == 3 else (1, X.shape[0])
    x = torch.from_numpy(X).to(DEV)
    n = B * K
    sel = torch.full((n + GUARD,), -1, dtype=torch.int64, device=DEV)
    radius = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device=DEV)
    points = torch.full((n + GUARD, 3), -7.0, dtype=torch.float64, device=DEV)
    if workspace is None:
        workspace = torch.empty(lib.cdx_fps_workspace(P, B, mode), dtype=torch.uint8, device=DEV)
    dtype = N.DTYPE_F32 if X.dtype == np.float32 else N.DTYPE_F64
    N.check(lib.cdx_fps(N.ptr(x), dtype, P, B, K, start, mode, N.ptr(workspace), N.ptr(sel), N.ptr(radius),
                        N.ptr(points), N.stream_ptr()), "cdx_fps")
    sel, radius, points = sel.cpu().numpy(), radius.cpu().numpy(), points.cpu().numpy()
    assert np.all(sel[n:] == -1) and np.all(radius[n:] == -7.0) and np.all(points[n:] == -7.0)
    return sel[:n].reshape(B, K), radius[:n].reshape(B, K), points[:n].reshape(B, K, 3)


def check(name, X, K, start, modes):
    rs, rr, rp = reference(name, X, K, start)
    for mode in modes:
        sel, radius, points = device_fps(X, K, start, mode)
        assert np.array_equal(sel[0], rs), (name, mode)
        assert same_bits(radius[0], rr) and same_bits(points[0], rp), (name, mode)


def modes_for(P, capacity):
    return (BLOCK, ROUNDS) if P <= capacity else (ROUNDS,)


def test_shared_cases_both_paths(capacity):
    """The host build's cases — the tiling edges of both paths, K = P, the banana cloud in both dtypes, start = P − 1,
    duplicates, non-finite rows, the small tie lattice — in both modes wherever the one-workgroup path admits P."""
    cases = _fps.shared_cases(capacity)
    assert {f"edge_P{P}" for P in (63, 64, 65, 1023, 1024, 1025, capacity - 1, capacity, capacity + 1)} <= set(cases)
    for name, (X, K, start) in cases.items():
        check(name, X, K, start, modes_for(len(X), capacity))


def test_goldens_on_the_device(capacity):
    X, K, start = _fps.shared_cases(capacity)["duplicates"]
    for mode in (BLOCK, ROUNDS):
        sel, radius, _ = device_fps(X, K, start, mode)
        assert sel[0].tolist() == _fps.DUPLICATES_SEL and radius[0].tolist() == _fps.DUPLICATES_RADIUS
        sel, radius, _ = device_fps(_fps.banana(), 200, 0, mode)
        assert sel[0, :4].tolist() == [0, 534, 1814, 1872] and len(set(sel[0].tolist())) == 200
        sel, radius, _ = device_fps(_fps.salted_cloud(), 40, 64, mode)
        assert radius[0, 0] == -1.0 and not set(sel[0, 1:].tolist()) & set(_fps.NONFINITE_ROWS)


def test_ties_across_workgroups(capacity):
    """The 35 × 35 × 33 lattice: equal maxima in different workgroups, the lowest index must win."""
    X, K, start = _fps.large_cases()["lattice"]
    check("lattice", X, K, start, modes_for(len(X), capacity))
    sel, radius, _ = device_fps(X, K, start, ROUNDS)
    assert sel[0, :4].tolist() == [0, 40424, 1138, 39286]
    assert radius[0, :4].tolist() == [np.inf, 3336.0, 1412.0, 1412.0]


def test_large_and_ragged():
    X, K, start = _fps.large_cases()["ragged_70001"]
    check("ragged_70001", X, K, start, (ROUNDS,))


def test_automatic_mode_equals_both(capacity):
    for P in (2048, capacity + 1):
        X = _fps.normal_cloud(P)
        rs = reference(f"edge_P{P}", X, 5, 0)[0]
        assert np.array_equal(device_fps(X, 5, 0, 0)[0][0], rs)


def test_mode_block_beyond_capacity_is_rejected(capacity):
    from compliancedex_amd import farthest_point_sample
    x = torch.zeros(capacity + 1, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="one workgroup"):
        farthest_point_sample(x, 4, mode="block")


def test_batch_rows_equal_single_cloud_calls(capacity):
    X = np.stack([_fps.normal_cloud(5000, seed=s) for s in (21, 22, 23)])
    X[1] *= 0.01
    X[2, :, 0] += 5.0
    for mode in modes_for(5000, capacity):
        sel, radius, points = device_fps(X, 40, 0, mode)
        for b in range(3):
            s1, r1, p1 = device_fps(X[b], 40, 0, mode)
            assert np.array_equal(sel[b], s1[0]) and same_bits(radius[b], r1[0]) and same_bits(points[b], p1[0])
            assert np.array_equal(sel[b], reference(f"batch{b}", X[b], 40, 0)[0])
    assert len({tuple(s) for s in sel.tolist()}) == 3  # different clouds, different samples


def test_workspace_reuse_without_clearing():
    """The same workspace for two different clouds back to back: the second result equals a fresh-workspace run."""
    from compliancedex_amd import _native as N
    A, Bc = _fps.normal_cloud(9000, seed=31), _fps.normal_cloud(9000, seed=32) * 3.0
    ws = torch.empty(N.load().cdx_fps_workspace(9000, 1, ROUNDS), dtype=torch.uint8, device=DEV)
    first = device_fps(A, 30, 0, ROUNDS, workspace=ws)
    second = device_fps(Bc, 30, 5, ROUNDS, workspace=ws)
    fresh = device_fps(Bc, 30, 5, ROUNDS)
    assert np.array_equal(second[0], fresh[0]) and same_bits(second[1], fresh[1]) and same_bits(second[2], fresh[2])
    assert np.array_equal(first[0][0], reference("reuse_a", A, 30, 0)[0])
    assert np.array_equal(second[0][0], reference("reuse_b", Bc, 30, 5)[0])


def test_python_sampling_entry_points(capacity):
    from compliancedex_amd import farthest_point_down_sample, farthest_point_sample
    X = _fps.banana()
    rs, rr, _ = reference("banana_f64", X, 200, 0)
    x = torch.from_numpy(X).to(DEV)
    for mode in ("auto", "block", "rounds"):
        sel, radius = farthest_point_sample(x, 200, return_radius=True, mode=mode)
        assert sel.dtype == torch.int64 and tuple(sel.shape) == (200,)
        assert np.array_equal(sel.cpu().numpy(), rs) and same_bits(radius.cpu().numpy(), rr)
    assert np.array_equal(farthest_point_sample(x, 50).cpu().numpy(), rs[:50])  # the prefix property
    # float32 in: sampled on the widened values
    x32 = x.float()
    r32 = reference("banana_f32", X.astype(np.float32), 200, 0)[0]
    assert np.array_equal(farthest_point_sample(x32, 200).cpu().numpy(), r32)
    # batched, a non-zero start, a non-contiguous view
    xb = torch.stack([x, x.flip(0)])
    sb = farthest_point_sample(xb, 20, start=2047)
    assert tuple(sb.shape) == (2, 20)
    assert np.array_equal(sb[0].cpu().numpy(), numpy_fps(X, 20, 2047)[0])
    assert np.array_equal(sb[1].cpu().numpy(), numpy_fps(X[::-1], 20, 2047)[0])
    assert np.array_equal(farthest_point_sample(x.flip(0), 20, start=2047).cpu().numpy(), sb[1].cpu().numpy())
    # open3d's contract: the chosen rows ascending by index, in the input dtype
    for t, ref in ((x, rs), (x32, r32)):
        down = farthest_point_down_sample(t, 200)
        assert down.dtype == t.dtype and tuple(down.shape) == (200, 3)
        assert torch.equal(down, t[torch.from_numpy(np.sort(ref)).to(DEV)])
    with pytest.raises(ValueError):
        farthest_point_sample(x, 0)
    with pytest.raises(ValueError):
        farthest_point_sample(x, 2049)
    with pytest.raises(ValueError):
        farthest_point_sample(x, 5, start=2048)


def torch_recipe(surface, bound, n_internal, sharpness, noise, center, weights):
    """optimize_pregrasp.py:905-922 with plain torch operators on the device."""
    b = bound
    ext = torch.tensor([[-b, -b, -b], [b, -b, -b], [-b, b, -b], [b, b, -b], [-b, -b, b], [b, -b, b], [-b, b, b],
                        [b, b, b], [-b, 0., 0.], [0., -b, 0.], [b, 0., 0.], [0., b, 0], [0., 0., b],
                        [0., 0., -b]]).double().to(DEV)
    if center is not None:
        ext = ext + center
    interior = torch.softmax(weights.double() * sharpness, dim=1) @ surface
    y = torch.vstack([b * torch.ones_like(ext[:, 0]).view(-1, 1), torch.zeros_like(surface[:, 0]).view(-1, 1),
                      -b * torch.ones_like(interior[:, 0]).view(-1, 1)])
    nz = torch.tensor([noise[0]] * len(ext) + [noise[1]] * len(surface) + [noise[2]] * len(interior)).double().to(DEV)
    return torch.vstack([ext, surface, interior]), y, nz, interior


def test_completion_arrays_against_plain_torch():
    from compliancedex_amd import completion_arrays
    X = torch.from_numpy(_fps.banana()).to(DEV)
    surface = X[torch.from_numpy(reference("banana_f64", _fps.banana(), 200, 0)[0]).to(DEV)]
    weights = torch.rand(50, 200, generator=torch.Generator().manual_seed(5)).to(DEV)
    center = torch.tensor([0.01, -0.02, 0.03], dtype=torch.float64, device=DEV)
    noise = (0.2, 0.005, 0.1)
    X1, y, nz = completion_arrays(surface, 0.15, 50, 30.0, noise, center=center, weights=weights)
    rX, ry, rn, rint = torch_recipe(surface, 0.15, 50, 30.0, noise, center, weights)
    assert tuple(X1.shape) == (264, 3) and tuple(y.shape) == (264, 1) and tuple(nz.shape) == (264,)
    assert X1.dtype == y.dtype == nz.dtype == torch.float64
    assert torch.equal(X1[:14], rX[:14]) and torch.equal(X1[14:214], surface)
    assert torch.equal(y, ry) and torch.equal(nz, rn)
    assert (y[:14] == 0.15).all() and (y[14:214] == 0).all() and (y[214:] == -0.15).all()
    lv = [float(np.float64(np.float32(v))) for v in noise]
    assert (nz[:14] == lv[0]).all() and (nz[14:214] == lv[1]).all() and (nz[214:] == lv[2]).all()
    err = float(((X1[214:] - rint).abs().max(dim=0).values / rint.abs().max(dim=0).values).max())
    assert err <= 1e-14, err
    # no centre: the exterior points stay at the origin; weights drawn from a generator are reproducible
    a = completion_arrays(surface, 0.1, 5, 10.0, (0.3, 0.005, 0.02), generator=torch.Generator(DEV).manual_seed(3))
    b = completion_arrays(surface, 0.1, 5, 10.0, (0.3, 0.005, 0.02), generator=torch.Generator(DEV).manual_seed(3))
    assert tuple(a[0].shape) == (219, 3) and torch.equal(a[0], b[0])
    assert float(a[0][:14].abs().max()) == float(np.float32(0.1)) != 0.1  # float32 then widened, as the states store
    assert torch.equal(a[0][:14], torch_recipe(surface, 0.1, 5, 10.0, (0.3, 0.005, 0.02), None,
                                               torch.zeros(5, 200, device=DEV))[0][:14])


def test_fit_pointcloud_on_the_banana_cloud():
    from compliancedex_amd import GPIS, completion_arrays
    from compliancedex_amd.pointcloud import bbox_center
    Xn = _fps.banana()
    X = torch.from_numpy(Xn).to(DEV)
    weights = torch.rand(50, 200, generator=torch.Generator().manual_seed(9)).to(DEV)
    g = GPIS(0.08, 1.0)
    assert g.fit_pointcloud(X, weights=weights) is g
    assert np.array_equal(g.sample_index.cpu().numpy(), reference("banana_f64", Xn, 200, 0)[0])
    center = bbox_center(X)
    assert np.array_equal(center.cpu().numpy(), 0.5 * (Xn.min(0) + Xn.max(0)))
    h = GPIS(0.08, 1.0)
    X1, y, nz = completion_arrays(X[g.sample_index], 0.15, 50, 30.0, (0.2, 0.005, 0.1), center=center, weights=weights)
    h.fit(X1, y, noise=nz)
    for name in ("X1", "y1", "R", "E11"):
        assert torch.equal(getattr(g, name), getattr(h, name)), name
    assert tuple(g.X1.shape) == (264, 3) and tuple(g.E11.shape) == (264, 264)
    mean, _ = g.pred(X[g.sample_index])
    assert float(mean.abs().max()) < 0.02  # 4 σ of the 0.005 surface noise; a sanity check, not a parity claim
    # non-finite rows in the cloud: never sampled, and left out of the bounding box
    Y = X.clone()
    Y[5, 0] = float("nan")
    Y[77, 2] = float("inf")
    g2 = GPIS(0.08, 1.0).fit_pointcloud(Y, num_points=64, weights=weights[:, :64])
    idx = g2.sample_index.cpu().numpy()
    assert np.array_equal(idx, numpy_fps(Y.cpu().numpy(), 64, 0)[0]) and not {5, 77} & set(idx.tolist())
    assert bool(torch.isfinite(g2.E11).all())
