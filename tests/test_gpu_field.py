"""GPIS lattice field and surface extraction on an MI355X: GPIS.field / get_visualization_data(fused=True) / topcd /
surface against the reference's fixtures (tests/golden/field_*.npz), against direct pred_mean / compute_normal calls,
and the compaction kernels against their host build (cdxh_surface_extract)."""
import numpy as np
import pytest
import torch

from tests._field import F32, F64, host_extract, point_axes, salted_mean
from tests._helpers import golden, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIXTURES = {"banana": "field_banana_s13.npz", "mug": "field_mug_s9.npz"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


@pytest.fixture(scope="module")
def gpis():
    """The stored states, built once for the module."""
    from compliancedex_amd.workloads import stored_gpis
    return {s: stored_gpis(s, DEV) for s in FIXTURES}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def device_extract(mean, normal, steps, flip, axes, capacity, rows):
    """cdx_gpis_surface_count + _place on host arrays uploaded in their own dtype: (total, cells, points, normals)
    with `rows` ≥ capacity rows preset to guard values."""
    from compliancedex_amd import _native as N
    lib = N.load()
    dtype = F32 if mean.dtype == np.float32 else F64
    m = torch.from_numpy(np.ascontiguousarray(mean)).to(DEV)
    nr = torch.from_numpy(np.ascontiguousarray(normal)).to(DEV)
    ax = torch.from_numpy(np.stack(axes)).to(DEV)
    ws = torch.empty(lib.cdx_gpis_surface_workspace(steps), dtype=torch.uint8, device=DEV)
    total = torch.full((1,), -5, dtype=torch.int64, device=DEV)
    cells = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    pts = torch.full((rows, 3), -7.0, dtype=torch.float64, device=DEV)
    nrm = torch.full((rows, 3), -7.0, dtype=m.dtype, device=DEV)
    s = N.stream_ptr()
    N.check(lib.cdx_gpis_surface_count(N.ptr(m), dtype, steps, flip, N.ptr(ws), N.ptr(total), s), "count")
    N.check(lib.cdx_gpis_surface_place(N.ptr(m), N.ptr(nr), dtype, steps, flip, N.ptr(ax[0]), N.ptr(ax[1]), N.ptr(ax[2]),
                                       N.ptr(ws), capacity, N.ptr(cells), N.ptr(pts), N.ptr(nrm), s), "place")
    return int(total.item()), cells.cpu().numpy(), pts.cpu().numpy(), nrm.cpu().numpy()


@pytest.mark.parametrize("state", list(FIXTURES))
def test_field_vs_reference(gpis, state):
    """1. field, cast to float32, against the reference's get_visualization_data: test_gpis_pred_normal_vs_reference's
    bounds for stored states (1e-8 mean / normal, 1e-6 std) widened by one float32 rounding (1e-7 mean / normal)."""
    d = golden(FIXTURES[state])
    steps = int(d["steps"])
    mean, std, normal = gpis[state].field(d["lb"], d["ub"], steps)
    assert mean.dtype == torch.float64 and tuple(mean.shape) == (steps,) * 3 and tuple(normal.shape) == (steps,) * 3 + (3,)
    errs = (rel_err(mean.float().cpu(), d["mean"]), rel_err(std.float().cpu(), d["std"]),
            rel_err(normal.float().cpu(), d["normal"]))
    print("field vs reference", state, errs)
    assert errs[0] < 1e-7 and errs[1] < 1e-6 and errs[2] < 1e-7


def test_field_bit_identity_and_chunking(gpis):
    """2. field's mean and normal are bit-identical to direct pred_mean / compute_normal calls at the same points, and
    between one chunk, ragged chunks of 1000 and chunks of 128 (a query is summed by its own lanes in a fixed order);
    std within 1e-9 (test_gpis_large_batch_vs_oracle_chunk's bound for batch independence)."""
    g = gpis["banana"]
    d = golden(FIXTURES["banana"])
    lb, ub, steps = d["lb"], d["ub"], 13
    grid = torch.stack(torch.meshgrid(torch.linspace(lb[0], ub[0], steps), torch.linspace(lb[1], ub[1], steps),
                                      torch.linspace(lb[2], ub[2], steps), indexing="xy"), dim=3).double().to(DEV)
    m0, s0, n0 = g.field(lb, ub, steps)
    assert torch.equal(m0, g.pred_mean(grid))
    assert torch.equal(n0, g.compute_normal(grid))
    for chunk in (1000, 128):
        m, s, n = g.field(lb, ub, steps, chunk=chunk)
        assert torch.equal(m, m0) and torch.equal(n, n0), chunk
        e = rel_err(s.cpu(), s0.cpu())
        print("std across chunkings", chunk, e)
        assert e < 1e-9
    only_mean = g.field(lb, ub, steps, std=False, normal=False)
    assert only_mean[1] is None and only_mean[2] is None and torch.equal(only_mean[0], m0)


def test_fused_visualization_equals_eager(gpis):
    """3. get_visualization_data(fused=True) against the per-slice path at steps 13: mean and normal array-equal after
    the float32 cast, std within 1e-6."""
    g = gpis["banana"]
    d = golden(FIXTURES["banana"])
    lb, ub = d["lb"].tolist(), d["ub"].tolist()
    e = g.get_visualization_data(lb, ub, steps=13)
    f = g.get_visualization_data(lb, ub, steps=13, fused=True)
    assert len(f) == 5
    for a, b in zip(e, f):
        assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(e[0], f[0]) and np.array_equal(e[2], f[2])
    assert rel_err(f[1], e[1]) < 1e-6
    assert np.array_equal(e[3], f[3]) and np.array_equal(e[4], f[4])


@pytest.mark.parametrize("state", list(FIXTURES))
def test_topcd_vs_reference(gpis, state):
    """4. topcd on the fixture's own field equals the reference's topcd exactly: numpy inputs, and tensor inputs
    (read flipped along k)."""
    d = golden(FIXTURES[state])
    steps = int(d["steps"])
    g = gpis[state]
    pts, nrm = g.topcd(d["mean"], d["normal"], d["lb"], d["ub"], steps=steps)
    assert same_bits(pts, d["pts_np"]) and same_bits(nrm, d["nrm_np"])
    for dev in ("cpu", DEV):
        pts, nrm = g.topcd(torch.from_numpy(d["mean"]).to(dev), torch.from_numpy(d["normal"]).to(dev), d["lb"], d["ub"],
                           steps=steps)
        assert same_bits(pts, d["pts_t"]) and same_bits(nrm, d["nrm_t"])
    p2, n2 = g.topcd(d["mean"][:2, :2, :2], d["normal"][:2, :2, :2], d["lb"], d["ub"], steps=2)
    assert p2.shape == (0, 3) and n2.shape == (0, 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("flip", [0, 1])
def test_compaction_many_workgroups_vs_host(dtype, flip):
    """5. A random mean at steps 33 (35 937 cells, 141 workgroups) with NaN and ±0 cells: count, order, cells, points
    and normals equal the host build's exactly."""
    steps = 33
    rng = np.random.default_rng(7 + flip)
    mean = salted_mean(rng, steps, dtype)
    normal = rng.standard_normal((steps, steps, steps, 3)).astype(dtype)
    axes = point_axes([-1.0, 0.5, 2.0], [1.0, 3.5, 2.5], steps)
    n, hc, hp, hn = host_extract(mean, normal, steps, flip, axes)
    assert n > 5000
    total, cells, pts, nrm = device_extract(mean, normal, steps, flip, axes, capacity=n + 3, rows=n + 3)
    assert total == n
    assert np.array_equal(cells[:n], hc[:n]) and same_bits(pts[:n], hp[:n]) and same_bits(nrm[:n], hn[:n])
    assert np.all(cells[n:] == -1) and np.all(pts[n:] == -7.0) and np.all(nrm[n:] == -7.0)


def test_compaction_capacity_cut():
    """6. A capacity below the count: the first `capacity` rows as without a cut, the full total, guard values past the
    capacity untouched."""
    steps = 33
    rng = np.random.default_rng(11)
    mean = salted_mean(rng, steps, np.float64)
    normal = rng.standard_normal((steps, steps, steps, 3))
    axes = point_axes([-1.0, 0.5, 2.0], [1.0, 3.5, 2.5], steps)
    n, hc, hp, hn = host_extract(mean, normal, steps, 0, axes)
    cap = 1000  # inside a workgroup's run of rows, several workgroups in
    assert n > cap + 100
    total, cells, pts, nrm = device_extract(mean, normal, steps, 0, axes, capacity=cap, rows=n)
    assert total == n
    assert np.array_equal(cells[:cap], hc[:cap]) and same_bits(pts[:cap], hp[:cap]) and same_bits(nrm[:cap], hn[:cap])
    assert np.all(cells[cap:] == -1) and np.all(pts[cap:] == -7.0) and np.all(nrm[cap:] == -7.0)


@pytest.mark.parametrize("state", list(FIXTURES))
def test_surface_vs_reference(gpis, state):
    """7. surface(): the points are the reference's topcd points exactly; the normals, cast to float32, within 2.4e-7
    absolute — two float32 ulps at 1: the reference's own rounding, and a rounding flip from the 1e-8 parity error."""
    d = golden(FIXTURES[state])
    pts, nrm = gpis[state].surface(d["lb"], d["ub"], steps=int(d["steps"]))
    assert pts.is_cuda and nrm.is_cuda and pts.dtype == torch.float64 and nrm.dtype == torch.float64
    assert same_bits(pts.cpu().numpy(), d["pts_np"])
    err = float(np.abs(nrm.float().cpu().numpy() - d["nrm_np"]).max())
    print("surface normals vs reference", state, err)
    assert err < 2.4e-7


def test_topcd_is_a_method():
    """8. The drop-in has the reference's last public method."""
    from compliancedex_amd import GPIS
    assert hasattr(GPIS, "topcd") and hasattr(GPIS, "field") and hasattr(GPIS, "surface")


def test_completion_workflow_runs(tmp_path, monkeypatch):
    """The reference's shape-completion sequence (train_gpis_completion.py:44-67) by import: fit →
    get_visualization_data → save_state_data → topcd, on 96 surface points of the packaged banana scan with the
    script's auxiliary points; the cloud is the host build's on the same lattice, and surface() gives its points."""
    import os
    from compliancedex_amd import GPIS
    from tests._helpers import DATA
    monkeypatch.chdir(tmp_path)
    b, steps = 0.1, 11
    pcd = torch.from_numpy(np.load(os.path.join(DATA, "partial_pcd_banana.npy"))[::22][:96]).double().to(DEV)
    ext = torch.tensor([[-b, -b, -b], [b, -b, -b], [-b, b, -b], [b, b, -b], [-b, -b, b], [b, -b, b], [-b, b, b], [b, b, b],
                        [-b, 0., 0.], [0., -b, 0.], [b, 0., 0.], [0., b, 0], [0., 0., b], [0., 0., -b]]).double().to(DEV)
    gen = torch.Generator().manual_seed(3)
    w = torch.softmax(torch.rand(16, len(pcd), generator=gen).double() * 10, dim=1).to(DEV)
    internal = w @ pcd
    y1 = torch.hstack([b * torch.ones(len(ext)), torch.zeros(len(pcd)), -b * torch.ones(len(internal))]).view(-1, 1)
    gpis = GPIS(0.08, 1.0)
    gpis.fit(X1=torch.vstack([ext, pcd, internal]), y1=y1.double().to(DEV),
             noise=torch.tensor([0.3] * len(ext) + [0.005] * len(pcd) + [0.02] * len(internal)).double().to(DEV))
    mean, var, normal, lb, ub = gpis.get_visualization_data([-b, -b, -b], [b, b, b], steps=steps)
    gpis.save_state_data("completion_state")
    assert os.path.exists("gpis_states/completion_state.npz")
    points, normals = gpis.topcd(mean, normal, [-b, -b, -b], [b, b, b], steps=steps)
    assert points.dtype == np.float64 and normals.dtype == np.float32 and points.shape == normals.shape
    n, _, hp, hn = host_extract(mean, normal, steps, 0, point_axes(lb, ub, steps))
    assert len(points) == n and n > 0
    assert same_bits(points, hp[:n]) and same_bits(normals, hn[:n])
    if np.abs(mean).min() >= 1e-6:  # (as the fixtures' generator demands: no sign within the 1e-8 parity error)
        assert same_bits(gpis.surface(lb, ub, steps=steps)[0].cpu().numpy(), points)
