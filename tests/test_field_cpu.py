"""GPIS.topcd's cell rule on the host (libcdx_host.so: cdxh_surface_extract, the same csrc/cdx_field.h the
compaction kernels compile) against the reference's own topcd outputs and a numpy statement of the rule.  CPU only."""
import numpy as np
import pytest

from tests._field import F32, F64, host_extract, numpy_extract, point_axes, salted_mean
from tests._helpers import golden

FIXTURES = ["field_banana_s13.npz", "field_mug_s9.npz"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("flip", [0, 1])
def test_host_extract_reproduces_reference_topcd(name, flip):
    """Count, order, point bits and normal bits of the reference's topcd: on numpy inputs (flip 0) and on tensor
    inputs, which it reads flipped along k (flip 1)."""
    d = golden(name)
    steps = int(d["steps"])
    pts, nrm = (d["pts_t"], d["nrm_t"]) if flip else (d["pts_np"], d["nrm_np"])
    n, cells, hp, hn = host_extract(d["mean"], d["normal"], steps, flip, point_axes(d["lb"], d["ub"], steps))
    assert n == len(pts) and n > 0
    assert same_bits(hp[:n], pts)
    assert same_bits(hn[:n], nrm)
    assert np.all(np.diff(cells[:n]) > 0)  # C order
    assert np.all(cells[n:] == -1)         # nothing written past the count


def test_fixture_counts():
    """What the generator printed for the reference: 81 of 105 internal cells (banana), 72 of 94 (mug)."""
    b, m = golden(FIXTURES[0]), golden(FIXTURES[1])
    assert (len(b["pts_np"]), int(b["n_internal"])) == (81, 105)
    assert (len(m["pts_np"]), int(m["n_internal"])) == (72, 94)
    assert float(b["min_abs_mean"]) >= 1e-6 and float(m["min_abs_mean"]) >= 1e-6


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_smallest_lattices(dtype):
    """steps 1 and 2 have no interior cell; steps 3 has exactly one."""
    for steps in (1, 2):
        mean = np.full((steps,) * 3, -1.0, dtype)
        n, _, _, _ = host_extract(mean, np.zeros(mean.shape + (3,), dtype), steps, 0, point_axes([0] * 3, [1] * 3, steps),
                                  capacity=4)
        assert n == 0
    axes = point_axes([0.0, 10.0, 20.0], [2.0, 14.0, 26.0], 3)
    normal = np.arange(81, dtype=dtype).reshape(3, 3, 3, 3)
    for flip in (0, 1):
        mean = np.full((3, 3, 3), -1.0, dtype)       # all internal: the centre has no open neighbour
        assert host_extract(mean, normal, 3, flip, axes)[0] == 0
        mean[1, 1, 2] = 1.0                          # one open face neighbour (k + 1, or k − 1 when flipped)
        n, cells, pts, nrm = host_extract(mean, normal, 3, flip, axes)
        assert n == 1 and cells[0] == 13
        assert pts[0].tolist() == [1.0, 12.0, 23.0]  # (ax[j], ay[i], az[k]) at (1, 1, 1)
        assert nrm[0].tolist() == normal[1, 1, 1].tolist()
        mean = np.full((3, 3, 3), 1.0, dtype)        # centre not internal
        assert host_extract(mean, normal, 3, flip, axes)[0] == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("steps", [5, 7])
@pytest.mark.parametrize("flip", [0, 1])
def test_random_means_against_numpy_rule(dtype, steps, flip):
    rng = np.random.default_rng(100 * steps + 10 * flip + (dtype == np.float64))
    mean = salted_mean(rng, steps, dtype)
    assert np.isnan(mean).any() and (mean == 0).any()
    normal = rng.standard_normal((steps, steps, steps, 3)).astype(dtype)
    axes = point_axes([-1.0, 0.5, 2.0], [1.0, 3.5, 2.5], steps)
    rc, rp, rn = numpy_extract(mean, normal, flip, axes)
    n, cells, pts, nrm = host_extract(mean, normal, steps, flip, axes)
    assert n == len(rc) and n > 0
    assert np.array_equal(cells[:n], rc)
    assert same_bits(pts[:n], rp) and same_bits(nrm[:n], rn)
    # a capacity below the count: the first rows, the full count, nothing beyond
    cap = n // 2
    n2, c2, p2, _ = host_extract(mean, normal, steps, flip, axes, capacity=cap)
    assert n2 == n and np.array_equal(c2, rc[:cap]) and same_bits(p2, rp[:cap])


def test_host_extract_rejects_bad_arguments():
    mean = np.zeros((3, 3, 3))
    normal = np.zeros((3, 3, 3, 3))
    axes = point_axes([0] * 3, [1] * 3, 3)
    assert host_extract(mean, normal, 0, 0, axes, capacity=1)[0] == -1
    assert host_extract(mean, normal, 1025, 0, axes, capacity=1)[0] == -1
    assert host_extract(mean, normal, 3, 0, axes, capacity=1, dtype=2)[0] == -1


def test_bad_arguments_are_rejected_without_launch():
    """The new device entry points return CDX_EINVAL before any launch (no GPU here), beside test_abi.py's checks of
    the others: steps < 1, steps > 1024, null required pointers, an unknown dtype, a negative capacity or chunk."""
    from compliancedex_amd import _native as N
    lib = N.load()
    g = N.CdxGpis()
    one = 256  # any non-null address: never dereferenced
    assert lib.cdx_gpis_field(g, one, one, one, 5, 0, one, None, None, one, None) == -1   # empty descriptor
    assert lib.cdx_gpis_field_workspace(g, 5, 0) == 0
    g.X1 = g.alpha = one
    g.N, g.N_pad = 1, 256
    for steps in (0, -3, 1025):
        assert lib.cdx_gpis_field(g, one, one, one, steps, 0, one, None, None, one, None) == -1
        assert lib.cdx_gpis_field_workspace(g, steps, 0) == 0
        assert lib.cdx_gpis_field_points(one, one, one, steps, None, 1, one, None) == -1
        assert lib.cdx_gpis_surface_workspace(steps) == 0
        assert lib.cdx_gpis_surface_count(one, F64, steps, 0, one, one, None) == -1
        assert lib.cdx_gpis_surface_place(one, one, F64, steps, 0, one, one, one, one, 4, one, one, one, None) == -1
    assert lib.cdx_gpis_field(g, one, one, one, 5, -1, one, None, None, one, None) == -1      # negative chunk
    assert lib.cdx_gpis_field_workspace(g, 5, -1) == 0
    assert lib.cdx_gpis_field(g, None, one, one, 5, 0, one, None, None, one, None) == -1      # null axis
    assert lib.cdx_gpis_field(g, one, one, one, 5, 0, None, None, None, one, None) == -1      # null mean
    assert lib.cdx_gpis_field(g, one, one, one, 5, 0, one, None, None, None, None) == -1      # null workspace
    assert lib.cdx_gpis_field(g, one, one, one, 5, 0, one, one, None, one, None) == -1        # std without Linv_t
    g.kernel = 7
    assert lib.cdx_gpis_field(g, one, one, one, 5, 0, one, None, None, one, None) == -2
    g.kernel = 0
    # a workspace size is host arithmetic: coordinates of the chunk plus the whitened pass's partials
    assert lib.cdx_gpis_field_workspace(g, 5, 0) >= 125 * 24
    assert lib.cdx_gpis_field_workspace(g, 5, 1000) == lib.cdx_gpis_field_workspace(g, 5, 125)
    assert lib.cdx_gpis_surface_workspace(5) == 256 and lib.cdx_gpis_surface_workspace(33) == 1280  # 141 counts
    assert lib.cdx_gpis_field_points(None, one, one, 5, None, 1, one, None) == -1
    assert lib.cdx_gpis_field_points(one, one, one, 5, None, -1, one, None) == -1
    assert lib.cdx_gpis_field_points(one, one, one, 5, None, 126, one, None) == -1            # more than the lattice
    assert lib.cdx_gpis_field_points(one, one, one, 5, None, 1, None, None) == -1
    assert lib.cdx_gpis_surface_count(None, F64, 5, 0, one, one, None) == -1
    assert lib.cdx_gpis_surface_count(one, F64, 5, 0, None, one, None) == -1
    assert lib.cdx_gpis_surface_count(one, F64, 5, 0, one, None, None) == -1
    assert lib.cdx_gpis_surface_count(one, 2, 5, 0, one, one, None) == -1                     # unknown dtype
    assert lib.cdx_gpis_surface_place(None, one, F32, 5, 0, one, one, one, one, 4, one, one, one, None) == -1
    assert lib.cdx_gpis_surface_place(one, one, F32, 5, 0, one, one, one, None, 4, one, one, one, None) == -1
    assert lib.cdx_gpis_surface_place(one, one, 5, 5, 0, one, one, one, one, 4, one, one, one, None) == -1
    assert lib.cdx_gpis_surface_place(one, one, F32, 5, 0, one, one, one, one, -1, one, one, one, None) == -1
    assert lib.cdx_gpis_surface_place(one, one, F32, 5, 0, None, one, one, one, 4, one, one, one, None) == -1  # points, no axis
    assert lib.cdx_gpis_surface_place(one, None, F32, 5, 0, one, one, one, one, 4, one, one, one, None) == -1  # normals, no input
