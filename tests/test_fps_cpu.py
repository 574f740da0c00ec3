"""Farthest-point sampling on the host (libcdx_host.so: cdxh_fps, the same csrc/cdx_fps.h the sampling kernels
compile) against a numpy statement of the rule, bit for bit, and the device entry point's argument checks.  CPU only."""
import numpy as np
import pytest

from tests import _fps
from tests._fps import host_fps, numpy_fps, same_bits


@pytest.fixture(scope="module")
def capacity():
    from compliancedex_amd import _native as N
    return int(N.load().cdx_fps_capacity())


@pytest.fixture(scope="module")
def cases(capacity):
    return {**_fps.shared_cases(capacity), **_fps.large_cases()}


def check(X, K, start):
    rs, rr, rp = numpy_fps(X, K, start)
    rc, sel, radius, points = host_fps(X, K, start)
    assert rc == 0
    assert np.array_equal(sel, rs)
    assert same_bits(radius, rr) and same_bits(points, rp)
    return sel, radius


def test_capacity_serves_the_reference_sizes(capacity):
    assert capacity >= 4096


def test_host_matches_numpy_on_every_shared_case(cases):
    assert len(cases) >= 25
    for name, (X, K, start) in cases.items():
        sel, radius = check(X, K, start)
        assert sel[0] == start, name
        assert np.all(np.diff(radius[1:]) <= 0), name  # radius[1:] never grows


def test_single_point():
    sel, radius = check(np.array([[0.5, -1.0, 2.0]]), 1, 0)
    assert sel.tolist() == [0] and radius.tolist() == [np.inf]


def test_k_equals_p_is_a_permutation():
    sel, radius = check(_fps.normal_cloud(65, seed=165), 65, 0)
    assert sorted(sel.tolist()) == list(range(65))
    assert np.all(radius[1:] > 0)


def test_duplicates_repeat_the_lowest_index():
    sel, radius = check(_fps.duplicates(), 9, 0)
    assert sel.tolist() == _fps.DUPLICATES_SEL
    assert radius.tolist() == _fps.DUPLICATES_RADIUS


def test_nonfinite_rows_are_chosen_only_as_start():
    X = _fps.salted_cloud()
    bad = sorted(_fps.NONFINITE_ROWS)
    sel, radius = check(X, 40, 0)
    assert not set(sel.tolist()) & set(bad) and radius[0] == np.inf
    for start in bad:
        sel, radius = check(X, 40, start)
        assert sel[0] == start and radius[0] == -1.0
        assert not set(sel[1:].tolist()) & set(bad)
        assert radius[1] == np.inf  # a non-finite centre moves no distance
    # every row but three non-finite, K beyond them: the rule repeats the lowest finite index
    Y = _fps.all_nonfinite(20)
    Y[[4, 9, 17]] = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 3.0, 0.0]]
    sel, radius = check(Y, 6, 9)
    assert sel.tolist() == [9, 17, 4, 4, 4, 4] and radius.tolist() == [np.inf, 10.0, 1.0, 0.0, 0.0, 0.0]


def test_all_rows_nonfinite():
    sel, radius = check(_fps.all_nonfinite(), 5, 2)
    assert sel.tolist() == [2, 0, 0, 0, 0] and np.all(radius == -1.0)


def test_banana_golden():
    """What the issue records for the reference's banana cloud: 200 distinct rows beginning 0, 534, 1814, 1872."""
    X = _fps.banana()
    assert X.shape == (2048, 3) and X.dtype == np.float64
    sel, radius = check(X, 200, 0)
    assert sel[:4].tolist() == [0, 534, 1814, 1872] and len(set(sel.tolist())) == 200
    assert np.all(np.diff(radius[1:]) <= 0)


def test_lattice_ties_go_to_the_lowest_index():
    X = _fps.lattice(35, 35, 33)
    assert len(X) == 40425
    sel, radius = check(X, 32, 0)
    assert sel[:4].tolist() == [0, 40424, 1138, 39286]
    assert radius[:4].tolist() == [np.inf, 3336.0, 1412.0, 1412.0]


def test_prefix_property():
    X = _fps.banana()
    assert np.array_equal(host_fps(X, 50)[1], host_fps(X, 200)[1][:50])
    assert same_bits(host_fps(X, 50)[2], host_fps(X, 200)[2][:50])


def test_float32_cloud_is_widened():
    X = _fps.banana().astype(np.float32)
    rc, sel, radius, points = host_fps(X, 200)
    rs, rr, rp = numpy_fps(X.astype(np.float64), 200)
    assert rc == 0 and np.array_equal(sel, rs) and same_bits(radius, rr) and same_bits(points, rp)


def test_host_batch_and_null_outputs():
    X = np.stack([_fps.normal_cloud(500, seed=s) for s in (1, 2, 3)])
    rc, sel, radius, points = host_fps(X, 20, 7)
    assert rc == 0
    for b in range(3):
        rs, rr, rp = numpy_fps(X[b], 20, 7)
        assert np.array_equal(sel[b], rs) and same_bits(radius[b], rr) and same_bits(points[b], rp)
    lib = _fps.host()
    assert lib.cdxh_fps(_fps.p(X), _fps.F64, 500, 3, 20, 7, None, None, None) == 0


def test_host_rejects_bad_arguments():
    X = _fps.normal_cloud(10)
    assert host_fps(X, 0)[0] == -1 and host_fps(X, 11)[0] == -1
    assert host_fps(X, 3, -1)[0] == -1 and host_fps(X, 3, 10)[0] == -1
    assert host_fps(X, 3, 0, dtype=2)[0] == -1


def test_bad_arguments_are_rejected_without_launch(capacity):
    """cdx_fps returns CDX_EINVAL before any launch (no GPU here): a null X or workspace, K < 1, K > P, start outside
    0 … P−1, B < 1, an unknown dtype or mode, P ≥ 2³¹, mode 1 beyond its capacity, and P·B = 0 with K = 0."""
    from compliancedex_amd import _native as N
    lib = N.load()
    one = 256  # any non-null address: never dereferenced
    F64 = N.DTYPE_F64

    def call(X=one, dtype=F64, P=100, B=1, K=10, start=0, mode=0, ws=one):
        return lib.cdx_fps(X, dtype, P, B, K, start, mode, ws, one, one, one, None)

    assert call(X=None) == -1 and call(ws=None) == -1
    assert call(K=0) == -1 and call(K=-4) == -1 and call(K=101) == -1
    assert call(start=-1) == -1 and call(start=100) == -1
    assert call(B=0) == -1 and call(B=-2) == -1
    assert call(dtype=2) == -1 and call(dtype=-1) == -1
    assert call(mode=3) == -1 and call(mode=-1) == -1
    assert call(P=2 ** 31, K=10) == -1 and call(P=2 ** 31, K=10, mode=2) == -1
    assert call(P=0, K=0) == -1 and call(P=5, B=0, K=0) == -1
    assert call(P=capacity + 1, mode=1) == -1
    # the workspace is host arithmetic: 0 for the same bad shapes, a token for the one-workgroup path, and for the
    # per-round path dist [B·P], a 16-byte slot per 1024 rows, the current centre and the counter, each on 256 bytes
    assert lib.cdx_fps_workspace(0, 1, 0) == 0 and lib.cdx_fps_workspace(100, 0, 0) == 0
    assert lib.cdx_fps_workspace(2 ** 31, 1, 2) == 0 and lib.cdx_fps_workspace(100, 1, 3) == 0
    assert lib.cdx_fps_workspace(capacity + 1, 1, 1) == 0
    assert 0 < lib.cdx_fps_workspace(capacity, 1, 1) <= 256
    assert lib.cdx_fps_workspace(capacity, 1, 0) == lib.cdx_fps_workspace(capacity, 1, 1)
    assert lib.cdx_fps_workspace(capacity + 1, 1, 0) == lib.cdx_fps_workspace(capacity + 1, 1, 2)
    assert lib.cdx_fps_workspace(70001, 3, 2) == (3 * 70001 * 8 + 255) // 256 * 256 + (3 * 69 * 16 + 255) // 256 * 256 + 512


def test_python_entry_points_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from compliancedex_amd import GPIS, completion_arrays, farthest_point_down_sample, farthest_point_sample
    X = torch.zeros(10, 3, dtype=torch.float64)
    for fn in (lambda: farthest_point_sample(X, 3), lambda: farthest_point_down_sample(X, 3),
               lambda: completion_arrays(X, 0.15, 5, 30.0, (0.2, 0.005, 0.1)),
               lambda: GPIS(0.08, 1.0).fit_pointcloud(X, 3)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()
