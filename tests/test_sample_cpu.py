"""Area-weighted surface sampling on the host (libcdx_host.so: cdxh_sample_prepare / cdxh_sample_draw, the same
csrc/cdx_sample.h the sampling kernels compile) against a numpy statement of the rule, bit for bit, the rule's
statistics on the packaged meshes and the Poisson composition.  CPU only."""
import numpy as np
import pytest

from tests import _sample as S
from tests._sample import host_draw, host_prepare, numpy_draw, numpy_prepare, same_bits, same_draw

K_STAT = 200_000
Z_MAX = 5.0


@pytest.fixture(scope="module")
def cases():
    return S.shared_cases()


_STAT = {}


def stat_draw(name):
    """(weights, faces drawn) of K_STAT samples at seed 0 of a packaged mesh by the host build (the numpy statement's
    bits: test_host_matches_numpy_on_every_shared_case), computed once for the module."""
    if name not in _STAT:
        faces = S.mesh(name)
        rc, cdf, info = host_prepare(faces)
        assert rc == 0 and info == 0
        _STAT[name] = (S.weights_of(cdf), host_draw(faces, cdf, 0, 0, K_STAT)[2])
    return _STAT[name]


def test_philox_known_answers_in_numpy_and_in_the_host_build():
    for counter, key, out in S.PHILOX_VECTORS:
        assert tuple(int(x) for x in S.numpy_philox(counter, key)) == out
        assert S.host_philox(counter, key) == out
    # the numpy statement's 64-bit multiply against Python integers
    rng = np.random.default_rng(5)
    a = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    a[:3] = [0, 2 ** 64 - 1, 2 ** 32]
    for b in (0, 1, 2 ** 32, 2 ** 60 + 12345, 2 ** 64 - 1, 0x9E3779B97F4A7C15):
        assert S.mulhi64(a, b).tolist() == [(int(x) * b) >> 64 for x in a]


def test_host_matches_numpy_on_every_shared_case(cases):
    assert len(cases) >= 15
    for name, faces in cases.items():
        cdf, info = numpy_prepare(faces)
        rc, hcdf, hinfo = host_prepare(faces)
        assert rc == 0 and hinfo == info and same_bits(hcdf, cdf), name
        for seed, first, K in ((0, 0, 1000), (1, 7, 65), (0xDEADBEEF12345678, 2 ** 32 - 3, 257), (3, 2 ** 40, 64),
                               (5, 2 ** 64 - 2, 5)):
            rc, *got = host_draw(faces, cdf, seed, first, K)
            assert rc == 0 and same_draw(got, numpy_draw(faces, cdf, seed, first, K)), (name, seed, first)


def test_weights_are_scaled_areas(cases):
    for name in ("cube", "sphere42", "banana", "random_F5000"):
        faces = cases[name]
        rc, cdf, _ = host_prepare(faces)
        w = S.weights_of(cdf).astype(np.float64)
        area = S.numpy_geometry(faces)[5]
        assert w.max() == 2.0 ** 32 and int(cdf[-1]) == int(S.weights_of(cdf).astype(object).sum())
        assert np.abs(w / 2.0 ** 32 - area / area.max()).max() <= 2.0 ** -32


def test_per_face_counts_on_cube_and_sphere():
    for name in ("cube", "sphere42"):
        w, face = stat_draw(name)
        z = S.binomial_z(np.bincount(face, minlength=len(w)), w, K_STAT)
        print(name, "largest |z| of the per-face counts:", z.max())
        assert z.max() <= Z_MAX, (name, z.max())


def test_face_group_counts_on_the_banana():
    w, face = stat_draw("banana")
    groups = np.array_split(np.arange(len(w)), 16)
    counts = np.bincount(face, minlength=len(w))
    z = S.binomial_z(np.array([counts[g].sum() for g in groups]),
                     np.array([w[g].astype(object).sum() for g in groups], dtype=np.float64), K_STAT)
    print("banana: largest |z| of 16 face groups:", z.max())
    assert z.max() <= Z_MAX, z.max()


def test_prefix_and_first_properties(cases):
    faces = cases["banana"]
    cdf, _ = numpy_prepare(faces)
    for fn in (lambda *a: tuple(host_draw(*a)[1:]), numpy_draw):
        whole = fn(faces, cdf, 9, 0, 1000)
        assert same_draw(fn(faces, cdf, 9, 0, 300), [x[:300] for x in whole])
        assert same_draw(fn(faces, cdf, 9, 300, 700), [x[300:] for x in whole])
        far = fn(faces, cdf, 9, 2 ** 40 - 10, 50)
        assert same_draw(fn(faces, cdf, 9, 2 ** 40, 40), [x[10:] for x in far])
        assert not same_bits(fn(faces, cdf, 10, 0, 300)[0], whole[0][:300])  # another seed, another stream


def test_barycentric_pairs_stay_in_the_triangle(cases):
    faces = cases["sphere42"]
    rc, cdf, _ = host_prepare(faces)
    rc, points, face, bary, normal = host_draw(faces, cdf, 0, 0, K_STAT)
    u, v = bary[:, 0], bary[:, 1]
    assert u.min() > 0 and v.min() > 0 and (u + v).max() <= 1.0
    f = faces.astype(np.float64)[face]
    direct = f[:, 0] + u[:, None] * (f[:, 1] - f[:, 0]) + v[:, None] * (f[:, 2] - f[:, 0])
    assert np.abs(points - direct).max() <= 1e-15 * np.abs(f).max()
    assert np.abs(np.linalg.norm(normal, axis=1) - 1.0).max() <= 1e-15
    assert np.abs(((points - f[:, 0]) * normal).sum(axis=1)).max() <= 1e-15 * np.abs(f).max()  # in the face's plane


def test_a_face_below_the_weight_resolution_is_never_drawn():
    faces = S.tiny_beside_unit()
    area = S.numpy_geometry(faces)[5]
    assert area.tolist() == [2.0 ** -40, 1.0, 2.0 ** -40]
    rc, cdf, info = host_prepare(faces)
    assert rc == 0 and info == 0 and cdf.tolist() == [0, 2 ** 32, 2 ** 32]
    for seed in (0, 1, 2):
        assert np.all(host_draw(faces, cdf, seed, 0, 20000)[2] == 1)


def test_zero_area_and_nonfinite_faces_are_never_drawn():
    faces = S.salted_faces()
    rc, cdf, info = host_prepare(faces)
    w = S.weights_of(cdf)
    assert rc == 0 and info == 0 and not w[list(S.DEAD_ROWS)].any()
    assert np.count_nonzero(w) >= len(w) - len(S.DEAD_ROWS) - 30  # the rest, but for faces below 2⁻³² of the largest
    rc, points, face, bary, normal = host_draw(faces, cdf, 0, 0, K_STAT)
    assert not set(face.tolist()) & set(S.DEAD_ROWS)
    assert np.isfinite(points).all() and np.isfinite(normal).all() and face.min() >= 0


def test_a_mesh_with_no_area():
    for faces in (S.all_degenerate(), S.all_degenerate(1)):
        rc, cdf, info = host_prepare(faces)
        assert rc == 0 and info == 1 and not cdf.any()
        assert same_bits(cdf, numpy_prepare(faces)[0]) and numpy_prepare(faces)[1] == 1
        rc, points, face, bary, normal = host_draw(faces, cdf, 4, 11, 100)
        assert rc == 0 and np.all(face == -1)
        assert np.isnan(points).all() and np.isnan(bary).all() and np.isnan(normal).all()


def test_host_argument_checks(cases):
    faces = cases["cube"]
    cdf, _ = numpy_prepare(faces)
    assert host_prepare(faces, dtype=2)[0] == -1 and host_prepare(faces, F=0)[0] == -1
    assert host_prepare(faces, F=0x7fffffff // 9 + 1)[0] == -1
    assert host_draw(faces, cdf, 0, 0, -1)[0] == -1
    rc, points, face, _, _ = host_draw(faces, cdf, 0, 0, 0)
    assert rc == 0 and points.shape == (0, 3)


def test_device_entry_points_reject_bad_arguments_before_any_launch():
    """libcdx.so loads without a GPU, and a bad argument returns before anything touches one."""
    from compliancedex_amd import _native as N
    lib = N.load()
    big = 0x7fffffff // 9 + 1
    assert lib.cdx_sample_table_capacity() == 16384 and lib.cdx_sample_scan_faces() >= 256
    assert lib.cdx_sample_prepare_workspace(0) == 0 and lib.cdx_sample_prepare_workspace(big) == 0
    assert lib.cdx_sample_prepare_workspace(1) > 0
    assert lib.cdx_sample_prepare_workspace(10 ** 6) >= 8 * 10 ** 6
    good = (1, N.DTYPE_F64, 12, 1, 1, 1, None)
    for i, bad in ((0, None), (1, 7), (2, 0), (2, big), (3, None), (4, None), (5, None)):
        args = list(good)
        args[i] = bad
        assert lib.cdx_sample_prepare(*args) == -1, (i, bad)
    good = (1, N.DTYPE_F64, 12, 1, 0, 0, 5, 0, 1, None, None, None, None)
    for i, bad in ((0, None), (1, 7), (2, 0), (2, big), (3, None), (6, -1), (7, 3), (7, -2)):
        args = list(good)
        args[i] = bad
        assert lib.cdx_sample_draw(*args) == -1, (i, bad)
    args = list(good)
    args[2], args[7] = 16385, 1  # the table path beyond its capacity
    assert lib.cdx_sample_draw(*args) == -1
    args = list(good)
    args[6] = 0  # K = 0 is a no-op
    assert lib.cdx_sample_draw(*args) == 0


def test_poisson_composition_on_the_banana(cases):
    K = 256
    faces = cases["banana"]
    chosen, face, normal, sel, radius, uniform = S.numpy_poisson(faces, K)
    assert len(np.unique(chosen, axis=0)) == K and len(set(sel.tolist())) == K
    spacing = S.min_pairwise(chosen)
    assert spacing == np.sqrt(radius[K - 1])
    crowd = S.min_pairwise(uniform[:K])
    print("minimum pairwise distance: Poisson", spacing, "uniform", crowd)
    assert spacing > crowd
    # the host build composes to the same bits
    from tests._fps import host_fps
    rc, cdf, _ = host_prepare(faces)
    _, hp, hf, _, hn = host_draw(faces, cdf, 0, 0, 5 * K)
    rc, hsel, hradius, hchosen = host_fps(hp, K, 0)
    assert rc == 0 and np.array_equal(hsel, sel) and same_bits(hchosen, chosen) and same_bits(hradius, radius)
    assert np.array_equal(hf[hsel], face) and same_bits(hn[hsel], normal)
