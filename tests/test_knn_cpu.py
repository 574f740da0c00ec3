"""The host build of csrc/cdx_knn.h (cdxh_knn, cdxh_cloud_normals, cdxh_sym3_eig, the grid functions) against the numpy
statements of tests/_knn.py, bit for bit; sym3_eig against np.linalg.eigh; the grid's lower bound on random and
adversarial rows; the outlier mask's rule on the salted banana cloud.  CPU only."""
import numpy as np
import pytest

from tests import _fps, _knn
from tests._knn import GRID, INF, SCAN, same_bits

CASES = _knn.shared_cases()
EYE = np.array([0.3, -0.2, 0.9])


@pytest.mark.parametrize("mode", [SCAN, GRID], ids=["scan", "grid"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_equals_numpy(name, mode):
    """Brute force and the ring walk of the host build give numpy's indices, distances and counts."""
    c = CASES[name]
    idx, d2, count = _knn.reference(name)
    rc, hi, hd, hc = _knn.host_knn(c["X"], c["K"], c["Q"], c["max_d2"], mode)
    assert rc == 0
    assert same_bits(hi, idx) and same_bits(hd, d2) and same_bits(hc, count)


def test_goldens():
    """Hand-checked lists."""
    X = _fps.duplicates()  # x = 0 0 0 5 5 5 2 2 2 10 10 10 7.5 7.5 7.5
    rc, idx, d2, count = _knn.host_knn(X, 5)
    assert rc == 0
    assert idx[0].tolist() == [0, 1, 2, 6, 7] and d2[0].tolist() == [0, 0, 0, 4, 4]
    assert idx[10].tolist() == [9, 10, 11, 12, 13] and d2[10].tolist() == [0, 0, 0, 6.25, 6.25]
    assert idx[4].tolist() == [3, 4, 5, 12, 13] and d2[4].tolist() == [0, 0, 0, 6.25, 6.25]
    assert count.tolist() == [5] * 15
    L = _fps.lattice(3, 3, 3)  # the centre is row 13: six face neighbours at 1, then twelve at 2
    for mode in (SCAN, GRID):
        rc, idx, d2, count = _knn.host_knn(L, 8, L[13:14], INF, mode)
        assert idx[0].tolist() == [13, 4, 10, 12, 14, 16, 22, 1] and d2[0].tolist() == [0, 1, 1, 1, 1, 1, 1, 2]
        rc, idx, d2, count = _knn.host_knn(L, 8, L[13:14], 1.0, mode)
        assert idx[0].tolist() == [13, 4, 10, 12, 14, 16, 22, -1] and d2[0][7] == INF and count[0] == 7
    rc, idx, d2, count = _knn.host_knn(L[:2], 4, np.array([[0.0, 0.0, 3.0], [np.nan, 0.0, 0.0]]))
    assert idx.tolist() == [[1, 0, -1, -1], [-1, -1, -1, -1]] and count.tolist() == [2, 0]
    assert d2[0].tolist() == [4, 9, INF, INF]


def test_ties_on_the_lattice_and_the_banana():
    """What the cases are for: the banana cloud's lists hold 154 equal-distance pairs inside and none at the K boundary;
    on the lattice the K-th distance is shared at the boundary of every query and the smallest index wins."""
    idx, d2, _ = _knn.reference("banana_f64")
    assert (d2[:, 1:] == d2[:, :-1]).sum() == 154
    idx31, d31, _ = _knn.numpy_knn(CASES["banana_f64"]["X"], 31)
    assert not (d31[:, 30] == d31[:, 29]).any()
    c = CASES["lattice"]
    idx, d2, _ = _knn.reference("lattice")
    i31, d31, _ = _knn.numpy_knn(c["X"], 31, c["Q"])
    tied = d31[:, 30] == d31[:, 29]
    assert tied.all()
    assert (i31[:, 30] > i31[:, 29]).all() and same_bits(i31[:, :30], idx)


def test_bad_arguments():
    X = _fps.normal_cloud(10)
    for K in (0, -1, 65):
        assert _knn.host_knn(X, K)[0] == -1
    assert _knn.host_knn(X, 3, mode=3)[0] == -1
    assert _knn.host_knn(X, 3, dtype=2)[0] == -1


# ---------------------------------------------------------------- normals

@pytest.mark.parametrize("eye", [None, EYE], ids=["sign_rule", "eye"])
@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n]["Q"] is None))
def test_normals_equal_numpy(name, eye):
    """Covariance entries, eigenvalues and normals of the host build are numpy's restatement, bit for bit."""
    c = CASES[name]
    idx, _, count = _knn.reference(name)
    n, w, cov = _knn.host_normals(c["X"], idx, count, eye)
    rn, rw, rcov = _knn.numpy_normals(c["X"], idx, count, eye)
    assert same_bits(cov, rcov)
    assert same_bits(w, rw)
    assert same_bits(n, rn)
    ok = np.isfinite(np.asarray(c["X"], np.float64)).all(axis=1)
    assert np.isnan(n[~ok]).all() and np.isfinite(n[ok]).all()
    if eye is None:
        a = np.abs(n[ok])
        lead = np.take_along_axis(n[ok], np.argmax(a, axis=1)[:, None], axis=1)
        assert (lead > 0).all()
    else:
        assert ((n[ok] * (eye - np.asarray(c["X"], np.float64)[ok])).sum(axis=1) >= -1e-18).all()
    few = ok & (count < 3)
    assert (np.abs(n[few]) == np.array([0.0, 0.0, 1.0])).all() and np.isnan(w[few]).all()


def _covariances():
    out = []
    for name in sorted(CASES):
        c = CASES[name]
        if c["Q"] is None:
            idx, _, count = _knn.reference(name)
            cov = _knn.numpy_covariance(c["X"], idx, count)
            out.append(cov[np.isfinite(cov).all(axis=1) & (count >= 3)])
    rng = np.random.default_rng(33)
    scale = 10.0 ** rng.uniform(-8, 8, (10000, 1))
    out.append(rng.standard_normal((10000, 6)) * scale)
    B = rng.standard_normal((2000, 3, 3))
    S = B @ B.transpose(0, 2, 1)  # positive semi-definite, some nearly singular
    S[:500] = B[:500, :, :2] @ B[:500, :, :2].transpose(0, 2, 1)
    out.append(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1))
    return np.concatenate(out)


def test_sym3_eig_against_eigh():
    """The smallest eigenpair of sym3_eig against np.linalg.eigh on the shared cases' covariances, 10⁴ random symmetric
    matrices over sixteen decades and 2000 Gram matrices.  The 256 is derived, not measured: the rule allows at most
    10 sweeps of 3 rotations, each an orthogonal similarity with a backward error of a few units in the last place of
    ‖C‖_F, so 30 rotations × ≲ 8 ulp stay below 256 · 2⁻⁵².  Where the gap λ₁ − λ₀ is at least 10⁻³ ‖C‖_F the angle to
    eigh's vector is bounded by twice that residual bound over the gap."""
    cov = _covariances()
    w, V = _knn.host_sym3_eig(cov)
    rw, rV = _knn.numpy_sym3_eig(cov)
    assert same_bits(w, rw) and same_bits(V, rV)
    Cm = np.zeros((len(cov), 3, 3))
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        Cm[:, i, j] = Cm[:, j, i] = cov[:, k]
    ew, eV = np.linalg.eigh(Cm)
    fro = np.sqrt((Cm * Cm).sum(axis=(1, 2)))
    bound = 256 * 2.0 ** -52 * fro
    n = V[:, :, 0]
    res = np.linalg.norm(np.einsum("nij,nj->ni", Cm, n) - w[:, :1] * n, axis=1)
    assert (res <= bound).all(), float((res / np.maximum(bound, 1e-300)).max())
    assert (np.abs(w[:, 0] - ew[:, 0]) <= bound).all()
    assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 64 * 2.0 ** -52).all()
    assert (w[:, 0] <= w[:, 1]).all() and (w[:, 1] <= w[:, 2]).all()
    gap = ew[:, 1] - ew[:, 0]
    wide = (gap >= 1e-3 * fro) & (fro > 0)  # the zero matrix (coincident neighbours) has no direction to compare
    assert wide.sum() > 0.5 * len(cov)
    # the sine through the cross product (1 − cos² loses everything below √2⁻⁵²)
    sinang = np.linalg.norm(np.cross(n[wide], eV[wide, :, 0]), axis=1)
    assert (sinang <= 2 * bound[wide] / gap[wide]).all()


def test_banana_rows_all_take_the_angle_check():
    """The smallest (λ₁ − λ₀)/λ₂ on the banana cloud is 0.19, far above the 10⁻³ gap the angle check asks for."""
    c = CASES["banana_f64"]
    idx, _, count = _knn.reference("banana_f64")
    w, _ = _knn.numpy_sym3_eig(_knn.numpy_covariance(c["X"], idx, count))
    assert round(float(((w[:, 1] - w[:, 0]) / w[:, 2]).min()), 2) == 0.19


# ---------------------------------------------------------------- the grid's bound

def _adversarial_cloud():
    """Rows on cell faces of their own grid, moved by ±1 ulp, at the box's corners, and random rows."""
    rng = np.random.default_rng(41)
    base = rng.uniform(0.0, 1.0, (600, 3))
    corners = np.array([[i, j, k] for i in (0.0, 1.0) for j in (0.0, 1.0) for k in (0.0, 1.0)])
    n0 = 11  # knn_grid_n0 of the ~1300 rows built here: faces at multiples of 1/11
    faces = rng.integers(0, n0 + 1, (200, 3)) / n0
    rows = [base, corners, faces, np.nextafter(faces, 2.0), np.nextafter(faces, -1.0)]
    mixed = base[:100].copy()
    mixed[:, 0] = faces[:100, 0]  # on a face along one axis only
    rows.append(mixed)
    return np.clip(np.concatenate(rows), 0.0, 1.0)


@pytest.mark.parametrize("cloud", ["adversarial", "normal", "two_clusters", "offset"])
def test_ring_bound_is_a_lower_bound(cloud):
    """For every query and every ring r, each row the rounded assignment put in a cell at Chebyshev distance > r from
    the query's cell has a d2 (the rule's rounded one) no smaller than knn_ring_bound(r), in the kernel's arithmetic
    through the host build's functions; and the bound is not vacuous."""
    X = {"adversarial": _adversarial_cloud(), "normal": _fps.normal_cloud(700, seed=2),
         "two_clusters": _knn.two_clusters(),
         "offset": _adversarial_cloud() * 1e-3 + np.array([1e5, -3e4, 7.0])}[cloud]  # faces no longer representable
    g = _knn.host_grid(X)
    assert g["dims"].max() > 1
    lo, hi = X.min(axis=0), X.max(axis=0)
    rng = np.random.default_rng(43)
    Q = np.concatenate([X[rng.choice(len(X), 150, replace=False)], np.nextafter(X[:50], INF), np.nextafter(X[50:100], -INF),
                        rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (150, 3)),
                        lo + (hi - lo) * _knn.outside_queries()[:21] / 6.0])
    d = X[None, :, :] - Q[:, None, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    useful = 0
    for r in range(int(g["dims"].max())):
        cq, bound, none = _knn.host_ring_bound(g, Q, r)
        cheb = np.abs(g["cell"][None, :, :] - cq[:, None, :]).max(axis=2)
        outside = cheb > r
        assert (d2[outside] >= np.broadcast_to(bound[:, None], d2.shape)[outside]).all()
        assert (none == ~outside.any(axis=1)).all()
        useful += int(((bound > 0) & ~none).sum())
    assert useful > len(Q)
    assert (g["cell"] >= 0).all() and (g["cell"] < g["dims"][None, :]).all()


# ---------------------------------------------------------------- the outlier mask

def test_mask_on_the_salted_banana():
    """(20, 2.0) rejects exactly the 12 moved rows: their mean neighbour distance is ≥ 0.076 m against a threshold of
    0.025 m and a largest clean value of 0.0103 m.  A farthest-point sample of the NaN-masked cloud holds none of them,
    while the 200-point sample of the unmasked cloud holds all 12 at selection positions 1–21."""
    X, rows = _knn.salted_banana()
    assert len(set(rows.tolist())) == 12 and 0 not in rows
    keep, avg, thr = _knn.numpy_outlier_mask(X, 20, 2.0)
    assert np.flatnonzero(~keep).tolist() == rows.tolist()
    assert avg[rows].min() >= 0.076 and round(thr, 3) == 0.025 and round(float(avg[keep].max()), 4) == 0.0103
    dirty, _, _ = _fps.numpy_fps(X, 200)
    where = sorted(int(np.flatnonzero(dirty == r)[0]) for r in rows)
    assert len(where) == 12 and where[0] == 1 and where[-1] == 21
    masked = np.where(keep[:, None], X, np.nan)
    clean, _, _ = _fps.numpy_fps(masked, 200)
    assert not set(rows.tolist()) & set(clean.tolist())
