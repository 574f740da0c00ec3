"""The GPIS joint posterior of value and gradient on the GPU: cdx_gpis_joint against the numpy statement of
tests/_joint.py and against the tested std pass, row independence, refusals, and the Python layer on top of it
(pred_joint, normal_uncertainty, sample_joint, sample_normals, shape_uncertainty_report).  GPU only."""
import numpy as np
import pytest
import torch

from tests import _joint, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNELS = ("tps", "rbf", "joint")
SIZES = (7, 63, 255, 257, 513)
BATCHES = (1, 3, 4, 5, 67, 300)  # the 4-query tile ragged and full, one wave, several workgroups
QUERY_POISONS = dict(_rows.POISONS, overflow=_rows.OVERFLOW)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _gpis(kernel, n):
    """(GPIS, X1, E11, R as numpy): a sphere state of tests/test_gpu_edges._random_gpis or "banana2000"."""
    if (kernel, n) not in _CACHE:
        if n == "banana2000":
            from compliancedex_amd.workloads import synthetic_banana_gpis
            g = synthetic_banana_gpis(2000, device=DEV)
        else:
            from tests.test_gpu_edges import _random_gpis
            g = _random_gpis(n, seed=n, kernel=kernel)[0]
        R = float(g.R) if kernel != "rbf" else 0.0
        _CACHE[kernel, n] = (g, host(g.X1.double()), host(g.E11), R)
    return _CACHE[kernel, n]


def _cov(g, X):
    from compliancedex_amd import gpis_joint_cov
    return host(gpis_joint_cov(g.native_state(), dev(X)))


def _case(kernel, n):
    """The 300 queries of a state, the statement there and the device's answer, computed once."""
    key = ("case", kernel, n)
    if key not in _CACHE:
        g, X1, E11, R = _gpis(kernel, n)
        X = _joint.queries(X1, 300, 1000 + n)
        _CACHE[key] = (X, _joint.np_joint(kernel, X1, E11, R, X, sigma=g.sigma), _cov(g, X))
    return _CACHE[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_parity_with_the_statement(kernel, n):
    """Scaled error ≤ 1e-9 at every M (three orders above what two float64 statements differ by), with the device's own
    L⁻¹; Σ positive definite at every one of the 300 queries; the first M rows of the batch alone have the bits they have
    in the batch — row 0 of an M = 1 call equals row 0 of the M = 300 call."""
    g, X1, E11, R = _gpis(kernel, n)
    X, want, got300 = _case(kernel, n)
    worst = 0.0
    for M in BATCHES:
        got = got300 if M == 300 else _cov(g, X[:M])
        assert got.shape == (M, 10) and np.isfinite(got).all()
        worst = max(worst, _joint.scaled_error(got, want[:M], kernel, R, g.sigma))
        assert _rows.same_bits(got, got300[:M]), M
    eig = np.linalg.eigvalsh(_joint.full(got300))
    print(f"joint {kernel} N={n}: scaled error {worst:.3g}, smallest eigenvalue / prior "
          f"{(eig[:, 0] / _joint.np_prior(kernel, R, g.sigma)[0]).min():.3g}")
    assert worst <= 1e-9
    assert (eig[:, 0] > 0.0).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_ties_to_the_std_pass(kernel, n):
    """|Σ00| = std² and Σ[0, 1 + i] = sign(Σ00)·std·∇std[i] (∂ᵢ Var f = 2·Cov(f, ∂ᵢf)) against cdx_gpis_std at the same
    queries, both within the scaled error 1e-9: the new kernel's operand generation and layout against the existing
    kernel with no statement in between."""
    from compliancedex_amd.gpis import gpis_std
    g, X1, E11, R = _gpis(kernel, n)
    X, _, got = _case(kernel, n)
    std, gstd = (host(t) for t in gpis_std(g.native_state(), dev(X), want_grad=True))
    p0 = _joint.np_prior(kernel, R, g.sigma)
    e_var = np.abs(np.abs(got[:, 0]) - std * std).max() / p0[0]
    e_cross = np.abs(got[:, 1:4] - np.sign(got[:, :1]) * std[:, None] * gstd).max() / np.sqrt(p0[0] * p0[1])
    print(f"joint {kernel} N={n}: against the std pass, variance {e_var:.3g}, cross terms {e_cross:.3g}")
    assert e_var <= 1e-9 and e_cross <= 1e-9


def test_far_queries():
    """RBF 5 m away: Σ = P0 to 1e-12.  TPS at 0.08·randn, where queries can lie farther than R from an inducing point:
    finite, signed and equal to the statement; no claim about definiteness either way."""
    g, X1, E11, R = _gpis("rbf", 63)
    got = _cov(g, _joint.queries(X1, 9, 5) + np.array([5.0, 0.0, 0.0]))
    prior = np.tile(np.diag(_joint.np_prior("rbf", R, g.sigma))[np.triu_indices(4)], (9, 1))
    assert _joint.scaled_error(got, prior, "rbf", R, g.sigma) <= 1e-12
    for n in (63, 257):
        g, X1, E11, R = _gpis("tps", n)
        X = 0.08 * np.random.default_rng(n).standard_normal((40, 3))
        got, want = _cov(g, X), _joint.np_joint("tps", X1, E11, R, X)
        assert np.isfinite(got).all()
        # WᵀW is up to a few tens of priors there: relative to the largest scaled entry, never below 1
        size = max(1.0, _joint.scaled_error(want, np.zeros_like(want), "tps", R))
        err = _joint.scaled_error(got, want, "tps", R)
        print(f"joint tps N={n} far: scaled error {err:.3g} at size {size:.3g}")
        assert err <= 1e-9 * size


def test_stripe_sized_state():
    """The N = 2000 synthetic banana (16 column blocks in 4 splits) with M = 4200: 50 rows against the statement."""
    g, X1, E11, R = _gpis("tps", "banana2000")
    X = _joint.queries(X1, 4200, 7)
    got = _cov(g, X)
    rows = np.random.default_rng(0).choice(4200, 50, replace=False)
    rows[:2] = (0, 4199)
    want = _joint.np_joint("tps", X1, E11, R, X[rows], sigma=g.sigma)
    err = _joint.scaled_error(got[rows], want, "tps", R)
    print(f"joint banana2000 M=4200: scaled error {err:.3g}")
    assert np.isfinite(got).all() and err <= 1e-9
    assert _rows.same_bits(_cov(g, X[:5]), got[:5])


@pytest.mark.parametrize("kernel,n", [("tps", 255), ("rbf", 257), ("joint", 63), ("tps", "banana2000")])
def test_rows(kernel, n):
    """A poisoned query (NaN, ±inf, 1e200 in its x) at M = 5 and 67: every other row keeps its bits, the poisoned row's 10
    entries are NaN — but for RBF at 1e200, a finite query infinitely far in floating point, whose Σ is the prior."""
    g, X1, E11, R = _gpis(kernel, n)
    for M in (5, 67):
        X = _joint.queries(X1, M, 200 + M)
        clean = dict(cov=_cov(g, X))
        assert np.isfinite(clean["cov"]).all()
        for P in _rows.query_sets(M):
            for name, v in QUERY_POISONS.items():
                out = dict(cov=_cov(g, _rows.poison(X, P, v)))
                far = kernel == "rbf" and name == "overflow"
                _rows.check(clean, out, P, M, () if far else None, tag=f"joint {kernel} N={n} M={M} {name}")
                if far:
                    assert np.array_equal(_joint.full(out["cov"][list(P)]),
                                          np.tile(np.diag(_joint.np_prior("rbf", R, g.sigma)), (len(P), 1, 1)))
                elif name != "overflow":
                    assert np.isnan(out["cov"][list(P)]).all(), (name, P)


def test_refusals_and_empty_batch():
    """Return codes as cdx_gpis_std; preset outputs stay untouched on every refusal and at M = 0."""
    import ctypes as C
    from compliancedex_amd import _native as N
    lib = N.load()
    g, X1, E11, R = _gpis("tps", 63)
    st = g.native_state()
    X = dev(_joint.queries(X1, 6, 0))
    cov = torch.full((6, 10), -7.0, dtype=torch.float64, device=DEV)
    assert lib.cdx_gpis_joint_workspace(st.desc, 6) == 1 * 6 * 10 * 8
    assert lib.cdx_gpis_joint_workspace(st.desc, 0) == 0 and lib.cdx_gpis_joint_workspace(None, 6) == 0
    ws = torch.empty(lib.cdx_gpis_joint_workspace(st.desc, 6), dtype=torch.uint8, device=DEV)
    s = N.stream_ptr(X.device)
    args = (N.ptr(X), 6, N.ptr(cov), N.ptr(ws), s)
    assert lib.cdx_gpis_joint(None, *args) == -1
    assert lib.cdx_gpis_joint(st.desc, None, 6, N.ptr(cov), N.ptr(ws), s) == -1
    assert lib.cdx_gpis_joint(st.desc, N.ptr(X), 6, None, N.ptr(ws), s) == -1
    assert lib.cdx_gpis_joint(st.desc, N.ptr(X), 6, N.ptr(cov), None, s) == -1
    assert lib.cdx_gpis_joint(st.desc, N.ptr(X), -1, N.ptr(cov), N.ptr(ws), s) == -1
    bad = N.CdxGpis.from_buffer_copy(st.desc)
    bad.kernel = 7
    assert lib.cdx_gpis_joint(bad, *args) == -2
    bad = N.CdxGpis.from_buffer_copy(st.desc)
    bad.Linv_t = None
    assert lib.cdx_gpis_joint(bad, *args) == -1
    assert lib.cdx_gpis_joint(st.desc, None, 0, None, None, s) == 0
    assert lib.cdx_gpis_joint(st.desc, N.ptr(X), 0, N.ptr(cov), N.ptr(ws), s) == 0
    torch.cuda.synchronize()
    assert (host(cov) == -7.0).all()
    assert lib.cdx_gpis_joint(st.desc, *args) == 0
    torch.cuda.synchronize()
    assert np.isfinite(host(cov)).all()
    from compliancedex_amd import gpis_joint_cov
    assert gpis_joint_cov(st, X[:0]).shape == (0, 10)
    assert C.sizeof(N.CdxGpis) == C.sizeof(bad)


def test_pred_joint_and_normal_uncertainty():
    """Shapes follow ``pred``; mean4 is (mean, ∇mean) of the mean kernel bit for bit, cov the symmetric fill; the
    named tuple's fields against their definitions in numpy."""
    from compliancedex_amd import NormalUncertainty
    from compliancedex_amd.gpis import gpis_mean
    g, X1, E11, R = _gpis("tps", 257)
    X = _joint.queries(X1, 12, 9).reshape(3, 4, 3)
    mean4, cov = g.pred_joint(dev(X))
    assert mean4.shape == (3, 4, 4) and cov.shape == (3, 4, 4, 4) and mean4.dtype == cov.dtype == torch.float64
    assert not mean4.requires_grad and not cov.requires_grad
    m, gm, _ = gpis_mean(g.native_state(), dev(X.reshape(-1, 3)), want_grad=True)
    assert _rows.same_bits(host(mean4).reshape(-1, 4), np.concatenate([host(m)[:, None], host(gm)], 1))
    assert _rows.same_bits(host(cov).reshape(-1, 4, 4), _joint.full(_cov(g, X.reshape(-1, 3))))
    unc = g.normal_uncertainty(dev(X))
    assert isinstance(unc, NormalUncertainty)
    assert unc.normal.shape == (3, 4, 3) and unc.cov_normal.shape == (3, 4, 3, 3)
    assert unc.angle_std.shape == unc.offset_std.shape == (3, 4)
    gm, S = host(gm), host(cov).reshape(-1, 4, 4)
    nrm = np.linalg.norm(gm, axis=1)
    n = gm / nrm[:, None]
    P = np.eye(3) - n[:, :, None] * n[:, None, :]
    cn = P @ S[:, 1:, 1:] @ P / (nrm * nrm)[:, None, None]
    assert np.abs(host(unc.normal).reshape(-1, 3) - n).max() <= 1e-15
    assert np.abs(host(unc.cov_normal).reshape(-1, 3, 3) - cn).max() <= 1e-12 * np.abs(cn).max()
    assert np.abs(host(unc.angle_std).reshape(-1) - np.sqrt(np.trace(cn, axis1=1, axis2=2))).max() <= 1e-12
    assert np.abs(host(unc.offset_std).reshape(-1) - np.sqrt(S[:, 0, 0]) / nrm).max() <= 1e-15
    # compute_normal divides by ‖∇mean‖ + 1e-8 (gpis.py:63-87); the tuple's normal is the unit vector
    assert np.abs(host(g.compute_normal(dev(X))).reshape(-1, 3) - gm / (nrm + 1e-8)[:, None]).max() <= 1e-14
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.pred_joint(torch.zeros(2, 3, dtype=torch.float64))


def test_sample_joint_moments():
    """S = 20 000 draws with a seeded generator at 3 queries: every entry of the sample covariance within six standard
    errors of a Gaussian sample covariance, 6·sqrt((Σaa·Σbb + Σab²)/S), of Σ, the sample mean within six standard errors
    of mean4; sample_normals returns unit vectors and the offsets of the same draws; a seed gives the same draws."""
    g, X1, E11, R = _gpis("tps", 257)
    X = dev(_joint.queries(X1, 3, 11))
    S = 20_000
    gen = torch.Generator(device=DEV).manual_seed(1234)
    draws = g.sample_joint(X, S, generator=gen)
    assert draws.shape == (3, S, 4) and draws.dtype == torch.float64
    mean4, cov = (host(t) for t in g.pred_joint(X))
    d = host(draws)
    for q in range(3):
        sc = np.cov(d[q].T)
        se = np.sqrt((np.outer(np.diag(cov[q]), np.diag(cov[q])) + cov[q] ** 2) / S)
        assert (np.abs(sc - cov[q]) <= 6.0 * se).all(), (q, np.abs(sc - cov[q]) / se)
        assert (np.abs(d[q].mean(0) - mean4[q]) <= 6.0 * np.sqrt(np.diag(cov[q]) / S)).all(), q
    gen = torch.Generator(device=DEV).manual_seed(1234)
    normals, offsets = g.sample_normals(X, S, generator=gen)
    assert normals.shape == (3, S, 3) and offsets.shape == (3, S)
    assert np.abs(np.linalg.norm(host(normals), axis=-1) - 1.0).max() <= 1e-15
    gn = np.linalg.norm(d[..., 1:], axis=-1)
    assert _rows.same_bits(host(normals), host(draws[..., 1:] / draws[..., 1:].norm(dim=-1, keepdim=True)))
    assert np.abs(host(offsets) + d[..., 0] / gn).max() <= 1e-15


def test_zero_noise_returns_the_mean_normal(monkeypatch):
    from compliancedex_amd import gpis as G
    g, X1, E11, R = _gpis("joint", 63)
    X = dev(_joint.queries(X1, 5, 13))
    monkeypatch.setattr(G, "_standard_normal", lambda shape, device, generator: torch.zeros(shape, dtype=torch.float64, device=device))
    normals, offsets = g.sample_normals(X, 1)
    unc = g.normal_uncertainty(X)
    mean4, _ = g.pred_joint(X)
    assert _rows.same_bits(host(normals[:, 0]), host(unc.normal))
    assert _rows.same_bits(host(offsets[:, 0]), host(-mean4[:, 0] / mean4[:, 1:].norm(dim=-1)))


def test_shape_uncertainty_report(monkeypatch):
    """The closing grasps of tests/_equil.py on the sphere state, E = 5, T = 4, W = 6, S = 16: holds_mean is
    disturbance_report with compute_normal bit for bit; with the sampler's noise forced to zero hold_probability is 0 or
    1 and agrees with holds_mean; shapes and dtypes; the same seed gives the same report."""
    from compliancedex_amd import (DisturbanceReport, ShapeUncertaintyReport, disturbance_report, gravity_loads,
                                   shape_uncertainty_report)
    from compliancedex_amd import gpis as G
    g, X1, E11, R = _gpis("tps", 257)
    E, T, W, S = 5, 4, 6, 16
    contact, target, k = (dev(a) for a in _joint.closing_grasps(E))
    f, _ = gravity_loads(0.2, directions=W)
    mu = 1.0

    def run(seed):
        return shape_uncertainty_report(g, contact, target, k, mu, f, samples=S,
                                        generator=torch.Generator(device=DEV).manual_seed(seed))
    rep = run(3)
    assert isinstance(rep, ShapeUncertaintyReport) and isinstance(rep.mean, DisturbanceReport)
    assert rep.hold_probability.shape == (E,) and rep.hold_probability.dtype == torch.float64
    assert rep.holds_mean.shape == (E,) and rep.holds_mean.dtype == torch.bool
    assert rep.angle_std.shape == rep.offset_std.shape == (E, T) and rep.angle_std.dtype == torch.float64
    assert rep.samples.holds.shape == (E * S,) and rep.samples.result.margin.shape == (E * S, W, T)
    p = host(rep.hold_probability)
    assert ((p >= 0) & (p <= 1)).all() and np.array_equal(p * S, np.round(p * S))
    assert np.array_equal(p, host(rep.samples.holds).reshape(E, S).mean(1))
    ref = disturbance_report(contact, target, k, g.compute_normal(contact), mu, f)
    assert _rows.same_bits(host(rep.holds_mean), host(ref.holds))
    assert _rows.same_bits(host(rep.mean.result.margin), host(ref.result.margin))
    unc = g.normal_uncertainty(contact)
    assert _rows.same_bits(host(rep.angle_std), host(unc.angle_std)) and _rows.same_bits(host(rep.offset_std), host(unc.offset_std))
    again, other = run(3), run(4)
    assert _rows.same_bits(host(again.samples.result.margin), host(rep.samples.result.margin))
    assert _rows.same_bits(host(again.hold_probability), p)
    assert not _rows.same_bits(host(other.samples.result.margin), host(rep.samples.result.margin))
    print("shape uncertainty: holds_mean", host(rep.holds_mean).tolist(), "hold probability", p.tolist(),
          "angle std (rad)", np.round(host(rep.angle_std), 3).tolist())
    # per-grasp loads and a centre of mass pass through to both runs
    fe = dev(np.tile(f, (E, 1, 1)))
    com = dev(np.tile([0.001, 0.0, -0.002], (E, 1)))
    per = shape_uncertainty_report(g, contact, target, k, mu, fe, samples=S, com=com, max_shift=0.01,
                                   generator=torch.Generator(device=DEV).manual_seed(3))
    ref = disturbance_report(contact, target, k, g.compute_normal(contact), mu, fe, com=com, max_shift=0.01)
    assert _rows.same_bits(host(per.holds_mean), host(ref.holds)) and per.samples.holds.shape == (E * S,)
    monkeypatch.setattr(G, "_standard_normal", lambda shape, device, generator: torch.zeros(shape, dtype=torch.float64, device=device))
    quiet = shape_uncertainty_report(g, contact, target, k, mu, f, samples=S)
    q = host(quiet.hold_probability)
    assert np.isin(q, (0.0, 1.0)).all() and np.array_equal(q == 1.0, host(quiet.holds_mean))
    assert _rows.same_bits(host(quiet.holds_mean), host(rep.holds_mean))
    with pytest.raises(ValueError):
        shape_uncertainty_report(g, contact, target, k, mu, f, samples=0)
