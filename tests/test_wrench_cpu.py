"""The minimum-wrench rule (csrc/cdx_wrench.h) on the host build: the numpy statements themselves, the duality-gap
certificate with no row allowed to miss, the closed forms, status 1 and 2, the gradient, the independence of rows and
the argument checks.  CPU only; tests/test_gpu_wrench.py asserts the same on the device."""
import ctypes as C

import numpy as np
import pytest

from tests import _host, _wrench as W
from tests._wrench import same_bits

solve = W.solve_host


def test_numpy_projection_is_the_projection():
    """The yardstick itself: P_C(v) is feasible, idempotent, and no feasible point is nearer to v (the variational
    inequality (v − P)·(w − P) ≤ 0 for feasible w)."""
    g = np.random.default_rng(0)
    for mu, fmin in ((1.0, 5.0), (0.3, 1.0), (0.5, 0.0)):
        nh = W.unit(g.normal(size=(4000, 3)))
        v = g.normal(scale=8.0, size=(4000, 3))
        P = W.np_project(v, nh, mu, fmin)
        W.check_feasible(P[:, None], nh[:, None], mu, fmin)
        assert np.abs(W.np_project(P, nh, mu, fmin) - P).max() <= 1e-12
        w = W.np_project(g.normal(scale=8.0, size=(4000, 3)), nh, mu, fmin)
        assert (((v - P) * (w - P)).sum(-1) <= 1e-10).all()


def test_dual_value_is_a_lower_bound():
    """Weak duality on arbitrary pairs: D(y) ≤ P(F) for any y in the balls and any feasible F."""
    g = np.random.default_rng(1)
    tips, normals = W.family("B")
    for _ in range(4):
        y = g.normal(size=(len(tips), 6))
        y[:, :3] *= 0.5 * g.random((len(tips), 1)) / np.linalg.norm(y[:, :3], axis=-1, keepdims=True)
        y[:, 3:] *= 0.5 * g.random((len(tips), 1)) / np.linalg.norm(y[:, 3:], axis=-1, keepdims=True)
        F = W.np_project(g.normal(scale=8.0, size=tips.shape), W.unit(normals), W.MU, W.FMIN)
        assert (W.np_dual(y, tips, normals, W.MU, W.FMIN, W.REG) <= W.np_primal(F, tips, W.REG) + 1e-12).all()


@pytest.mark.parametrize("name,T,kw", W.CERT_CASES, ids=[f"{n}{t}{'-'.join(map(str, k.values()))}" for n, t, k in W.CERT_CASES])
def test_certificate_every_row(name, T, kw):
    W.run_cert_case(solve, name, T, kw)


def test_closed_forms():
    W.check_closed_forms(solve)


def test_status_one():
    W.check_status_one(solve)


def test_gradient():
    W.check_gradient(solve)


def test_grad_is_optional():
    tips, normals = W.family("A")
    out = W.outputs(len(tips), 4)
    fn = _host.host().cdxh_min_wrench
    par = W.params()
    args = [_host.p(out[k]) for k in W.FIELDS[:-1]]
    assert fn(C.byref(par), len(tips), _host.p(tips), _host.p(normals), *args, None) == 0
    ref = solve(tips, normals)
    for k in W.FIELDS[:-1]:
        assert same_bits(out[k], ref[k]), k


def test_rows_do_not_depend_on_the_batch():
    tips, normals = W.family("E")
    full = solve(tips, normals)
    for E in (1, 17, 64):
        part = solve(tips[:E], normals[:E])
        for k in W.FIELDS:
            assert same_bits(part[k], full[k][:E]), (E, k)


def test_bad_rows_stay_in_their_row():
    W.check_bad_rows(solve)


def test_argument_errors():
    tips, normals = W.family("A")
    E = len(tips)
    fn = _host.host().cdxh_min_wrench
    out = W.outputs(E, 4)
    p = _host.p

    def call(par, E=E, tips_p=p(tips), drop=None):
        args = [None if k == drop else p(out[k]) for k in W.FIELDS]
        return fn(C.byref(par) if par is not None else None, E, tips_p, p(normals), *args)

    assert call(None) == -1
    assert call(W.params(), E=-1) == -1
    assert call(W.params(), tips_p=None) == -1
    for k in W.FIELDS[:-1]:
        assert call(W.params(), drop=k) == -1, k
    for bad in (dict(T=0), dict(T=9), dict(mu=0.0), dict(mu=-1.0), dict(mu=float("nan")), dict(min_force=-1.0),
                dict(reg=0.0), dict(rho=0.0), dict(rho=float("inf")), dict(tol=0.0), dict(max_iters=-1),
                dict(check_every=0)):
        assert call(W.params(**bad)) == -1, bad
    for k, v in W.outputs(E, 4).items():
        assert same_bits(out[k], v), k  # nothing was written
    assert call(W.params(), E=0, tips_p=None) == 0
    assert call(W.params()) == 0


def test_product_library_checks_without_a_launch():
    """The gfx950 library's entry refuses bad arguments before any launch (so this runs without a GPU), its struct
    matches the binding, and the Python entry refuses CPU tensors."""
    import torch
    from compliancedex_amd import _native as N, min_wrench
    lib = N.load()
    assert lib.cdx_wrench_abi_size() == C.sizeof(N.CdxWrenchParams)
    assert [lib.cdx_wrench_rows_per_block(T) for T in (0, 1, 4, 5, 8, 9)] == [0, 64, 64, 32, 32, 0]
    one = 8  # (any non-null address: nothing is dereferenced before the checks)
    assert lib.cdx_min_wrench(None, 4, *[one] * 11, None) == -1
    for bad in (dict(T=0), dict(T=9), dict(mu=0.0), dict(min_force=-1.0), dict(reg=0.0), dict(rho=-1.0),
                dict(tol=float("nan")), dict(max_iters=-1), dict(check_every=0)):
        assert lib.cdx_min_wrench(C.byref(W.params(**bad)), 4, *[one] * 11, None) == -1, bad
    assert lib.cdx_min_wrench(C.byref(W.params()), -1, *[one] * 11, None) == -1
    assert lib.cdx_min_wrench(C.byref(W.params()), 4, None, *[one] * 10, None) == -1
    assert lib.cdx_min_wrench(C.byref(W.params()), 0, *[None] * 11, None) == 0
    tips, normals = W.family("A")
    with pytest.raises(RuntimeError, match="no CPU path"):
        min_wrench(torch.from_numpy(tips), torch.from_numpy(normals), 1.0)
