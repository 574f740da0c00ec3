"""The disturbance-load test's rule (csrc/cdx_equil.h) on the host build: the certificate recomputed from the outputs
alone, the closed forms, one iteration and the whole solve against the numpy statement, independence of items, the
statuses, the reduction against its numpy statement, the argument checks, and the host-side pieces of
compliancedex_amd.stability.  CPU only; tests/test_gpu_equil.py holds the device to the same assertions."""
import ctypes as C

import numpy as np
import pytest

from tests import _equil as Q
from tests._host import host, p


def test_certificate_from_the_outputs_alone():
    Q.check_certificate(Q.solve_host, report="host build")
    Q.check_certificate(Q.np_equil, report="numpy statement")  # the statement says the same: every item status 0


def test_closed_form_tetrahedron():
    seen = Q.closed_a_error(Q.np_equil)
    got = Q.closed_a_error(Q.solve_host)
    print("tetrahedron: numpy statement", seen, "host build", got, "allowed", Q.CLOSED_A_TOL)
    assert seen <= Q.CLOSED_A_SEEN * 1.5  # (the figure the tolerance was taken from still stands)
    assert got <= Q.CLOSED_A_TOL


def test_closed_form_weighted_kabsch():
    seen = Q.closed_b_error(Q.np_equil, "numpy statement")
    got = Q.closed_b_error(Q.solve_host, "host build")
    print("Kabsch: numpy statement", seen, "host build", got, "allowed", Q.CLOSED_B_TOL)
    assert seen <= Q.CLOSED_B_SEEN * 1.5
    assert got <= Q.CLOSED_B_TOL


def test_one_iteration_against_numpy():
    Q.check_one_iteration(Q.solve_host, report="host build to numpy, one iteration:")
    worst = Q.one_iteration_error(Q.solve_host)
    # the written figures are the measured ones, not a bound chosen after the fact: none is off by more than 4×
    for name, v in worst.items():
        assert v <= 4 * Q.ONE_ITER_SEEN[name], (name, v)


def test_converged_against_numpy():
    Q.check_converged_against_numpy(Q.solve_host)


def test_exact_hessian_is_the_derivative_of_the_gradient():
    """The numpy statement's Hessian (the one both builds are held to in one iteration) against central differences of
    U along Cayley steps: the second-order terms are there and have the right sign."""
    pts, tgt, k, nrm = Q.family("deep", 1, 4)
    f, c = Q.loads(pts, k, 1, 3.0)
    o = Q.centre(pts, k)[0]
    P, G, Cv, ff = pts[0] - o, tgt[0] - o, c[0, 0] - o, f[0, 0]

    def U(d):
        a = 0.5 * d[:3]
        s = a @ a
        R = ((1 - s) * np.eye(3) + 2 * np.outer(a, a) + 2 * Q.skew(a[None])[0]) / (1 + s)
        x = P @ R.T + d[3:]
        return 0.5 * (k[0] * ((x - G) ** 2).sum(-1)).sum() - ff @ (R @ Cv + d[3:])
    h = 1e-4
    H = np.zeros((6, 6))
    for i in range(6):
        for j in range(6):
            ei, ej = np.eye(6)[i] * h, np.eye(6)[j] * h
            H[i, j] = (U(ei + ej) - U(ei - ej) - U(ej - ei) + U(-ei - ej)) / (4 * h * h)
    a, r = P, P - G
    ww = sum(kk * ((ai @ ai - ai @ ri) * np.eye(3) - np.outer(ai, ai) + 0.5 * (np.outer(ai, ri) + np.outer(ri, ai)))
             for kk, ai, ri in zip(k[0], a, r))
    ww = ww - (0.5 * (np.outer(Cv, ff) + np.outer(ff, Cv)) - (Cv @ ff) * np.eye(3))
    S = Q.skew((k[0][:, None] * a).sum(0)[None])[0]
    want = np.block([[ww, S], [-S, k[0].sum() * np.eye(3)]])
    # block by block: the ωω entries are 1e-3 of the vv ones, and the cross block Σ k·a vanishes about the stiffness centre
    assert np.abs(H[:3, :3] - want[:3, :3]).max() <= 1e-5 * np.abs(want[:3, :3]).max()
    assert np.abs(H[3:, 3:] - want[3:, 3:]).max() <= 1e-5 * np.abs(want[3:, 3:]).max()
    assert np.abs(H[:3, 3:] - want[:3, 3:]).max() <= 1e-6 and np.abs(want[:3, 3:]).max() <= 1e-12
    gn = want.copy()
    gn[:3, :3] = sum(kk * ((ai @ ai) * np.eye(3) - np.outer(ai, ai)) for kk, ai in zip(k[0], a))
    assert np.abs(H - gn).max() >= 1e-2 * np.abs(want[:3, :3]).max()  # (Gauss–Newton alone is not this matrix)


def test_deep_family_wanders():
    """What makes the "deep" family worth comparing bit for bit: some of its items need many more iterations than the
    3 … 4 of a direct descent — trials rejected and the damping raised on the way (the device has the same counts:
    tests/test_gpu_equil.py compares them bit for bit)."""
    pts, tgt, k, nrm = Q.family("deep", 5, 3)
    f, c = Q.loads(pts, k, 64, (0.0, 4.0))
    it = Q.solve_host(pts, tgt, k, nrm, f, c)["iters"]
    assert np.median(it) <= 5 and it.max() >= 12


def test_no_stall_at_the_default_tolerance():
    Q.check_no_stall(Q.solve_host)
    Q.check_no_stall(Q.np_equil)


def test_independence():
    Q.check_independence(Q.solve_host)


def test_statuses():
    Q.check_statuses(Q.solve_host)
    Q.check_statuses(Q.np_equil)


def test_reduction():
    Q.check_reduction(Q.reduce_host)


def test_reduction_of_a_real_solve():
    E, W, T = 7, 26, 4
    pts, tgt, k, nrm = Q.family("firm", E, T)
    f, c = Q.loads(pts, k, W, (0.1, 4.0))
    out = Q.solve_host(pts, tgt, k, nrm, f, c)
    red, ref = Q.reduce_host(out, E, W, T), Q.np_reduce(out, E, W, T)
    for name in Q.RED_FIELDS:
        assert Q.same_bits(red[name], ref[name]), name
    assert 0 < red["n_failed"].sum() < E * W  # (the loads were chosen so that both verdicts occur)


def test_bad_arguments_host():
    lib = host()
    E, W, T = 2, 3, 4
    pts, tgt, k, nrm = (x.copy() for x in Q.family("shallow", E, T))
    f, c = Q.loads(pts, k, W, 1.0)
    out = Q.outputs(E * W, T)
    ins = [pts, tgt, k, nrm, f, c]

    def call(par, E=E, W=W, drop_in=None, drop_out=None):
        a = [None if i == drop_in else p(x) for i, x in enumerate(ins)]
        o = [None if n == drop_out else p(out[n]) for n in Q.FIELDS]
        return lib.cdxh_grasp_equilibrium(C.byref(par) if par is not None else None, E, W, *a, 0, *o)
    assert call(None) == -1 and call(Q.params(T), E=-1) == -1 and call(Q.params(T), W=-1) == -1
    for i in range(6):
        assert call(Q.params(T), drop_in=i) == -1, i
    for n in Q.FIELDS[3:]:
        assert call(Q.params(T), drop_out=n) == -1, n
    for bad in (dict(T=0), dict(T=9), dict(mu=0.0), dict(mu=float("nan")), dict(tol=0.0), dict(tol=float("inf")),
                dict(max_iters=-1), dict(mu0=0.0), dict(mu_min=-1.0), dict(mu_max=float("nan")), dict(nu=0.0)):
        assert call(Q.params(**{"T": T, **bad})) == -1, bad
    assert call(Q.params(T), E=0, drop_in=0) == 0 and call(Q.params(T), W=0, drop_in=4) == 0
    assert call(Q.params(T), E=1 << 40, W=1 << 40) == -1
    for n, v in Q.outputs(E * W, T).items():
        assert Q.same_bits(out[n], v), n  # nothing was written
    for n in Q.FIELDS[:3]:  # rot, trans, force are optional
        assert call(Q.params(T), drop_out=n) == 0
    lm = Q.limits()
    red = Q.reduce_outputs(E)
    items = [out[n] for n in ("margin", "normal_force", "shift", "chord", "stable", "status")]

    def reduce(lim=lm, E=E, W=W, T=T, drop=None):
        a = [None if i == drop else p(x) for i, x in enumerate(items + [red[n] for n in Q.RED_FIELDS])]
        return lib.cdxh_equil_reduce(C.byref(lim) if lim is not None else None, E, W, T, *a)
    assert reduce(None) == -1 and reduce(E=-1) == -1 and reduce(W=-1) == -1 and reduce(T=0) == -1 and reduce(T=9) == -1
    for i in range(13):
        assert reduce(drop=i) == -1, i
    assert reduce(E=0, drop=0) == 0 and reduce(W=0, drop=0) == 0
    for n, v in Q.reduce_outputs(E).items():
        assert Q.same_bits(red[n], v), n
    assert reduce() == 0


def test_load_directions():
    from compliancedex_amd.stability import load_directions
    for n in (6, 14, 26, 1, 7, 40):
        d = load_directions(n)
        assert d.shape == (n, 3) and d.dtype == np.float64
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-15
        gram = d @ d.T - 2.0 * np.eye(n)
        assert gram.max() < 1.0 - 1e-6, n  # distinct
    assert sorted(map(tuple, load_directions(6).tolist())) == sorted(
        [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)])
    d = load_directions(26)
    assert np.abs(d.sum(0)).max() <= 1e-14 and np.abs(load_directions(40).sum(0)).max() <= 0.1
    assert any(np.allclose(r, (0.0, 0.0, -1.0)) for r in d)  # gravity with the hand upright is among them
    with pytest.raises(ValueError):
        load_directions(0)


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from compliancedex_amd import disturbance_report, grasp_equilibrium, gravity_loads, max_payload
    pts, tgt, k, nrm = (torch.from_numpy(x.copy()) for x in Q.family("shallow", 2, 4))
    f = torch.zeros(3, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        grasp_equilibrium(pts, tgt, k, nrm, 1.0, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        disturbance_report(pts, tgt, k, nrm, 1.0, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        max_payload(pts, tgt, k, nrm, 1.0, hi=5.0)
    with pytest.raises(ValueError):
        gravity_loads(-1.0)
    force, point = gravity_loads(0.4, directions=14)
    assert force.shape == (14, 3) and point is None
    assert np.abs(np.linalg.norm(force, axis=1) - 0.4 * 9.81).max() <= 1e-14
