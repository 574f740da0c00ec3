"""Test helpers of the minimum-wrench solve (csrc/cdx_wrench.h): a ctypes wrapper of the host build's entry, the numpy
statement of the cone projection, of the primal and dual values and of the gradient, the input families and the checks
shared by the host file (tests/test_wrench_cpu.py) and the device file (tests/test_gpu_wrench.py)."""
import ctypes as C
import functools

import numpy as np

from compliancedex_amd._native import CdxWrenchParams
from tests._host import host, p

MU, FMIN, REG, TOL, RHO, MAX_ITERS, CHECK_EVERY = 1.0, 5.0, 1e-2, 1e-9, 0.05, 2000, 10
FIELDS = ("forces", "wrench", "margin", "dual", "gap", "iters", "status", "grad")


def params(T=4, mu=MU, min_force=FMIN, reg=REG, rho=RHO, tol=TOL, max_iters=MAX_ITERS, check_every=CHECK_EVERY):
    q = CdxWrenchParams()
    q.n_tips, q.max_iters, q.check_every = int(T), int(max_iters), int(check_every)
    q.mu, q.min_force, q.reg, q.rho, q.tol = float(mu), float(min_force), float(reg), float(rho), float(tol)
    return q


def outputs(E, T, fill=-7.0):
    """Preset output arrays of E rows."""
    return dict(forces=np.full((E, T, 3), fill), wrench=np.full(E, fill), margin=np.full((E, T), fill),
                dual=np.full((E, 6), fill), gap=np.full(E, fill), iters=np.full(E, -7, np.int32),
                status=np.full(E, -7, np.int32), grad=np.full((E, T, 3), fill))


def solve_host(tips, normals, **kw):
    """cdxh_min_wrench on host arrays [E, T, 3] → dict of FIELDS."""
    tips, normals = np.ascontiguousarray(tips, np.float64), np.ascontiguousarray(normals, np.float64)
    E, T = tips.shape[:2]
    out = outputs(E, T)
    par = params(T, **kw)
    rc = host().cdxh_min_wrench(C.byref(par), E, p(tips), p(normals), *[p(out[k]) for k in FIELDS])
    assert rc == 0, rc
    return out


# ------------------------------------------------------------------ numpy statement
def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def np_project(v, nh, mu, fmin):
    """P_C of the forces v [..., 3] for unit normals nh: with v = −(a·nh + t), (a, t) onto the cone ‖t‖ ≤ mu·a, and if
    that lands below a = fmin, a = fmin with the original t clipped to the radius mu·fmin."""
    a = -(v * nh).sum(-1)
    t = -v - a[..., None] * nh
    tn = np.linalg.norm(t, axis=-1)
    inside = tn <= mu * a
    apex = ~inside & (mu * tn <= -a)
    safe = np.where(tn > 0, tn, 1.0)
    ab = (mu * tn + a) / (1.0 + mu * mu)
    a2 = np.where(inside, a, np.where(apex, 0.0, ab))
    sc = np.where(inside, 1.0, np.where(apex, 0.0, mu * ab / safe))
    low = ~(a2 >= fmin)
    rad = mu * fmin
    a2 = np.where(low, fmin, a2)
    sc = np.where(low, np.where(tn > rad, rad / safe, 1.0), sc)
    return -(a2[..., None] * nh + sc[..., None] * t)


def centred(tips):
    return tips - tips.mean(axis=1, keepdims=True)


def np_primal(F, tips, reg):
    r = centred(tips)
    return (0.5 * np.linalg.norm(F.sum(1), axis=-1) + 0.5 * np.linalg.norm(np.cross(r, F).sum(1), axis=-1) +
            0.5 * reg * (F * F).sum((1, 2)))


def np_dual(y, tips, normals, mu, fmin, reg):
    r, nh = centred(tips), unit(normals)
    g = y[:, None, :3] + np.cross(y[:, None, 3:], r)
    x = np_project(-g / reg, nh, mu, fmin)
    return (0.5 * reg * (x * x).sum(-1) + (g * x).sum(-1)).sum(1)


def np_wrench(F, tips):
    return np.linalg.norm(F.sum(1), axis=-1) + np.linalg.norm(np.cross(centred(tips), F).sum(1), axis=-1)


def np_margin(F, normals, mu):
    return (-unit(F) * unit(normals)).sum(-1) - 1.0 / np.sqrt(1.0 + mu * mu)


def np_torque(F, tips):
    return np.cross(centred(tips), F).sum(1)


def np_grad(F, tips):
    """∂‖Σ r×F‖/∂tips with F held constant: F_j × τ̂ − mean_i(F_i × τ̂); 0 where ‖τ‖ = 0."""
    tau = np_torque(F, tips)
    tn = np.linalg.norm(tau, axis=-1, keepdims=True)
    th = np.where(tn > 0, tau / np.where(tn > 0, tn, 1.0), 0.0)
    c = np.cross(F, th[:, None, :])
    return c - c.mean(axis=1, keepdims=True)


# ------------------------------------------------------------------ inputs
def inst(seed, B, T=4, noise=0.0, random_normals=False):
    g = np.random.default_rng(seed)
    pts = g.normal(size=(B, T, 3))
    pts /= np.linalg.norm(pts, axis=-1, keepdims=True)
    pts = pts * g.uniform(0.02, 0.08, (B, T, 1))
    pts = pts + g.normal(scale=0.05, size=(B, 1, 3))
    if random_normals:
        n = unit(g.normal(size=(B, T, 3)))
    else:
        n = unit(pts - pts.mean(axis=1, keepdims=True))
        n = unit(n + noise * g.normal(size=(B, T, 3)))
    return pts, n


@functools.lru_cache(None)
def family(name, T=4):
    if name == "A":
        return inst(0, 128, noise=0.1)
    if name == "B":
        return inst(1, 128, noise=0.5)
    if name == "C":
        return inst(2, 64, T, noise=0.3)
    if name == "D":
        return inst(3, 128, random_normals=True)
    if name == "E":
        return inst(4, 257, noise=0.3)
    raise KeyError(name)


# (family, T, solver options): every case of check 1
CERT_CASES = [("A", 4, {}), ("B", 4, {}), ("C", 2, {}), ("C", 3, {}), ("C", 5, {}), ("C", 8, {}), ("D", 4, {}),
              ("E", 4, {}), ("A", 4, dict(mu=0.5, min_force=1.0)), ("B", 4, dict(mu=0.3))]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ shared checks; solve(tips, normals, **kw) → dict
def check_feasible(F, normals, mu=MU, min_force=FMIN):
    nh = unit(normals)
    fn = np.linalg.norm(F, axis=-1)
    allow = 1e-12 * np.maximum(1.0, fn)
    nf = (nh * F).sum(-1)
    assert (nf <= -min_force + allow).all(), float((nf + min_force - allow).max())
    assert (nf <= -fn / np.sqrt(1.0 + mu * mu) + allow).all()


def check_certificate(out, tips, normals, mu=MU, min_force=FMIN, reg=REG, tol=TOL, report=None):
    """Check 1: every row certified, recomputed in numpy from the returned forces and dual."""
    assert (out["status"] == 0).all(), (np.flatnonzero(out["status"] != 0), out["iters"].max())
    F, y = out["forces"], out["dual"]
    check_feasible(F, normals, mu, min_force)
    assert (np.linalg.norm(y[:, :3], axis=-1) <= 0.5 + 1e-15).all()
    assert (np.linalg.norm(y[:, 3:], axis=-1) <= 0.5 + 1e-15).all()
    P, D = np_primal(F, tips, reg), np_dual(y, tips, normals, mu, min_force, reg)
    scale = np.maximum(1.0, np.abs(P))
    if report is not None:
        print(report, "iters median / max", int(np.median(out["iters"])), int(out["iters"].max()), "worst gap / scale",
              float(((P - D) / scale).max()))
    assert (P - D <= tol * scale + 1e-12 * scale).all(), float(((P - D) / scale).max())
    w, mg = np_wrench(F, tips), np_margin(F, normals, mu)
    assert (np.abs(out["wrench"] - w) <= 1e-12 * np.maximum(1.0, np.abs(w))).all()
    assert (np.abs(out["margin"] - mg) <= 1e-12).all()
    assert (np.abs(out["gap"] - (P - D)) <= 1e-12 * scale).all()
    assert (out["iters"] >= 0).all() and (out["iters"] <= MAX_ITERS).all()


def run_cert_case(solve, name, T, kw):
    tips, normals = family(name, T)
    out = solve(tips, normals, **kw)
    check_certificate(out, tips, normals, kw.get("mu", MU), kw.get("min_force", FMIN), report=(name, T, kw))
    return out


def tetrahedron():
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)
    return (0.05 * v + np.array([0.02, -0.01, 0.3]))[None], v[None].copy()


def check_closed_forms(solve):
    """Check 2, to 1e-9 absolute."""
    c = 1.0 / np.sqrt(1.0 + MU * MU)
    for reg in (1e-2, 1e-3):
        tips, n = tetrahedron()
        out = solve(tips, n, reg=reg)
        assert (out["status"] == 0).all()
        assert np.abs(out["forces"] + FMIN * n).max() <= 1e-9
        assert out["wrench"][0] <= 1e-9
        assert np.abs(out["margin"] - (1.0 - c)).max() <= 1e-9
        g = np.random.default_rng(7)
        for T in (2, 4, 7):
            tips = g.normal(scale=0.05, size=(3, T, 3))
            n = np.zeros((3, T, 3))
            n[..., 2] = np.array([1.0, 2.5, 0.3])[:, None]  # (not unit: the rule normalises)
            out = solve(tips, n, reg=reg)
            assert (out["status"] == 0).all(), out["iters"]
            assert np.abs(out["forces"] + FMIN * unit(n)).max() <= 1e-9
            assert np.abs(out["wrench"] - T * FMIN).max() <= 1e-9
    g = np.random.default_rng(8)
    tips, n = g.normal(scale=0.05, size=(9, 1, 3)), unit(g.normal(size=(9, 1, 3)))
    out = solve(tips, n)
    assert (out["status"] == 0).all()
    assert np.abs(out["forces"] + FMIN * n).max() <= 1e-9
    assert np.abs(out["wrench"] - FMIN).max() <= 1e-9


def check_status_one(solve):
    """Check 5: D with max_iters = 20."""
    tips, normals = family("D")
    out = solve(tips, normals, max_iters=20)
    early = out["status"] == 1
    assert early.any() and np.isin(out["status"], (0, 1)).all()
    assert (out["iters"][early] == 20).all()
    for k in ("forces", "wrench", "margin", "dual", "gap", "grad"):
        assert np.isfinite(out[k][early]).all(), k
    check_feasible(out["forces"][early], normals[early])
    P = np_primal(out["forces"], tips, REG)
    D = np_dual(out["dual"], tips, normals, MU, FMIN, REG)
    assert (np.abs(out["gap"] - (P - D)) <= 1e-12 * np.maximum(1.0, np.abs(P))).all()
    assert (out["gap"][early] > TOL * np.maximum(1.0, np.abs(P[early]))).all()
    zero = solve(tips, normals, max_iters=0)
    assert (zero["iters"] == 0).all() and (zero["status"] == 1).all()
    assert np.abs(zero["forces"] + FMIN * normals).max() <= 1e-14


def check_gradient(solve):
    """Check 6, the kernel's grad_tips: the numpy formula to 1e-12 on B, and central differences of ‖Σ r×F‖ with F
    frozen (h = 1e-6) to 1e-6 on rows with ‖τ‖ > 1e-3."""
    tips, normals = family("B")
    out = solve(tips, normals)
    F = out["forces"]
    assert np.abs(out["grad"] - np_grad(F, tips)).max() <= 1e-12
    rows = np.linalg.norm(np_torque(F, tips), axis=-1) > 1e-3
    assert rows.sum() >= 8
    h = 1e-6
    fd = np.zeros_like(tips)
    for j in range(tips.shape[1]):
        for k in range(3):
            d = np.zeros_like(tips)
            d[:, j, k] = h
            fd[:, j, k] = (np.linalg.norm(np_torque(F, tips + d), axis=-1) -
                           np.linalg.norm(np_torque(F, tips - d), axis=-1)) / (2 * h)
    assert np.abs(out["grad"][rows] - fd[rows]).max() <= 1e-6
    return out


def bad_rows_case(group):
    """Family E rows with bad ones first, last and on both sides of a workgroup boundary."""
    tips, normals = family("E")
    E = min(2 * group + 5, len(tips))
    tips, normals = tips[:E].copy(), normals[:E].copy()
    bad = sorted({0, group - 1, group, E - 1} & set(range(E)))
    tb, nb = tips.copy(), normals.copy()
    kinds = [("tip", np.nan), ("normal", np.inf), ("zero", 0.0), ("normal", np.nan)]
    for row, (kind, val) in zip(bad, kinds):
        if kind == "tip":
            tb[row, 1, 2] = val
        elif kind == "zero":
            nb[row, 2] = 0.0
        else:
            nb[row, 0, 1] = val
    return tips, normals, tb, nb, bad


def check_bad_rows(solve, group=16):
    tips, normals, tb, nb, bad = bad_rows_case(group)
    E = len(tips)
    clean = solve(tips, normals)
    out = solve(tb, nb)
    good = np.setdiff1d(np.arange(E), bad)
    assert (out["status"][bad] == 2).all() and (out["iters"][bad] == 0).all()
    for k in ("forces", "wrench", "margin", "dual", "gap", "grad"):
        assert np.isnan(out[k][bad]).all(), k
    for k in FIELDS:
        assert same_bits(out[k][good], clean[k][good]), k
    assert (clean["status"] == 0).all()
