"""Test helpers of the disturbance-load test (csrc/cdx_equil.h): ctypes wrappers of the host build's two entries, the
numpy statement of the rule and of its reduction, the input families and the checks shared by the host file
(tests/test_equil_cpu.py) and the device file (tests/test_gpu_equil.py).

Every solve returns item-major arrays: item e·W + w of E rows and W loads is entry e·W + w of each field."""
import ctypes as C
import functools

import numpy as np

from compliancedex_amd._native import CdxEquilLimits, CdxEquilParams
from tests._host import host, p

MU, TOL, MAX_ITERS = 1.0, 1e-8, 60
LM = dict(mu0=1e-3, mu_min=1e-9, mu_max=1e6, nu=10.0)
FIELDS = ("rot", "trans", "force", "normal_force", "margin", "shift", "chord", "stable", "iters", "status")
FLOATS = FIELDS[:7]
RED_FIELDS = ("worst_margin", "worst_load", "worst_tip", "max_shift", "max_chord", "n_failed", "holds")
LIMITS = dict(margin_min=0.0, min_normal_force=0.0, max_shift=0.02, max_chord=0.35)

# Tolerances that the issue ties to a CPU measurement.  Each is the stated multiple of the figure measured with the
# host build and the numpy statement below on the CPU; tests/test_equil_cpu.py prints the figures again.
# 2(a): 16 × the worst difference of the numpy statement from R = I, t = f/K over closed_a_cases() (measured 3.1e-15).
# 2(b): 16 × the worst difference of the numpy statement from the stiffness-weighted Kabsch fit on family "shallow",
#       T = 3 … 8, 24 rows each, in any entry of rot or trans: measured 1.07e-6 (at T = 3; 1.3e-8 at T = 4, ≤ 1.2e-9
#       beyond) — what the stop test at tol = 1e-8 leaves of a torque on three contacts.
# 3:    64 × the largest host-build-to-numpy difference after one iteration over ONE_ITER_CASES, per field.
CLOSED_A_SEEN, CLOSED_B_SEEN = 3.1e-15, 1.07e-6
CLOSED_A_TOL, CLOSED_B_TOL = 16 * CLOSED_A_SEEN, 16 * CLOSED_B_SEEN
ONE_ITER_SEEN = dict(rot=4.8e-15, trans=1.6e-16, force=1.5e-14, normal_force=7.1e-15, margin=3.7e-15, shift=5.2e-18,
                     chord=6.1e-15)
ONE_ITER_TOL = {k: 64 * v for k, v in ONE_ITER_SEEN.items()}


def params(T=4, mu=MU, tol=TOL, max_iters=MAX_ITERS, **lm):
    q = CdxEquilParams()
    q.n_tips, q.max_iters, q.mu, q.tol = int(T), int(max_iters), float(mu), float(tol)
    lm = {**LM, **lm}
    q.mu0, q.mu_min, q.mu_max, q.nu = (float(lm[k]) for k in ("mu0", "mu_min", "mu_max", "nu"))
    return q


def limits(**kw):
    q = CdxEquilLimits()
    for k, v in {**LIMITS, **kw}.items():
        setattr(q, k, float(v))
    return q


def outputs(N, T, fill=-7.0):
    """Preset output arrays of N items."""
    return dict(rot=np.full((N, 9), fill), trans=np.full((N, 3), fill), force=np.full((N, T, 3), fill),
                normal_force=np.full((N, T), fill), margin=np.full((N, T), fill), shift=np.full(N, fill),
                chord=np.full(N, fill), stable=np.full(N, 7, np.uint8), iters=np.full(N, -7, np.int32),
                status=np.full(N, -7, np.int32))


def reduce_outputs(E, fill=-7.0):
    return dict(worst_margin=np.full(E, fill), worst_load=np.full(E, -7, np.int32), worst_tip=np.full(E, -7, np.int32),
                max_shift=np.full(E, fill), max_chord=np.full(E, fill), n_failed=np.full(E, -7, np.int32),
                holds=np.full(E, 7, np.uint8))


def as_inputs(contact, target, k, normal, f, c):
    """Contiguous float64 copies, E, W, T and whether the loads are one [W, 3] set for every row."""
    a = [np.ascontiguousarray(x, np.float64) for x in (contact, target, k, normal, f, c)]
    E, T = a[2].shape
    shared = a[4].ndim == 2
    W = a[4].shape[0] if shared else a[4].shape[1]
    assert a[4].shape == a[5].shape == ((W, 3) if shared else (E, W, 3))
    return a, E, W, T, shared


def solve_host(contact, target, k, normal, f, c, **kw):
    """cdxh_grasp_equilibrium on host arrays → dict of FIELDS, item-major."""
    a, E, W, T, shared = as_inputs(contact, target, k, normal, f, c)
    out = outputs(E * W, T)
    par = params(T, **kw)
    rc = host().cdxh_grasp_equilibrium(C.byref(par), E, W, *[p(x) for x in a], int(shared), *[p(out[n]) for n in FIELDS])
    assert rc == 0, rc
    return out


def reduce_host(out, E, W, T, **lim):
    """cdxh_equil_reduce on the item-major outputs of a solve → dict of RED_FIELDS."""
    red = reduce_outputs(E)
    lm = limits(**lim)
    ins = [np.ascontiguousarray(out[n]) for n in ("margin", "normal_force", "shift", "chord", "stable", "status")]
    rc = host().cdxh_equil_reduce(C.byref(lm), E, W, T, *[p(x) for x in ins], *[p(red[n]) for n in RED_FIELDS])
    assert rc == 0, rc
    return red


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ numpy statement
def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def norm(v):
    return np.linalg.norm(v, axis=-1)


def skew(s):
    z = np.zeros(len(s))
    return np.stack([np.stack([z, -s[:, 2], s[:, 1]], -1), np.stack([s[:, 2], z, -s[:, 0]], -1),
                     np.stack([-s[:, 1], s[:, 0], z], -1)], 1)


def np_cholesky(A):
    """Lower factors [M, 6, 6] of the symmetric A [M, 6, 6] and, per matrix, whether all six pivots were > 0."""
    L = np.zeros_like(A)
    pd = np.ones(len(A), bool)
    for a in range(6):
        for b in range(a + 1):
            s = A[:, a, b] - (L[:, a, :b] * L[:, b, :b]).sum(-1)
            if a == b:
                pd &= s > 0
                L[:, a, a] = np.sqrt(s)
            else:
                L[:, a, b] = s / L[:, b, b]
    return L, pd


def np_cholesky_solve(L, h):
    y = np.zeros_like(h)
    for a in range(6):
        y[:, a] = (h[:, a] - (L[:, a, :a] * y[:, :a]).sum(-1)) / L[:, a, a]
    x = np.zeros_like(h)
    for a in range(5, -1, -1):
        x[:, a] = (y[:, a] - (L[:, a + 1:, a] * x[:, a + 1:]).sum(-1)) / L[:, a, a]
    return x


def np_equil(contact, target, k, normal, f, c, mu=MU, tol=TOL, max_iters=MAX_ITERS, **lm):
    """The rule of cdx_equil.h in numpy, all items at once with a mask for the ones still running."""
    (contact, target, k, normal, f, c), E, W, T, shared = as_inputs(contact, target, k, normal, f, c)
    lm = {**LM, **lm}
    if shared:
        f, c = np.broadcast_to(f, (E, W, 3)), np.broadcast_to(c, (E, W, 3))
    N = E * W
    pts, tgt, kk, nrm = (np.repeat(x, W, axis=0) for x in (contact, target, k, normal))
    f, c = f.reshape(N, 3), c.reshape(N, 3)
    with np.errstate(all="ignore"):
        nn = (nrm * nrm).sum(-1)
        ok = (np.isfinite(pts).all((1, 2)) & np.isfinite(tgt).all((1, 2)) & np.isfinite(kk).all(1) & (kk > 0).all(1) &
              np.isfinite(nn).all(1) & (nn > 0).all(1) & np.isfinite(f).all(1) & np.isfinite(c).all(1))
    out = outputs(N, T, np.nan)
    out["stable"][:], out["iters"][:], out["status"][:] = 0, 0, 2
    at = np.flatnonzero(ok)
    if len(at) == 0:
        return out
    pts, tgt, kk, nrm, f, c = (x[at] for x in (pts, tgt, kk, nrm, f, c))
    M = len(at)
    K = kk.sum(1)
    o = (kk[..., None] * pts).sum(1) / K[:, None]
    P, G, Cv = pts - o[:, None], tgt - o[:, None], c - o
    ell = np.maximum(norm(P).max(1), norm(Cv))
    ell = np.where(ell > 0, ell, 1.0)
    Fs = (kk * norm(P - G)).sum(1) + norm(f)
    eye3, eye6 = np.eye(3), np.eye(6)

    def energy_change(R, t, D, dv):
        a = np.einsum("mij,mtj->mti", R, P)
        r = a + t[:, None] - G
        d = np.einsum("mij,mtj->mti", D, a) + dv[:, None]
        db = np.einsum("mij,mj->mi", D, np.einsum("mij,mj->mi", R, Cv))
        return (kk * (d * (r + 0.5 * d)).sum(-1)).sum(1) - (f * (db + dv)).sum(1)

    def derivatives(R, t):
        a = np.einsum("mij,mtj->mti", R, P)
        r = a + t[:, None] - G
        b = np.einsum("mij,mj->mi", R, Cv)
        gv = (kk[..., None] * r).sum(1) - f
        gw = (kk[..., None] * np.cross(a, r)).sum(1) - np.cross(b, f)
        ar = np.einsum("mti,mtj->mtij", a, r)
        aa = np.einsum("mti,mtj->mtij", a, a)
        ww = ((a * a).sum(-1) - (a * r).sum(-1))[..., None, None] * eye3 - aa + 0.5 * (ar + ar.transpose(0, 1, 3, 2))
        ww = (kk[..., None, None] * ww).sum(1)
        bf = np.einsum("mi,mj->mij", b, f)
        ww = ww - (0.5 * (bf + bf.transpose(0, 2, 1)) - (b * f).sum(-1)[:, None, None] * eye3)
        S = skew((kk[..., None] * a).sum(1))
        H = np.zeros((M, 6, 6))
        H[:, :3, :3], H[:, :3, 3:], H[:, 3:, :3], H[:, 3:, 3:] = ww, S, -S, K[:, None, None] * eye3
        d = np.concatenate([1.0 / ell[:, None].repeat(3, 1), np.ones((M, 3))], 1)
        return gv, gw, H * d[:, :, None] * d[:, None, :]

    R, t = np.tile(eye3, (M, 1, 1)), np.zeros((M, 3))
    damp = np.full(M, lm["mu0"])
    iters, status, stable = np.zeros(M, np.int32), np.full(M, -1, np.int32), np.zeros(M, bool)
    active = np.ones(M, bool)
    with np.errstate(all="ignore"):
        while True:
            gv, gw, H = derivatives(R, t)
            conv = (norm(gv) <= tol * Fs) & (norm(gw) <= tol * Fs * ell)
            stop = active & (conv | (iters >= max_iters))
            status[stop] = np.where(conv[stop], 0, 1)
            stable[stop] = np_cholesky(H[stop])[1]
            active &= ~stop
            if not active.any():
                break
            iters[active] += 1
            L, pd = np_cholesky(H + (damp * K)[:, None, None] * eye6)
            d = np_cholesky_solve(L, -np.concatenate([gw / ell[:, None], gv], 1))
            a = 0.5 * d[:, :3] / ell[:, None]
            s = (a * a).sum(-1)[:, None, None]
            aa = 2.0 * np.einsum("mi,mj->mij", a, a) + 2.0 * skew(a)
            cay, D = ((1.0 - s) * eye3 + aa) / (1.0 + s), (aa - 2.0 * s * eye3) / (1.0 + s)
            Rn, tn = cay @ R, t + d[:, 3:]
            acc = active & pd & (energy_change(R, t, D, d[:, 3:]) < 0)
            R[acc], t[acc] = Rn[acc], tn[acc]
            damp = np.where(active, np.where(acc, np.maximum(damp / lm["nu"], lm["mu_min"]),
                                             np.minimum(damp * lm["nu"], lm["mu_max"])), damp)
    res = derived(R, o + t - np.einsum("mij,mj->mi", R, o), pts, tgt, kk, nrm, mu)
    res["shift"] = norm(t)
    res.update(stable=stable.astype(np.uint8), iters=iters, status=status)
    for name in FIELDS:
        out[name][at] = res[name].reshape(out[name][at].shape)
    return out


def derived(R, trans, pts, tgt, kk, nrm, mu):
    """force, normal_force, margin, chord (and rot, trans as given) of the poses x = R·p + trans, per item."""
    x = np.einsum("mij,mtj->mti", R, pts) + trans[:, None]
    force = kk[..., None] * (tgt - x)
    m = np.einsum("mij,mtj->mti", R, unit(nrm))
    dn, fn = (force * m).sum(-1), norm(force)
    with np.errstate(all="ignore"):
        margin = np.where(fn > 0, -dn / np.where(fn > 0, fn, 1.0) - 1.0 / np.sqrt(1.0 + mu * mu), 0.0)
    chord = np.sqrt(np.maximum(3.0 - np.trace(R, axis1=1, axis2=2), 0.0))
    return dict(rot=R.reshape(-1, 9), trans=trans, force=force, normal_force=-dn, margin=margin, chord=chord)


def np_reduce(out, E, W, T, **lim):
    """The reduction of cdx_equil.h from item-major outputs."""
    lim = {**LIMITS, **lim}
    margin, nf = out["margin"].reshape(E, W, T), out["normal_force"].reshape(E, W, T)
    shift, chord = out["shift"].reshape(E, W), out["chord"].reshape(E, W)
    stable, status = out["stable"].reshape(E, W), out["status"].reshape(E, W)
    red = reduce_outputs(E)
    with np.errstate(all="ignore"):
        hold = ((status == 0) & (stable != 0) & (margin > lim["margin_min"]).all(-1) &
                (nf >= lim["min_normal_force"]).all(-1) & (shift <= lim["max_shift"]) & (chord <= lim["max_chord"]))
    for e in range(E):
        live = status[e] != 2
        flat = margin[e].reshape(-1)
        cand = np.flatnonzero((live[:, None] & ~np.isnan(margin[e])).reshape(-1))
        j = int(cand[np.argmin(flat[cand])]) if len(cand) else -1  # (argmin: the first of equal minima)
        red["worst_margin"][e] = flat[j] if j >= 0 else np.nan
        red["worst_load"][e], red["worst_tip"][e] = (j // T, j % T) if j >= 0 else (-1, -1)
        red["max_shift"][e] = shift[e][live].max() if live.any() else np.nan
        red["max_chord"][e] = chord[e][live].max() if live.any() else np.nan
        red["n_failed"][e] = int((~hold[e]).sum())
        red["holds"][e] = 1 if hold[e].all() else 0
    return red


def np_kabsch(pts, tgt, kk):
    """The stiffness-weighted Kabsch fit of pts onto tgt per row: (R [E, 3, 3], trans [E, 3]) of x = R·p + trans."""
    K = kk.sum(1)
    cp, cg = (kk[..., None] * pts).sum(1) / K[:, None], (kk[..., None] * tgt).sum(1) / K[:, None]
    H = np.einsum("et,eti,etj->eij", kk, pts - cp[:, None], tgt - cg[:, None])
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.einsum("eji,ekj->eik", Vt, U)))
    D = np.tile(np.eye(3), (len(pts), 1, 1))
    D[:, 2, 2] = d
    R = np.einsum("eji,ejk,elk->eil", Vt, D, U)
    return R, cg - np.einsum("eij,ej->ei", R, cp)


# ------------------------------------------------------------------ inputs
AXES = np.array([0.05, 0.03, 0.03])


TETRA = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)


@functools.lru_cache(None)
def family(name, E, T, seed=0):
    """Contacts on an ellipsoid with its outward normals (not unit), targets pressed in by a depth drawn per contact
    plus noise, stiffness 80 … 400 N/m.  "shallow": random places, 4 … 12 mm deep, 3 mm of noise (few of these hold
    anything: four random contacts rarely oppose each other); "deep": the same 10 … 30 mm deep; "firm" (T = 4): the
    contacts within 0.25 of the directions of a tetrahedron, 8 … 12 mm deep, 0.5 mm of noise — grasps that hold."""
    lo, hi, noise = {"shallow": (0.004, 0.012, 0.003), "deep": (0.01, 0.03, 0.003), "firm": (0.008, 0.012, 0.0005)}[name]
    g = np.random.default_rng([seed, E, T, len(name)])
    u = unit(g.normal(size=(E, T, 3)))
    if name == "firm":
        u = unit(TETRA + 0.25 * g.normal(size=(E, 4, 3)))
    pts = u * AXES
    nh = unit(pts / AXES ** 2)
    tgt = pts - nh * g.uniform(lo, hi, (E, T, 1)) + g.normal(scale=noise, size=(E, T, 3))
    k = g.uniform(80.0, 400.0, (E, T))
    return pts, tgt, k, nh * g.uniform(0.5, 2.0, (E, T, 1))


def centre(pts, k):
    return (k[..., None] * pts).sum(1) / k.sum(1)[:, None]


def loads(pts, k, W, mag, shared=False, seed=1):
    """W loads of magnitude ``mag`` (a number, or (lo, hi) for a uniform draw) in random directions, acting within 1 cm
    of each row's stiffness centre — or, shared, within 1 cm of the origin."""
    E = len(pts)
    g = np.random.default_rng([seed, E, W, int(shared)])
    shape = (W, 3) if shared else (E, W, 3)
    m = mag if np.isscalar(mag) else g.uniform(mag[0], mag[1], shape[:-1] + (1,))
    f = unit(g.normal(size=shape)) * m
    off = unit(g.normal(size=shape)) * g.uniform(0.0, 0.01, shape[:-1] + (1,))
    return f, (off if shared else centre(pts, k)[:, None] + off)


def stall_rows():
    """Rows 3158 and 3681 of the 4096 grasps that tools/equil.py times (its recipe, seed 0) under the weight of 0.4 kg
    in 26 directions: on each, one load ended a first version of the rule at max_iters with a net force of 1.3 … 1.8
    × tol·Fs — the decrease of its steps was below the last place of the energy, so U′ < U, taken as a difference of
    two rounded energies, failed for ever."""
    from compliancedex_amd.stability import gravity_loads
    g = np.random.default_rng(0)
    u = unit(g.normal(size=(4096, 4, 3)))
    pts = u * AXES
    nh = unit(pts / AXES ** 2)
    tgt = pts - nh * g.uniform(0.004, 0.012, (4096, 4, 1)) + g.normal(scale=0.003, size=(4096, 4, 3))
    k = g.uniform(80.0, 400.0, (4096, 4))
    rows = [3158, 3681]
    pts, tgt, k, nh = pts[rows], tgt[rows], k[rows], nh[rows]
    f = np.tile(gravity_loads(0.4)[0], (2, 1, 1))
    return pts, tgt, k, nh, f, np.tile(centre(pts, k)[:, None], (1, 26, 1))


def check_no_stall(solve):
    out = solve(*stall_rows())
    assert (out["status"] == 0).all() and out["iters"].max() <= 10, (out["status"], out["iters"])


def tetrahedron(s=0.8, k=150.0):
    v = TETRA
    o = np.array([0.02, -0.01, 0.3])
    return (0.05 * v + o)[None], (s * 0.05 * v + o)[None], np.full((1, 4), k), v[None].copy()


# ------------------------------------------------------------------ shared checks; solve(contact, …, c, **kw) → dict
def scales(pts, tgt, k, f, c):
    """(ℓ, Fs) per item for [E, W, 3] loads."""
    o = centre(pts, k)
    P = pts - o[:, None]
    ell = np.maximum(norm(P).max(1)[:, None], norm(c - o[:, None]))
    ell = np.where(ell > 0, ell, 1.0)
    return ell.reshape(-1), ((k * norm(pts - tgt)).sum(1)[:, None] + norm(f)).reshape(-1)


def check_certificate(solve, report=None):
    """Check 1: E = 37, W = 26, T = 4, 1 N loads: every item status 0, the balance of forces and of torques recomputed
    from rot, trans and force alone within 2·tol of the scales, and the other outputs recomputed from rot and trans."""
    E, W, T = 37, 26, 4
    pts, tgt, k, nrm = family("shallow", E, T)
    f, c = loads(pts, k, W, 1.0)
    out = solve(pts, tgt, k, nrm, f, c)
    assert (out["status"] == 0).all(), (np.flatnonzero(out["status"] != 0), out["iters"].max())
    assert (out["iters"] <= MAX_ITERS).all() and (out["stable"] == 1).all()
    N = E * W
    rep = [np.repeat(x, W, axis=0) for x in (pts, tgt, k, nrm)]
    R, trans, F = out["rot"].reshape(N, 3, 3), out["trans"], out["force"]
    ff, cc = f.reshape(N, 3), c.reshape(N, 3)
    o = np.repeat(centre(pts, k), W, axis=0)
    on = np.einsum("mij,mj->mi", R, o) + trans  # the stiffness centre, moved
    x = np.einsum("mij,mtj->mti", R, rep[0]) + trans[:, None]
    cn = np.einsum("mij,mj->mi", R, cc) + trans
    net = F.sum(1) + ff
    tau = np.cross(x - on[:, None], F).sum(1) + np.cross(cn - on, ff)
    ell, Fs = scales(pts, tgt, k, f, c)
    if report is not None:
        print(report, "iters median / max", int(np.median(out["iters"])), int(out["iters"].max()),
              "worst |net| / (tol·Fs)", float((norm(net) / (TOL * Fs)).max()),
              "worst |tau| / (tol·Fs·l)", float((norm(tau) / (TOL * Fs * ell)).max()))
    assert (norm(net) <= 2 * TOL * Fs).all() and (norm(tau) <= 2 * TOL * Fs * ell).all()
    d = derived(R, trans, *rep, MU)
    assert np.abs(out["force"] - d["force"]).max() <= 1e-12  # (forces of a few newtons)
    assert np.abs(out["normal_force"] - d["normal_force"]).max() <= 1e-12
    assert np.abs(out["margin"] - d["margin"]).max() <= 1e-12
    assert np.abs(out["shift"] - norm(on - o)).max() <= 1e-15
    # chord: both sides subtract a trace from 3, and sqrt turns the last place of that into 1e-8
    assert np.abs(out["chord"] - d["chord"]).max() <= 1e-7
    axis_angle = np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0))
    assert np.abs(out["chord"] - 2.0 * np.sin(axis_angle / 2.0)).max() <= 1e-7
    assert np.abs(np.einsum("mij,mkj->mik", R, R) - np.eye(3)).max() <= 1e-14  # (no re-orthonormalisation needed)
    return out


def closed_a_cases():
    g = np.random.default_rng(5)
    return [(s, kk, unit(g.normal(size=3)) * mag) for s, kk, mag in ((0.8, 150.0, 1.0), (0.6, 300.0, 4.0), (1.0, 80.0, 0.5))]


def closed_a_error(solve):
    """Check 2(a): the tetrahedron with equal stiffness, g = o + s·(p − o), the load at o: R = I and t = f/K."""
    worst = 0.0
    for s, kk, f in closed_a_cases():
        pts, tgt, k, nrm = tetrahedron(s, kk)
        o = centre(pts, k)
        out = solve(pts, tgt, k, nrm, f[None, None], o[:, None])
        assert out["status"][0] == 0 and out["stable"][0] == 1
        worst = max(worst, np.abs(out["rot"][0] - np.eye(3).reshape(9)).max(), np.abs(out["trans"][0] - f / (4 * kk)).max())
        # the springs share the load equally on top of their preload
        assert np.abs(out["force"][0] - (kk * (tgt[0] - pts[0]) - f / 4)).max() <= 1e-12
    return worst


KABSCH_T, KABSCH_E = (3, 4, 5, 6, 7, 8), 24


def closed_b_error(solve, report=None):
    """Check 2(b): zero load on family "shallow", T = 3 … 8: the stiffness-weighted Kabsch fit."""
    worst = 0.0
    for T in KABSCH_T:
        pts, tgt, k, nrm = family("shallow", KABSCH_E, T)
        out = solve(pts, tgt, k, nrm, np.zeros((1, 3)), np.zeros((1, 3)))
        assert (out["status"] == 0).all() and (out["stable"] == 1).all(), (T, out["status"], out["iters"])
        R, trans = np_kabsch(pts, tgt, k)
        err = max(np.abs(out["rot"] - R.reshape(-1, 9)).max(), np.abs(out["trans"] - trans).max())
        if report is not None:
            print(report, "T", T, "iters max", int(out["iters"].max()), "difference to Kabsch", float(err))
        worst = max(worst, err)
    return worst


ONE_ITER_CASES = [("shallow", 16, 4), ("deep", 16, 4), ("shallow", 8, 3), ("deep", 8, 8), ("shallow", 8, 5)]


def one_iteration_error(solve):
    """Check 3: max_iters = 1 against the numpy statement → the largest difference per float field."""
    worst = {name: 0.0 for name in FLOATS}
    for name, E, T in ONE_ITER_CASES:
        pts, tgt, k, nrm = family(name, E, T)
        f, c = loads(pts, k, 7, (0.0, 4.0))
        out, ref = solve(pts, tgt, k, nrm, f, c, max_iters=1), np_equil(pts, tgt, k, nrm, f, c, max_iters=1)
        assert (out["iters"] == 1).all() and same_bits(out["iters"], ref["iters"])
        assert same_bits(out["status"], ref["status"]) and same_bits(out["stable"], ref["stable"])
        assert (np.abs(out["rot"].reshape(-1, 3, 3) - np.eye(3)).max((1, 2)) > 1e-6).any()  # (a step was taken)
        for fld in FLOATS:
            worst[fld] = max(worst[fld], float(np.abs(out[fld] - ref[fld]).max()))
    return worst


def check_one_iteration(solve, report=None):
    worst = one_iteration_error(solve)
    if report is not None:
        print(report, {k: f"{v:.2e}" for k, v in worst.items()}, "allowed", ONE_ITER_TOL)
    for fld in FLOATS:
        assert worst[fld] <= ONE_ITER_TOL[fld], (fld, worst[fld])


def check_converged_against_numpy(solve):
    """The whole solve against the numpy statement on 4 N loads: the same statuses, and both within the stop test of
    the same equilibrium (positions to 1e-7 of the 5 cm object)."""
    pts, tgt, k, nrm = family("shallow", 9, 4)
    f, c = loads(pts, k, 26, 4.0)
    out, ref = solve(pts, tgt, k, nrm, f, c), np_equil(pts, tgt, k, nrm, f, c)
    assert (out["status"] == 0).all() and (ref["status"] == 0).all() and out["iters"].max() <= 8
    assert np.abs(out["rot"] - ref["rot"]).max() <= 1e-6 and np.abs(out["trans"] - ref["trans"]).max() <= 1e-7


def check_independence(solve):
    """Check 5: an item alone has the bits it had in the batch; permuting rows permutes the outputs."""
    E, W, T = 3, 5, 4
    pts, tgt, k, nrm = family("deep", E, T)
    f, c = loads(pts, k, W, (0.0, 4.0))
    full = solve(pts, tgt, k, nrm, f, c)
    for e in range(E):
        for w in range(W):
            one = solve(pts[e:e + 1], tgt[e:e + 1], k[e:e + 1], nrm[e:e + 1], f[e:e + 1, w:w + 1], c[e:e + 1, w:w + 1])
            for name in FIELDS:
                assert same_bits(one[name][0], full[name][e * W + w]), (e, w, name)
    perm = np.array([2, 0, 1])
    moved = solve(pts[perm], tgt[perm], k[perm], nrm[perm], f[perm], c[perm])
    for name in FIELDS:
        a = full[name].reshape((E, W) + full[name].shape[1:])[perm]
        assert same_bits(moved[name], a.reshape(full[name].shape)), name
    # a shared load set is the same set repeated for every row
    fs, cs = loads(pts, k, W, 2.0, shared=True)
    a = solve(pts, tgt, k, nrm, fs, cs)
    b = solve(pts, tgt, k, nrm, np.tile(fs, (E, 1, 1)), np.tile(cs, (E, 1, 1)))
    for name in FIELDS:
        assert same_bits(a[name], b[name]), name


def check_statuses(solve):
    """Check 6: status 1 with finite outputs; each kind of bad input gives status 2 exactly where stated and every
    other item keeps its bits."""
    E, W, T = 6, 5, 4
    pts, tgt, k, nrm = family("deep", E, T)
    f, c = loads(pts, k, W, (0.5, 4.0))
    one = solve(pts, tgt, k, nrm, f, c, max_iters=1)
    assert (one["status"] == 1).all() and (one["iters"] == 1).all()
    for name in FLOATS:
        assert np.isfinite(one[name]).all(), name
    zero = solve(pts, tgt, k, nrm, f, c, max_iters=0)
    assert (zero["status"] == 1).all() and (zero["iters"] == 0).all()
    assert same_bits(zero["rot"], np.tile(np.eye(3).reshape(9), (E * W, 1))) and np.abs(zero["trans"]).max() <= 1e-17
    clean = solve(pts, tgt, k, nrm, f, c)
    assert np.isin(clean["status"], (0, 1)).all()
    row_kinds = [("contact", np.nan), ("contact", np.inf), ("target", np.nan), ("target", -np.inf), ("k", np.nan),
                 ("k", np.inf), ("k", 0.0), ("k", -3.0), ("normal", np.nan), ("normal", np.inf), ("normal", "zero")]
    for j, (kind, val) in enumerate(row_kinds):
        a = dict(contact=pts.copy(), target=tgt.copy(), k=k.copy(), normal=nrm.copy())
        e, i = j % E, j % T
        if val == "zero":
            a["normal"][e, i] = 0.0
        elif kind == "k":
            a["k"][e, i] = val
        else:
            a[kind][e, i, j % 3] = val
        out = solve(a["contact"], a["target"], a["k"], a["normal"], f, c)
        bad = np.zeros((E, W), bool)
        bad[e] = True
        _bad_items(out, clean, bad.reshape(-1), (kind, val))
    for j, (kind, val) in enumerate([("f", np.nan), ("f", np.inf), ("c", np.nan), ("c", -np.inf)]):
        ff, cc = f.copy(), c.copy()
        e, w = (j + 1) % E, (2 * j) % W
        (ff if kind == "f" else cc)[e, w, j % 3] = val
        out = solve(pts, tgt, k, nrm, ff, cc)
        bad = np.zeros((E, W), bool)
        bad[e, w] = True
        _bad_items(out, clean, bad.reshape(-1), (kind, val))
    # a shared load that is not finite is bad in every row
    fs, cs = loads(pts, k, W, 2.0, shared=True)
    ok = solve(pts, tgt, k, nrm, fs, cs)
    fs = fs.copy()
    fs[3, 1] = np.nan
    out = solve(pts, tgt, k, nrm, fs, cs)
    bad = np.zeros((E, W), bool)
    bad[:, 3] = True
    _bad_items(out, ok, bad.reshape(-1), "shared f")


def _bad_items(out, clean, bad, what):
    assert (out["status"][bad] == 2).all() and (out["iters"][bad] == 0).all() and (out["stable"][bad] == 0).all(), what
    for name in FLOATS:
        assert np.isnan(out[name][bad]).all(), (what, name)
    for name in FIELDS:
        assert same_bits(out[name][~bad], clean[name][~bad]), (what, name)


def reduce_cases():
    """Item-major outputs made by hand (the reduction reads nothing else) → [(label, out, E, W, T, limits)]."""
    E, W, T = 5, 4, 3
    g = np.random.default_rng(11)
    base = dict(margin=g.uniform(0.05, 0.3, (E * W, T)), normal_force=g.uniform(0.5, 3.0, (E * W, T)),
                shift=g.uniform(0.001, 0.01, E * W), chord=g.uniform(0.01, 0.2, E * W),
                stable=np.ones(E * W, np.uint8), status=np.zeros(E * W, np.int32))
    cases = [("all hold", base, {})]

    def variant(label, lim=None, **edit):
        out = {k: v.copy() for k, v in base.items()}
        for name, (at, val) in edit.items():
            out[name][at] = val
        cases.append((label, out, lim or {}))
        return out
    variant("tie", margin=((slice(4, 8), slice(None)), 0.01))  # row 1: every margin equal → (0, 0)
    variant("tie later", margin=(([9, 10], [2, 1]), 0.001))  # row 2: items 1 and 2 tie → load 1, tip 2
    o = variant("row of status 2", status=(slice(8, 12), 2))
    for name in ("margin", "normal_force", "shift", "chord"):
        o[name][8:12] = np.nan
    o["stable"][8:12] = 0
    o = variant("one item of status 2", status=(13, 2))
    o["margin"][13], o["shift"][13], o["chord"][13] = np.nan, np.nan, np.nan
    variant("status 1", status=(6, 1))
    variant("unstable", stable=(17, 0))
    variant("negative margin", margin=((2, 1), -0.2))
    variant("pulling contact", normal_force=((19, 0), -0.1))
    variant("shift", shift=(5, 0.05))
    variant("chord", chord=(10, 0.5))
    # every threshold moved until exactly one item of row 3 (items 12 … 15) switches
    variant("margin_min switches one", dict(margin_min=0.04), margin=((14, 2), 0.03))
    variant("min_normal_force switches one", dict(min_normal_force=0.4), normal_force=((15, 1), 0.3))
    variant("max_shift switches one", dict(max_shift=0.0105), shift=(12, 0.0107))
    variant("max_chord switches one", dict(max_chord=0.21), chord=(13, 0.22))
    met = dict(min_normal_force=0.4, max_shift=0.0125, max_chord=0.25)
    variant("limits met with equality hold", met, normal_force=((3, 0), 0.4), shift=(3, 0.0125), chord=(3, 0.25))
    variant("margin_min met with equality fails", dict(margin_min=0.04), margin=((3, 2), 0.04))
    return [(label, out, E, W, T, lim) for label, out, lim in cases]


def check_reduction(reduce):
    """Check 7: reduce(out, E, W, T, **limits) against np_reduce, bit for bit on the floats, equal on the integers."""
    seen = {}
    for label, out, E, W, T, lim in reduce_cases():
        red, ref = reduce(out, E, W, T, **lim), np_reduce(out, E, W, T, **lim)
        for name in RED_FIELDS:
            assert same_bits(red[name], ref[name]), (label, name, red[name], ref[name])
        seen[label] = red
    assert seen["all hold"]["holds"].all() and not seen["all hold"]["n_failed"].any()
    assert (seen["tie"]["worst_load"][1], seen["tie"]["worst_tip"][1]) == (0, 0)
    assert (seen["tie later"]["worst_load"][2], seen["tie later"]["worst_tip"][2]) == (1, 2)
    r = seen["row of status 2"]
    assert np.isnan(r["worst_margin"][2]) and np.isnan(r["max_shift"][2]) and np.isnan(r["max_chord"][2])
    assert (r["worst_load"][2], r["worst_tip"][2], r["n_failed"][2], r["holds"][2]) == (-1, -1, 4, 0)
    for label, row in (("one item of status 2", 3), ("status 1", 1), ("unstable", 4), ("negative margin", 0),
                       ("pulling contact", 4), ("shift", 1), ("chord", 2), ("margin_min switches one", 3),
                       ("min_normal_force switches one", 3), ("max_shift switches one", 3),
                       ("max_chord switches one", 3), ("margin_min met with equality fails", 0)):
        want = np.zeros(5, np.int32)
        want[row] = 1
        assert (seen[label]["n_failed"] == want).all() and (seen[label]["holds"] == 1 - want).all(), label
    assert seen["limits met with equality hold"]["holds"].all()
