"""Does the object stay in the hand: the batched disturbance-load test (cdx_grasp_equilibrium, cdx_equil_reduce; the
rule is csrc/cdx_equil.h).  The reference answers this with a PyBullet rollout (verify_pregrasp.py:82-121); a rollout
stays out of scope here, and this is its quasi-static stand-in: the reference's own model of a compliant grasp
(force_eq_reward, optimize_pregrasp.py:73-118 — contacts stick, every fingertip is a spring of stiffness ``compliance``
towards its target), solved exactly for E grasps under W dead loads each in one launch.  Per (grasp, load) it reports
the friction-cone margins, the normal forces and how far the object moved at the equilibrium, and per grasp a verdict.
Contact loss and sliding are not modelled: a negative margin or normal force says that the sticking equilibrium needs
a force the contact cannot give, not where the object goes then.  Parity with PyBullet is not attempted.

No autograd: every output is detached, and gradients of the margins are out of scope.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _native as N

EquilibriumResult = namedtuple("EquilibriumResult", ["rot", "trans", "force", "normal_force", "margin", "shift", "chord",
                                                     "stable", "iters", "status"])
EquilibriumResult.__doc__ = """Per (grasp, load): rot [E, W, 3, 3] and trans [E, W, 3], the object's displacement
x = rot·p + trans; force [E, W, T, 3] of each spring on the object; normal_force [E, W, T]; margin [E, W, T] =
(−F/‖F‖)·(rot·n̂) − 1/sqrt(1 + mu²); shift [E, W] the displacement of the stiffness centre (m); chord [E, W] =
2·sin(θ/2) of rot; stable [E, W] bool: the energy's Hessian at the returned pose is positive definite; iters [E, W]
int32; status [E, W] int32: 0 balanced within tol, 1 max_iters used (finite outputs), 2 a non-finite input, a stiffness
≤ 0 or a zero normal in the row, or a non-finite load (float outputs NaN).  Device float64 tensors, detached."""

DisturbanceReport = namedtuple("DisturbanceReport", ["holds", "n_failed", "worst_margin", "worst_load", "worst_tip",
                                                     "max_shift", "max_chord", "result"])
DisturbanceReport.__doc__ = """Per grasp: holds [E] bool (every load holds), n_failed [E] int32, worst_margin [E] (the
least margin over the loads of status ≠ 2, NaN if none) with worst_load / worst_tip [E] int32 (−1 if none), max_shift
and max_chord [E] over the same loads, and ``result``, the EquilibriumResult they were reduced from."""

PayloadResult = namedtuple("PayloadResult", ["payload", "upper"])
PayloadResult.__doc__ = """payload [E]: the largest load magnitude tried at which the grasp held in every direction (NaN
where it does not hold unloaded); upper [E]: the smallest magnitude tried at which it failed (``hi`` where none did:
payload == hi then means "at least hi")."""

ShapeUncertaintyReport = namedtuple("ShapeUncertaintyReport", ["hold_probability", "holds_mean", "angle_std",
                                                               "offset_std", "mean", "samples"])
ShapeUncertaintyReport.__doc__ = """Per grasp: hold_probability [E] float64, the fraction of the drawn sets of normals
under which the grasp holds; holds_mean [E] bool, the verdict with the mean normals; angle_std [E, T] (rad) and
offset_std [E, T] (m) of ``GPIS.normal_uncertainty`` at the contacts; ``mean``, the DisturbanceReport of the mean
normals, and ``samples``, the one of the E·S drawn rows (row e·S + s)."""

# Defaults of the verdict: a contact may not leave its friction cone (margin > 0) nor pull (normal force ≥ 0), and the
# object may not move more than 2 cm or turn more than 2·asin(0.35/2) ≈ 20° — beyond that the fingertip springs of the
# model are no longer the hand.
LIMITS = dict(margin_min=0.0, min_normal_force=0.0, max_shift=0.02, max_chord=0.35)
LM_DEFAULTS = dict(mu0=1e-3, mu_min=1e-9, mu_max=1e6, nu=10.0)


def equil_params(n_tips, mu, tol=1e-8, max_iters=60, lm=None):
    p = N.CdxEquilParams()
    lm = {**LM_DEFAULTS, **(lm or {})}
    p.n_tips, p.max_iters, p.mu, p.tol = int(n_tips), int(max_iters), float(mu), float(tol)
    p.mu0, p.mu_min, p.mu_max, p.nu = (float(lm[k]) for k in ("mu0", "mu_min", "mu_max", "nu"))
    return p


def equil_limits(**kw):
    unknown = set(kw) - set(LIMITS)
    if unknown:
        raise TypeError(f"unknown limits {sorted(unknown)}: the verdict takes {sorted(LIMITS)}")
    q = N.CdxEquilLimits()
    for k, v in {**LIMITS, **kw}.items():
        setattr(q, k, float(v))
    return q


def load_directions(n=26):
    """n unit vectors [n, 3] float64, computed in numpy on the host: for n = 6, 14 or 26 the directions of the cube
    lattice {−1, 0, 1}³ \\ {0} with one, up to three (6 faces + 8 corners) or any number of non-zero entries; for any
    other n a Fibonacci sphere."""
    n = int(n)
    if n < 1:
        raise ValueError("at least one direction")
    if n in (6, 14, 26):
        grid = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.float64)
        count = np.abs(grid).sum(1)
        keep = {6: count == 1, 14: (count == 1) | (count == 3), 26: count > 0}[n]
        d = grid[keep]
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def gravity_loads(mass, g=9.81, directions=26, com=None):
    """The weight of ``mass`` kg in every direction of ``load_directions(directions)`` (or of a given [W, 3] array of
    unit vectors) — gravity seen from a hand in any orientation → (load_force [W, 3] numpy, load_point = ``com``)."""
    if not mass >= 0.0:
        raise ValueError("mass must be ≥ 0")
    d = load_directions(directions) if np.isscalar(directions) else np.asarray(directions, np.float64)
    return float(mass) * float(g) * d, com


def _rows(x, name, last):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if not x.is_cuda:
        raise RuntimeError(f"compliancedex_amd has no CPU path: {name} must be a device tensor")
    if x.ndim != len(last) + 1 or tuple(x.shape[1:]) != tuple(last):
        raise ValueError(f"{name} must have shape [E, {', '.join(map(str, last))}], got {tuple(x.shape)}")
    return x.detach().to(torch.float64).contiguous()


def _inputs(contact, target, compliance, normals, load_force, load_point, com):
    """Checked, contiguous float64 device tensors and the shapes: (contact, target, k, normals, f, c, shared, E, W, T)."""
    if not isinstance(contact, torch.Tensor) or contact.ndim != 3 or contact.shape[2] != 3:
        if isinstance(contact, torch.Tensor):
            raise ValueError(f"contact must have shape [E, T, 3], got {tuple(contact.shape)}")
        raise TypeError("contact must be a tensor")
    E, T = contact.shape[0], contact.shape[1]
    if not 1 <= T <= N.MAX_TIPS:
        raise ValueError(f"1 … {N.MAX_TIPS} contacts per grasp, got {T}")
    contact = _rows(contact, "contact", (T, 3))
    target, normals = _rows(target, "target", (T, 3)), _rows(normals, "normals", (T, 3))
    k = _rows(compliance, "compliance", (T,))
    dev = contact.device
    f = torch.as_tensor(load_force, dtype=torch.float64, device=dev)
    if f.ndim not in (2, 3) or f.shape[-1] != 3 or (f.ndim == 3 and f.shape[0] != E):
        raise ValueError(f"load_force must have shape [W, 3] or [E, W, 3], got {tuple(f.shape)}")
    W = f.shape[-2]
    if load_point is None:
        # every load at the centre of mass; without one, at each grasp's stiffness centre Σ k·p / Σ k
        c = (k.unsqueeze(2) * contact).sum(1) / k.sum(1, keepdim=True) if com is None else \
            torch.as_tensor(com, dtype=torch.float64, device=dev)
        if c.shape not in ((3,), (E, 3)):
            raise ValueError(f"com must have shape [3] or [E, 3], got {tuple(c.shape)}")
        c = c.expand(W, 3) if c.ndim == 1 else c.unsqueeze(1).expand(E, W, 3)
    else:
        c = torch.as_tensor(load_point, dtype=torch.float64, device=dev)
        if c.ndim not in (2, 3) or tuple(c.shape[-2:]) != (W, 3) or (c.ndim == 3 and c.shape[0] != E):
            raise ValueError(f"load_point must have shape [W, 3] or [E, W, 3] like load_force, got {tuple(c.shape)}")
    shared = f.ndim == 2 and c.ndim == 2
    if not shared:
        f = f.expand(E, W, 3) if f.ndim == 2 else f
        c = c.expand(E, W, 3) if c.ndim == 2 else c
    return contact, target, k, normals, f.detach().contiguous(), c.detach().contiguous(), shared, E, W, T


def _solve(params, contact, target, k, normals, f, c, shared, E, W, T):
    lib = N.load()
    dev = contact.device
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(rot=torch.empty(E, W, 3, 3, **f64), trans=torch.empty(E, W, 3, **f64),
               force=torch.empty(E, W, T, 3, **f64), normal_force=torch.empty(E, W, T, **f64),
               margin=torch.empty(E, W, T, **f64), shift=torch.empty(E, W, **f64), chord=torch.empty(E, W, **f64),
               stable=torch.empty(E, W, dtype=torch.uint8, device=dev), iters=torch.empty(E, W, **i32),
               status=torch.empty(E, W, **i32))
    N.check(lib.cdx_grasp_equilibrium(C.byref(params), E, W, N.ptr(contact), N.ptr(target), N.ptr(k), N.ptr(normals),
                                      N.ptr(f), N.ptr(c), int(shared), *[N.ptr(out[n]) for n in EquilibriumResult._fields],
                                      N.stream_ptr(dev)), "cdx_grasp_equilibrium")
    return out


def _reduce(lim, out, E, W, T):
    lib = N.load()
    dev = out["margin"].device
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    red = dict(worst_margin=torch.empty(E, **f64), worst_load=torch.empty(E, **i32), worst_tip=torch.empty(E, **i32),
               max_shift=torch.empty(E, **f64), max_chord=torch.empty(E, **f64), n_failed=torch.empty(E, **i32),
               holds=torch.empty(E, dtype=torch.uint8, device=dev))
    N.check(lib.cdx_equil_reduce(C.byref(lim), E, W, T, *[N.ptr(out[n]) for n in ("margin", "normal_force", "shift",
                                                                                 "chord", "stable", "status")],
                                 *[N.ptr(red[n]) for n in ("worst_margin", "worst_load", "worst_tip", "max_shift",
                                                            "max_chord", "n_failed", "holds")],
                                 N.stream_ptr(dev)), "cdx_equil_reduce")
    return red


def _result(out):
    return EquilibriumResult(**{**out, "stable": out["stable"].bool()})


def grasp_equilibrium(contact, target, compliance, normals, mu, load_force, load_point=None, com=None, tol=1e-8,
                      max_iters=60, lm=None):
    """The spring equilibrium of E grasps under W dead loads each → EquilibriumResult.

    contact, target, normals [E, T, 3] and compliance [E, T] (T ≤ 8; the fingertip stiffness, > 0; normals outward, need
    not be unit): device tensors.  ``load_force`` [W, 3] (the same loads for every grasp) or [E, W, 3]: constant
    world-frame forces; ``load_point`` of the same shapes: where each acts on the object, in world coordinates at the
    nominal pose.  ``load_point=None`` puts every load at ``com`` ([3] or [E, 3]), and with ``com`` None as well at each
    grasp's stiffness centre.  ``lm``: mu0, mu_min, mu_max, nu of the Levenberg–Marquardt loop.  Runs on the current
    stream, reads nothing back; a bad parameter raises before any launch.  No autograd."""
    a = _inputs(contact, target, compliance, normals, load_force, load_point, com)
    if a[7] == 0 or a[8] == 0:
        raise ValueError("at least one grasp and one load")
    return _result(_solve(equil_params(a[9], mu, tol, max_iters, lm), *a))


def disturbance_report(contact, target, compliance, normals, mu, load_force, load_point=None, com=None, tol=1e-8,
                       max_iters=60, lm=None, **limits):
    """``grasp_equilibrium`` and the verdict per grasp, two launches → DisturbanceReport.  A load holds when its solve
    converged onto a stable equilibrium (status 0, ``stable``), every margin > ``margin_min`` (default 0), every normal
    force ≥ ``min_normal_force`` (0 N), shift ≤ ``max_shift`` (0.02 m) and chord ≤ ``max_chord`` (0.35, about 20°)."""
    lim = equil_limits(**limits)
    a = _inputs(contact, target, compliance, normals, load_force, load_point, com)
    if a[7] == 0 or a[8] == 0:
        raise ValueError("at least one grasp and one load")
    out = _solve(equil_params(a[9], mu, tol, max_iters, lm), *a)
    red = _reduce(lim, out, *a[7:])
    return DisturbanceReport(red["holds"].bool(), red["n_failed"], red["worst_margin"], red["worst_load"],
                             red["worst_tip"], red["max_shift"], red["max_chord"], _result(out))


def max_payload(contact, target, compliance, normals, mu, directions=26, hi=20.0, steps=12, com=None, tol=1e-8,
                max_iters=60, lm=None, **limits):
    """Per grasp, the largest load magnitude (newtons) in 0 … ``hi`` at which it holds in every direction of
    ``load_directions(directions)`` (or of a given [W, 3] array of unit vectors), acting at ``com`` (None: the stiffness
    centre) → PayloadResult.  Magnitudes 0 and ``hi`` are tried first, then ``steps`` bisection steps, the same number
    for every grasp; the brackets live on the device and nothing is read back (steps + 2 solves and reductions).

    Bisection assumes that "holds" is monotone in the magnitude — that a grasp which fails at some load fails at every
    larger one.  Nothing guarantees this: the verdict is a conjunction of thresholds on a nonlinear equilibrium, and a
    larger load can push a contact back into its cone.  What is returned is therefore a magnitude that was tried and
    held, next to one that was tried and failed, not a proof about the magnitudes between or below."""
    if not (np.isfinite(hi) and hi > 0.0) or int(steps) < 0:
        raise ValueError("hi must be finite and positive, steps ≥ 0")
    lim = equil_limits(**limits)
    d = load_directions(directions) if np.isscalar(directions) else np.asarray(directions, np.float64)
    zero = np.zeros((len(d), 3))
    contact, target, k, normals, _, c, _, E, W, T = _inputs(contact, target, compliance, normals, zero, None, com)
    if E == 0:
        raise ValueError("at least one grasp")
    params = equil_params(T, mu, tol, max_iters, lm)
    dirs = torch.as_tensor(d, dtype=torch.float64, device=contact.device)
    c = c.expand(E, W, 3).contiguous()

    def holds_at(mag):
        f = (mag.view(E, 1, 1) * dirs).contiguous()
        return _reduce(lim, _solve(params, contact, target, k, normals, f, c, False, E, W, T), E, W, T)["holds"].bool()
    lo = torch.zeros(E, dtype=torch.float64, device=contact.device)
    up = torch.full_like(lo, float(hi))
    at_zero, at_hi = holds_at(lo), holds_at(up)
    lo = torch.where(at_hi, up, lo)
    for _ in range(int(steps)):
        mid = 0.5 * (lo + up)
        ok = holds_at(mid)
        lo, up = torch.where(ok, mid, lo), torch.where(ok | at_hi, up, mid)
    nan = torch.full_like(lo, float("nan"))
    return PayloadResult(torch.where(at_zero, lo, nan), torch.where(at_zero, up, torch.zeros_like(up)))


def shape_uncertainty_report(gpis, contact, target, compliance, mu, load_force, samples=64, generator=None,
                             load_point=None, com=None, **kw):
    """With which probability does a grasp hold under the loads of ``disturbance_report`` when the shape is only known
    as the GPIS knows it → ShapeUncertaintyReport.

    ``gpis``: the GPIS the contacts lie on; contact, target [E, T, 3] and compliance [E, T] as in ``disturbance_report``,
    whose remaining arguments (load_point, com, tol, max_iters, lm, the limits) pass through.  ``samples`` sets of
    normals are drawn per grasp, every contact's from the pointwise posterior of (f, ∇f) there
    (``GPIS.sample_normals``, ``generator`` a generator of the contacts' device), and ``disturbance_report`` runs once on
    the E·samples rows and once on the mean normals (``GPIS.compute_normal``).  hold_probability is the fraction of a
    grasp's sets under which it holds.

    Out of scope: the contacts are drawn independently of each other — the posterior's cross-covariance between two
    contacts, which is large for neighbouring fingertips, is not modelled — and only the normals are drawn: the contact
    positions stay where they are, although the surface's position is uncertain as well (``offset_std`` says by how
    much).  It adds no kernel of its own and reads nothing back."""
    from . import gpis as G
    S = int(samples)
    if S < 1:
        raise ValueError("at least one sample")
    if not isinstance(contact, torch.Tensor) or contact.ndim != 3 or contact.shape[2] != 3:
        raise ValueError("contact must be a tensor of shape [E, T, 3]")
    E, T = contact.shape[0], contact.shape[1]
    pts = contact.detach().to(torch.float64)
    mean4, cov = gpis.pred_joint(pts)
    unc = G.normal_covariance(mean4[..., 1:], cov)
    normals, _ = G.normals_from_samples(gpis._draw_joint(mean4, cov, S, generator))  # [E, T, S, 3]
    rep_mean = disturbance_report(contact, target, compliance, gpis.compute_normal(pts), mu, load_force,
                                  load_point=load_point, com=com, **kw)

    def rows(x, per_grasp_ndim):
        """A per-grasp argument repeated for the grasp's S rows; anything shared by the grasps as it is."""
        if x is None:
            return None
        if isinstance(x, torch.Tensor) and x.ndim == per_grasp_ndim and x.shape[0] == E:
            return x.repeat_interleave(S, 0)
        x = torch.as_tensor(x, dtype=torch.float64, device=contact.device)
        return x.repeat_interleave(S, 0) if x.ndim == per_grasp_ndim else x
    rep = disturbance_report(rows(contact, 3), rows(target, 3), rows(compliance, 2),
                             normals.permute(0, 2, 1, 3).reshape(E * S, T, 3), mu, rows(load_force, 3),
                             load_point=rows(load_point, 3), com=rows(com, 2), **kw)
    prob = rep.holds.view(E, S).to(torch.float64).mean(1)
    return ShapeUncertaintyReport(prob, rep_mean.holds, unc.angle_std, unc.offset_std, rep_mean, rep)
