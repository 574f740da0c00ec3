"""Batched minimum-wrench contact forces on the device (cdx_min_wrench; the rule is csrc/cdx_wrench.h): for every
candidate, the forces inside their friction cones that press at least ``min_force`` along the normals and leave the
smallest net force and torque, with a duality-gap certificate per row.  The reference asks this of cvxpy / cvxpylayers
(math_utils.py:6-57); here it is one launch for E candidates, every candidate its own problem, and a small ``reg`` picks
the least-effort member of the reference's (solver-defined) optimal family, so the answer is a function of the inputs.
Parity with cvxpy / SCS is not attempted.

``wrench`` is differentiable with respect to the tips by the explicit partial with the forces held constant — what the
reference's autograd delivers (its skew matrices and normals are detached); forces and margins carry no gradient, and
the implicit sensitivity dF*/d(tips, normals) is out of scope.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import torch

from . import _native as N

MinWrenchResult = namedtuple("MinWrenchResult", ["forces", "wrench", "margin", "dual", "gap", "iters", "status"])
MinWrenchResult.__doc__ = """forces [E, T, 3], wrench [E] = ‖ΣF‖ + ‖Σ r×F‖ (attached to autograd through the tips),
margin [E, T] = (−F/‖F‖)·n̂ − 1/sqrt(1 + mu²), dual [E, 6], gap [E] = P − D ≥ reg/2·‖F − F*‖², iters [E] int32,
status [E] int32: 0 certified (gap ≤ tol·max(1, |P|)), 1 max_iters used (best pair checked, finite and feasible),
2 a non-finite input or a zero normal in the row (float outputs NaN).  Device float64 tensors."""

CHECK_EVERY = 10


def wrench_params(n_tips, mu, min_force=5.0, reg=1e-2, max_iters=2000, tol=1e-9, rho=0.05, check_every=CHECK_EVERY):
    p = N.CdxWrenchParams()
    p.n_tips, p.max_iters, p.check_every = int(n_tips), int(max_iters), int(check_every)
    p.mu, p.min_force, p.reg, p.rho, p.tol = float(mu), float(min_force), float(reg), float(rho), float(tol)
    return p


def _launch(params, tips, normals):
    """tips / normals: contiguous float64 device tensors [E, T, 3] → (forces, wrench, margin, dual, gap, iters,
    status, grad_tips).  Runs on the current stream without waiting for it."""
    lib = N.load()
    E, T = tips.shape[0], tips.shape[1]
    dev = tips.device
    f64 = dict(dtype=torch.float64, device=dev)
    forces, grad = torch.empty(E, T, 3, **f64), torch.empty(E, T, 3, **f64)
    wrench, gap = torch.empty(E, **f64), torch.empty(E, **f64)
    margin, dual = torch.empty(E, T, **f64), torch.empty(E, 6, **f64)
    iters = torch.empty(E, dtype=torch.int32, device=dev)
    status = torch.empty(E, dtype=torch.int32, device=dev)
    N.check(lib.cdx_min_wrench(C.byref(params), E, N.ptr(tips), N.ptr(normals), N.ptr(forces), N.ptr(wrench),
                               N.ptr(margin), N.ptr(dual), N.ptr(gap), N.ptr(iters), N.ptr(status), N.ptr(grad),
                               N.stream_ptr(dev)), "cdx_min_wrench")
    return forces, wrench, margin, dual, gap, iters, status, grad


class _MinWrench(torch.autograd.Function):
    """cdx_min_wrench with ∂wrench/∂tips = grad_tips (forces held constant); no other output carries a gradient."""

    @staticmethod
    def forward(ctx, tips, normals, params):
        forces, wrench, margin, dual, gap, iters, status, grad = _launch(params, tips.detach().contiguous(),
                                                                         normals.detach().contiguous())
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(forces, margin, dual, gap, iters, status)
        return wrench, forces, margin, dual, gap, iters, status

    @staticmethod
    def backward(ctx, g_wrench, *_):
        (grad,) = ctx.saved_tensors
        return g_wrench.view(-1, 1, 1) * grad, None, None


def _batched(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"{name} must have shape [E, T, 3], got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError("compliancedex_amd has no CPU path: min_wrench needs device tensors")
    return x if x.dtype == torch.float64 else x.double()


def min_wrench(tips, normals, mu, min_force=5.0, reg=1e-2, max_iters=2000, tol=1e-9, rho=0.05,
               check_every=CHECK_EVERY):
    """Minimum-wrench forces of E candidates: tips, normals [E, T, 3] (T ≤ 8; normals need not be unit) →
    MinWrenchResult.  Nothing is read back; a bad parameter raises before any launch."""
    tips, normals = _batched(tips, "tips"), _batched(normals, "normals")
    if normals.shape != tips.shape:
        raise ValueError(f"normals must have the shape of tips, got {tuple(normals.shape)} vs {tuple(tips.shape)}")
    if not 1 <= tips.shape[1] <= N.MAX_TIPS:
        raise ValueError(f"1 … {N.MAX_TIPS} tips per candidate, got {tips.shape[1]}")
    params = wrench_params(tips.shape[1], mu, min_force, reg, max_iters, tol, rho, check_every)
    wrench, forces, margin, dual, gap, iters, status = _MinWrench.apply(tips, normals, params)
    return MinWrenchResult(forces, wrench, margin, dual, gap, iters, status)


def solve_minimum_wrench(tip_poses, contact_normals, mu, min_force=5.0):
    """math_utils.py:6-35.  [T, 3] inputs → (forces [T, 3], wrench scalar); [E, T, 3] → ([E, T, 3], [E]), every
    candidate its own problem."""
    single = tip_poses.ndim == 2
    tips = tip_poses.unsqueeze(0) if single else tip_poses
    normals = contact_normals.reshape(tips.shape)
    r = min_wrench(tips, normals, mu, min_force)
    return (r.forces[0], r.wrench[0]) if single else (r.forces, r.wrench)


def compute_margin(forces, normals, mu):
    """math_utils.py:47-57 on [T, 3] → [T] or [E, T, 3] → [E, T]: the normals are used as given."""
    forces_dir = -forces / torch.norm(forces, dim=-1, keepdim=True)
    return torch.sum(forces_dir * normals, dim=-1) - math.sqrt(1.0 / (1.0 + mu ** 2))


def minimum_wrench_reward(tip_pose, contact_normals, mu, min_force):
    """math_utils.py:37-45.  [T, 3] inputs → (wrench scalar, margin [1, T], forces [T, 3]); [E, T, 3] →
    ([E], [E, T], [E, T, 3])."""
    forces, total_wrench = solve_minimum_wrench(tip_pose, contact_normals, mu, min_force)
    margin = compute_margin(forces, contact_normals.reshape(forces.shape).to(forces.dtype), mu)
    return total_wrench, (margin.unsqueeze(0) if forces.ndim == 2 else margin), forces
