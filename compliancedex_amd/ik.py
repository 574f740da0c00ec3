"""Batched inverse kinematics on the device: fingertip positions → joint angles (cdx_ik_solve; the rule is
csrc/cdx_ik.h).  The reference leaves this to PyBullet's calculateInverseKinematics (verify_pregrasp.py:50-53,
bullet_robot.py:262-280); here it is one launch for E candidates: Levenberg–Marquardt within the joint limits, float32
FK (the fingertips are ``compute_forward_kinematics``'s bit for bit) and float64 algebra, with the TRUE geometric
Jacobian — not the FK module's autograd gradient, which keeps the reference's detached quaternion scale.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import torch

from . import _native as N

IKResult = namedtuple("IKResult", ["q", "err", "iters", "status"])
IKResult.__doc__ = """q [E, D] (the dtype of q0, float32 values), err [E, T] float64 fingertip distances at q,
iters [E] int32, status [E] int32: 0 converged (largest weighted fingertip error ≤ tol), 1 max_iters used,
2 a non-finite input in the row (q = q0, err = NaN).  Device tensors."""

LM_DEFAULTS = dict(mu0=1e-3, mu_min=1e-9, mu_max=1e6, nu=4.0)


def joint_box(limits):
    """(lower, upper) lists from ``get_joint_limits()``: a joint whose URDF gives lower == upper == 0 (or no limit)
    is unbounded."""
    lo, hi = [], []
    for lim in limits:
        a, b = lim.get("lower"), lim.get("upper")
        if a is None or b is None or (float(a) == 0.0 and float(b) == 0.0):
            a, b = -math.inf, math.inf
        lo.append(float(a))
        hi.append(float(b))
    return lo, hi


def ik_params(lower, upper, ref_q=None, rho=0.0, max_iters=50, tol=1e-5, **lm):
    """cdx_ik_params from host sequences.  ``ref_q`` None: the middle of the limits (0 for an unbounded joint)."""
    unknown = set(lm) - set(LM_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown IK option(s): {sorted(unknown)}")
    lm = {**LM_DEFAULTS, **lm}
    D = len(lower)
    if D > N.MAX_DOFS or len(upper) != D:
        raise ValueError("lower / upper: one entry per joint, at most %d" % N.MAX_DOFS)
    if ref_q is None:
        ref_q = [0.5 * (a + b) if math.isfinite(a) and math.isfinite(b) else
                 (a if math.isfinite(a) else (b if math.isfinite(b) else 0.0)) for a, b in zip(lower, upper)]
    ref_q = [float(v) for v in ref_q]
    if len(ref_q) != D:
        raise ValueError(f"ref_q must have {D} entries")
    p = N.CdxIkParams()
    for d in range(D):
        p.lower[d], p.upper[d], p.ref_q[d] = float(lower[d]), float(upper[d]), ref_q[d]
    p.rho, p.tol, p.max_iters = float(rho), float(tol), int(max_iters)
    p.mu0, p.mu_min, p.mu_max, p.nu = (float(lm[k]) for k in ("mu0", "mu_min", "mu_max", "nu"))
    return p


def _host_list(x):
    """A host list of floats (a device tensor is copied to the host, which waits for it: pass host data)."""
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu()
    return [float(v) for v in (x.reshape(-1).tolist() if hasattr(x, "reshape") else x)]


def _rows(x, E, shape, name, device):
    """x as a contiguous float64 device tensor [E, *shape]; one row is repeated for every candidate."""
    if x is None:
        return None
    x = torch.as_tensor(x, dtype=torch.float64, device=device)
    if x.shape == tuple(shape):
        x = x.expand(E, *shape)
    if x.shape != (E, *shape):
        raise ValueError(f"{name} must have shape {(E, *shape)} or {tuple(shape)}, got {tuple(x.shape)}")
    return x.contiguous()


def solve_ik(robot_model, target, link_names, offsets=None, q0=None, palm_pose=None, palm_offset=None, weights=None,
             ref_q=None, rho=0.0, max_iters=50, tol=1e-5, **lm):
    """Joint angles whose fingertips ``link_names`` (+ ``offsets``) reach ``target`` [E, T, 3] → IKResult.

    ``q0`` [E, D] or [D] (float32 / float64; None: ``ref_q``, or the middle of the limits without one);
    ``palm_pose`` [E, 6] or [6]: position + XYZ Euler angles held fixed, as ProbabilisticGraspOptimizer.forward_kinematics
    (None: identity); ``palm_offset`` 3 host floats added to every fingertip, as the Kin optimisers do; ``weights``
    [E, T] or [T] ≥ 0, 0 drops a fingertip; ``ref_q`` (host sequence) and ``rho`` the rest-pose term; ``lm``: mu0,
    mu_min, mu_max, nu.  Limits come from ``get_joint_limits()``.  Runs on the current stream without waiting for it."""
    lib = N.load()
    dev = robot_model._device
    T, D = len(link_names), robot_model._n_dofs
    target = torch.as_tensor(target, dtype=torch.float64, device=dev)
    if target.ndim == 2 and target.shape == (T, 3):
        target = target.unsqueeze(0)
    if target.ndim != 3 or target.shape[1:] != (T, 3):
        raise ValueError(f"target must have shape [E, {T}, 3], got {tuple(target.shape)}")
    if not target.is_cuda:
        raise RuntimeError("compliancedex_amd IK runs on the GPU only")
    E = target.shape[0]
    target = target.contiguous()
    lower, upper = joint_box(robot_model.get_joint_limits())
    ref = _host_list(ref_q)
    params = ik_params(lower, upper, ref, rho, max_iters, tol, **lm)
    if q0 is None:
        q0 = torch.tensor([params.ref_q[d] for d in range(D)], dtype=torch.float64, device=dev)
    else:
        q0 = torch.as_tensor(q0, device=dev)
        if q0.dtype not in (torch.float32, torch.float64):
            q0 = q0.to(torch.float64)
    if q0.shape == (D,):
        q0 = q0.expand(E, D)
    if q0.shape != (E, D):
        raise ValueError(f"q0 must have shape {(E, D)} or {(D,)}, got {tuple(q0.shape)}")
    q0 = q0.detach().contiguous()
    palm = _rows(palm_pose, E, (6,), "palm_pose", dev)
    w = _rows(weights, E, (T,), "weights", dev)
    po = _host_list(palm_offset)
    if po is not None and len(po) != 3:
        raise ValueError("palm_offset must have 3 entries")
    po_c = (C.c_double * 3)(*po) if po is not None else None
    q = torch.empty_like(q0)
    err = torch.empty(E, T, dtype=torch.float64, device=dev)
    iters = torch.empty(E, dtype=torch.int32, device=dev)
    status = torch.empty(E, dtype=torch.int32, device=dev)
    chain = robot_model._descriptor(link_names, offsets)
    dtype = N.DTYPE_F64 if q0.dtype == torch.float64 else N.DTYPE_F32
    N.check(lib.cdx_ik_solve(chain, C.byref(params), E, N.ptr(q0), dtype, N.ptr(target), N.ptr(palm), po_c, N.ptr(w),
                             None, N.ptr(q), N.ptr(err), N.ptr(iters), N.ptr(status), N.stream_ptr(dev)),
            "cdx_ik_solve")
    return IKResult(q, err, iters, status)
