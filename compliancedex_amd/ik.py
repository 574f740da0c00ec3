"""Batched inverse kinematics on the device: fingertip positions → joint angles (cdx_ik_solve; the rule is
csrc/cdx_ik.h), with the palm's pose as an unknown (solve_ik_pose), or with link orientations as targets and some
joints held (solve_ik_frames).  The reference leaves this to PyBullet's calculateInverseKinematics (verify_pregrasp.py:50-53,
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

IKPoseResult = namedtuple("IKPoseResult", ["q", "palm_pose", "palm_pos", "palm_rot", "err", "iters", "status"])
IKPoseResult.__doc__ = """The free-wrist solve's result: q, err, iters, status as IKResult; palm_pos [E, 3] and palm_rot
[E, 3, 3] float64, the palm pose the solve returns (fingertips = palm_rot·FK(q) + palm_pos + palm_offset), and
palm_pose [E, 6] = palm_pos + the XYZ Euler angles of palm_rot, the form the optimisers and ``forward_kinematics`` take.
A status-2 row has NaN in the three pose fields.  Device tensors."""

IKFrameResult = namedtuple("IKFrameResult", ["q", "err", "rot_err", "iters", "status"])
IKFrameResult.__doc__ = """The pose-target solve's result: q, err, iters, status as IKResult (status 0: every weighted
position AND orientation error ≤ tol); rot_err [E, T] float64, the angle in radians left between each oriented link's
frame and its target (0 for a link without an orientation target, NaN in a status-2 row).  Device tensors."""

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

_Call = namedtuple("_Call", ["lib", "dev", "E", "T", "D", "target", "params", "q0", "dtype", "w", "po", "q", "err",
                             "iters", "status", "chain"])


def _prepare(robot_model, target, target_name, link_names, offsets, q0, palm_offset, weights, ref_q, rho, max_iters,
             tol, lm):
    """What the three solves share → _Call: the target [E, T, 3] (``target_name``: the argument's name in messages),
    the joint box and cdx_ik_params, q0 [E, D], the weights, palm_offset as a ctypes array, the outputs every solve
    has (q, err, iters, status), the chain descriptor and q0's dtype code."""
    lib = N.load()
    dev = robot_model._device
    T, D = len(link_names), robot_model._n_dofs
    target = torch.as_tensor(target, dtype=torch.float64, device=dev)
    if target.ndim == 2 and target.shape == (T, 3):
        target = target.unsqueeze(0)
    if target.ndim != 3 or target.shape[1:] != (T, 3):
        raise ValueError(f"{target_name} must have shape [E, {T}, 3], got {tuple(target.shape)}")
    if not target.is_cuda:
        raise RuntimeError("compliancedex_amd IK runs on the GPU only")
    E = target.shape[0]
    target = target.contiguous()
    lower, upper = joint_box(robot_model.get_joint_limits())
    params = ik_params(lower, upper, _host_list(ref_q), rho, max_iters, tol, **lm)
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
    return _Call(lib, dev, E, T, D, target, params, q0, dtype, w, po_c, q, err, iters, status, chain)


def solve_ik(robot_model, target, link_names, offsets=None, q0=None, palm_pose=None, palm_offset=None, weights=None,
             ref_q=None, rho=0.0, max_iters=50, tol=1e-5, **lm):
    """Joint angles whose fingertips ``link_names`` (+ ``offsets``) reach ``target`` [E, T, 3] → IKResult.

    ``q0`` [E, D] or [D] (float32 / float64; None: ``ref_q``, or the middle of the limits without one);
    ``palm_pose`` [E, 6] or [6]: position + XYZ Euler angles held fixed, as ProbabilisticGraspOptimizer.forward_kinematics
    (None: identity); ``palm_offset`` 3 host floats added to every fingertip, as the Kin optimisers do; ``weights``
    [E, T] or [T] ≥ 0, 0 drops a fingertip; ``ref_q`` (host sequence) and ``rho`` the rest-pose term; ``lm``: mu0,
    mu_min, mu_max, nu.  Limits come from ``get_joint_limits()``.  Runs on the current stream without waiting for it."""
    c = _prepare(robot_model, target, "target", link_names, offsets, q0, palm_offset, weights, ref_q, rho, max_iters,
                 tol, lm)
    palm = _rows(palm_pose, c.E, (6,), "palm_pose", c.dev)
    N.check(c.lib.cdx_ik_solve(c.chain, C.byref(c.params), c.E, N.ptr(c.q0), c.dtype, N.ptr(c.target), N.ptr(palm),
                               c.po, N.ptr(c.w), None, N.ptr(c.q), N.ptr(c.err), N.ptr(c.iters), N.ptr(c.status),
                               N.stream_ptr(c.dev)), "cdx_ik_solve")
    return IKResult(c.q, c.err, c.iters, c.status)


def euler_xyz_matrix(angles):
    """R = (Rx(a)·Ry(b))·Rz(c) [..., 3, 3] float64 of XYZ Euler angles [..., 3], as csrc/cdx_cost.h's euler_xyz builds
    the palm rotation.  Any device, batched."""
    ang = torch.as_tensor(angles, dtype=torch.float64)
    s, c = torch.sin(ang), torch.cos(ang)
    one, zero = torch.ones_like(s[..., 0]), torch.zeros_like(s[..., 0])

    def mat(*rows):
        return torch.stack([torch.stack(r, -1) for r in rows], -2)
    X = mat((one, zero, zero), (zero, c[..., 0], -s[..., 0]), (zero, s[..., 0], c[..., 0]))
    Y = mat((c[..., 1], zero, s[..., 1]), (zero, one, zero), (-s[..., 1], zero, c[..., 1]))
    Z = mat((c[..., 2], -s[..., 2], zero), (s[..., 2], c[..., 2], zero), (zero, zero, one))
    return torch.matmul(torch.matmul(X, Y), Z)


def matrix_to_euler_xyz(R):
    """The inverse of ``euler_xyz_matrix`` for rotations [..., 3, 3] → angles [..., 3] float64 with |b| ≤ π/2.  From
    R = [[cb·cc, −cb·sc, sb], [·, ·, −sa·cb], [·, ·, ca·cb]]: b = atan2(R02, hypot(R00, R01)), a = atan2(−R12, R22),
    c = atan2(−R01, R00).  Where hypot(R00, R01) = 0 (b = ±π/2: a and c act about one axis) c = 0 and
    a = atan2(R21, R11), which is what the matrix reads at c = 0."""
    R = torch.as_tensor(R, dtype=torch.float64)
    h = torch.hypot(R[..., 0, 0], R[..., 0, 1])
    lock = h == 0
    b = torch.atan2(R[..., 0, 2], h)
    a = torch.where(lock, torch.atan2(R[..., 2, 1], R[..., 1, 1]), torch.atan2(-R[..., 1, 2], R[..., 2, 2]))
    c = torch.where(lock, torch.zeros_like(h), torch.atan2(-R[..., 0, 1], R[..., 0, 0]))
    return torch.stack([a, b, c], -1)


def _start_pose(palm_pose0, E, dev):
    """(pos [E, 3], rot [E, 3, 3]) contiguous float64 device tensors of a start pose given as [E, 6] / [6] (position +
    XYZ Euler angles) or as a (pos, rot) pair; (None, None) for None."""
    if palm_pose0 is None:
        return None, None
    if isinstance(palm_pose0, (tuple, list)) and len(palm_pose0) == 2 and hasattr(palm_pose0[1], "shape") \
            and tuple(palm_pose0[1].shape[-2:]) == (3, 3):
        return _rows(palm_pose0[0], E, (3,), "palm_pose0 position", dev), _rows(palm_pose0[1], E, (3, 3),
                                                                               "palm_pose0 rotation", dev)
    pose = _rows(palm_pose0, E, (6,), "palm_pose0", dev)
    return pose[:, :3].contiguous(), euler_xyz_matrix(pose[:, 3:]).contiguous()


def solve_ik_pose(robot_model, target, link_names, offsets=None, q0=None, palm_pose0=None, palm_offset=None,
                  weights=None, ref_q=None, rho=0.0, max_iters=100, tol=1e-5, **lm):
    """Joint angles AND the palm's rigid pose with which the fingertips reach ``target`` [E, T, 3] → IKPoseResult
    (cdx_ik_solve_pose; the rule is ik_pose_row in csrc/cdx_ik.h).  Arguments as ``solve_ik``, but the palm is an
    unknown: ``palm_pose0`` [E, 6] or [6] (position + XYZ Euler angles) or a (pos [E, 3], rot [E, 3, 3]) pair is only the
    start; None starts every row at the weighted Kabsch fit of its start's fingertips onto its targets.  ``rho`` pulls
    the joints towards ``ref_q`` and damps the pose's step; it never pulls the pose.  The pose is not unique where the
    joints can make up for it: different starts give different, equally valid hands
    (results.hand_pose_from_contacts ranks them).  Runs on the current stream without waiting for it."""
    c = _prepare(robot_model, target, "target", link_names, offsets, q0, palm_offset, weights, ref_q, rho, max_iters,
                 tol, lm)
    pos0, rot0 = _start_pose(palm_pose0, c.E, c.dev)
    palm_pos = torch.empty(c.E, 3, dtype=torch.float64, device=c.dev)
    palm_rot = torch.empty(c.E, 3, 3, dtype=torch.float64, device=c.dev)
    N.check(c.lib.cdx_ik_solve_pose(c.chain, C.byref(c.params), c.E, N.ptr(c.q0), c.dtype, N.ptr(c.target),
                                    N.ptr(pos0), N.ptr(rot0), c.po, N.ptr(c.w), None, N.ptr(c.q), N.ptr(palm_pos),
                                    N.ptr(palm_rot), N.ptr(c.err), N.ptr(c.iters), N.ptr(c.status),
                                    N.stream_ptr(c.dev)), "cdx_ik_solve_pose")
    palm_pose = torch.cat([palm_pos, matrix_to_euler_xyz(palm_rot)], 1)
    return IKPoseResult(c.q, palm_pose, palm_pos, palm_rot, c.err, c.iters, c.status)


def quaternion_matrix(quat):
    """Rotation matrices [..., 3, 3] float64 of xyzw quaternions [..., 4] (the convention of
    ``compute_forward_kinematics``), normalised first.  Any device, batched."""
    q = torch.as_tensor(quat).to(torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    rows = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
            2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
            2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]
    return torch.stack(rows, -1).reshape(*q.shape[:-1], 3, 3)


def joint_indices(robot_model, joints):
    """DOF indices of ``joints``: integers, joint names or the names of the links the joints move."""
    chain = robot_model.chain
    by_name = {}
    for i, b in enumerate(chain.bodies):
        if chain.dof[i] >= 0:
            by_name.setdefault(b["name"], chain.dof[i])
            if b.get("joint_name"):
                by_name[b["joint_name"]] = chain.dof[i]
    out = []
    for j in joints:
        if isinstance(j, str):
            if j not in by_name:
                raise KeyError(f"no moving joint named {j!r}")
            j = by_name[j]
        j = int(j)
        if not 0 <= j < chain.n_dofs:
            raise ValueError(f"joint index {j} outside [0, {chain.n_dofs})")
        out.append(j)
    return out


def solve_ik_frames(robot_model, target_pos, target_rot, link_names, offsets=None, q0=None, base_pose=None,
                    palm_offset=None, weights=None, rot_weights=0.1, oriented=None, joints=None, ref_q=None, rho=0.0,
                    max_iters=100, tol=1e-5, **lm):
    """Joint angles with which the links ``link_names`` (+ ``offsets``) reach positions ``target_pos`` [E, T, 3] AND
    orientations ``target_rot`` → IKFrameResult (cdx_ik_solve_frames; the rule is frame_ik_row in csrc/cdx_ik.h).  What
    the reference asks of PyBullet's calculateInverseKinematics with a position and an orientation
    (verify_grasp_robot.py:48-63).

    ``target_rot`` [E, T, 3, 3] rotation matrices or [E, T, 4] xyzw quaternions (the convention of
    ``compute_forward_kinematics``), world frame, converted with torch operators on the device; ``oriented``: one bool
    per link, whether it has an orientation target (default all); ``rot_weights`` a float, [T] or [E, T] in metres per
    radian: the one ``tol`` stops a link when its position error ≤ tol AND rot_weights × its chord ≤ tol (1e-5 m at
    0.1 is 1e-4 rad).  ``joints``: the joints that are solved, by name or index (default all); the others keep their
    ``q0`` (clamped to the limits) and take no part in the ``rho`` term.  ``base_pose`` [E, 6] or [6]: the pose of the
    chain's root (position + XYZ Euler angles; None: identity).  The other arguments are ``solve_ik``'s.  Runs on the
    current stream without waiting for it."""
    c = _prepare(robot_model, target_pos, "target_pos", link_names, offsets, q0, palm_offset, weights, ref_q, rho,
                 max_iters, tol, lm)
    E, T, D, dev = c.E, c.T, c.D, c.dev
    rot = torch.as_tensor(target_rot, device=dev)
    if rot.shape[-1] == 4 and rot.shape[-2:] != (3, 3):
        rot = quaternion_matrix(rot)
    rot = rot.to(torch.float64)
    if rot.shape == (T, 3, 3):
        rot = rot.expand(E, T, 3, 3)
    if rot.shape != (E, T, 3, 3):
        raise ValueError(f"target_rot must have shape [E, {T}, 3, 3] or [E, {T}, 4], got {tuple(rot.shape)}")
    rot = rot.contiguous()
    oriented = [True] * T if oriented is None else [bool(v) for v in oriented]
    if len(oriented) != T:
        raise ValueError(f"oriented must have {T} entries")
    rot_mask = sum(1 << k for k, v in enumerate(oriented) if v)
    solved = range(D) if joints is None else joint_indices(robot_model, joints)
    dof_mask = 0
    for d in solved:
        dof_mask |= 1 << d
    if not dof_mask:
        raise ValueError("joints: at least one joint must be solved")
    base = _rows(base_pose, E, (6,), "base_pose", dev)
    if isinstance(rot_weights, (int, float)):
        rot_weights = [float(rot_weights)] * T
    wr = _rows(rot_weights, E, (T,), "rot_weights", dev)
    chord = torch.empty(E, T, dtype=torch.float64, device=dev)
    N.check(c.lib.cdx_ik_solve_frames(c.chain, C.byref(c.params), E, N.ptr(c.q0), c.dtype, N.ptr(c.target), N.ptr(rot),
                                      N.ptr(base), c.po, N.ptr(c.w), N.ptr(wr), rot_mask, dof_mask, None, N.ptr(c.q),
                                      N.ptr(c.err), N.ptr(chord), N.ptr(c.iters), N.ptr(c.status), N.stream_ptr(dev)),
            "cdx_ik_solve_frames")
    rot_err = 2.0 * torch.asin(torch.clamp(0.5 * chord, max=1.0))
    return IKFrameResult(c.q, c.err, rot_err, c.iters, c.status)
