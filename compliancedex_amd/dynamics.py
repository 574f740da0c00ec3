"""Can the joints hold a compliant grasp?  Joint torques of an optimiser result, and the validator's control law.

The optimisers return springs: fingertip t presses with ``compliance_t · (target_t − contact_t)``.  The reference's
validator turns them into joint torques with ``Jᵀ·F + gravity_compensation()`` (pybullet_robot/controllers/
os_impedance_ctrl.py:32-63) and takes both terms from PyBullet; here they come from the device dynamics of
``DifferentiableRobotModel`` (cdx_dyn_inverse, csrc/cdx_dyn.h).  Nothing here carries autograd.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from .ik import euler_xyz_matrix

HoldingReport = namedtuple("HoldingReport", ["tau", "margin", "feasible", "worst_joint"])
HoldingReport.__doc__ = """tau [E, D] the torques the joints must supply (N·m), margin [E, D] = effort − |tau|,
feasible [E] = every margin ≥ 0, worst_joint [E] = the joint with the smallest margin."""


def _wrist_rotation(wrist, E, device):
    """Rp [E, 3, 3] of wrist [E, 6] = position + XYZ Euler angles (None: identity), the convention of
    ``results.joint_angles_from_contacts``: a world point is Rp·(hand point) + position."""
    if wrist is None:
        return torch.eye(3, dtype=torch.float64, device=device).expand(E, 3, 3)
    wrist = torch.as_tensor(wrist, dtype=torch.float64, device=device)
    if wrist.shape != (E, 6):
        raise ValueError(f"wrist must have shape {(E, 6)}, got {tuple(wrist.shape)}")
    return euler_xyz_matrix(wrist[:, 3:])


def holding_torques(robot_model, hand_config, q, contact, target, compliance, wrist=None,
                    gravity_world=(0.0, 0.0, -9.81), effort=None):
    """The joint torques that hold a result set's grasp, and whether the joints can supply them → HoldingReport.

    ``q`` [E, D] joint angles, ``contact`` / ``target`` [E, T, 3] (world frame) and ``compliance`` [E, T] as the
    optimisers return them, ``wrist`` [E, 6] the palm pose (None: identity).  One cdx_dyn_inverse launch at
    q̇ = q̈ = 0: the fingertips (``hand_config``'s ee_link_name / ee_link_offset) carry the reaction to their springs,
    −compliance·(target − contact), and gravity acts along ``gravity_world``; both are rotated into the hand's base
    frame by the wrist's rotation.  ``effort`` [D] (or a scalar) overrides the URDF's ``limit effort`` — the Allegro
    URDF says 15 N·m, far above the real hand."""
    dev = robot_model._device
    q = torch.as_tensor(q, device=dev)
    if q.dtype not in (torch.float32, torch.float64):
        q = q.to(torch.float64)
    E, D = q.shape
    links, offsets = hand_config["ee_link_name"], hand_config.get("ee_link_offset")
    T = len(links)
    contact = torch.as_tensor(contact, dtype=torch.float64, device=dev).reshape(E, T, 3)
    target = torch.as_tensor(target, dtype=torch.float64, device=dev).reshape(E, T, 3)
    comp = torch.as_tensor(compliance, dtype=torch.float64, device=dev).reshape(E, T)
    Rp = _wrist_rotation(wrist, E, dev)
    reaction = -comp[:, :, None] * (target - contact)                       # on the fingertips, world frame
    tip_forces = torch.einsum("eji,etj->eti", Rp, reaction)                  # Rpᵀ·F
    g = torch.einsum("eji,j->ei", Rp, torch.as_tensor(gravity_world, dtype=torch.float64, device=dev))
    tau = robot_model.compute_inverse_dynamics(q, None, None, True, False, gravity=g, tip_forces=tip_forces,
                                               link_names=links, offsets=offsets)
    limit = robot_model.get_joint_effort_limits() if effort is None else effort
    limit = torch.as_tensor(limit, dtype=tau.dtype, device=dev).expand(D)
    margin = limit - tau.abs()
    return HoldingReport(tau, margin, (margin >= 0).all(1), margin.argmin(1))


def impedance_torques(robot_model, hand_config, q, qd, goal, kP, kD, ref_q=None, gravity=None):
    """The validator's operational-space impedance law (os_impedance_ctrl.py:32-63) → tau [E, D] float64.

    F = kP·(goal − tip) − kD·(J·q̇) per fingertip (``goal`` [E, T, 3] in the hand's base frame, ``kP`` / ``kD`` [T, 3],
    [E, T, 3] or scalars); per finger, over the joints on that finger's path, J_fᵀ·F_f plus the null-space pull
    (I − J_fᵀ·J_f⁺ᵀ)·(ref_q_f − q_f) (``ref_q`` None: the config's); plus ``gravity_compensation``
    (``gravity`` in the base frame).  Torch operators over compute_fingertip_jacobians and the dynamics kernel."""
    dev = robot_model._device
    q = torch.as_tensor(q, device=dev)
    E, D = q.shape
    links, offsets = hand_config["ee_link_name"], hand_config.get("ee_link_offset")
    T = len(links)
    q64 = q.detach().to(torch.float64)
    qd64 = torch.as_tensor(qd, dtype=torch.float64, device=dev).reshape(E, D)
    goal = torch.as_tensor(goal, dtype=torch.float64, device=dev).reshape(E, T, 3)
    kP = torch.as_tensor(kP, dtype=torch.float64, device=dev).expand(E, T, 3)
    kD = torch.as_tensor(kD, dtype=torch.float64, device=dev).expand(E, T, 3)
    ref = torch.as_tensor(hand_config.get("ref_q") if ref_q is None else ref_q, dtype=torch.float64, device=dev).expand(E, D)
    pos, _ = robot_model.compute_forward_kinematics(q.detach(), links, offsets=offsets)
    tip = pos.to(torch.float64).view(E, T, 3)
    J = robot_model.compute_fingertip_jacobians(q, links, offsets)[0].to(torch.float64)   # [E, T, 3, D]
    F = kP * (goal - tip) - kD * torch.einsum("etid,ed->eti", J, qd64)
    tau = torch.zeros(E, D, dtype=torch.float64, device=dev)
    d = robot_model._descriptor(links, offsets)
    for t in range(T):
        joints, b = [], d.tip_body[t]
        while b > 0:
            if d.bodies[b].dof >= 0:
                joints.append(int(d.bodies[b].dof))
            b = d.bodies[b].parent
        joints = sorted(joints)
        Jf = J[:, t][:, :, joints]                                                           # [E, 3, n]
        null = torch.eye(len(joints), dtype=torch.float64, device=dev) - Jf.transpose(1, 2) @ torch.linalg.pinv(Jf).transpose(1, 2)
        tau[:, joints] += torch.einsum("eid,ei->ed", Jf, F[:, t]) + torch.einsum("eij,ej->ei", null, (ref - q64)[:, joints])
    return tau + robot_model.gravity_compensation(q64, gravity=gravity)
