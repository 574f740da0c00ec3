"""Optimiser results in the reference's on-disk format.

Writer: optimize_pregrasp.py:1016-1020 saves five float64 arrays per experiment under data/:
  contact_<exp>.npy [E,4,3] (fingertips at the optimum: forward_kinematics(q, palm), :1009),
  target_<exp>.npy [E,4,3], wrist_<exp>.npy [E,6], compliance_<exp>.npy [E,4],
  joint_angle_<exp>.npy [E,16].
Readers: verify_pregrasp.py:147-155 (contact / target / compliance), verify_grasp_robot.py:150-154.
"""
from __future__ import annotations

import os

import numpy as np

NAMES = ("contact", "target", "wrist", "compliance", "joint_angle")


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def save_results(exp_name, contact, target, wrist, compliance, joint_angle, data_dir="data"):
    os.makedirs(data_dir, exist_ok=True)
    paths = []
    for name, arr in zip(NAMES, (contact, target, wrist, compliance, joint_angle)):
        path = os.path.join(data_dir, f"{name}_{exp_name}.npy")
        np.save(path, _np(arr))
        paths.append(path)
    return paths


def load_results(exp_name, data_dir="data"):
    return {name: np.load(os.path.join(data_dir, f"{name}_{exp_name}.npy")) for name in NAMES}


def optimize_and_save(optimizer, gpis, init_joint_angles, target_pose, compliance, exp_name, friction_mu=1,
                      data_dir="data", **kw):
    """optimize → FK of the optimum → save, as optimize_pregrasp.py:1008-1020 does (headless)."""
    q, comp, target, palm, margin = optimizer.optimize(init_joint_angles, target_pose, compliance, friction_mu, gpis,
                                                       **kw)
    contact = optimizer.forward_kinematics(q, palm)
    save_results(exp_name, contact, target, palm, comp, q, data_dir)
    return dict(joint_angle=q, compliance=comp, target=target, wrist=palm, margin=margin, contact=contact)


def joint_angles_from_contacts(robot_model, hand_config, contact, wrist=None, q0=None, **ik):
    """Joint angles for a result set's ``contact`` [E, T, 3] (and its ``wrist`` [E, 6] rows, if it has them) by the
    device IK → (joint_angle [E, D] float64, status [E] int32; 0 = reached within tol).  This fills
    ``save_results(..., joint_angle)`` for the fingertip-space optimisers (GPISGraspOptimizer, SDFGraspOptimizer), whose
    result the reference's writer cannot complete (optimize_pregrasp.py:1005, :1020).  ``hand_config``: the robot's
    config dict (ee_link_name, ee_link_offset, ref_q); ``q0`` None starts at ref_q; ``ik``: options of
    ik.solve_ik (palm_offset, weights, rho, max_iters, tol, …).  Copies the result to the host.  ``wrist`` None holds the
    palm at the identity; a result without a wrist wants ``hand_pose_from_contacts``, which solves for it."""
    import torch
    dev = robot_model._device
    contact = torch.as_tensor(contact, dtype=torch.float64, device=dev)
    if wrist is not None:
        wrist = torch.as_tensor(wrist, dtype=torch.float64, device=dev)
    ref_q = ik.pop("ref_q", hand_config.get("ref_q"))
    res = robot_model.inverse_kinematics(contact, hand_config["ee_link_name"], hand_config.get("ee_link_offset"), q0=q0,
                                         palm_pose=wrist, ref_q=ref_q, **ik)
    return res.q.double().cpu().numpy(), res.status.cpu().numpy()


def pick_start(status, clear, werr):
    """The best start per grasp of [E, S] device tensors → index [E] int64: lexicographic on (status ≠ 0, not clear,
    largest weighted error); a NaN error counts as +inf.  Torch operators only."""
    import torch
    cls = (status != 0).to(torch.int64) * 2 + (~clear).to(torch.int64)
    werr = torch.where(torch.isnan(werr), torch.full_like(werr, float("inf")), werr)
    best = cls == cls.amin(1, keepdim=True)
    return torch.where(best, werr, torch.full_like(werr, float("inf"))).argmin(1)


def hand_pose_from_contacts(robot_model, hand_config, contact, starts=8, spread=0.25, seed=0, hand=None, obj=None,
                            floor_z=None, allow=0.0, **ik):
    """A whole hand for a result set that has contacts but no wrist (GPISGraspOptimizer, SDFGraspOptimizer): joint
    angles and palm pose by the free-wrist IK (ik.solve_ik_pose) → (joint_angle [E, D] float64, wrist [E, 6] float64,
    status [E] int32, info), so that ``save_results`` can write the reference's five files.

    The pose is not unique, so every grasp is solved from ``starts`` joint starts in ONE launch of E·starts rows: start 0
    is ref_q, start k is ref_q + spread·(upper − lower)·u with u uniform in [−1, 1) from a ``torch.Generator`` seeded
    with ``seed`` (2π stands for the range of an unbounded joint), clamped to the limits; every start takes the Kabsch
    start for its pose, so different joint starts give different wrist fits.  With ``hand`` (a HandSpheres) and ``obj``
    / ``floor_z``, ``penetration_report(hand, q, wrist, obj, floor_z, allow)`` runs on all rows.  The start kept per
    grasp is the least in the order (status ≠ 0, not clear, largest weighted fingertip error) — ``pick_start``.

    ``info``: start [E] the kept start, n_converged [E], n_clear [E] (every start counts as clear without ``hand``), and
    ``all`` = dict(q [E, S, D], wrist [E, S, 6], status, werr, clear [E, S] (+ depth [E, S, 3] with ``hand``)), device
    tensors; with ``hand`` also depth [E, 3] and clear [E] of the kept rows, numpy.  ``ik``: options of
    ik.solve_ik_pose (palm_offset, weights [E, T] or [T], rho, max_iters, tol, …).  Only the final copy to numpy waits for
    the device."""
    import torch
    from .ik import joint_box, solve_ik_pose
    dev = robot_model._device
    contact = torch.as_tensor(contact, dtype=torch.float64, device=dev)
    E, T, S, D = contact.shape[0], contact.shape[1], int(starts), robot_model._n_dofs
    if S < 1:
        raise ValueError("starts must be at least 1")
    ref_q = ik.pop("ref_q", hand_config.get("ref_q"))
    lower, upper = joint_box(robot_model.get_joint_limits())
    lo, hi = torch.tensor(lower, dtype=torch.float64), torch.tensor(upper, dtype=torch.float64)
    if ref_q is None:
        ref_q = [0.5 * (a + b) if np.isfinite(a) and np.isfinite(b) else 0.0 for a, b in zip(lower, upper)]
    ref = torch.as_tensor(np.asarray(_np(ref_q), np.float64).reshape(-1))
    span = torch.where(torch.isfinite(hi - lo), hi - lo, torch.full_like(lo, 2.0 * np.pi))
    u = 2.0 * torch.rand(E, S, D, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64) - 1.0
    u[:, 0] = 0.0
    q0 = torch.minimum(torch.maximum(ref + float(spread) * span * u, lo), hi).reshape(E * S, D).to(dev)
    w = ik.pop("weights", None)
    if w is not None:
        w = torch.as_tensor(w, dtype=torch.float64, device=dev)
        w = (w.expand(E, T) if w.ndim == 1 else w).repeat_interleave(S, 0)
    res = solve_ik_pose(robot_model, contact.repeat_interleave(S, 0), hand_config["ee_link_name"],
                        hand_config.get("ee_link_offset"), q0=q0, weights=w, ref_q=ref.tolist(), **ik)
    werr = (res.err if w is None else res.err * w).amax(1).view(E, S)
    status = res.status.view(E, S)
    every = dict(q=res.q.view(E, S, D), wrist=res.palm_pose.view(E, S, 6), status=status, werr=werr)
    if hand is not None:
        from .hand import penetration_report
        good = (res.status != 2).unsqueeze(1)  # (a status-2 row has no pose: report it at the start, never clear)
        rep = penetration_report(hand, torch.where(good, res.q, q0),
                                 torch.where(good, res.palm_pose, torch.zeros_like(res.palm_pose)), obj, floor_z, allow)
        every["depth"] = rep["depth"].view(E, S, 3)
        every["clear"] = (rep["clear"] & good[:, 0]).view(E, S)
    else:
        every["clear"] = torch.ones(E, S, dtype=torch.bool, device=dev)
    pick = pick_start(status, every["clear"], werr)
    rows = torch.arange(E, device=dev)
    info = dict(start=pick, n_converged=(status == 0).sum(1), n_clear=every["clear"].sum(1))
    if hand is not None:
        info["depth"], info["clear"] = every["depth"][rows, pick], every["clear"][rows, pick]
    out = (every["q"][rows, pick].double(), every["wrist"][rows, pick], status[rows, pick])
    joint_angle, wrist, st = (t.cpu().numpy() for t in out)
    info = {k: v.cpu().numpy() for k, v in info.items()}
    info["all"] = every
    return joint_angle, wrist, st, info


def approach_for_results(robot_model, hand, q_start, results, obj, floor_z=None, exp_name=None, data_dir="data", **plan):
    """Approach paths from ``q_start`` [D] (or [E, D]) to every stored grasp: ``results`` is ``load_results``' dict (or
    None: loaded from ``exp_name`` / ``data_dir``); the goal of grasp e is its ``joint_angle`` row, the chain's root
    stands at its ``wrist`` row.  → trajectory.ApproachPlan; ``plan``: options of trajectory.plan_approach."""
    import torch
    from .trajectory import plan_approach
    if results is None:
        results = load_results(exp_name, data_dir)
    dev = hand.device
    goal = torch.as_tensor(_np(results["joint_angle"]), dtype=torch.float64, device=dev)
    wrist = results.get("wrist")
    wrist = None if wrist is None else torch.as_tensor(_np(wrist), dtype=torch.float64, device=dev)
    return plan_approach(robot_model, hand, torch.as_tensor(_np(q_start), dtype=torch.float64, device=dev), goal, obj,
                         palm_pose=wrist, floor_z=floor_z, **plan)
