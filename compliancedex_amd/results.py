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


def robustness_for_results(results, obj, mu, mass, com=None, directions=26, g=9.81, exp_name=None, data_dir="data",
                           device="cuda", **report):
    """Does every stored grasp hold an object of ``mass`` kg in any orientation of the hand: ``results`` is
    ``load_results``' dict (or None: the five files are loaded from ``exp_name`` / ``data_dir``); the springs are its
    ``contact``, ``target`` and ``compliance`` rows; the outward normals at the contacts come from ``obj`` — a GPIS
    (``compute_normal``) or a mesh as ``hand.object_distance`` takes it (the signed normal of the TorchSDF query); the
    loads are the weight in ``directions`` directions (``stability.gravity_loads``) acting at ``com`` ([3] or [E, 3];
    None: each grasp's stiffness centre).  → stability.DisturbanceReport; ``report``: options of
    ``stability.disturbance_report`` (limits, tol, max_iters)."""
    import torch
    from .gpis import GPIS
    from .stability import disturbance_report, gravity_loads
    if results is None:
        results = load_results(exp_name, data_dir)
    contact, target, comp = (torch.as_tensor(_np(results[k]), dtype=torch.float64, device=device)
                             for k in ("contact", "target", "compliance"))
    X = contact.reshape(-1, 3).contiguous()
    if isinstance(obj, GPIS):
        normal = obj.compute_normal(X)
    else:
        from .hand import object_distance
        normal = object_distance(obj, X)[1]
    force, point = gravity_loads(mass, g, directions, com)
    return disturbance_report(contact, target, comp, normal.reshape(contact.shape).to(torch.float64), mu, force,
                              com=point, **report)


# ------------------------------------------------------------------ from a stored grasp to the arm
def _chain_of(model):
    return model.chain if hasattr(model, "chain") else model


def _np_fk(desc, q):
    """Float64 FK of a cdx_chain descriptor on the host → (tip positions [B, T, 3], tip-link rotations [B, T, 3, 3]):
    R′ = R·F·A(sign·q), t′ = R·t_b + t, the tip offset rotated by the link.  Set-up arithmetic of ``hand_mount``; the
    solves themselves run on the device."""
    q = np.asarray(q, np.float64)
    B, T = q.shape[0], desc.n_tips
    pos, rot = np.zeros((B, T, 3)), np.zeros((B, T, 3, 3))
    for k in range(T):
        path, b = [], desc.tip_body[k]
        while b > 0:
            path.append(b)
            b = desc.bodies[b].parent
        R, t = np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3))
        for bi in reversed(path):
            body = desc.bodies[bi]
            t = t + R @ np.array(list(body.t), np.float64)
            R = R @ np.array(list(body.F), np.float64).reshape(3, 3)
            if body.dof >= 0:
                th = float(body.sign) * q[:, body.dof]
                A = np.zeros((B, 3, 3))
                i, j = [(1, 2), (2, 0), (0, 1)][body.axis]
                A[:, body.axis, body.axis] = 1.0
                A[:, i, i] = A[:, j, j] = np.cos(th)
                A[:, i, j], A[:, j, i] = -np.sin(th), np.sin(th)
                R = R @ A
        if desc.has_offsets:
            t = t + R @ np.array(list(desc.tip_offset[k]), np.float64)
        pos[:, k], rot[:, k] = t, R
    return pos, rot


def hand_mount(arm_model, hand_model, hand_config, palm_link="palm_link", rows=4, seed=0, residual=False):
    """How the hand-only model sits in the arm model → (R_x [3, 3], t_x [3], joint_map [D_hand]): a point p of the hand
    model's root frame lies at R_x·p + t_x in the arm model's ``palm_link`` frame, and hand joint d is the arm model's
    joint joint_map[d] (matched by the name of the body it moves — the two models order their fingers differently).

    The transform is the Kabsch fit of the hand model's fingertips (``hand_config``'s ee_link_name / ee_link_offset, root
    frame) onto the arm model's fingertips seen from ``palm_link``, over ``rows`` seeded joint rows inside the hand's
    limits, in float64 on the host.  A fit whose largest residual exceeds 1e-6 m raises ValueError: the two models are
    then not the same hand.  ``residual=True`` appends that residual (metres).  The models may be
    DifferentiableRobotModels or Chains."""
    from .ik import joint_box
    arm, hnd = _chain_of(arm_model), _chain_of(hand_model)
    links, offsets = list(hand_config["ee_link_name"]), hand_config.get("ee_link_offset")
    if palm_link not in arm.index:
        raise KeyError(palm_link)
    jmap = []
    for i, b in enumerate(hnd.bodies):
        if hnd.dof[i] < 0:
            continue
        j = arm.index.get(b["name"])
        if j is None or arm.dof[j] < 0:
            raise ValueError(f"the arm model has no moving body named {b['name']!r}")
        jmap.append(arm.dof[j])
    lower, upper = joint_box([dict(lower=b["lower"], upper=b["upper"]) for i, b in enumerate(hnd.bodies) if hnd.dof[i] >= 0])
    lo = np.where(np.isfinite(lower), lower, -np.pi)
    hi = np.where(np.isfinite(upper), upper, np.pi)
    qh = lo + (hi - lo) * np.random.default_rng(seed).random((int(rows), hnd.n_dofs))
    qa = np.zeros((int(rows), arm.n_dofs))
    qa[:, jmap] = qh
    tips_h = _np_fk(hnd.descriptor(links, offsets), qh)[0]
    tips_a = _np_fk(arm.descriptor(links, offsets, check_depth=False), qa)[0]
    pp, Rp = _np_fk(arm.descriptor([palm_link], None, check_depth=False), qa)
    seen = np.einsum("bji,btj->bti", Rp[:, 0], tips_a - pp)  # Rpᵀ·(tip − p_palm)
    a, b = tips_h.reshape(-1, 3), seen.reshape(-1, 3)
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    t = cb - R @ ca
    worst = float(np.linalg.norm(a @ R.T + t - b, axis=1).max())
    if not worst <= 1e-6:
        raise ValueError(f"hand_mount: the fingertips of the two models differ by {worst:.3g} m after the best rigid fit "
                         f"(limit 1e-6 m): they do not describe the same hand")
    out = (R, t, jmap)
    return out + (worst,) if residual else out


def arm_goal_for_results(arm_model, hand_model, hand_config, results, palm_link="palm_link", base_pose=None, q_rest=None,
                         starts=8, spread=0.25, seed=0, hand=None, obj=None, floor_z=None, allow=0.0, lift=None, **ik):
    """Arm-and-hand goal configurations for stored grasps → (q_goal [E, D_arm] float64, status [E] int32, info): what
    the reference asks of PyBullet's calculateInverseKinematics with a position and an orientation
    (verify_grasp_robot.py:48-63, :192-228).

    ``results``: ``load_results``' dict; a grasp is its ``wrist`` row (position + XYZ Euler angles of the hand model's
    root) and its ``joint_angle`` row in the hand-only model.  Through ``hand_mount`` the wrist becomes the target pose
    of the arm model's ``palm_link``, (Rp·R_xᵀ, palm_pos + palm_offset − Rp·R_xᵀ·t_x); the finger joints go into the
    start through the joint map and are HELD, the other joints are solved by ik.solve_ik_frames.  ``base_pose`` [6] or
    [E, 6]: where the arm's root stands.  All E·``starts`` rows run in one launch: start 0 is ``q_rest`` (default: the
    middle of the limits), start k is q_rest + spread·(upper − lower)·u, u uniform in [−1, 1) from a torch.Generator
    seeded with ``seed``, clamped — as ``hand_pose_from_contacts`` seeds its own.  With ``hand`` (the arm model's
    HandSpheres) and ``obj`` / ``floor_z``, ``penetration_report`` runs on every row; ``pick_start`` keeps one start
    per grasp.  ``lift`` = (dx, dy, dz) adds info["lift_goal"] / info["lift_status"]: a second solve, started at each
    kept goal, for the same orientation with the position shifted (the reference's 0.1 m lift, :225-228).

    ``info`` as ``hand_pose_from_contacts``': start, n_converged, n_clear, err / rot_err [E] of the kept rows, ``all`` =
    dict(q [E, S, D], status, werr, clear [E, S] (+ depth)) device tensors; with ``hand`` also depth / clear of the kept
    rows.  ``ik``: options of ik.solve_ik_frames (palm_offset, rot_weights, rho, max_iters, tol, …); ``palm_offset``
    is the hand-only model's, added to the wrist position.  Only the final copy to numpy waits for the device."""
    import torch
    from .ik import euler_xyz_matrix, joint_box, solve_ik_frames
    dev = arm_model._device
    R_x, t_x, jmap = hand_mount(arm_model, hand_model, hand_config, palm_link)
    wrist = torch.as_tensor(_np(results["wrist"]), dtype=torch.float64, device=dev).reshape(-1, 6)
    fingers = torch.as_tensor(_np(results["joint_angle"]), dtype=torch.float64, device=dev)
    E, S, D = wrist.shape[0], int(starts), arm_model._n_dofs
    if S < 1:
        raise ValueError("starts must be at least 1")
    if fingers.shape != (E, len(jmap)):
        raise ValueError(f"joint_angle must have shape {(E, len(jmap))}, got {tuple(fingers.shape)}")
    po = ik.pop("palm_offset", None)
    po = torch.zeros(3, dtype=torch.float64) if po is None else torch.as_tensor(_np(po), dtype=torch.float64).reshape(3)
    Rx = torch.as_tensor(R_x, dtype=torch.float64, device=dev)
    R_l = torch.matmul(euler_xyz_matrix(wrist[:, 3:]), Rx.T)
    p_l = wrist[:, :3] + po.to(dev) - torch.matmul(R_l, torch.as_tensor(t_x, dtype=torch.float64, device=dev))
    lower, upper = joint_box(arm_model.get_joint_limits())
    lo, hi = torch.tensor(lower, dtype=torch.float64), torch.tensor(upper, dtype=torch.float64)
    if q_rest is None:
        q_rest = [0.5 * (a + b) if np.isfinite(a) and np.isfinite(b) else 0.0 for a, b in zip(lower, upper)]
    rest = torch.as_tensor(np.asarray(_np(q_rest), np.float64).reshape(-1))
    span = torch.where(torch.isfinite(hi - lo), hi - lo, torch.full_like(lo, 2.0 * np.pi))
    u = 2.0 * torch.rand(E, S, D, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64) - 1.0
    u[:, 0] = 0.0
    q0 = torch.minimum(torch.maximum(rest + float(spread) * span * u, lo), hi).to(dev)
    q0[:, :, jmap] = fingers[:, None, :]
    q0 = q0.reshape(E * S, D)
    solved = [d for d in range(D) if d not in set(jmap)]
    wr = ik.get("rot_weights", 0.1)
    base = None if base_pose is None else torch.as_tensor(_np(base_pose), dtype=torch.float64, device=dev)
    base_rows = None if base is None else (base.expand(E, 6) if base.ndim == 1 else base).repeat_interleave(S, 0)
    ref_q = ik.pop("ref_q", rest.tolist())

    def run(q_start, pos, rot, palm):
        return solve_ik_frames(arm_model, pos.unsqueeze(1), rot.unsqueeze(1), [palm_link], q0=q_start, base_pose=palm,
                               joints=solved, ref_q=ref_q, **ik)
    res = run(q0, p_l.repeat_interleave(S, 0), R_l.repeat_interleave(S, 0), base_rows)
    werr = torch.maximum(res.err[:, 0], float(wr) * res.rot_err[:, 0]).view(E, S) if isinstance(wr, (int, float)) \
        else torch.maximum(res.err[:, 0], res.rot_err[:, 0]).view(E, S)
    status = res.status.view(E, S)
    every = dict(q=res.q.view(E, S, D), status=status, werr=werr, err=res.err.view(E, S), rot_err=res.rot_err.view(E, S))
    if hand is not None:
        from .hand import penetration_report
        good = (res.status != 2).unsqueeze(1)
        root = torch.zeros(E * S, 6, dtype=torch.float64, device=dev) if base_rows is None else base_rows
        rep = penetration_report(hand, torch.where(good, res.q, q0), root, obj, floor_z, allow)
        every["depth"] = rep["depth"].view(E, S, 3)
        every["clear"] = (rep["clear"] & good[:, 0]).view(E, S)
    else:
        every["clear"] = torch.ones(E, S, dtype=torch.bool, device=dev)
    pick = pick_start(status, every["clear"], werr)
    rows = torch.arange(E, device=dev)
    goal = every["q"][rows, pick].double()
    info = dict(start=pick, n_converged=(status == 0).sum(1), n_clear=every["clear"].sum(1), err=every["err"][rows, pick],
                rot_err=every["rot_err"][rows, pick])
    if hand is not None:
        info["depth"], info["clear"] = every["depth"][rows, pick], every["clear"][rows, pick]
    if lift is not None:
        shift = torch.as_tensor(np.asarray(_np(lift), np.float64).reshape(3), device=dev)
        up = run(goal, p_l + shift, R_l, None if base is None else (base.expand(E, 6) if base.ndim == 1 else base))
        info["lift_goal"], info["lift_status"] = up.q.double(), up.status
    q_goal, st = goal.cpu().numpy(), status[rows, pick].cpu().numpy()
    info = {k: v.cpu().numpy() for k, v in info.items()}
    info["all"] = every
    return q_goal, st, info


def arm_approach_for_results(arm_model, hand_model, hand_config, hand_spheres, q_start, results, obj, floor_z=None,
                             base_pose=None, exp_name=None, data_dir="data", goal=None, **plan):
    """Approach paths of the whole arm from ``q_start`` [D_arm] (or [E, D_arm]) to every stored grasp:
    ``arm_goal_for_results`` (options in the dict ``goal``; ``hand_spheres``, ``obj`` and ``floor_z`` rank its starts
    as well) chained into trajectory.plan_approach with the arm's root at ``base_pose`` → (ApproachPlan, q_goal [E, D_arm],
    status [E], info).  A grasp whose goal has status ≠ 0 has ``success`` False, whatever its path looks like.
    ``results`` None: loaded from ``exp_name`` / ``data_dir``; ``plan``: options of plan_approach."""
    import torch
    from .trajectory import plan_approach
    if results is None:
        results = load_results(exp_name, data_dir)
    q_goal, status, info = arm_goal_for_results(arm_model, hand_model, hand_config, results, base_pose=base_pose,
                                                hand=hand_spheres, obj=obj, floor_z=floor_z, **(goal or {}))
    dev = hand_spheres.device
    base = None if base_pose is None else torch.as_tensor(_np(base_pose), dtype=torch.float64, device=dev)
    out = plan_approach(arm_model, hand_spheres, torch.as_tensor(_np(q_start), dtype=torch.float64, device=dev),
                        torch.as_tensor(q_goal, dtype=torch.float64, device=dev), obj, palm_pose=base, floor_z=floor_z,
                        **plan)
    out.success = out.success & torch.as_tensor(status == 0, device=dev)
    return out, q_goal, status, info
