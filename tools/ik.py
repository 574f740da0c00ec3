"""Batched inverse kinematics (cdx_ik_solve) timed on the GPU: E = 4096, 16 384 and 65 536 candidates of the Allegro hand
(D = 16) and of iiwa7_allegro (D = 23, the fingertip links and offsets of the FK fixture's case), targets FK(q*) with q*
in the inner 80 % of every joint range, starts q* ± 0.3 rad (± 0.2 rad for the arm) clamped to the limits.

Per shape: the one-launch solve (the time of ``solve_ik``, which allocates its four outputs); a torch statement of the
same rule on the device — fingertips from ``compute_forward_kinematics``, the Jacobian from
``compute_fingertip_jacobians``, batched ``torch.linalg.solve_ex`` for the 3T × 3T systems, row masks for the per-row stop and one
``any()`` per iteration to end the loop —; and the host build of the rule on one core (cdxh_ik_solve, wall clock) up
to --host-rows.  Besides the times the record keeps the share of rows each path converged, the iteration counts, and how
far the torch statement's joint angles are from the kernel's.

The free-wrist solve (cdx_ik_solve_pose, ``solve_ik_pose``) is timed beside it on the same q* and q0: targets the
fingertips of (q*, palm*) with palm* within ±0.2 m and XYZ angles (±π, ±1.2, ±π), the start pose palm* moved by ≤ 0.05 m
per axis and turned by ≤ 0.3 rad about a random axis — the family of tests/_ik_pose.py —, once with that start pose and
once with the Kabsch start; its own torch statement (``torch_ik_pose``) and its host build on one core
(cdxh_ik_solve_pose) are the yardsticks, and ``pose_over_fixed`` is its time over the fixed-palm solve's at the same E.
Iteration medians and the share of rows that use all ``max_iters`` iterations (status 1) are kept for every path.

The pose-target solve (cdx_ik_solve_frames, ``solve_ik_frames``) is the ``frames`` shape: on iiwa7_allegro the one link
``palm_link`` with its orientation, the seven arm joints solved and the sixteen finger joints held — the arm goal of a
stored grasp —, on the Allegro hand its four fingertips with the first one oriented; targets the FK pose of q*, starts
q* ± 0.3 rad.  Its yardsticks are the same rule in torch operators (``torch_ik_frames``) and the host build on one core
(cdxh_ik_solve_frames).

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.

Without --robot the tool is the driver: every shape runs in a child process of its own under ``timeout``, one after the
other, and the first that fails, faults or runs out of time ends the run.  One JSON line per shape is printed and
appended to the record (default profiles/ik.jsonl).  Needs a GPU: there is no fallback.

  python tools/ik.py [--reps 7] [--rows 4096,16384,65536] [--robots allegro,iiwa7_allegro] [--shapes fingertips,frames]
                     [--out PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.fps import event_ms, stats  # noqa: E402

IIWA7_LINKS = ["link_3.0_tip", "link_7.0_tip", "link_11.0_tip", "link_15.0_tip"]
IIWA7_OFFSETS = [[0.0, -0.04, 0.015], [0.0, -0.04, 0.015], [0.0, -0.04, 0.015], [0.0, -0.05, -0.015]]


def inputs(rm, links, offsets, E, spread, seed=0):
    """(q0, target, lo, hi, q*) — all but q* on the device: q* in the inner 80 % of the joint box, q0 = q* ± spread
    clamped."""
    import torch
    from compliancedex_amd.ik import joint_box
    lower, upper = joint_box(rm.get_joint_limits())
    lo, hi = torch.tensor(lower, dtype=torch.float64), torch.tensor(upper, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    qs = mid + 0.8 * half * (2.0 * torch.rand(E, len(lower), generator=g, dtype=torch.float64) - 1.0)
    q0 = torch.minimum(torch.maximum(qs + spread * (2.0 * torch.rand(qs.shape, generator=g, dtype=torch.float64) - 1.0),
                                     lo), hi)
    target = rm.compute_forward_kinematics(qs.cuda().float(), links, offsets=offsets)[0].double().view(E, len(links), 3)
    return q0.cuda(), target, lo.cuda(), hi.cuda(), qs


def torch_ik(rm, links, offsets, q0, target, lo, hi, max_iters=50, tol=1e-5, mu0=1e-3, mu_min=1e-9, mu_max=1e6, nu=4.0):
    """The rule of csrc/cdx_ik.h (ρ = 0, no palm, unit weights) with torch operators on the device."""
    import torch
    E, D = q0.shape
    T = len(links)
    lo32, hi32 = lo.float(), hi.float()

    def residual(q32):
        tips = rm.compute_forward_kinematics(q32, links, offsets=offsets)[0].double().view(E, T, 3)
        return (target - tips).reshape(E, 3 * T)

    q = torch.minimum(torch.maximum(q0.float(), lo32), hi32)
    r = residual(q)
    cost = 0.5 * (r * r).sum(1)
    mu = torch.full((E,), mu0, dtype=torch.float64, device=q0.device)
    iters = torch.zeros(E, dtype=torch.int32, device=q0.device)
    eye = torch.eye(3 * T, dtype=torch.float64, device=q0.device)
    for _ in range(max_iters):
        act = r.view(E, T, 3).norm(dim=2).amax(1) > tol
        if not bool(act.any()):
            break
        iters += act
        J = rm.compute_fingertip_jacobians(q, links, offsets)[0].double().view(E, 3 * T, D)
        g = torch.bmm(J.transpose(1, 2), r.unsqueeze(2)).squeeze(2)
        qd = q.double()
        free = ~(((qd <= lo) & (g < 0)) | ((qd >= hi) & (g > 0)))
        J = J * free.unsqueeze(1)
        g = g * free
        A = torch.bmm(J, J.transpose(1, 2)) + mu.view(E, 1, 1) * eye
        # (solve_ex, not cholesky_ex: with the Cholesky pair no row converged at E = 65 536 and fewer did as E grew,
        # though both are right on well-conditioned batches of that size; LU with pivoting has no pivot to fail on)
        y, info = torch.linalg.solve_ex(A, torch.bmm(J, g.unsqueeze(2)))
        delta = (g - torch.bmm(J.transpose(1, 2), y).squeeze(2)) / mu.view(E, 1)
        qn = torch.minimum(torch.maximum(qd + delta, lo), hi).float()
        rn = residual(qn)
        cn = 0.5 * (rn * rn).sum(1)
        ok = act & (info == 0) & (cn < cost)
        q = torch.where(ok.unsqueeze(1), qn, q)
        r = torch.where(ok.unsqueeze(1), rn, r)
        cost = torch.where(ok, cn, cost)
        mu = torch.where(act, torch.where(ok, (mu / nu).clamp(min=mu_min), (mu * nu).clamp(max=mu_max)), mu)
    return q, r.view(E, T, 3).norm(dim=2), iters


def pose_inputs(rm, links, offsets, qs, E, seed=1):
    """(target, pos0, rot0) on the device for q* ``qs``: the fingertips of (q*, palm*) and the displaced start pose."""
    import math
    import torch
    from compliancedex_amd.ik import euler_xyz_matrix
    g = torch.Generator().manual_seed(seed)

    def rand(*shape):
        return 2.0 * torch.rand(*shape, generator=g, dtype=torch.float64) - 1.0
    pos = 0.2 * rand(E, 3)
    rot = euler_xyz_matrix(rand(E, 3) * torch.tensor([math.pi, 1.2, math.pi], dtype=torch.float64))
    axis = torch.nn.functional.normalize(torch.randn(E, 3, generator=g, dtype=torch.float64), dim=1)
    ang = 0.3 * rand(E, 1)
    K = torch.zeros(E, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -axis[:, 2], axis[:, 1], axis[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 0], -axis[:, 1], axis[:, 0]
    turn = torch.eye(3, dtype=torch.float64) + torch.sin(ang)[:, :, None] * K + (1 - torch.cos(ang))[:, :, None] * (K @ K)
    pos0, rot0 = pos + 0.05 * rand(E, 3), rot @ turn
    local = rm.compute_forward_kinematics(qs.cuda().float(), links, offsets=offsets)[0].double().view(E, len(links), 3)
    target = torch.einsum("eij,etj->eti", rot.cuda(), local) + pos.cuda()[:, None]
    return target.contiguous(), pos0.cuda().contiguous(), rot0.cuda().contiguous()


def torch_ik_pose(rm, links, offsets, q0, target, pos0, rot0, lo, hi, max_iters=100, tol=1e-5, mu0=1e-3, mu_min=1e-9,
                  mu_max=1e6, nu=4.0):
    """ik_pose_row of csrc/cdx_ik.h (ρ = 0, unit weights, a given start pose) with torch operators on the device."""
    import torch
    E, D = q0.shape
    T = len(links)
    lo32, hi32 = lo.float(), hi.float()
    dev = q0.device

    def residual(q32, R, p):
        v = rm.compute_forward_kinematics(q32, links, offsets=offsets)[0].double().view(E, T, 3)
        return target - (torch.einsum("eij,etj->eti", R, v) + p[:, None]), v

    q, R, p = torch.minimum(torch.maximum(q0.float(), lo32), hi32), rot0.clone(), pos0.clone()
    r, v = residual(q, R, p)
    cost = 0.5 * (r * r).sum((1, 2))
    mu = torch.full((E,), mu0, dtype=torch.float64, device=dev)
    iters = torch.zeros(E, dtype=torch.int32, device=dev)
    eye = torch.eye(3 * T, dtype=torch.float64, device=dev)
    eye3 = torch.eye(3, dtype=torch.float64, device=dev)
    for _ in range(max_iters):
        act = r.norm(dim=2).amax(1) > tol
        if not bool(act.any()):
            break
        iters += act
        J = torch.zeros(E, T, 3, D + 6, dtype=torch.float64, device=dev)
        J[..., :D] = rm.compute_fingertip_jacobians(q, links, offsets)[0].double()
        J[..., D:D + 3] = eye3
        J[:, :, 0, D + 4], J[:, :, 0, D + 5] = v[:, :, 2], -v[:, :, 1]
        J[:, :, 1, D + 3], J[:, :, 1, D + 5] = -v[:, :, 2], v[:, :, 0]
        J[:, :, 2, D + 3], J[:, :, 2, D + 4] = v[:, :, 1], -v[:, :, 0]
        J = J.view(E, 3 * T, D + 6)
        u = torch.einsum("eji,etj->eti", R, r).reshape(E, 3 * T)
        g = torch.bmm(J.transpose(1, 2), u.unsqueeze(2)).squeeze(2)
        qd = q.double()
        free = torch.ones(E, D + 6, dtype=torch.bool, device=dev)
        free[:, :D] = ~(((qd <= lo) & (g[:, :D] < 0)) | ((qd >= hi) & (g[:, :D] > 0)))
        J = J * free.unsqueeze(1)
        g = g * free
        A = torch.bmm(J, J.transpose(1, 2)) + mu.view(E, 1, 1) * eye
        y, info = torch.linalg.solve_ex(A, torch.bmm(J, g.unsqueeze(2)))
        delta = (g - torch.bmm(J.transpose(1, 2), y).squeeze(2)) / mu.view(E, 1)
        qn = torch.minimum(torch.maximum(qd + delta[:, :D], lo), hi).float()
        pn = p + torch.einsum("eij,ej->ei", R, delta[:, D:D + 3])
        a = 0.5 * delta[:, D + 3:]
        s = (a * a).sum(1).view(E, 1, 1)
        ax = torch.zeros(E, 3, 3, dtype=torch.float64, device=dev)
        ax[:, 0, 1], ax[:, 0, 2], ax[:, 1, 0] = -a[:, 2], a[:, 1], a[:, 2]
        ax[:, 1, 2], ax[:, 2, 0], ax[:, 2, 1] = -a[:, 0], -a[:, 1], a[:, 0]
        Rn = R @ (((1 - s) * eye3 + 2 * a[:, :, None] * a[:, None, :] + 2 * ax) / (1 + s))
        rn, vn = residual(qn, Rn, pn)
        cn = 0.5 * (rn * rn).sum((1, 2))
        ok = act & (info == 0) & (cn < cost)
        q = torch.where(ok.unsqueeze(1), qn, q)
        p = torch.where(ok.unsqueeze(1), pn, p)
        R = torch.where(ok.view(E, 1, 1), Rn, R)
        r = torch.where(ok.view(E, 1, 1), rn, r)
        v = torch.where(ok.view(E, 1, 1), vn, v)
        cost = torch.where(ok, cn, cost)
        mu = torch.where(act, torch.where(ok, (mu / nu).clamp(min=mu_min), (mu * nu).clamp(max=mu_max)), mu)
    return q, r.norm(dim=2), iters


def host_pose_seconds(rm, links, offsets, q0, target, pos0, rot0):
    """Seconds of cdxh_ik_solve_pose on one core, and its status / iteration arrays."""
    import numpy as np
    from compliancedex_amd import _host, _native as N
    from compliancedex_amd.ik import ik_params, joint_box
    lib, p = _host.load(), _host.ptr
    params = ik_params(*joint_box(rm.get_joint_limits()), max_iters=100)
    desc = rm._descriptor(links, offsets)
    q0, target, pos0, rot0 = (np.ascontiguousarray(t.cpu().numpy()) for t in (q0, target, pos0, rot0))
    E, T = q0.shape[0], len(links)
    q, pp, pr, err = np.empty_like(q0), np.empty((E, 3)), np.empty((E, 9)), np.empty((E, T))
    iters, status = np.empty(E, np.int32), np.empty(E, np.int32)
    t = time.perf_counter()
    rc = lib.cdxh_ik_solve_pose(desc, params, E, p(q0), N.DTYPE_F64, p(target), p(pos0), p(rot0), None, None, p(q), p(pp),
                                p(pr), p(err), p(iters), p(status))
    dt = time.perf_counter() - t
    assert rc == 0
    return dt, status, iters


def host_seconds(rm, links, offsets, q0, target):
    """Seconds of cdxh_ik_solve on one core, and its status / iteration arrays."""
    import numpy as np
    from compliancedex_amd import _host, _native as N
    from compliancedex_amd.ik import ik_params, joint_box
    lib, p = _host.load(), _host.ptr
    params = ik_params(*joint_box(rm.get_joint_limits()))
    desc = rm._descriptor(links, offsets)
    q0, target = np.ascontiguousarray(q0.cpu().numpy()), np.ascontiguousarray(target.cpu().numpy())
    E, T = q0.shape[0], len(links)
    q, err = np.empty_like(q0), np.empty((E, T))
    iters, status = np.empty(E, np.int32), np.empty(E, np.int32)
    t = time.perf_counter()
    rc = lib.cdxh_ik_solve(desc, params, E, p(q0), N.DTYPE_F64, p(target), None, None, None, p(q), p(err), p(iters),
                           p(status))
    dt = time.perf_counter() - t
    assert rc == 0
    return dt, status, iters


def run_shape(robot, E, args):
    import numpy as np
    import torch
    from compliancedex_amd import DifferentiableRobotModel, solve_ik, solve_ik_pose
    rm = DifferentiableRobotModel(robot, device="cuda")
    if robot == "iiwa7_allegro":
        links, offsets, spread = IIWA7_LINKS, IIWA7_OFFSETS, 0.2
    else:
        links, offsets, spread = rm.chain.config["ee_link_name"], rm.chain.config["ee_link_offset"], 0.3
    q0, target, lo, hi, qs = inputs(rm, links, offsets, E, spread)
    ptarget, pos0, rot0 = pose_inputs(rm, links, offsets, qs, E)
    paths = {"kernel": lambda: solve_ik(rm, target, links, offsets, q0=q0),
             "torch": lambda: torch_ik(rm, links, offsets, q0, target, lo, hi),
             "pose_kernel": lambda: solve_ik_pose(rm, ptarget, links, offsets, q0=q0, palm_pose0=(pos0, rot0)),
             "pose_kernel_kabsch": lambda: solve_ik_pose(rm, ptarget, links, offsets, q0=q0),
             "pose_torch": lambda: torch_ik_pose(rm, links, offsets, q0, ptarget, pos0, rot0, lo, hi)}
    for f in paths.values():  # warm-up: code objects, allocator blocks
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(args.reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    rec = {"robot": robot, "E": E, "D": rm._n_dofs, "T": len(links), **{n: stats(v) for n, v in ms.items()}}
    res = paths["kernel"]()
    tq, terr, titers = paths["torch"]()
    rec["kernel_converged"] = round(float((res.status == 0).double().mean()), 5)
    rec["kernel_iters_median_max"] = [int(res.iters.median()), int(res.iters.max())]
    rec["torch_converged"] = round(float((terr.amax(1) <= 1e-5).double().mean()), 5)
    rec["torch_iters_median_max"] = [int(titers.median()), int(titers.max())]
    rec["torch_q_max_abs_diff"] = float((tq.double() - res.q).abs().max())
    rec["torch_over_kernel"] = round(rec["torch"]["median_ms"] / rec["kernel"]["median_ms"], 1)
    if E <= args.host_rows:
        sec, hstatus, hiters = host_seconds(rm, links, offsets, q0, target)
        rec["host_one_core_ms"] = round(sec * 1e3, 2)
        rec["host_converged"] = round(float((hstatus == 0).mean()), 5)
        rec["host_over_kernel"] = round(sec * 1e3 / rec["kernel"]["median_ms"], 1)
    for name in ("pose_kernel", "pose_kernel_kabsch"):
        pres = paths[name]()
        rec[name + "_converged"] = round(float((pres.status == 0).double().mean()), 5)
        rec[name + "_all_iters_share"] = round(float((pres.status == 1).double().mean()), 5)
        rec[name + "_iters_median_max"] = [int(pres.iters.median()), int(pres.iters.max())]
    pres = paths["pose_kernel"]()
    pq, perr, piters = paths["pose_torch"]()
    rec["pose_torch_converged"] = round(float((perr.amax(1) <= 1e-5).double().mean()), 5)
    rec["pose_torch_iters_median_max"] = [int(piters.median()), int(piters.max())]
    rec["pose_torch_q_max_abs_diff"] = float((pq.double() - pres.q).abs().max())
    rec["pose_torch_over_kernel"] = round(rec["pose_torch"]["median_ms"] / rec["pose_kernel"]["median_ms"], 1)
    rec["pose_over_fixed"] = round(rec["pose_kernel"]["median_ms"] / rec["kernel"]["median_ms"], 2)
    rec["kernel_all_iters_share"] = round(float((res.status == 1).double().mean()), 5)
    if E <= args.host_rows:
        sec, hstatus, hiters = host_pose_seconds(rm, links, offsets, q0, ptarget, pos0, rot0)
        rec["pose_host_one_core_ms"] = round(sec * 1e3, 2)
        rec["pose_host_converged"] = round(float((hstatus == 0).mean()), 5)
        rec["pose_host_iters_median_max"] = [int(np.median(hiters)), int(hiters.max())]
        rec["pose_host_over_kernel"] = round(sec * 1e3 / rec["pose_kernel"]["median_ms"], 1)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def frames_case(rm, robot, E, spread=0.3, seed=2):
    """(links, offsets, oriented, solved joints, q0, target, rot, lo, hi) of the ``frames`` shape, tensors on the device."""
    import torch
    from compliancedex_amd.ik import quaternion_matrix
    if robot == "iiwa7_allegro":
        links, offsets, oriented, solved = ["palm_link"], None, [True], list(range(7))
    else:
        links, offsets = rm.chain.config["ee_link_name"], rm.chain.config["ee_link_offset"]
        oriented, solved = [True] + [False] * (len(links) - 1), list(range(rm._n_dofs))
    q0, target, lo, hi, qs = inputs(rm, links, offsets, E, spread, seed)
    quat = rm.compute_forward_kinematics(qs.cuda().float(), links, offsets=offsets)[1].view(E, len(links), 4)
    held = [d for d in range(rm._n_dofs) if d not in solved]
    q0[:, held] = qs.cuda()[:, held]
    return links, offsets, oriented, solved, q0, target, quaternion_matrix(quat).contiguous(), lo, hi


def torch_ik_frames(rm, links, offsets, oriented, solved, q0, target, rot, lo, hi, wr=0.1, max_iters=100, tol=1e-5,
                    mu0=1e-3, mu_min=1e-9, mu_max=1e6, nu=4.0):
    """frame_ik_row of csrc/cdx_ik.h (ρ = 0, no base pose, unit position weights) with torch operators on the device; the
    chord vector from the skew part of Rt·Rcᵀ over cos(θ/2), which is the rule's quaternion formula away from θ = π."""
    import torch
    from compliancedex_amd.ik import quaternion_matrix
    E, D = q0.shape
    T = len(links)
    dev = q0.device
    tips = [k for k in range(T) if oriented[k]]
    M = 3 * T + 3 * len(tips)
    lo32, hi32 = lo.float(), hi.float()
    W = torch.cat([torch.ones(3 * T, dtype=torch.float64), torch.full((3 * len(tips),), wr, dtype=torch.float64)]).to(dev)
    may = torch.zeros(D, dtype=torch.bool)
    may[solved] = True
    may = may.to(dev)

    def residual(q32):
        pos, quat = rm.compute_forward_kinematics(q32, links, offsets=offsets)
        d = (target - pos.double().view(E, T, 3)).reshape(E, 3 * T)
        Re = rot[:, tips] @ quaternion_matrix(quat.view(E, T, 4)[:, tips]).transpose(-1, -2)
        v = 0.5 * torch.stack([Re[..., 2, 1] - Re[..., 1, 2], Re[..., 0, 2] - Re[..., 2, 0], Re[..., 1, 0] - Re[..., 0, 1]], -1)
        cos = 0.5 * (Re.diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0).clamp(-1.0, 1.0)
        return torch.cat([d, (v / torch.sqrt(0.5 * (1.0 + cos)).unsqueeze(-1)).reshape(E, -1)], 1)

    def emax(r):
        return (W * r).view(E, M // 3, 3).norm(dim=2).amax(1)

    q = torch.minimum(torch.maximum(q0.float(), lo32), hi32)
    r = residual(q)
    cost = 0.5 * ((W * r) ** 2).sum(1)
    mu = torch.full((E,), mu0, dtype=torch.float64, device=dev)
    iters = torch.zeros(E, dtype=torch.int32, device=dev)
    eye = torch.eye(M, dtype=torch.float64, device=dev)
    for _ in range(max_iters):
        act = emax(r) > tol
        if not bool(act.any()):
            break
        iters += act
        lin, ang = rm.compute_fingertip_jacobians(q, links, offsets)
        J = torch.cat([lin.double().view(E, 3 * T, D), ang.double()[:, tips].reshape(E, 3 * len(tips), D)], 1)
        g = torch.bmm(J.transpose(1, 2), (W * W * r).unsqueeze(2)).squeeze(2)
        qd = q.double()
        free = may & ~(((qd <= lo) & (g < 0)) | ((qd >= hi) & (g > 0)))
        J = J * free.unsqueeze(1) * W.view(1, M, 1)
        g = g * free
        A = torch.bmm(J, J.transpose(1, 2)) + mu.view(E, 1, 1) * eye
        y, info = torch.linalg.solve_ex(A, torch.bmm(J, g.unsqueeze(2)))
        delta = (g - torch.bmm(J.transpose(1, 2), y).squeeze(2)) / mu.view(E, 1)
        qn = torch.where(may, torch.minimum(torch.maximum(qd + delta, lo), hi).float(), q)
        rn = residual(qn)
        cn = 0.5 * ((W * rn) ** 2).sum(1)
        ok = act & (info == 0) & (cn < cost)
        q = torch.where(ok.unsqueeze(1), qn, q)
        r = torch.where(ok.unsqueeze(1), rn, r)
        cost = torch.where(ok, cn, cost)
        mu = torch.where(act, torch.where(ok, (mu / nu).clamp(min=mu_min), (mu * nu).clamp(max=mu_max)), mu)
    return q, emax(r), iters


def host_frames_seconds(rm, links, offsets, oriented, solved, q0, target, rot):
    """Seconds of cdxh_ik_solve_frames on one core, and its status / iteration arrays."""
    import numpy as np
    from compliancedex_amd import _host, _native as N
    from compliancedex_amd.ik import ik_params, joint_box
    lib, p = _host.load(), _host.ptr
    params = ik_params(*joint_box(rm.get_joint_limits()), max_iters=100)
    desc = rm._descriptor(links, offsets)
    q0, target, rot = (np.ascontiguousarray(t.cpu().numpy()) for t in (q0, target, rot))
    E, T = q0.shape[0], len(links)
    q, err, rerr = np.empty_like(q0), np.empty((E, T)), np.empty((E, T))
    iters, status = np.empty(E, np.int32), np.empty(E, np.int32)
    rot_mask = sum(1 << k for k, v in enumerate(oriented) if v)
    dof_mask = sum(1 << d for d in solved)
    t = time.perf_counter()
    rc = lib.cdxh_ik_solve_frames(desc, params, E, p(q0), N.DTYPE_F64, p(target), p(rot), None, None, None, None, rot_mask,
                                  dof_mask, p(q), p(err), p(rerr), p(iters), p(status), 0)
    dt = time.perf_counter() - t
    assert rc == 0
    return dt, status, iters


def run_frames(robot, E, args):
    import numpy as np
    import torch
    from compliancedex_amd import DifferentiableRobotModel, solve_ik_frames
    rm = DifferentiableRobotModel(robot, device="cuda")
    links, offsets, oriented, solved, q0, target, rot, lo, hi = frames_case(rm, robot, E)
    paths = {"frames_kernel": lambda: solve_ik_frames(rm, target, rot, links, offsets, q0=q0, oriented=oriented,
                                                      joints=solved),
             "frames_torch": lambda: torch_ik_frames(rm, links, offsets, oriented, solved, q0, target, rot, lo, hi)}
    for f in paths.values():
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(args.reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    rec = {"shape": "frames", "robot": robot, "E": E, "D": rm._n_dofs, "T": len(links), "oriented": sum(oriented),
           "solved_joints": len(solved), **{n: stats(v) for n, v in ms.items()}}
    res = paths["frames_kernel"]()
    tq, terr, titers = paths["frames_torch"]()
    rec["frames_kernel_converged"] = round(float((res.status == 0).double().mean()), 5)
    rec["frames_kernel_all_iters_share"] = round(float((res.status == 1).double().mean()), 5)
    rec["frames_kernel_iters_median_max"] = [int(res.iters.median()), int(res.iters.max())]
    rec["frames_torch_converged"] = round(float((terr <= 1e-5).double().mean()), 5)
    rec["frames_torch_iters_median_max"] = [int(titers.median()), int(titers.max())]
    rec["frames_torch_q_max_abs_diff"] = float((tq.double() - res.q).abs().max())
    rec["frames_torch_over_kernel"] = round(rec["frames_torch"]["median_ms"] / rec["frames_kernel"]["median_ms"], 1)
    if E <= args.host_rows:
        sec, hstatus, hiters = host_frames_seconds(rm, links, offsets, oriented, solved, q0, target, rot)
        rec["frames_host_one_core_ms"] = round(sec * 1e3, 2)
        rec["frames_host_converged"] = round(float((hstatus == 0).mean()), 5)
        rec["frames_host_iters_median_max"] = [int(np.median(hiters)), int(hiters.max())]
        rec["frames_host_over_kernel"] = round(sec * 1e3 / rec["frames_kernel"]["median_ms"], 1)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--robots", default="allegro,iiwa7_allegro")
    ap.add_argument("--robot", default=None, help="child mode: one shape in this process (with --rows one size)")
    ap.add_argument("--shapes", default="fingertips,frames", help="driver: the shapes to run")
    ap.add_argument("--shape", default="fingertips", help="child mode: fingertips (the two position solves) or frames")
    ap.add_argument("--host-rows", type=int, default=65536)
    ap.add_argument("--step-seconds", type=int, default=150, help="time limit of each shape's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ik.jsonl"))
    args = ap.parse_args()
    rows = [int(v) for v in args.rows.split(",")]
    if args.robot is None:
        for shape in args.shapes.split(","):
            for robot in args.robots.split(","):
                for E in rows:
                    cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__),
                           "--robot", robot, "--shape", shape, "--rows", str(E), "--reps", str(args.reps), "--host-rows",
                           str(args.host_rows), "--out", args.out]
                    rc = subprocess.run(cmd).returncode
                    if rc != 0:
                        raise SystemExit(f"{shape} {robot} E={E} ended with status {rc}: nothing more is started")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/ik.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = (run_frames if args.shape == "frames" else run_shape)(args.robot, rows[0], args)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
