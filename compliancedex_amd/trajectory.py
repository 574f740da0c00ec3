"""Collision-free approach trajectories: batched CHOMP on the device (cdx_traj_seed / cdx_traj_step; the rule is
csrc/cdx_traj.h).

The reference plans the approach with cuRobo's ``MotionGen`` (traj_gen.py) and replays it in verify_grasp_robot.py.
Here a trajectory is q [T, D] float64 with fixed ends; ``TrajectoryOptimizer`` runs the covariant gradient step of
Ratliff et al. (ICRA 2009) on E of them at once — smoothness, the whole-robot sphere penetration cost of ``hand.py``
at every waypoint and a joint-limit hinge —, ``trajectory_report`` checks a path between its waypoints as well, and
``plan_approach`` seeds several paths per goal, optimises them and keeps the smoothest clear one, on the device.
Parity with cuRobo (its seeds, its cost weights, its graph planner, its time-optimal retiming) is not attempted.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N
from .hand import HandSpheres, object_distance, penetration_report
from .ik import joint_box

MAX_T = N.TRAJ_MAX_T


def smoothness_matrix(T):
    """A_T: the n×n (n = T − 2) Toeplitz pentadiagonal [1 −4 6 −4 1], the Hessian of U_s per joint (numpy float64)."""
    n = int(T) - 2
    if n < 1:
        raise ValueError("T must be at least 3")
    A = 6.0 * np.eye(n)
    for k, v in ((1, -4.0), (2, 1.0)):
        if n > k:
            A += v * (np.eye(n, k=k) + np.eye(n, k=-k))
    return A


def step_size(T, w_smooth, w_col, gain=1.0):
    """gain / (w_smooth + w_col / λ_min(A_T)): in the metric A_T the smoothness term has curvature w_smooth and an obstacle
    term whose Hessian is at most w_col per waypoint at most w_col / λ_min (the joint-space Jacobian scales that bound;
    ``gain`` absorbs it)."""
    lam = float(np.linalg.eigvalsh(smoothness_matrix(T))[0])
    return float(gain) / (float(w_smooth) + float(w_col) / lam)


def _limits_of(source):
    """(lower, upper) lists of a robot model, a HandSpheres, a Chain or a (lower, upper) pair."""
    if isinstance(source, (tuple, list)) and len(source) == 2:
        return [float(v) for v in source[0]], [float(v) for v in source[1]]
    chain = source.chain
    return joint_box([dict(lower=b["lower"], upper=b["upper"]) for i, b in enumerate(chain.bodies) if chain.dof[i] >= 0])


def traj_params(lower, upper, T, w_smooth, w_col, w_lim, m_lim, step):
    p = N.CdxTrajParams()
    D = len(lower)
    if len(upper) != D or not 1 <= D <= N.MAX_DOFS:
        raise ValueError(f"limits must have 1 … {N.MAX_DOFS} entries each")
    for d in range(D):
        p.lower[d], p.upper[d] = float(lower[d]), float(upper[d])
    p.w_smooth, p.w_col, p.w_lim, p.m_lim, p.step = (float(v) for v in (w_smooth, w_col, w_lim, m_lim, step))
    p.T, p.n_dofs = int(T), D
    return p


def _traj(x, D, name="traj"):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if x.ndim == 2:
        x = x.unsqueeze(0)
    if x.ndim != 3 or x.shape[2] != D or x.shape[1] < 2:
        raise ValueError(f"{name} must have shape [E, T, {D}], got {tuple(x.shape)}")
    return x.to(torch.float64)


def _palm_rows(palm_pose, E, reps, dev):
    """palm_pose [E, 6] or [6] → [E·reps, 6] contiguous float64 on dev (one row per waypoint or sample); None stays."""
    if palm_pose is None:
        return None
    p = torch.as_tensor(palm_pose, dtype=torch.float64, device=dev)
    if p.shape == (6,):
        p = p.expand(E, 6)
    if p.shape != (E, 6):
        raise ValueError(f"palm_pose must have shape {(E, 6)} or (6,), got {tuple(p.shape)}")
    return p.repeat_interleave(reps, 0).contiguous()


def seed_trajectories(q_start, q_goal, T, seeds=1, amp=0.3, seed=0):
    """cdx_traj_seed: q_start, q_goal [G, D] → [G·seeds, T, D]; row g·seeds + s is the straight line plus
    a_d·16u²(1−u)², a_d uniform in ±amp from Philox keyed by ``seed``; s = 0 is the line itself."""
    lib = N.load()
    qs = torch.as_tensor(q_start)
    if not qs.is_cuda:
        raise RuntimeError("compliancedex_amd has no CPU path: q_start must be a device tensor")
    qs = qs.to(torch.float64).reshape(-1, qs.shape[-1]).contiguous()
    qg = torch.as_tensor(q_goal, device=qs.device).to(torch.float64).reshape(-1, qs.shape[-1]).contiguous()
    if qg.shape != qs.shape:
        raise ValueError("q_start and q_goal must have the same shape")
    G, D = qs.shape
    out = torch.empty(G * int(seeds), int(T), D, dtype=torch.float64, device=qs.device)
    N.check(lib.cdx_traj_seed(G, int(seeds), int(T), D, N.ptr(qs), N.ptr(qg), float(amp), int(seed) & (2 ** 64 - 1),
                              N.ptr(out), N.stream_ptr(qs.device)), "cdx_traj_seed")
    return out


@dataclass
class TrajectoryResult:
    trajectory: torch.Tensor  # [E, T, D] the best iterate
    cost: torch.Tensor        # [E] its U
    iteration: torch.Tensor   # [E] int32 the iteration it was met at (−1: never)
    last: torch.Tensor        # [E, T, D] the iterate after the last step
    parts: torch.Tensor       # [E, 3] (U_s, U_c, U_l) of the last evaluated iterate


class _Buffers:
    def __init__(self, E, T, D, hand, dev):
        f64 = dict(dtype=torch.float64, device=dev)
        S, R = hand.n_spheres, E * T
        self.traj = torch.empty(E, T, D, **f64)
        self.poses = torch.empty(R, hand.desc.n_bodies, 12, dtype=torch.float32, device=dev)
        self.centers = torch.empty(R * S, 3, **f64)
        self.dist, self.gdist = torch.empty(R * S, **f64), torch.empty(R * S, 3, **f64)
        self.cost_t, self.g_c = torch.empty(R, **f64), torch.empty(R, D, **f64)
        self.cost = torch.empty(E, 3, **f64)
        self.best_cost = torch.empty(E, **f64)
        self.best_iter = torch.empty(E, dtype=torch.int32, device=dev)
        self.best_traj = torch.empty(E, T, D, **f64)


class TrajectoryOptimizer:
    """CHOMP on E trajectories of T waypoints.  ``robot_model``: a DifferentiableRobotModel (its joint limits);
    ``hand``: the HandSpheres model of the same chain.  Per iteration four launches — cdx_hand_spheres on the E·T
    waypoints, the object's distance at the centres (a GPIS: one cdx_gpis_mean launch; a mesh or a callable:
    hand.object_distance), cdx_hand_term at weight 1, cdx_traj_step — with no allocation of its own and no host
    synchronisation; the buffers are allocated once per batch size.  Margins and weights of the sphere cost are
    ``m_obj … w_floor`` as in ``hand_collision``."""

    def __init__(self, robot_model, hand, T=32, w_smooth=1.0, w_col=100.0, w_lim=100.0, m_lim=0.02, gain=1.0, m_obj=0.0,
                 m_self=0.0, m_floor=0.0, w_obj=1.0, w_self=1.0, w_floor=1.0, limits=None):
        if not isinstance(hand, HandSpheres):
            raise TypeError("hand must be a HandSpheres")
        self.hand, self.T, self.D = hand, int(T), hand.desc.n_dofs
        if not 3 <= self.T <= MAX_T:
            raise ValueError(f"T must be in 3 … {MAX_T}, got {T}")
        if limits is None and robot_model is None:
            raise ValueError("TrajectoryOptimizer needs a robot_model or limits=(lower, upper)")
        lower, upper = _limits_of(limits if limits is not None else robot_model)
        if len(lower) != self.D:
            raise ValueError(f"the robot model has {len(lower)} joints, the sphere model {self.D}")
        self.lower, self.upper = lower, upper
        self.gain = float(gain)
        self.step = step_size(self.T, w_smooth, w_col, gain)
        self.params = traj_params(lower, upper, self.T, w_smooth, w_col, w_lim, m_lim, self.step)
        hp = N.CdxHandParams()
        hp.m_obj, hp.m_self, hp.m_floor = float(m_obj), float(m_self), float(m_floor)
        hp.w_obj, hp.w_self, hp.w_floor = float(w_obj), float(w_self), float(w_floor)
        self.hand_params = hp
        vals = (w_smooth, w_col, w_lim, m_lim, gain, m_obj, m_self, m_floor, w_obj, w_self, w_floor)
        if not all(math.isfinite(float(v)) for v in vals):
            raise ValueError("weights, margins and gain must be finite")
        self._buf = {}

    def buffers(self, E, dev):
        key = (int(E), str(dev))
        if key not in self._buf:
            self._buf[key] = _Buffers(int(E), self.T, self.D, self.hand, dev)
        return self._buf[key]

    def optimize(self, traj, obj, palm_pose=None, floor_z=None, iters=100):
        """traj [E, T, D] (or [T, D]) device tensor, not modified → TrajectoryResult.  ``obj``: a GPIS, a PreparedMesh /
        face vertices / TriangleMesh, a callable X → (d, ∇d), or None (no object); ``palm_pose`` [E, 6] or [6]: where
        the chain's root stands (None: the identity); ``floor_z`` None: no floor.  U is evaluated before each step, so
        the best iterate is one of the ``iters`` iterates the steps start from."""
        from .gpis import GPIS
        from .hand import _mesh_of
        lib = N.load()
        traj = _traj(traj, self.D)
        if not traj.is_cuda:
            raise RuntimeError("compliancedex_amd has no CPU path: traj must be a device tensor")
        E, T, D, dev = traj.shape[0], self.T, self.D, traj.device
        if traj.shape[1] != T:
            raise ValueError(f"traj has {traj.shape[1]} waypoints, the optimiser {T}")
        b = self.buffers(E, dev)
        b.traj.copy_(traj)
        b.best_cost.fill_(float("inf"))
        b.best_iter.fill_(-1)
        b.best_traj.copy_(traj)
        palm = _palm_rows(palm_pose, E, T, dev)
        pp = None if palm is None else palm[:, :3].contiguous()
        po = None if palm is None else palm[:, 3:].contiguous()
        hp = self.hand_params
        hp.floor_on = 0 if floor_z is None else 1
        hp.floor_z = 0.0 if floor_z is None else float(floor_z)
        hs, S, R = self.hand, self.hand.n_spheres, E * T
        state = obj.native_state() if isinstance(obj, GPIS) else None
        if obj is not None and state is None and not callable(obj):
            mesh = _mesh_of(obj, dev)  # (prepared once, not per iteration)
            obj = obj if mesh is None else mesh
        chain, model, st = C.byref(hs.desc), C.byref(hs.native()), N.stream_ptr(dev)
        q = b.traj.view(R, D)
        for it in range(int(iters)):
            N.check(lib.cdx_hand_spheres(chain, model, R, N.ptr(q), N.ptr(pp), N.ptr(po), N.ptr(b.poses),
                                         N.ptr(b.centers), st), "cdx_hand_spheres")
            dist, gdist = b.dist, b.gdist
            if state is not None:
                N.check(lib.cdx_gpis_mean(state.desc, N.ptr(b.centers), R * S, N.ptr(dist), N.ptr(gdist), None, st),
                        "cdx_gpis_mean")
            elif obj is not None:
                dist, gdist = object_distance(obj, b.centers)
                dist, gdist = dist.to(torch.float64).contiguous(), gdist.to(torch.float64).contiguous()
            else:
                dist = gdist = None
            N.check(lib.cdx_hand_term(chain, model, C.byref(hp), R, N.ptr(b.poses), N.ptr(b.centers), N.ptr(dist),
                                      N.ptr(gdist), N.ptr(po), 1.0, 0, N.ptr(b.cost_t), N.ptr(b.g_c), None, None, None,
                                      None, st), "cdx_hand_term")
            N.check(lib.cdx_traj_step(C.byref(self.params), E, N.ptr(b.traj), N.ptr(b.g_c), N.ptr(b.cost_t), it,
                                      N.ptr(b.cost), N.ptr(b.best_cost), N.ptr(b.best_iter), N.ptr(b.best_traj), st),
                    "cdx_traj_step")
        return TrajectoryResult(b.best_traj.clone(), b.best_cost.clone(), b.best_iter.clone(), b.traj.clone(),
                                b.cost.clone())


# ------------------------------------------------------------------ reports
def smoothness(traj):
    """U_s [E] of traj [E, T, D]: ½·Σ a², a_t = q[t−1] − 2q[t] + q[t+1] with the rest-to-rest virtual points."""
    q = torch.cat([traj[:, :1], traj, traj[:, -1:]], 1)
    a = q[:, :-2] - 2.0 * q[:, 1:-1] + q[:, 2:]
    return 0.5 * (a * a).sum((1, 2))


def path_samples(traj, refine=1):
    """Every waypoint and refine − 1 linear sub-steps of every segment: [E, (T − 1)·refine + 1, D], waypoint t at index
    t·refine with its own bits."""
    r = int(refine)
    if r < 1:
        raise ValueError("refine must be at least 1")
    if r == 1:
        return traj
    E, T, D = traj.shape
    a, d = traj[:, :-1, None, :], (traj[:, 1:] - traj[:, :-1])[:, :, None, :]
    f = (torch.arange(r, dtype=torch.float64, device=traj.device) / r).view(1, 1, r, 1)
    mid = torch.where(f == 0, a, a + f * d).reshape(E, (T - 1) * r, D)
    return torch.cat([mid, traj[:, -1:]], 1)


def trajectory_report(hand, traj, obj, palm_pose=None, floor_z=None, refine=4, allow=0.0, limits=None):
    """Clearance of whole paths, between the waypoints too: ``penetration_report`` on every sample of ``path_samples``
    (a path whose waypoints are all clear can still sag into the obstacle between two of them) → dict(depth [E, 3] the
    largest penetration over the path per class (object, self, floor), at [E, 3] the sample index that attains it,
    clear [E] every depth ≤ allow, within_limits [E] every waypoint inside ``limits`` ((lower, upper); None: the
    hand model's URDF limits), max_step [E] the largest |Δq| of a segment, smoothness [E] = U_s).  Device tensors,
    nothing is read back."""
    traj = _traj(traj, hand.desc.n_dofs)
    E, T, D = traj.shape
    x = path_samples(traj, refine)
    Ns = x.shape[1]
    palm = _palm_rows(palm_pose, E, Ns, traj.device)
    rep = penetration_report(hand, x.reshape(E * Ns, D).contiguous(), palm, obj, floor_z=floor_z, allow=allow)
    depth = rep["depth"].view(E, Ns, 3)
    lower, upper = _limits_of(limits if limits is not None else hand)
    lo = torch.tensor(lower, dtype=torch.float64, device=traj.device)
    hi = torch.tensor(upper, dtype=torch.float64, device=traj.device)
    top = depth.amax(1)
    return dict(depth=top, at=depth.argmax(1), clear=(top <= float(allow)).all(1),
                within_limits=((traj >= lo) & (traj <= hi)).all(2).all(1),
                max_step=(traj[:, 1:] - traj[:, :-1]).abs().amax((1, 2)), smoothness=smoothness(traj))


def pick_seed(clear, within_limits, smooth, depth_obj):
    """Per goal of [G, seeds] device tensors → (index [G] int64, success [G] bool): the clear seed within limits of the
    smallest U_s; without one the smallest object depth, success False.  A NaN counts as +inf.  Torch operators only."""
    inf = torch.full_like(smooth, float("inf"))
    ok = clear & within_limits & ~torch.isnan(smooth)
    any_ok = ok.any(1)
    d = torch.where(torch.isnan(depth_obj), inf, depth_obj)
    return torch.where(any_ok, torch.where(ok, smooth, inf).argmin(1), d.argmin(1)), any_ok


@dataclass
class ApproachPlan:
    trajectory: torch.Tensor        # [G, T, D] the kept path per goal
    seed: torch.Tensor              # [G] int64 the seed it grew from
    success: torch.Tensor           # [G] bool: clear and within limits
    report: dict                    # trajectory_report's entries of the kept paths
    all_trajectories: torch.Tensor  # [G, seeds, T, D] every seed's best iterate
    all_report: dict                # trajectory_report of all of them, [G·seeds, …]
    cost: torch.Tensor              # [G] U of the kept paths
    all_cost: torch.Tensor          # [G, seeds] U of every seed's best iterate


def plan_approach(robot_model, hand, q_start, q_goal, obj, palm_pose=None, floor_z=None, seeds=8, amp=0.3, seed=0,
                  refine=4, allow=0.0, T=32, iters=100, optimizer=None, **options):
    """Approach paths from q_start [G, D] (or [D]) to q_goal [G, D] → ApproachPlan.  Seeds ``seeds`` paths per goal
    (``seed_trajectories``), optimises all G·seeds in one batch (``optimizer``: a TrajectoryOptimizer to reuse, else one
    is built from T and ``options``), runs ``trajectory_report`` on the best iterates and keeps one seed per goal
    (``pick_seed``) — all on the device."""
    opt = optimizer if optimizer is not None else TrajectoryOptimizer(robot_model, hand, T=T, **options)
    D = opt.D
    dev = hand.device
    qg = torch.as_tensor(q_goal, dtype=torch.float64, device=dev).reshape(-1, D)
    G = qg.shape[0]
    qs = torch.as_tensor(q_start, dtype=torch.float64, device=dev).reshape(-1, D).expand(G, D)
    S = int(seeds)
    palm = _palm_rows(palm_pose, G, S, dev)
    res = opt.optimize(seed_trajectories(qs, qg, opt.T, S, amp, seed), obj, palm, floor_z, iters)
    rep = trajectory_report(hand, res.trajectory, obj, palm, floor_z, refine, allow, (opt.lower, opt.upper))
    pick, ok = pick_seed(rep["clear"].view(G, S), rep["within_limits"].view(G, S), rep["smoothness"].view(G, S),
                         rep["depth"][:, 0].reshape(G, S))
    rows = torch.arange(G, device=dev) * S + pick
    return ApproachPlan(res.trajectory[rows], pick, ok, {k: v[rows] for k, v in rep.items()},
                        res.trajectory.view(G, S, opt.T, D), rep, res.cost[rows], res.cost.view(G, S))


# ------------------------------------------------------------------ after planning
def interpolate(traj, n):
    """traj [E, T, D] resampled at n uniformly spaced parameters by linear interpolation → [E, n, D] (the counterpart of
    cuRobo's get_interpolated_plan; the ends keep their bits)."""
    single = traj.ndim == 2
    traj = _traj(traj, traj.shape[-1])
    E, T, D = traj.shape
    n = int(n)
    if n < 2:
        raise ValueError("n must be at least 2")
    s = torch.arange(n, dtype=torch.float64, device=traj.device) * ((T - 1) / (n - 1))
    i = s.floor().clamp(0, T - 2).to(torch.int64)
    f = (s - i.to(torch.float64)).view(1, n, 1)
    a, b = traj[:, i], traj[:, i + 1]
    out = torch.where(f == 0, a, a + f * (b - a))
    out[:, -1] = traj[:, -1]
    return out[0] if single else out


def retime(traj, v_max=None, robot_model=None):
    """The smallest uniform time step dt [E] with which no joint exceeds its velocity limit on any segment:
    max over segments and joints of |Δq| / v_max.  ``v_max`` [D]: the limits (None: the URDF's ``limit velocity`` of
    ``robot_model``); a joint whose limit is 0 or missing does not constrain."""
    traj = _traj(traj, traj.shape[-1])
    if v_max is None:
        if robot_model is None:
            raise ValueError("retime needs v_max or a robot_model to read the URDF's velocity limits from")
        v_max = robot_model.chain.velocity_limits()
    v = torch.as_tensor(v_max, dtype=torch.float64, device=traj.device).reshape(-1)
    if v.shape[0] != traj.shape[2]:
        raise ValueError(f"v_max must have {traj.shape[2]} entries")
    v = torch.where(v > 0, v, torch.full_like(v, float("inf")))
    return ((traj[:, 1:] - traj[:, :-1]).abs() / v).amax((1, 2))
