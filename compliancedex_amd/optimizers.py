"""Drop-ins for the other pregrasp optimisers of optimize_pregrasp.py:

  KinGraspOptimizer      :121-227  joint space, TorchSDF mesh distance, Adam
  SDFGraspOptimizer      :229-320  fingertip space, TorchSDF mesh distance, RMSprop, box clamps
  GPISGraspOptimizer     :322-406  fingertip space, GPIS distance / variance, RMSprop
  KinGPISGraspOptimizer  :408-511  joint space, GPIS distance / log-variance, RMSprop
  WCKinGPISGraspOptimizer :513-612 joint space, minimum-wrench contact forces (wrench.py), RMSprop

Each loop runs on the same gfx950 kernels as the prob-mode closure — GPIS mean/normal/std
(cdx_gpis_*), FK (cdx_fk_*), TorchSDF (cdx_sdf_*), the Kabsch/force-equilibrium reward
(cdx_force_eq_*) and, for the WC optimiser, the minimum-wrench solve (cdx_min_wrench) — with
the per-candidate cost glue as device tensor ops and torch's own RMSprop / Adam, as in the reference.  Differences in *how*: the best-iterate bookkeeping
(:215-224 etc.) is done with masked device updates instead of ``if update_flag.sum()`` host syncs
(same result: ``opt_margin`` is the margin of the last iteration that improved any candidate);
``kabsch_noise`` (optional, one [E, 3, 3] tensor per iteration) replays the reference's
``rand_like(H)`` draws.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from . import hand as _hand
from .force_eq import force_eq_descriptor, force_eq_reward
from .optimizer import EE_OFFSETS, FINGERTIP_LB, FINGERTIP_UB, WRIST_OFFSET
from .robot_model import DifferentiableRobotModel
from .torchsdf import BatchSchedule, PreparedMesh, QueryWorkspace, compute_sdf, query_batch


class TriangleMesh:
    """The part of open3d.geometry.TriangleMesh the SDF optimisers use: ``vertices``,
    ``triangles`` and ``scale(factor, center)`` (in place, like open3d)."""

    def __init__(self, vertices, triangles):
        self.vertices = np.asarray(vertices, dtype=np.float64).copy()
        self.triangles = np.asarray(triangles, dtype=np.int64).copy()

    @classmethod
    def from_npz(cls, path):
        d = np.load(path)
        return cls(d["vertices"], d["triangles"])

    @classmethod
    def from_obj(cls, path):
        vs, fs = [], []
        with open(path) as f:
            for line in f:
                if line.startswith("v "):
                    vs.append([float(x) for x in line.split()[1:4]])
                elif line.startswith("f "):
                    fs.append([int(tok.split("/")[0]) - 1 for tok in line.split()[1:4]])
        return cls(vs, fs)

    def scale(self, factor, center):
        c = np.asarray(center, dtype=np.float64)
        self.vertices = (self.vertices - c) * factor + c
        return self

    def sample_points_uniformly(self, number_of_points, seed=0, device="cuda", **kw):
        """``sampling.sample_points_uniformly`` on this mesh: a device tensor [K, 3] float64, not an open3d cloud."""
        from .sampling import sample_points_uniformly
        return sample_points_uniformly(self, number_of_points, seed=seed, device=device, **kw)

    def sample_points_poisson_disk(self, number_of_points, init_factor=5, seed=0, device="cuda", **kw):
        """``sampling.sample_points_poisson_disk`` on this mesh: a device tensor [K, 3] float64, not an open3d
        cloud."""
        from .sampling import sample_points_poisson_disk
        return sample_points_poisson_disk(self, number_of_points, init_factor=init_factor, seed=seed, device=device,
                                          **kw)


def _face_vertices(mesh, device):
    tri = np.asarray(mesh.triangles)
    v = np.asarray(mesh.vertices)
    return torch.from_numpy(v[tri.flatten()].reshape(len(tri), 3, 3)).to(device).float()


def _force_cost(force_norm, clamp_max):
    return -(force_norm * torch.nn.functional.softmin(force_norm, dim=1)).clamp(max=clamp_max).sum(dim=1)


def _sdf_normal(points, faces, faces_deflate):
    """SDF distance / sign / blended normal (:182-187): the normal averages the deflated and the
    true mesh's signed normals (flips inside the object)."""
    _, sign1, n1, _ = compute_sdf(points, faces_deflate)
    dist, sign2, n2, _ = compute_sdf(points, faces)
    n = 0.5 * sign1.unsqueeze(1) * n1 + 0.5 * sign2.unsqueeze(1) * n2
    return dist, n / n.norm(dim=1).unsqueeze(1)


class _Best:
    """Best-iterate tracking of the eager loops without host syncs."""

    def __init__(self, l0_dtype, E, T, device, **params):
        self.value = torch.full((E,), float("inf"), dtype=l0_dtype, device=device)
        self.margin = torch.zeros(E, T, dtype=torch.float64, device=device)
        self.normal = None
        self.params = {k: v.detach().clone() for k, v in params.items()}

    @torch.no_grad()
    def update(self, l, margin, normal, **params):
        flag = l < self.value
        anyf = flag.any()
        self.margin = torch.where(anyf, margin, self.margin)
        self.normal = normal if self.normal is None else torch.where(anyf, normal, self.normal)
        self.value = torch.where(flag, l.to(self.value.dtype), self.value)
        for k, v in params.items():
            m = flag.view((-1,) + (1,) * (v.dim() - 1))
            self.params[k] = torch.where(m, v.detach(), self.params[k])

    def flag(self):
        return (self.margin > 0.0).all()


def _noise(tape, s):
    return None if tape is None else tape[s]


def _tip_box(tip_bounding_box, device):
    """The fingertip box (lower, upper) as two [·, 3] device tensors."""
    return [torch.tensor(tip_bounding_box[0]).to(device).view(-1, 3),
            torch.tensor(tip_bounding_box[1]).to(device).view(-1, 3)]


def _set_box(cfg, box, T, dtype):
    """Copy the fingertip box into a native optimiser struct's ``box_lb`` / ``box_ub`` (3·T values each)."""
    lb = box[0].to(dtype).expand(T, 3).reshape(-1).cpu().tolist()
    ub = box[1].to(dtype).expand(T, 3).reshape(-1).cpu().tolist()
    for i in range(3 * T):
        cfg.box_lb[i], cfg.box_ub[i] = lb[i], ub[i]


def _set_ref_palm(ref_dst, palm_dst, ref_q, palm_offset, dtype):
    """Copy ``ref_q`` into ``ref_dst.ref_q`` and ``palm_offset`` into ``palm_dst.palm_offset`` (native structs),
    rounded to ``dtype`` first."""
    for i, v in enumerate(ref_q.to(dtype).tolist()):
        ref_dst.ref_q[i] = v
    off = palm_offset.to(dtype).cpu().tolist()
    for i in range(3):
        palm_dst.palm_offset[i] = off[i]


def _eager_loop(opt, optim_cls, best_dtype, pose, target, comp, lrs, optimize_target, cost, clamp=None, hand=None,
                verbose=True, trace_rows=False):
    """The autograd loop of the five optimisers, as the reference writes it, on clones of ``pose`` and ``comp`` (and
    of ``target`` when it is optimised: a frozen target is no param group and stays the caller's tensor).  ``lrs``:
    the learning rates of pose, target and compliance.  Per iteration ``cost(s, pose, target, comp)`` →
    ``(l, margin, normal, best_target, extras)``: the per-candidate loss, what ``_Best`` keeps with it, the target to
    store for an improved candidate, and a callable giving what ``verbose`` prints after the loss (evaluated only
    then: nothing syncs with ``verbose=False``).  ``hand``: ``(term, palm, field)`` — ``l += term.cost(pose, palm,
    field)`` before the backward, and ``last_hand_report`` from the returned pose.  ``clamp(pose, target, comp)`` runs
    under no_grad after every step.  ``loop_events``, when set, are recorded around the iterations."""
    pose = pose.clone().requires_grad_(True)
    comp = comp.clone().requires_grad_(True)
    groups = [{"params": pose, "lr": lrs[0]}, {"params": comp, "lr": lrs[2]}]
    if optimize_target:
        target = target.clone().requires_grad_(True)
        groups.insert(1, {"params": target, "lr": lrs[1]})
    optim = optim_cls(groups)
    best = _Best(best_dtype, target.shape[0], target.shape[1], opt.device, pose=pose, comp=comp, target=target)
    if opt.loop_events:
        opt.loop_events[0].record()
    for s in range(opt.num_iters):
        optim.zero_grad()
        l, margin, normal, best_target, extras = cost(s, pose, target, comp)
        if hand is not None:
            l = l + hand[0].cost(pose, hand[1], hand[2]).to(l.dtype)
        l.sum().backward()
        opt.loss_history.append(l.detach().sum())  # device scalar, no sync
        if trace_rows:
            opt.loss_rows.append(l.detach().clone())
        if verbose:
            print("Loss:", float(l.sum()), *extras())
        best.update(l, margin, normal, pose=pose, comp=comp, target=best_target)
        optim.step()
        if clamp is not None:
            with torch.no_grad():
                clamp(pose, target, comp)
    if opt.loop_events:
        opt.loop_events[1].record()
    if verbose:
        print(best.margin, best.normal)
    opt.best_loss = best.value
    if hand is not None:
        opt.last_hand_report = hand[0].report(best.params["pose"], hand[1], hand[2])
    return best.params["pose"], best.params["comp"], best.params["target"], best.flag()


def _fused_loop(opt, st, queries, iterate, cost, step, split_step=False, term=None, verbose=True, kabsch_noise=None,
                trace_rows=False, extras=()):
    """The fused loops' driver on the loop state ``st``: no autograd graph and, without ``verbose``, no host sync.
    Per iteration ``qr = queries()`` (the distance queries' launches), then ONE launch ``iterate(qr, noise, seed, s)``
    (cost, backward and step) or — with ``split_step`` True, ``verbose`` (the loss printed before the step, with
    ``extras`` after it, as the reference prints) or a ``term`` — ``cost(qr, noise, seed, s, loss)``, ``term(loss)``
    and ``step(s, 0)``; ``split_step="alt"``: even iterations take the two launches, odd ones the one.  ``step(iters,
    1)`` finalises.  → the last iteration's loss row (None without iterations)."""
    dev, iters = opt.device, opt.num_iters
    alt = split_step == "alt"
    two = bool(verbose or term is not None or (split_step and not alt))
    loss = None
    if opt.loop_events:
        opt.loop_events[0].record()
    for s in range(iters):
        nz = _noise(kabsch_noise, s)
        nz = None if nz is None else nz.detach().to(device=dev, dtype=torch.float64).contiguous()
        opt._seed += 1
        loss = st.loss_slot(s, iters)
        qr = queries()
        if two or (alt and s % 2 == 0):
            cost(qr, N.ptr(nz), opt._seed, s, loss)
            if term is not None:
                term(loss)
            if verbose:
                print("Loss:", float(loss.sum()), *extras)
            step(s, 0)
        else:
            iterate(qr, N.ptr(nz), opt._seed, s)
        if st.hist is None:
            opt.loss_history.append(loss.sum())  # device scalar, no sync
        if trace_rows:
            opt.loss_rows.append(loss.clone())
    step(iters, 1)
    st.loss_sums(opt.loss_history)
    if opt.loop_events:
        opt.loop_events[1].record()
    if verbose:
        print(st.opt_margin, st.opt_normal)
    opt.best_loss = st.opt_value
    return loss


def kin_fk_cache_view(fk_state, max_depth):
    """The fused Kin loop's FK-walk cache (``last_loop.fk_state``, csrc/cdx_kin.hip) as host arrays, one row per lane
    (lane 4·e + f holds fingertip f of candidate e; the last workgroup's lanes past 4·E are there too):
    ``tag`` [L] uint32 — the iteration that wrote the lane's slots + 1; ``qcheck`` [L, 8] uint32 — the bits of the joint
    angles the walk read (the lane's DOFs f + 4·u in slot u, 0 past the row); ``pose`` [L, 12] float32 — the walk's
    final R and t.  ``max_depth``: the chain's deepest tip path (it picks the kernel's level bound, 8 or 16, and with
    it the slots of the q-check and the tag).  Slot s of lane l of a workgroup lies at float (s / 4)·256 + 4·l + s % 4
    of the workgroup's block of (12 + 6·16 + 8 + 4)·64 floats."""
    maxd = 8 if max_depth <= 8 else N.MAX_DEPTH
    slots = 12 + 6 * N.MAX_DEPTH + N.MAX_DOFS // 4 + 4
    w = fk_state.detach().cpu().numpy().view(np.uint32).reshape(-1, slots // 4, 64, 4)
    w = np.ascontiguousarray(w.transpose(0, 2, 1, 3)).reshape(-1, slots)  # [lane, slot]
    qc = 12 + 6 * maxd
    return dict(tag=w[:, qc + N.MAX_DOFS // 4], qcheck=w[:, qc:qc + N.MAX_DOFS // 4],
                pose=np.ascontiguousarray(w[:, :12]).view(np.float32))


def kin_fk_cache_qcheck(pose):
    """What the cache's q-check slots hold after a walk on the joint rows ``pose`` [E, D] (float32): [4·E, 8] uint32,
    lane 4·e + f's slot u the bits of pose[e, f + 4·u], 0 past the row."""
    pose = np.ascontiguousarray(pose.detach().cpu().numpy(), np.float32)
    E, D = pose.shape
    want = np.zeros((E, 4, N.MAX_DOFS // 4), np.uint32)
    for f in range(4):
        cols = np.arange(f, D, 4)
        want[:, f, :len(cols)] = pose[:, cols].view(np.uint32)
    return want.reshape(4 * E, -1)


class _LoopState:
    """What the fused loops' device states share: the native buffer struct, the per-call loss history and the best
    iterate's return tuple."""

    hist = None

    def fill(self, b, pairs):
        """Set the native buffer struct ``b``'s fields from (name, tensor or None) pairs; it becomes ``buffers``."""
        for name, t in pairs:
            setattr(b, name, N.ptr(t))
        self.buffers = b

    def loss_slot(self, s, iters):
        """Iteration s's loss vector: a row of a per-call [iters, E] history (the per-iteration sums are taken in one
        reduction after the loop, not one per iteration), or the single buffer when the history would pass 1 GiB."""
        E = self.loss.shape[0]
        if s == 0:
            self.hist = (torch.empty(iters, E, dtype=torch.float64, device=self.loss.device)
                         if iters * E * 8 <= (1 << 30) else None)
        row = self.hist[s] if self.hist is not None else self.loss
        self.buffers.loss = N.ptr(row)
        return row

    def loss_sums(self, history):
        """Append the loop's per-iteration loss sums (device scalars) to ``history``."""
        if self.hist is not None:
            history.extend(self.hist.sum(dim=1).unbind(0))

    def best(self):
        return self.opt[0], self.opt[2], self.opt[1], (self.opt_margin > 0.0).all()


class _FusedLoop(_LoopState):
    """Device state of a fused Kin / SDF loop: the two prepared meshes, cdx_kin_cost's outputs (margin / normal
    in two alternating slots), the optimiser moments, the best iterate and the cdx_kin_step buffers.  Per
    iteration the loop is three TorchSDF queries, cdx_kin_cost and cdx_kin_step (optimiser, best iterate,
    clamps and — Kin — the next fingertips' FK): no autograd graph, no host sync."""

    def __init__(self, E, T, pose, target, comp, faces, faces_deflate, dev, concurrent=3, resort=16):
        """``concurrent``: how the iteration's three queries are launched — 3 (default) in one launch
        (cdx_sdf_query_batch), 1 on three streams (also what 3 falls back to for a mesh with NaN-capable faces), 0 one
        after the other on the caller's stream (the sequential oracle of the tests).  ``resort``: iterations per
        point sort."""
        if concurrent not in (0, 1, 3):
            raise ValueError(f"_FusedLoop: concurrent must be 0, 1 or 3, got {concurrent!r}")
        f32 = dict(dtype=torch.float32, device=dev)
        self.mesh, self.mesh_def = PreparedMesh(faces), PreparedMesh(faces_deflate)
        self.ws_tips, self.ws_tgt = QueryWorkspace(), QueryWorkspace()
        # the batched launch's schedule (heaviest point groups of the last iteration first)
        self.sched = BatchSchedule()
        self.iteration = 0
        # iterations per point sort: 16 (A/B with the batched launch's schedule, profiles/r05ba_config4_resort_sched_ab.jsonl:
        # 4 / 8 / 16 / never = 0.327 / 0.316 / 0.316 / 0.311 ms around the mesh, 0.461 / 0.445 / 0.442 / 0.469 far)
        self.resort = max(1, int(resort))
        # the three queries' outputs (dist, sign, normals, clst)
        self.q_out = [(torch.empty(E * T, **f32), torch.empty(E * T, dtype=torch.int32, device=dev),
                       torch.empty(E * T, 3, **f32), torch.empty(E * T, 3, **f32)) for _ in range(3)]
        self.concurrent = concurrent
        if self.concurrent == 3 and not (self.mesh.kind == N.SDF_MESH_CULLED and self.mesh_def.kind == N.SDF_MESH_CULLED):
            self.concurrent = 1  # (a mesh with NaN-capable faces: the batch launch has no exact path)
        if self.concurrent == 1:  # the two side streams the second and third query run on beside the first
            self.side = [torch.cuda.Stream(device=dev) for _ in range(2)]
            self.ev = [torch.cuda.Event() for _ in range(4)]
        self.pose, self.target, self.comp = pose, target, comp
        self.loss = torch.empty(E, dtype=torch.float64, device=dev)
        self.margin = [torch.zeros(E, T, dtype=torch.float64, device=dev) for _ in range(2)]
        self.normal = [torch.zeros(E * T, 3, **f32) for _ in range(2)]
        self.g = [torch.empty_like(pose), torch.empty_like(target), torch.empty_like(comp)]
        self.m = [torch.zeros_like(pose), torch.zeros_like(target), torch.zeros_like(comp)]
        self.v = [torch.zeros_like(pose), torch.zeros_like(target), torch.zeros_like(comp)]
        self.opt_value = torch.full((E,), float("inf"), **f32)
        self.opt_margin = torch.zeros(E, T, dtype=torch.float64, device=dev)
        self.opt_normal = torch.zeros(E * T, 3, **f32)
        self.opt = [pose.clone(), target.clone(), comp.clone()]
        self.any = torch.zeros(3, dtype=torch.int32, device=dev)
        self.tips = torch.empty(E * T, 3, **f32)
        b = N.CdxKinOptBuffers()
        self.fill(b, (("pose", pose), ("target", target), ("comp", comp), ("g_pose", self.g[0]),
                      ("g_target", self.g[1]), ("g_comp", self.g[2]), ("m_pose", self.m[0]), ("v_pose", self.v[0]),
                      ("m_target", self.m[1]), ("v_target", self.v[1]), ("m_comp", self.m[2]), ("v_comp", self.v[2]),
                      ("loss", self.loss), ("opt_value", self.opt_value), ("opt_margin", self.opt_margin),
                      ("opt_normal", self.opt_normal), ("opt_pose", self.opt[0]), ("opt_target", self.opt[1]),
                      ("opt_comp", self.opt[2]), ("any", self.any)))
        for i in range(2):
            b.margin[i], b.normal[i] = N.ptr(self.margin[i]), N.ptr(self.normal[i])

    def queries(self, tips, target):
        """The iteration's three TorchSDF calls (:186-188).  The fingertips are sorted once for both meshes, and the
        fingertips' and targets' orders are re-sorted only every ``resort`` iterations: a query's results do not
        depend on the order its points are walked in (each point's winner is exact), only the culling's speed does,
        and the points move little between iterations."""
        fresh = self.iteration % self.resort == 0
        self.iteration += 1
        tgt = target.view(-1, 3)
        o = self.q_out
        if self.concurrent == 3:
            # one launch: each culled kernel's tail (a few point groups far from the mesh) leaves most of the chip idle,
            # which the other queries' groups fill — no side stream, no event
            if fresh:
                self.ws_tips.sort(tips)
                self.ws_tgt.sort(tgt)
            query_batch([(self.mesh_def, tips, self.ws_tips, o[0]), (self.mesh, tips, self.ws_tips, o[1]),
                         (self.mesh, tgt, self.ws_tgt, o[2])], schedule=self.sched)
        elif not self.concurrent:
            if fresh:  # (sorted explicitly: a query on a mesh with NaN-capable faces neither sorts nor walks)
                self.ws_tips.sort(tips)
                self.ws_tgt.sort(tgt)
            self.mesh_def.query(tips, workspace=self.ws_tips, reuse_order=True, out=o[0])
            self.mesh.query(tips, workspace=self.ws_tips, reuse_order=True, out=o[1])
            self.mesh.query(tgt, workspace=self.ws_tgt, reuse_order=True, out=o[2])
        else:
            # The three queries are independent: each culled kernel's tail (a few point groups far from the mesh)
            # leaves most of the chip idle, which the others fill.  The targets are sorted (when fresh) and queried
            # on side stream 2, the fingertips sorted on the caller's stream and queried against the full mesh on
            # side stream 1 and against the deflated mesh on the caller's, which waits for both before cdx_kin_cost.
            main = torch.cuda.current_stream(tips.device)
            ev_start, ev_tips, ev_full, ev_tgt = self.ev
            ev_start.record(main)
            s1, s2 = self.side
            s2.wait_event(ev_start)
            with torch.cuda.stream(s2):
                if fresh:
                    self.ws_tgt.sort(tgt)
                self.mesh.query(tgt, workspace=self.ws_tgt, reuse_order=True, out=o[2])
            ev_tgt.record(s2)
            if fresh:
                self.ws_tips.sort(tips)
            ev_tips.record(main)
            s1.wait_event(ev_tips)
            with torch.cuda.stream(s1):
                self.mesh.query(tips, workspace=self.ws_tips, reuse_order=True, out=o[1])
            ev_full.record(s1)
            self.mesh_def.query(tips, workspace=self.ws_tips, reuse_order=True, out=o[0])
            main.wait_event(ev_full)
            main.wait_event(ev_tgt)
        return o[0][1], o[0][2], o[1][0], o[1][1], o[1][2], o[1][3], o[2][0], o[2][1], o[2][3]


def _kin_mode_run(self, chain, prm, cfg, st, q, pts, verbose, kabsch_noise, trace_rows, split_step, extras=()):
    """The fused loop of the Kin (``chain``, joints ``q``) and SDF (neither) optimisers on the loop state ``st``;
    ``pts``: the [E·T, 3] fingertips the queries and the cost read.  → the last iteration's loss row."""
    lib = N.load()
    tgt, comp = st.target, st.comp
    E, T = tgt.shape[0], tgt.shape[1]
    stream = N.stream_ptr(self.device)
    # cdx_kin_cost's gradient outputs: joints, targets, compliances, fingertips
    grads = (st.g[0], st.g[1], st.g[2], None) if chain is not None else (None, st.g[1], st.g[2], st.g[0])

    def queries():
        return [N.ptr(t) for t in st.queries(pts, tgt)]

    def iterate(qr, nz, seed, s):  # cost, backward and step in one launch (cdx_kin_iteration)
        N.check(lib.cdx_kin_iteration(chain, prm, cfg, st.buffers, E, T, *qr, nz, seed, s, stream), "cdx_kin_iteration")

    def cost(qr, nz, seed, s, loss):
        N.check(lib.cdx_kin_cost(chain, prm, E, N.ptr(q), N.ptr(pts), N.ptr(tgt), N.ptr(comp), *qr, nz, seed,
                                 N.ptr(loss), N.ptr(st.margin[s & 1]), N.ptr(st.normal[s & 1]), N.ptr(grads[0]),
                                 N.ptr(grads[1]), N.ptr(grads[2]), N.ptr(grads[3]), stream), "cdx_kin_cost")

    def step(s, finalize):
        N.check(lib.cdx_kin_step(chain, cfg, st.buffers, E, T, s, finalize, stream), "cdx_kin_step")

    return _fused_loop(self, st, queries, iterate, cost, step, split_step, None, verbose, kabsch_noise, trace_rows,
                       extras)


def _fe_kwargs(opt):
    """force_eq_reward's keyword arguments from an optimiser's mass, centre of mass and gravity switch."""
    return dict(mass=opt.mass, COM=opt.com, gravity=10.0 if opt.gravity else None)


class _JointSpace:
    """What the three joint-space optimisers share: the robot model, the fingertip links, ``ref_q``, FK and the hand
    term's set-up."""

    def _init_chain(self, robot_urdf, ee_link_names, ee_link_offsets, ref_q, device):
        self.ref_q = torch.tensor(list(ref_q)).to(self.device)
        self.robot_model = DifferentiableRobotModel(robot_urdf, device=device)
        self.ee_link_names = list(ee_link_names)
        self.ee_link_offsets = ee_link_offsets

    def forward_kinematics(self, joint_angles):
        """[E·T, 3] fingertips: FK (recursive=True, :148) + palm offset."""
        tips = self.robot_model.compute_forward_kinematics(joint_angles, self.ee_link_names,
                                                          offsets=self.ee_link_offsets, recursive=True)[0]
        return (tips.view(-1, 3) + self.palm_offset).view(-1, 3)

    def _hand_palm(self, hand_term, joint_angles):
        """Clear ``last_hand_report``, check ``hand_term`` against the joint rows and → the term's palm rows (the palm
        at ``palm_offset``, zero angles), or None without a term."""
        self.last_hand_report = None
        if hand_term is None:
            return None
        hand_term.check(joint_angles.shape[1], self.device)
        return _hand.palm_rows(self.palm_offset, joint_angles.shape[0])

    def _clamp_comp_target(self, joint_angles, target_pose, compliance):
        """KinGPIS's and WC's clamps after a step (:503-505 / :606-608)."""
        compliance.clamp_(min=40.0)
        target_pose.clamp_(min=self.tip_bounding_box[0], max=self.tip_bounding_box[1])


class KinGraspOptimizer(_JointSpace):
    """Joint-space optimiser on the TorchSDF mesh distance (optimize_pregrasp.py:121-227)."""

    def __init__(self, robot_urdf, ee_link_names, ee_link_offsets=EE_OFFSETS, palm_offset=(-0.01, 0.015, 0.12),
                 num_iters=1000, optimize_target=False, ref_q=None, mass=0.1, com=(0.0, 0.0, 0.0), gravity=True,
                 uncertainty=0.0, device="cuda", seed=0):
        """``seed``: key of the fused loop's on-device Kabsch noise (used when no ``kabsch_noise`` tape is given);
        iteration k of this optimiser's n-th fused call draws with key seed + (iterations before it) + k + 1."""
        self.device = torch.device(device)
        self._seed = int(seed)
        self.loop_events = None  # optional (start, end) CUDA events recorded around the iterations, eager or fused
        self._init_chain(robot_urdf, ee_link_names, ee_link_offsets, ref_q, device)
        self.num_iters = num_iters
        self.palm_offset = torch.tensor(palm_offset).to(self.device)
        self.optimize_target = optimize_target
        self.gravity, self.mass, self.com = gravity, mass, list(com)

    def optimize(self, joint_angles, target_pose, compliance, friction_mu, object_mesh, verbose=True,
                 kabsch_noise=None, trace_rows=False, fused=True, hand_term=None, split_step=False, fk_cache=True):
        """``trace_rows``: also keep every iteration's per-candidate loss in ``loss_rows`` (device).
        ``hand_term`` (a ``HandTerm``, ``fused=False`` only: the fused loop has no mesh query at the sphere centres):
        per iteration ``l += weight · hand_collision(hand, q, palm, obj or the mesh, …)`` with the palm at
        ``palm_offset`` and zero angles; ``last_hand_report`` is ``penetration_report`` of the returned joints.
        ``fused`` (default): per iteration the three TorchSDF queries on prepared meshes and ONE cost, backward and
        step kernel (cdx_kin_iteration: force_eq_reward, the six cost terms and the backward through them, TorchSDF
        and the FK chain, then Adam, the best iterate and the next fingertips' FK) — no autograd graph, no host sync;
        with ``split_step`` or ``verbose`` cdx_kin_cost then cdx_kin_step (``split_step="alt"``, a test hook: the two
        forms alternating, even iterations two launches, so that the one-launch iterations find the FK-walk cache one
        step stale and must walk).  ``fk_cache=False``: the one-launch iteration keeps no FK-walk cache, every
        iteration walks.  ``fused=False``: the same loop through the autograd drop-ins (compute_sdf, force_eq_reward,
        the FK module), torch tensor ops and torch.optim.Adam, as the reference writes it."""
        if fused and hand_term is not None:
            raise ValueError("KinGraspOptimizer: hand_term needs fused=False (the fused loop has no mesh query at the "
                             "sphere centres)")
        self.loss_history, self.loss_rows = [], []
        faces = _face_vertices(object_mesh, self.device)
        palm = self._hand_palm(hand_term, joint_angles)
        hand = None if palm is None else (hand_term, palm, PreparedMesh(faces) if hand_term.obj is None else None)
        object_mesh.scale(0.9, center=[0, 0, 0])
        faces_deflate = _face_vertices(object_mesh, self.device)
        E, T = target_pose.shape[0], target_pose.shape[1]
        lrs = (2e-3, 1e-5, 0.2) if self.optimize_target else (1e-2, 0.0, 0.2)  # q, target, compliance (:168-176)
        if fused:
            return self._optimize_fused(joint_angles, target_pose, compliance, friction_mu, faces, faces_deflate, lrs,
                                        verbose, kabsch_noise, trace_rows, split_step, fk_cache)

        def cost(s, joint_angles, target_pose, compliance):
            all_tip = self.forward_kinematics(joint_angles)
            dist, normal = _sdf_normal(all_tip, faces, faces_deflate)
            tar_dist, tar_sign, _, _ = compute_sdf(target_pose.reshape(-1, 3), faces)
            reward, margin, force_norm = force_eq_reward(
                all_tip.view(target_pose.shape), target_pose, compliance, friction_mu, normal.view(target_pose.shape),
                kabsch_noise=_noise(kabsch_noise, s), **_fe_kwargs(self))
            c = -reward * 5.0
            center_cost = (all_tip.view(target_pose.shape).mean(dim=1) - target_pose.mean(dim=1)).norm(dim=1) * 10.0
            ref_cost = (joint_angles - self.ref_q).norm(dim=1) * 10.0
            dist_cost = 1000 * torch.sqrt(dist).view(E, T).sum(dim=1)
            # the reference multiplies tar_sign [E·T] into the [E, T] view (:211), which only broadcasts
            # for E = 1; the [E, T] sign is what that line means and what it computes at E = 1
            tar_dist_cost = 10 * (tar_sign.view(E, T) * torch.sqrt(tar_dist).view(E, T)).sum(dim=1)
            l = c + dist_cost + tar_dist_cost + center_cost + _force_cost(force_norm, 1.0) + ref_cost
            return l, margin, normal, target_pose, lambda: (compliance,)

        return _eager_loop(self, torch.optim.Adam, torch.float32, joint_angles, target_pose, compliance, lrs,
                           self.optimize_target, cost, None, hand, verbose, trace_rows)

    def _optimize_fused(self, joint_angles, target_pose, compliance, friction_mu, faces, faces_deflate, lrs, verbose,
                        kabsch_noise, trace_rows, split_step, fk_cache):
        lib = N.load()
        dev = self.device
        E, T = target_pose.shape[0], target_pose.shape[1]
        q, tgt, comp = (x.detach().clone().contiguous() for x in (joint_angles, target_pose, compliance))
        if any(x.dtype != torch.float32 for x in (q, tgt, comp)):
            raise ValueError("KinGraspOptimizer: joint angles, targets and compliances must be float32 (the "
                             "reference's dtype on this path)")
        chain = self.robot_model._descriptor(self.ee_link_names, self.ee_link_offsets)
        prm = N.CdxKinParams()
        prm.fe = force_eq_descriptor(T, friction_mu, self.mass, 10.0 if self.gravity else None, 2.0, self.com)
        cfg = N.CdxKinOpt()
        cfg.rule, cfg.clamp_box = 0, 0
        cfg.lr[0], cfg.lr[1], cfg.lr[2] = lrs
        cfg.beta1, cfg.beta2, cfg.eps = 0.9, 0.999, 1e-8  # torch.optim.Adam defaults (:171)
        _set_ref_palm(prm, cfg, self.ref_q, self.palm_offset, torch.float32)
        st = _FusedLoop(E, T, q, tgt, comp, faces, faces_deflate, dev)
        st.buffers.tips = N.ptr(st.tips)
        nb = int(lib.cdx_kin_fk_state_bytes(E, T))
        if (split_step == "alt" or not split_step) and nb and fk_cache:
            # the step's FK walk kept for the next iteration's FK backward (any contents: the kernel tags what it wrote)
            st.fk_state = torch.full((nb // 4,), -1, dtype=torch.int32, device=dev)
            st.buffers.fk_state = N.ptr(st.fk_state)
        N.check(lib.cdx_fk_forward(chain, N.ptr(q), E, N.ptr(st.tips), None, N.stream_ptr(dev)), "cdx_fk_forward")
        st.tips.add_(self.palm_offset.float())  # FK + palm offset (:148); later iterations: cdx_kin_step
        # (verbose: the compliances printed before the step, as the reference prints them)
        loss = _kin_mode_run(self, chain, prm, cfg, st, q, st.tips, verbose, kabsch_noise, trace_rows, split_step,
                             (comp,))
        # the last iteration's per-candidate loss and fingertips (device, no copy; the reference prints the
        # non-finite case at :212-213)
        self.last_loss, self.last_tips = loss, st.tips
        self.last_params = (q, tgt, comp)  # the parameters after the last step (device, updated in place)
        # (trace_rows: the loop's device state too — moments, best iterate — for state-injection checks)
        self.last_loop = st if trace_rows else None
        return st.best()


class SDFGraspOptimizer:
    """Fingertip-space optimiser on the TorchSDF mesh distance (optimize_pregrasp.py:229-320)."""

    def __init__(self, tip_bounding_box, num_iters=2000, optimize_target=False, mass=0.1, com=(0.0, 0.0, 0.0),
                 gravity=True, uncertainty=0.0, device="cuda", seed=0):
        """``seed``: key of the fused loop's on-device Kabsch noise (as KinGraspOptimizer's)."""
        self.device = torch.device(device)
        self._seed = int(seed)
        self.loop_events = None  # optional (start, end) CUDA events recorded around the iterations, eager or fused
        self.tip_bounding_box = _tip_box(tip_bounding_box, self.device)
        self.num_iters = num_iters
        self.optimize_target = optimize_target
        self.mass, self.com, self.gravity = mass, list(com), gravity

    def optimize(self, tip_pose, target_pose, compliance, friction_mu, object_mesh, verbose=True, kabsch_noise=None,
                 trace_rows=False, fused=True, split_step=False):
        """``trace_rows``: also keep every iteration's per-candidate loss in ``loss_rows`` (device).
        ``fused`` (default): per iteration the three TorchSDF queries on prepared meshes and ONE cost, backward and
        step kernel (cdx_kin_iteration without a chain: RMSprop, the best iterate, the box clamps; with ``split_step``
        or ``verbose`` cdx_kin_cost then cdx_kin_step); ``fused=False``: the autograd loop with torch.optim.RMSprop."""
        self.loss_history, self.loss_rows = [], []
        faces = _face_vertices(object_mesh, self.device)
        object_mesh.scale(0.9, center=[0, 0, 0])
        faces_deflate = _face_vertices(object_mesh, self.device)
        E, T = tip_pose.shape[0], tip_pose.shape[1]
        lrs = (1e-3, 1e-3 if self.optimize_target else 0.0, 0.2)  # tips, target, compliance (:250-259)
        if fused:
            return self._optimize_fused(tip_pose, target_pose, compliance, friction_mu, faces, faces_deflate, lrs,
                                        verbose, kabsch_noise, trace_rows, split_step)

        def cost(s, tip_pose, target_pose, compliance):
            all_tip = tip_pose.view(-1, 3)
            dist, normal = _sdf_normal(all_tip, faces, faces_deflate)
            tar_dist, tar_sign, _, _ = compute_sdf(target_pose.reshape(-1, 3), faces)
            reward, margin, force_norm = force_eq_reward(
                tip_pose, target_pose, compliance, friction_mu, normal.view(tip_pose.shape),
                kabsch_noise=_noise(kabsch_noise, s), **_fe_kwargs(self))
            c = -reward * 5.0
            center_cost = (tip_pose.mean(dim=1) - target_pose.mean(dim=1)).norm(dim=1) * 10.0
            dist_cost = 1000 * torch.sqrt(dist).view(E, T).sum(dim=1)
            tar_dist_cost = 10 * (torch.sqrt(tar_dist).view(E, T) * tar_sign.view(E, T)).sum(dim=1)  # see :297
            l = c + dist_cost + tar_dist_cost + center_cost + _force_cost(force_norm, 1.0)
            return l, margin, normal, target_pose, lambda: (float(dist_cost.sum()), float(tar_dist_cost.sum()))

        def clamp(tip_pose, target_pose, compliance):  # bounding-box constraints (:312-314)
            tip_pose.clamp_(min=self.tip_bounding_box[0], max=self.tip_bounding_box[1])
            target_pose.clamp_(min=self.tip_bounding_box[0], max=self.tip_bounding_box[1])

        return _eager_loop(self, torch.optim.RMSprop, torch.float32, tip_pose, target_pose, compliance, lrs,
                           self.optimize_target, cost, clamp, None, verbose, trace_rows)

    def _optimize_fused(self, tip_pose, target_pose, compliance, friction_mu, faces, faces_deflate, lrs, verbose,
                        kabsch_noise, trace_rows, split_step):
        E, T = tip_pose.shape[0], tip_pose.shape[1]
        tips, tgt, comp = (x.detach().clone().contiguous() for x in (tip_pose, target_pose, compliance))
        if any(x.dtype != torch.float32 for x in (tips, tgt, comp)):
            raise ValueError("SDFGraspOptimizer: tip poses, targets and compliances must be float32 (TorchSDF's path)")
        prm = N.CdxKinParams()
        prm.fe = force_eq_descriptor(T, friction_mu, self.mass, 10.0 if self.gravity else None, 2.0, self.com)
        cfg = N.CdxKinOpt()
        cfg.rule, cfg.clamp_box = 1, 1
        cfg.lr[0], cfg.lr[1], cfg.lr[2] = lrs
        cfg.alpha, cfg.eps = 0.99, 1e-8  # torch.optim.RMSprop defaults (:253)
        _set_box(cfg, self.tip_bounding_box, T, torch.float32)
        st = _FusedLoop(E, T, tips, tgt, comp, faces, faces_deflate, self.device)
        _kin_mode_run(self, None, prm, cfg, st, None, tips.view(-1, 3), verbose, kabsch_noise, trace_rows,
                      bool(split_step))
        return st.best()


_MEAN_TILE = 32  # queries per workgroup of cdx_gpis_mean


class _GpisModeLoop(_LoopState):
    """Device state of a fused GPIS / KinGPIS loop (cdx_gpis_mode_*): the query points [tips; targets] in one
    buffer, the per-point GPIS outputs, the gradients, RMSprop's square averages, the two margin / normal slots and
    the best iterate.  Per iteration the loop is ONE cdx_gpis_mean launch over the 2·E·T points (mean, ∇mean, normal),
    ONE cdx_gpis_std launch over the E·T fingertips (the reference's variance of the targets is never used) and
    cdx_gpis_mode_iteration: no autograd graph, no host sync."""

    term = None  # KinGPIS with a hand term: its hand.TermLoop, with ``term_palm``

    def __init__(self, mode, pose, target, comp, gpis, dev):
        f64 = dict(dtype=torch.float64, device=dev)
        E, T = target.shape[0], target.shape[1]
        self.E, self.T, self.mode = E, T, mode
        self.state = gpis.native_state()
        # the iteration's query points in one buffer: the fingertips, then — from the next multiple of the mean
        # kernel's 32-query workgroup on, so that every row is computed exactly as by a launch of its own — the
        # targets; the rows between hold a finite filler point.  (A non-finite query stays in its own row of
        # cdx_gpis_mean whatever shares its workgroup: tests/test_gpu_rows.py, test_gpu_gpis_mode.py.)
        M = E * T
        Mp = (M + _MEAN_TILE - 1) // _MEAN_TILE * _MEAN_TILE
        self.Mp = Mp
        self.X = self.state.X1[:1].repeat(Mp + M, 1).contiguous()
        self.tips, self.target = self.X[:M].view(E, T, 3), self.X[Mp:].view(E, T, 3)
        self.target.copy_(target)
        if mode == 0:
            self.tips.copy_(pose)
            self.pose = self.tips
        else:
            self.pose = pose.detach().clone().contiguous()
        self.comp = comp.detach().clone().contiguous()
        Q = Mp + M
        self.mean, self.gmean, self.nrm = torch.empty(Q, **f64), torch.empty(Q, 3, **f64), torch.empty(Q, 3, **f64)
        self.std, self.gstd = torch.empty(M, **f64), torch.empty(M, 3, **f64)
        self.ws = self.state.workspace(M)
        self.loss = torch.empty(E, **f64)
        self.margin = [torch.zeros(E, T, **f64) for _ in range(2)]
        self.normal = [torch.zeros(M, 3, **f64) for _ in range(2)]
        params = (self.pose, self.target, self.comp)
        self.g = [torch.zeros_like(x) for x in params]
        self.g_tip = torch.zeros(M, 3, **f64) if mode == 1 else None
        self.v = [torch.zeros_like(x) for x in params]
        self.opt_value = torch.full((E,), float("inf"), **f64)
        self.opt_margin = torch.zeros(E, T, **f64)
        self.opt_normal = torch.zeros(M, 3, **f64)
        self.opt = [x.clone() for x in params]
        self.any = torch.zeros(3, dtype=torch.int32, device=dev)
        b = N.CdxGpisModeBuffers()
        self.fill(b, (("pose", self.pose), ("target", self.target), ("comp", self.comp),
                      ("tips", self.tips if mode == 1 else None), ("mean", self.mean[:M]), ("gmean", self.gmean[:M]),
                      ("normal", self.nrm[:M]), ("std", self.std), ("gstd", self.gstd), ("tmean", self.mean[Mp:]),
                      ("tgmean", self.gmean[Mp:]), ("g_pose", self.g[0]), ("g_target", self.g[1]),
                      ("g_comp", self.g[2]), ("g_tip", self.g_tip), ("v_pose", self.v[0]), ("v_target", self.v[1]),
                      ("v_comp", self.v[2]), ("loss", self.loss), ("opt_value", self.opt_value),
                      ("opt_margin", self.opt_margin), ("opt_normal", self.opt_normal), ("opt_pose", self.opt[0]),
                      ("opt_target", self.opt[1]), ("opt_comp", self.opt[2]), ("any", self.any)))
        for i in range(2):
            b.margin[i], b.normal_slot[i] = N.ptr(self.margin[i]), N.ptr(self.normal[i])

    def queries(self, lib, stream):
        """The iteration's two GPIS launches: mean / ∇mean / normal at [tips; targets], std / ∇std at the tips."""
        M = self.E * self.T
        N.check(lib.cdx_gpis_mean(self.state.desc, N.ptr(self.X), self.Mp + M, N.ptr(self.mean), N.ptr(self.gmean),
                                  N.ptr(self.nrm), stream), "cdx_gpis_mean")
        N.check(lib.cdx_gpis_std(self.state.desc, N.ptr(self.X), M, N.ptr(self.std), N.ptr(self.gstd), N.ptr(self.ws),
                                 stream), "cdx_gpis_std")


def _gpis_mode_run(self, chain, prm, cfg, st, verbose, kabsch_noise, trace_rows, split_step):
    """The fused loop of the two GPIS-mode optimisers on the loop state ``st``."""
    lib = N.load()
    E, T = st.E, st.T
    stream = N.stream_ptr(self.device)

    def queries():
        st.queries(lib, stream)

    def iterate(_, nz, seed, s):  # cost, backward and step in one launch (four fingertips)
        N.check(lib.cdx_gpis_mode_iteration(chain, prm, cfg, st.buffers, E, T, nz, seed, s, stream),
                "cdx_gpis_mode_iteration")

    def cost(_, nz, seed, s, loss):
        N.check(lib.cdx_gpis_mode_cost(chain, prm, st.buffers, E, T, nz, seed, s, stream), "cdx_gpis_mode_cost")

    def step(s, finalize):
        N.check(lib.cdx_gpis_mode_step(chain, prm, cfg, st.buffers, E, T, s, finalize, stream), "cdx_gpis_mode_step")

    def term(loss):  # (KinGPIS with a hand term) loss and g_q += weight · the hand's term at the current joints
        st.term.place(lib, st.pose, st.term_palm, None, stream)
        st.term.query(lib, stream)
        st.term.add(lib, None, loss, st.g[0], None, None, stream)

    _fused_loop(self, st, queries, iterate, cost, step, bool(split_step), term if st.term is not None else None,
                verbose, kabsch_noise, trace_rows)
    self._loop_state = st if self._keep_loop_state else None
    return st.best()


def _gpis_mode_inputs(name, dev, **tensors):
    """The fused GPIS-mode loops take float64 device tensors (the reference runs these two modes in double)."""
    from .gpis import _require_cuda
    for k, t in tensors.items():
        _require_cuda(t, f"{name} {k}")
        if t.dtype != torch.float64:
            raise ValueError(f"{name}: {k} must be float64 (the reference's dtype on this path), got {t.dtype}")


def _gpis_mode_setup(self, mode, T, friction_mu, lrs):
    prm = N.CdxGpisModeParams()
    prm.mode = mode
    prm.fe = force_eq_descriptor(T, friction_mu, self.mass, 10.0 if self.gravity else None, 2.0, self.com)
    prm.uncertainty = float(self.uncertainty)
    cfg = N.CdxGpisModeOpt()
    cfg.lr[0], cfg.lr[1], cfg.lr[2] = lrs
    cfg.alpha, cfg.eps, cfg.comp_min = 0.99, 1e-8, 40.0  # torch.optim.RMSprop defaults (:348 / :454); :401 / :506
    _set_box(cfg, self.tip_bounding_box, T, torch.float64)
    return prm, cfg


class GPISGraspOptimizer:
    """Fingertip-space optimiser on the GPIS distance and variance (optimize_pregrasp.py:322-406)."""

    def __init__(self, tip_bounding_box, num_iters=2000, optimize_target=False, mass=0.1, com=(0.0, 0.0, 0.0),
                 gravity=True, uncertainty=20.0, device="cuda", seed=0):
        """``seed``: key of the fused loop's on-device Kabsch noise (as KinGraspOptimizer's)."""
        self.device = torch.device(device)
        self._seed = int(seed)
        self.loop_events = None  # optional (start, end) CUDA events recorded around the iterations, eager or fused
        self._keep_loop_state = False  # tests: keep the fused loop's device state in ``_loop_state`` after the call
        self.tip_bounding_box = _tip_box(tip_bounding_box, self.device)
        self.num_iters = num_iters
        self.optimize_target = optimize_target
        self.mass, self.com, self.gravity, self.uncertainty = mass, list(com), gravity, uncertainty

    def optimize(self, tip_pose, target_pose, compliance, friction_mu, gpis, verbose=True, kabsch_noise=None,
                 fused=False, trace_rows=False, split_step=False):
        """``fused``: per iteration ONE cdx_gpis_mean launch over [tips; targets], ONE cdx_gpis_std launch over the
        tips and ONE cost / backward / RMSprop / best-iterate / clamp launch (cdx_gpis_mode_iteration; with
        ``split_step`` or ``verbose`` cdx_gpis_mode_cost then cdx_gpis_mode_step) — no autograd graph, no host sync,
        float64 device inputs, the caller's tensors untouched; ``fused=False`` (default): the autograd loop with
        torch.optim.RMSprop, as the reference writes it.  ``trace_rows``: also keep every iteration's per-candidate
        loss in ``loss_rows`` (device)."""
        self.loss_history, self.loss_rows = [], []
        E, T = tip_pose.shape[0], tip_pose.shape[1]
        lrs = (1e-3, 1e-3 if self.optimize_target else 0.0, 0.2)  # tips, target, compliance (:348-355)
        if fused:
            _gpis_mode_inputs("GPISGraspOptimizer", self.device, tip_pose=tip_pose, target_pose=target_pose,
                              compliance=compliance)
            prm, cfg = _gpis_mode_setup(self, 0, T, friction_mu, lrs)
            st = _GpisModeLoop(0, tip_pose.detach(), target_pose.detach(), compliance, gpis, self.device)
            return _gpis_mode_run(self, None, prm, cfg, st, verbose, kabsch_noise, trace_rows, split_step)

        def cost(s, tip_pose, target_pose, compliance):
            all_tip = tip_pose.view(-1, 3)
            dist, var = gpis.pred(all_tip)
            tar_dist, _ = gpis.pred(target_pose.reshape(-1, 3))
            normal = gpis.compute_normal(all_tip)
            reward, margin, force_norm = force_eq_reward(
                tip_pose, target_pose, compliance, friction_mu, normal.view(tip_pose.shape),
                kabsch_noise=_noise(kabsch_noise, s), **_fe_kwargs(self))
            c = -reward * 25.0
            center_cost = (tip_pose.mean(dim=1) - target_pose.mean(dim=1)).norm(dim=1) * 10.0
            dist_cost = 1000 * torch.abs(dist).view(E, T).sum(dim=1)
            tar_dist_cost = 10 * tar_dist.view(E, T).sum(dim=1)
            variance_cost = self.uncertainty * var.view(E, T).sum(dim=1)
            l = c + dist_cost + tar_dist_cost + center_cost + _force_cost(force_norm, 1.0) + variance_cost
            return l, margin, normal, target_pose, lambda: (float(dist_cost.sum()), float(variance_cost.sum()))

        def clamp(tip_pose, target_pose, compliance):  # (:399-401)
            tip_pose.clamp_(min=self.tip_bounding_box[0], max=self.tip_bounding_box[1])
            compliance.clamp_(min=40.0)

        return _eager_loop(self, torch.optim.RMSprop, torch.float64, tip_pose, target_pose, compliance, lrs,
                           self.optimize_target, cost, clamp, None, verbose, trace_rows)


class KinGPISGraspOptimizer(_JointSpace):
    """Joint-space optimiser on the GPIS distance and log-variance (optimize_pregrasp.py:408-511)."""

    def __init__(self, robot_urdf, ee_link_names, ee_link_offsets=EE_OFFSETS, palm_offset=WRIST_OFFSET, num_iters=1000,
                 optimize_target=False, ref_q=None, tip_bounding_box=(FINGERTIP_LB, FINGERTIP_UB), mass=0.1,
                 com=(0.0, 0.0, 0.0), gravity=True, uncertainty=10.0, device="cuda", seed=0):
        """``seed``: key of the fused loop's on-device Kabsch noise (as KinGraspOptimizer's)."""
        self.device = torch.device(device)
        self._seed = int(seed)
        self.loop_events = None  # optional (start, end) CUDA events recorded around the iterations, eager or fused
        self._keep_loop_state = False  # tests: keep the fused loop's device state in ``_loop_state`` after the call
        self._init_chain(robot_urdf, ee_link_names, ee_link_offsets, ref_q, device)
        self.num_iters = num_iters
        self.palm_offset = torch.tensor(np.asarray(palm_offset)).double().to(self.device)
        self.optimize_target = optimize_target
        self.tip_bounding_box = _tip_box(tip_bounding_box, self.device)
        self.mass, self.com, self.gravity, self.uncertainty = mass, list(com), gravity, uncertainty

    def optimize(self, joint_angles, target_pose, compliance, friction_mu, gpis, verbose=True, kabsch_noise=None,
                 fused=False, trace_rows=False, split_step=False, hand_term=None):
        """``fused`` / ``trace_rows`` / ``split_step``: as GPISGraspOptimizer.optimize; the fused step also clamps the
        targets (optimised or not, :505-507) and computes the next iteration's fingertips, so the loop has one FK
        launch in all (iteration 0's).  ``hand_term`` (a ``HandTerm``): per iteration ``l += weight ·
        hand_collision(hand, q, palm, obj or gpis, …)`` with the palm at ``palm_offset`` and zero angles, before the
        best-iterate comparison and the step; fused: cdx_gpis_mode_cost, then cdx_hand_spheres, cdx_gpis_mean at the
        sphere centres and cdx_hand_term (accumulating into the loss and the joint gradient), then cdx_gpis_mode_step.
        ``last_hand_report`` is then ``penetration_report`` of the returned joints."""
        self.loss_history, self.loss_rows = [], []
        palm = self._hand_palm(hand_term, joint_angles)
        lrs = (2e-3, 1e-3, 0.2) if self.optimize_target else (1e-2, 0.0, 0.2)  # q, target, compliance (:454-460)
        if fused:
            _gpis_mode_inputs("KinGPISGraspOptimizer", self.device, joint_angles=joint_angles, target_pose=target_pose,
                              compliance=compliance)
            res = self._optimize_fused(joint_angles, target_pose, compliance, friction_mu, gpis, lrs, verbose,
                                       kabsch_noise, trace_rows, split_step, hand_term)
            if hand_term is not None:
                self.last_hand_report = hand_term.report(res[0], palm, gpis)
            return res

        E, T = target_pose.shape[0], target_pose.shape[1]

        def cost(s, joint_angles, target_pose, compliance):
            all_tip = self.forward_kinematics(joint_angles)
            dist, var = gpis.pred(all_tip)
            tar_dist, _ = gpis.pred(target_pose.reshape(-1, 3))
            normal = gpis.compute_normal(all_tip)
            reward, margin, force_norm = force_eq_reward(
                all_tip.view(target_pose.shape), target_pose, compliance, friction_mu, normal.view(target_pose.shape),
                kabsch_noise=_noise(kabsch_noise, s), **_fe_kwargs(self))
            c = -reward * 5.0
            center_cost = (all_tip.view(target_pose.shape).mean(dim=1) - target_pose.mean(dim=1)).norm(dim=1) * 10.0
            ref_cost = (joint_angles - self.ref_q).norm(dim=1) * 20.0
            variance_cost = self.uncertainty * torch.log(100 * var).view(E, T)
            dist_cost = 1000 * torch.abs(dist).view(E, T).sum(dim=1)
            tar_dist_cost = 10 * tar_dist.view(E, T).sum(dim=1)
            l = (c + dist_cost + tar_dist_cost + center_cost + _force_cost(force_norm, 1.0) + ref_cost +
                 variance_cost.max(dim=1)[0])
            return l, margin, normal, target_pose, lambda: (variance_cost.detach(),)

        return _eager_loop(self, torch.optim.RMSprop, torch.float64, joint_angles, target_pose, compliance, lrs,
                           self.optimize_target, cost, self._clamp_comp_target,
                           None if palm is None else (hand_term, palm, gpis), verbose, trace_rows)

    def _optimize_fused(self, joint_angles, target_pose, compliance, friction_mu, gpis, lrs, verbose, kabsch_noise,
                        trace_rows, split_step, hand_term=None):
        lib = N.load()
        dev = self.device
        E, T = target_pose.shape[0], target_pose.shape[1]
        prm, cfg = _gpis_mode_setup(self, 1, T, friction_mu, lrs)
        _set_ref_palm(prm, prm, self.ref_q, self.palm_offset, torch.float64)
        chain = self.robot_model._descriptor(self.ee_link_names, self.ee_link_offsets)
        st = _GpisModeLoop(1, joint_angles.detach(), target_pose.detach(), compliance, gpis, dev)
        # iteration 0's fingertips: double(FK_f32(float(q))) + palm offset (:462); later ones: cdx_gpis_mode_step
        tips32 = torch.empty(E, T, 3, dtype=torch.float32, device=dev)
        N.check(lib.cdx_fk_forward(chain, N.ptr(st.pose.float().contiguous()), E, N.ptr(tips32), None, N.stream_ptr(dev)),
                "cdx_fk_forward")
        st.tips.copy_(tips32.double() + self.palm_offset.to(torch.float64))
        if hand_term is not None:  # the term's buffers, with the loop state; the palm: palm_offset, no rotation
            st.term = _hand.TermLoop(hand_term, E, gpis, dev)
            st.term_palm = _hand.palm_rows(self.palm_offset, E)[:, :3].contiguous()
        return _gpis_mode_run(self, chain, prm, cfg, st, verbose, kabsch_noise, trace_rows, split_step)


class WCKinGPISGraspOptimizer(_JointSpace):
    """Joint-space optimiser on the minimum-wrench certificate (optimize_pregrasp.py:513-612): the cost of a candidate
    is the smallest net force and torque its contacts can leave (wrench.min_wrench — the reference solves it through
    cvxpylayers) instead of the Kabsch equilibrium of springs.  An eager loop like KinGPISGraspOptimizer.optimize, with
    two deliberate differences from the reference: every candidate is its own force problem (the reference's solve
    couples the candidates of a batch: it centres on the mean of all E·T tips and puts only the first four forces in
    the objective, so it is only well-formed for E = 1, where the two coincide), and the forces are the unique
    least-effort minimiser (csrc/cdx_wrench.h), not whichever one SCS lands on.  As in the reference, ``uncertainty``
    is accepted and ignored (the variance weight is the literal 20), ``optimize_target`` is a dummy, the compliance
    receives no gradient (it only scales the returned targets), and the loss reaches the joints through the explicit
    partial ∂wrench/∂tips alone."""

    def __init__(self, robot_urdf, ee_link_names, ee_link_offsets=EE_OFFSETS, palm_offset=WRIST_OFFSET, num_iters=1000,
                 optimize_target=False, ref_q=None, tip_bounding_box=(FINGERTIP_LB, FINGERTIP_UB), min_force=5.0,
                 mass=0.1, com=(0.0, 0.0, 0.0), gravity=True, uncertainty=0.0, device="cuda"):
        self.device = torch.device(device)
        self.loop_events = None  # optional (start, end) CUDA events recorded around the iterations
        self._init_chain(robot_urdf, ee_link_names, ee_link_offsets, ref_q, device)
        self.num_iters = num_iters
        self.palm_offset = torch.tensor(np.asarray(palm_offset)).double().to(self.device)
        self.tip_bounding_box = _tip_box(tip_bounding_box, self.device)
        self.min_force = min_force
        self.mass, self.com, self.gravity = mass, list(com), gravity

    def optimize(self, joint_angles, target_pose, compliance, friction_mu, gpis, verbose=True, trace_rows=False,
                 hand_term=None):
        """→ (q, compliance, target, flag).  The returned target of a candidate is ``tip + forces / compliance`` of
        its best iteration (:603): the springs that would exert the certified forces.  ``loss_rows`` (with
        ``trace_rows``) keeps the per-candidate losses, ``wrench_rows`` the min_wrench result of every iteration.
        ``hand_term`` (a ``HandTerm``): as KinGPISGraspOptimizer.optimize's, through autograd."""
        from .wrench import min_wrench
        self.loss_history, self.loss_rows, self.wrench_rows = [], [], []
        palm = self._hand_palm(hand_term, joint_angles)

        E, T = target_pose.shape[0], target_pose.shape[1]

        def cost(s, joint_angles, target_pose, compliance):
            all_tip = self.forward_kinematics(joint_angles)
            dist, var = gpis.pred(all_tip)
            tar_dist, _ = gpis.pred(target_pose.reshape(-1, 3))
            normal = gpis.compute_normal(all_tip)
            tips = all_tip.view(target_pose.shape)
            res = min_wrench(tips, normal.view(target_pose.shape), friction_mu, min_force=self.min_force)
            if trace_rows:
                self.wrench_rows.append(res)
            margin, forces = res.margin, res.forces
            force_norm = forces.norm(dim=2)
            c = res.wrench * 5.0
            center_cost = (tips.mean(dim=1) - target_pose.mean(dim=1)).norm(dim=1) * 10.0
            ref_cost = (joint_angles - self.ref_q).norm(dim=1) * 20.0
            variance_cost = 20 * torch.log(100 * var).view(E, T)  # (:587: the literal 20, not ``uncertainty``)
            dist_cost = 1000 * torch.abs(dist).view(E, T).sum(dim=1)
            tar_dist_cost = 10 * tar_dist.view(E, T).sum(dim=1)
            l = (c + dist_cost + tar_dist_cost + center_cost + _force_cost(force_norm, 1.0) + ref_cost +
                 variance_cost.max(dim=1)[0])
            # the target kept for an improved candidate: the springs that would exert the certified forces (:603)
            return l, margin, normal, tips + forces / compliance.unsqueeze(2), lambda: (res.wrench.detach(),)

        # q and compliance at 1e-2 and 0.2 (:553-556); the target is a frozen copy, clamped but never optimised
        return _eager_loop(self, torch.optim.RMSprop, torch.float64, joint_angles, target_pose.clone(), compliance,
                           (1e-2, 0.0, 0.2), False, cost, self._clamp_comp_target,
                           None if palm is None else (hand_term, palm, gpis), verbose, trace_rows)
