"""The hand's volume as spheres fixed to its links, a differentiable penetration cost and a per-candidate report
(cdx_hand_spheres / cdx_hand_cost / cdx_hand_pullback; the rule is csrc/cdx_hand.h).

The optimisers know the hand at its fingertips only.  ``HandSpheres`` fills every link with spheres (given, or inscribed
in a URDF's ``<collision>`` primitives), ``hand_collision`` scores their penetration of an object (a GPIS, a mesh or any
signed-distance callable), of each other and of a floor for E candidates, with the gradient in joint space and palm
pose, and ``penetration_report`` turns the same launch into a filter next to ``inverse_kinematics`` and ``min_wrench``.
The reference leaves this to PyBullet (verify_pregrasp.py) and cuRobo's collision spheres (traj_gen.py); parity with
either is not attempted.  ``HandTerm`` makes the cost a term of the joint-space optimisers' loss
(``optimize(..., hand_term=…)``): through autograd in the eager loops, through cdx_hand_term — the cost and its pull-back
in one accumulating launch — in the fused ones.
"""
from __future__ import annotations

import ctypes as C
import math
import xml.etree.ElementTree as ET

import numpy as np
import torch

from . import _native as N
from .chain import Chain
from .urdf import _vec, load_robot

MAX_SPHERES, MAX_PAIRS = N.HAND_MAX_SPHERES, N.HAND_MAX_PAIRS
CLASSES = ("object", "self", "floor")


# ------------------------------------------------------------------ spheres from URDF collision primitives
def _grid(e, a):
    """Centres along an axis of extent e for spheres of diameter a: −e/2 + r + i·(e − 2r)/(n − 1)."""
    n = max(1, math.ceil(e / a - 1e-9))
    r = 0.5 * a
    return [0.0] if n == 1 else [-0.5 * e + r + i * (e - 2.0 * r) / (n - 1) for i in range(n)]


def box_spheres(size):
    """Inscribed spheres of a box: r = half the smallest extent, a grid that is connected and stays inside."""
    a = min(size)
    if not (a > 0 and all(math.isfinite(v) for v in size)):
        raise ValueError(f"box size must be positive and finite, got {size}")
    gx, gy, gz = (_grid(e, a) for e in size)
    return [((x, y, z), 0.5 * a) for x in gx for y in gy for z in gz]


def cylinder_spheres(radius, length):
    if not (radius > 0 and length > 0 and math.isfinite(radius) and math.isfinite(length)):
        raise ValueError(f"cylinder radius and length must be positive and finite, got {radius}, {length}")
    if length >= 2.0 * radius:
        return [((0.0, 0.0, z), radius) for z in _grid(length, 2.0 * radius)]
    return box_spheres((2.0 * radius, 2.0 * radius, length))


def _rpy_matrix(rpy):
    """Rz(yaw)·Ry(pitch)·Rx(roll) in float64 (the order of chain.fixed_rotation)."""
    cr, sr, cp, sp, cy, sy = (f(v) for v in rpy for f in (math.cos, math.sin))
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], np.float64)
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], np.float64)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], np.float64)
    return Rz @ Ry @ Rx


def spheres_from_urdf(path, strict=False):
    """({link: [((x, y, z), r), …]}, skipped) from the ``<collision>`` primitives of a URDF: boxes, cylinders and
    spheres by the rules above, the primitive's ``<origin>`` applied in float64.  A ``<mesh>`` geometry is skipped and
    listed as (link, filename); ``strict`` raises instead."""
    root = ET.parse(path).getroot()
    out, skipped = {}, []
    for link in root:
        if link.tag != "link":
            continue
        for col in link.findall("collision"):
            org, geo = col.find("origin"), col.find("geometry")
            if geo is None:
                continue
            xyz = np.array(_vec(org.get("xyz") if org is not None else None, (0, 0, 0)), np.float64)
            R = _rpy_matrix(_vec(org.get("rpy") if org is not None else None, (0, 0, 0)))
            box, cyl, sph, mesh = (geo.find(k) for k in ("box", "cylinder", "sphere", "mesh"))
            if box is not None:
                prim = box_spheres(tuple(_vec(box.get("size"), ())))
            elif cyl is not None:
                prim = cylinder_spheres(float(cyl.get("radius")), float(cyl.get("length")))
            elif sph is not None:
                prim = [((0.0, 0.0, 0.0), float(sph.get("radius")))]
            else:
                what = (link.get("name"), mesh.get("filename") if mesh is not None else None)
                if strict:
                    raise ValueError(f"collision geometry of link {what[0]!r} is not a primitive: {what[1]!r}")
                skipped.append(what)
                continue
            for c, r in prim:
                w = R @ np.array(c, np.float64) + xyz
                out.setdefault(link.get("name"), []).append((tuple(float(v) for v in w), float(r)))
    return out, skipped


# ------------------------------------------------------------------ host float64 FK of every body
def fk_all_f64(desc, q):
    """Poses of every body of a cdx_chain at q [D] in float64 → (R [n, 3, 3], t [n, 3]) in the hand frame."""
    n = desc.n_bodies
    R, t = np.zeros((n, 3, 3)), np.zeros((n, 3))
    R[0] = np.eye(3)
    for i in range(1, n):
        b = desc.bodies[i]
        F = np.array(list(b.F), np.float64).reshape(3, 3)
        A = np.eye(3)
        if b.dof >= 0:
            th = float(b.sign) * float(q[b.dof])
            c, s = math.cos(th), math.sin(th)
            j, k = [(1, 2), (2, 0), (0, 1)][b.axis]
            A[j, j] = A[k, k] = c
            A[j, k], A[k, j] = -s, s
        t[i] = R[b.parent] @ np.array(list(b.t), np.float64) + t[b.parent]
        R[i] = R[b.parent] @ F @ A
    return R, t


class HandSpheres:
    """Spheres fixed to a robot's links.  ``robot``: whatever ``load_robot`` accepts (or its dict); ``spheres``:
    {link name: [(centre xyz in the link frame, radius), …]}.  Stored sorted by body index, rounded to float32 once
    (``local`` [S, 3] float32, ``radius`` [S] float64 holding float32 values, ``body`` [S] int32, ``links`` the name per
    sphere), S ≤ 256.

    ``pairs`` [P, 2] int32 is the self-collision list: every a < b on different bodies more than ``skip`` joints apart
    in the tree (through their lowest common ancestor; skip = 1 drops same-body and parent–child pairs) that do not
    already overlap at ``rest_q`` (float64 FK on the host; default ``config.ref_q``, else zeros) — a box-filled hand
    would otherwise carry a permanent cost.  ``pairs=`` overrides the list.  The device tables are built on first
    use, so the model itself needs no GPU."""

    def __init__(self, robot, spheres, skip=1, rest_q=None, device="cuda", pairs=None):
        desc = robot if isinstance(robot, dict) else load_robot(robot)
        self.chain = Chain(desc)
        self.device = torch.device(device)
        root = self.chain.bodies[0]["name"]
        self.desc = self.chain.descriptor([root])
        rows = []
        for link, items in spheres.items():
            if link not in self.chain.index:
                raise ValueError(f"unknown link {link!r}")
            for c, r in items:
                c32 = np.asarray(c, np.float64).astype(np.float32)
                r32 = float(np.float32(r))
                if c32.shape != (3,) or not np.isfinite(c32).all():
                    raise ValueError(f"sphere centre on {link!r} must be 3 finite numbers, got {c!r}")
                if not (math.isfinite(r32) and r32 > 0.0):
                    raise ValueError(f"sphere radius on {link!r} must be finite and > 0, got {r!r}")
                rows.append((self.chain.index[link], len(rows), c32, r32, link))
        if not rows:
            raise ValueError("a hand model needs at least one sphere")
        if len(rows) > MAX_SPHERES:
            raise ValueError(f"{len(rows)} spheres; the kernels hold {MAX_SPHERES} (CDX_MAX_SPHERES)")
        rows.sort(key=lambda x: (x[0], x[1]))
        self.body = np.array([x[0] for x in rows], np.int32)
        self.local = np.stack([x[2] for x in rows]).astype(np.float32)
        self.radius = np.array([x[3] for x in rows], np.float64)
        self.links = [x[4] for x in rows]
        self.skipped = []
        self.skip = int(skip)
        D = self.chain.n_dofs
        if rest_q is None:
            rest_q = self.chain.config.get("ref_q") or [0.0] * D
        self.rest_q = np.asarray(rest_q, np.float64).reshape(-1)
        if self.rest_q.shape != (D,):
            raise ValueError(f"rest_q must have {D} entries, got {self.rest_q.shape}")
        if pairs is None:
            pairs = self._default_pairs()
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        S = len(self.body)
        if len(pairs) > MAX_PAIRS:
            raise ValueError(f"{len(pairs)} pairs; the kernels hold {MAX_PAIRS} (CDX_HAND_MAX_PAIRS)")
        if len(pairs) and not ((pairs[:, 0] >= 0) & (pairs[:, 0] < pairs[:, 1]) & (pairs[:, 1] < S)).all():
            raise ValueError("pairs must be sphere indices with 0 <= a < b < S")
        self.pairs = np.ascontiguousarray(pairs)
        self._dev = None

    @classmethod
    def from_urdf(cls, path, robot=None, strict=False, **kw):
        """The model of a URDF's collision primitives on ``robot`` (default: the URDF's own chain)."""
        spheres, skipped = spheres_from_urdf(path, strict=strict)
        hs = cls(robot if robot is not None else path, spheres, **kw)
        hs.skipped = skipped
        return hs

    @classmethod
    def along_links(cls, robot, radius, **kw):
        """Spheres of one radius along the skeleton: one at every body's origin and, on the segment from a body's origin
        to each child's origin (length L), ceil(L / 2r) − 1 more at equal spacing, so neighbours touch or overlap.  For
        chains whose ``<collision>`` geometry is meshes (``spheres_from_urdf`` skips those: iiwa7_allegro's arm would
        have no volume)."""
        desc = robot if isinstance(robot, dict) else load_robot(robot)
        r = float(radius)
        if not (math.isfinite(r) and r > 0.0):
            raise ValueError(f"radius must be finite and > 0, got {radius!r}")
        bodies = desc["bodies"]
        spheres = {b["name"]: [((0.0, 0.0, 0.0), r)] for b in bodies}
        for i, b in enumerate(bodies):
            if i == 0:
                continue
            v = np.array([float(x) for x in b["xyz"]], np.float64)
            k = math.ceil(float(np.linalg.norm(v)) / (2.0 * r) - 1e-9)
            parent = bodies[b["parent"]]["name"]
            spheres[parent] += [(tuple(float(x) for x in v * (j / k)), r) for j in range(1, k)]
        return cls(desc, spheres, **kw)

    @property
    def n_spheres(self):
        return len(self.body)

    def tree_distance(self, a, b):
        """Joints on the path between bodies a and b through their lowest common ancestor."""
        parent = [x["parent"] for x in self.chain.bodies]
        up = {}
        d = 0
        while a >= 0:
            up[a] = d
            a, d = parent[a], d + 1
        d = 0
        while b not in up:
            b, d = parent[b], d + 1
        return d + up[b]

    def rest_centers(self):
        """The sphere centres at rest_q in the hand frame, float64 [S, 3]."""
        R, t = fk_all_f64(self.desc, self.rest_q)
        return np.einsum("sij,sj->si", R[self.body], self.local.astype(np.float64)) + t[self.body]

    def _default_pairs(self):
        S = len(self.body)
        c = self.rest_centers()
        nb = len(self.chain.bodies)
        far = np.array([[self.tree_distance(i, j) > self.skip for j in range(nb)] for i in range(nb)])
        out = []
        for a in range(S):
            for b in range(a + 1, S):
                ba, bb = int(self.body[a]), int(self.body[b])
                if ba == bb or not far[ba, bb]:
                    continue
                if self.radius[a] + self.radius[b] - float(np.linalg.norm(c[a] - c[b])) > 0.0:
                    continue
                out.append((a, b))
        return np.array(out, np.int32).reshape(-1, 2)

    # -------------------------------------------------------------- device side
    def native(self):
        """(cdx_hand descriptor, its device tables), prepared once."""
        if self._dev is None:
            lib = N.load()
            S, P = len(self.body), len(self.pairs)
            tables = torch.empty(lib.cdx_hand_bytes(S, P), dtype=torch.uint8, device=self.device)
            h = N.CdxHand()
            N.check(lib.cdx_hand_prepare(self.desc.n_bodies, S, self.local.ctypes.data, self.radius.ctypes.data,
                                         self.body.ctypes.data, P, self.pairs.ctypes.data if P else None,
                                         N.ptr(tables), C.byref(h), N.stream_ptr(self.device)), "cdx_hand_prepare")
            self._dev = (h, tables)
        return self._dev[0]

    def centers(self, q, palm_pose=None):
        """World-frame sphere centres [E, S, 3] float64 of q [E, D] and palm_pose [E, 6] (position, XYZ Euler angles;
        None: identity), differentiable in both."""
        q = _rows(q, self.chain.n_dofs, "q")
        if palm_pose is not None:
            palm_pose = _rows(palm_pose, 6, "palm_pose")
            if palm_pose.shape[0] != q.shape[0]:
                raise ValueError("palm_pose must have one row per row of q")
        return _Centers.apply(q, palm_pose, self)

    def cost(self, centers, dist=None, gdist=None, m_obj=0.0, m_self=0.0, m_floor=0.0, w_obj=1.0, w_self=1.0,
             w_floor=1.0, floor_z=None):
        """(cost [E], depth [E, 3], worst [E, 3] int32) of centres [E, S, 3]; dist [E, S] / gdist [E, S, 3]: the
        object's signed distance (positive outside) and its gradient at the centres (None: no object term);
        floor_z None: no floor term.  cost is differentiable in centers; the distance field enters through the
        given dist / gdist only.  depth and worst are ordered (object, self, floor)."""
        S = self.n_spheres
        if not (isinstance(centers, torch.Tensor) and centers.ndim == 3 and centers.shape[1:] == (S, 3)):
            raise ValueError(f"centers must be a tensor [E, {S}, 3]")
        if not centers.is_cuda:
            raise RuntimeError("compliancedex_amd has no CPU path: the hand cost needs device tensors")
        if (dist is None) != (gdist is None):
            raise ValueError("dist and gdist come together")
        E = centers.shape[0]
        if dist is not None:
            dist = dist.detach().to(torch.float64).reshape(E, S).contiguous()
            gdist = gdist.detach().to(torch.float64).reshape(E, S, 3).contiguous()
        p = N.CdxHandParams()
        p.m_obj, p.m_self, p.m_floor = float(m_obj), float(m_self), float(m_floor)
        p.w_obj, p.w_self, p.w_floor = float(w_obj), float(w_self), float(w_floor)
        p.floor_on = 0 if floor_z is None else 1
        p.floor_z = 0.0 if floor_z is None else float(floor_z)
        return _Cost.apply(centers.to(torch.float64), dist, gdist, self, p)

    def names(self, worst):
        """Link names of a ``worst`` array [E, 3] (reads it back): per row (object link, (self link a, self link b),
        floor link), None where the class is off."""
        w = worst.detach().cpu().numpy() if isinstance(worst, torch.Tensor) else np.asarray(worst)
        out = []
        for o, s, f in w.reshape(-1, 3):
            pair = None if s < 0 else tuple(self.links[int(k)] for k in self.pairs[int(s)])
            out.append((None if o < 0 else self.links[int(o)], pair, None if f < 0 else self.links[int(f)]))
        return out


def _rows(x, width, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if x.ndim != 2 or x.shape[1] != width:
        raise ValueError(f"{name} must have shape [E, {width}], got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError(f"compliancedex_amd has no CPU path: {name} must be a device tensor")
    return x if x.dtype == torch.float64 else x.double()


def spheres_launch(hs, q, palm_pos, palm_ori):
    """cdx_hand_spheres on contiguous float64 device tensors → (poses [E, n_bodies, 12] float32, centers [E, S, 3])."""
    lib = N.load()
    E, dev = q.shape[0], q.device
    poses = torch.empty(E, hs.desc.n_bodies, 12, dtype=torch.float32, device=dev)
    centers = torch.empty(E, hs.n_spheres, 3, dtype=torch.float64, device=dev)
    N.check(lib.cdx_hand_spheres(C.byref(hs.desc), C.byref(hs.native()), E, N.ptr(q), N.ptr(palm_pos), N.ptr(palm_ori),
                                 N.ptr(poses), N.ptr(centers), N.stream_ptr(dev)), "cdx_hand_spheres")
    return poses, centers


def cost_launch(hs, params, centers, dist, gdist):
    """cdx_hand_cost → (cost [E], depth [E, 3], worst [E, 3] int32, g_centers [E, S, 3])."""
    lib = N.load()
    E, dev = centers.shape[0], centers.device
    cost = torch.empty(E, dtype=torch.float64, device=dev)
    depth = torch.empty(E, 3, dtype=torch.float64, device=dev)
    worst = torch.empty(E, 3, dtype=torch.int32, device=dev)
    g = torch.empty(E, hs.n_spheres, 3, dtype=torch.float64, device=dev)
    N.check(lib.cdx_hand_cost(C.byref(hs.native()), C.byref(params), E, N.ptr(centers), N.ptr(dist), N.ptr(gdist),
                              N.ptr(cost), N.ptr(depth), N.ptr(worst), N.ptr(g), N.stream_ptr(dev)), "cdx_hand_cost")
    return cost, depth, worst, g


def pullback_launch(hs, poses, g_centers, palm_ori):
    """cdx_hand_pullback → (g_q [E, D], g_palm_pos [E, 3], g_palm_ori [E, 3])."""
    lib = N.load()
    E, dev = poses.shape[0], poses.device
    g_q = torch.empty(E, hs.desc.n_dofs, dtype=torch.float64, device=dev)
    g_pp = torch.empty(E, 3, dtype=torch.float64, device=dev)
    g_po = torch.empty(E, 3, dtype=torch.float64, device=dev)
    N.check(lib.cdx_hand_pullback(C.byref(hs.desc), C.byref(hs.native()), E, N.ptr(poses), N.ptr(g_centers),
                                  N.ptr(palm_ori), N.ptr(g_q), N.ptr(g_pp), N.ptr(g_po), N.stream_ptr(dev)),
            "cdx_hand_pullback")
    return g_q, g_pp, g_po


class _Centers(torch.autograd.Function):
    """cdx_hand_spheres; backward is cdx_hand_pullback."""

    @staticmethod
    def forward(ctx, q, palm_pose, hs):
        q = q.detach().contiguous()
        pp = po = None
        if palm_pose is not None:
            pp = palm_pose.detach()[:, :3].contiguous()
            po = palm_pose.detach()[:, 3:].contiguous()
        poses, centers = spheres_launch(hs, q, pp, po)
        ctx.hs, ctx.has_palm = hs, palm_pose is not None
        ctx.save_for_backward(poses, po)
        return centers

    @staticmethod
    def backward(ctx, g):
        poses, po = ctx.saved_tensors
        g_q, g_pp, g_po = pullback_launch(ctx.hs, poses, g.contiguous(), po)
        return g_q, (torch.cat([g_pp, g_po], 1) if ctx.has_palm else None), None


class _Cost(torch.autograd.Function):
    """cdx_hand_cost; ∂cost/∂centers = g_centers."""

    @staticmethod
    def forward(ctx, centers, dist, gdist, hs, params):
        cost, depth, worst, g = cost_launch(hs, params, centers.detach().contiguous(), dist, gdist)
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(depth, worst)
        return cost, depth, worst

    @staticmethod
    def backward(ctx, g_cost, *_):
        (g,) = ctx.saved_tensors
        return g_cost.view(-1, 1, 1) * g, None, None, None, None


# ------------------------------------------------------------------ the object's distance at the centres
def _mesh_of(obj, device):
    from .torchsdf import PreparedMesh
    if isinstance(obj, PreparedMesh):
        return obj
    if isinstance(obj, torch.Tensor):
        return PreparedMesh(obj.to(device=device, dtype=torch.float32))
    if hasattr(obj, "vertices") and hasattr(obj, "triangles"):
        v = torch.as_tensor(np.asarray(obj.vertices), dtype=torch.float32, device=device)
        f = torch.as_tensor(np.asarray(obj.triangles), dtype=torch.int64, device=device)
        return PreparedMesh(v[f])
    return None


def object_distance(obj, X):
    """(d [M], ∇d [M, 3]) float64 of ``obj`` at X [M, 3] float64, positive outside: a GPIS (the posterior mean and its
    gradient, one cdx_gpis_mean launch — the reference treats the mean as a distance), a PreparedMesh / face vertices
    [F, 3, 3] / TriangleMesh (one PreparedMesh.query on float32 points: sign·√sqdist and sign·normal) or a callable
    X → (d, ∇d)."""
    from .gpis import GPIS, gpis_mean
    if isinstance(obj, GPIS):
        mean, gmean, _ = gpis_mean(obj.native_state(), X, want_grad=True)
        return mean, gmean
    mesh = _mesh_of(obj, X.device)
    if mesh is not None:
        sq, sign, normal, _, _ = mesh.query(X.to(torch.float32))
        s = sign.to(torch.float64)
        return s * torch.sqrt(sq.to(torch.float64)), s[:, None] * normal.to(torch.float64)
    if callable(obj):
        d, gd = obj(X)
        return d, gd
    raise TypeError(f"obj must be a GPIS, a PreparedMesh, face vertices, a TriangleMesh or a callable, got {type(obj)}")


def hand_collision(hs, q, palm_pose=None, obj=None, floor_z=None, **margins_weights):
    """Whole-hand penetration cost of E candidates: places the spheres, queries the object once, scores.  →
    (cost [E], report) with report = dict(depth [E, 3], worst [E, 3], centers [E, S, 3], dist [E, S] | None), classes
    ordered (object, self, floor).  ``cost.sum().backward()`` fills ``q.grad`` and ``palm_pose.grad``.  A mesh given
    as face vertices or a TriangleMesh is prepared on every call: pass a PreparedMesh in a loop."""
    centers = hs.centers(q, palm_pose)
    dist = gdist = None
    if obj is not None:
        E, S = centers.shape[0], centers.shape[1]
        dist, gdist = object_distance(obj, centers.detach().reshape(E * S, 3))
        dist, gdist = dist.reshape(E, S), gdist.reshape(E, S, 3)
    cost, depth, worst = hs.cost(centers, dist, gdist, floor_z=floor_z, **margins_weights)
    return cost, dict(depth=depth, worst=worst, centers=centers.detach(), dist=dist)


# ------------------------------------------------------------------ the term of the optimisers' losses
class HandTerm:
    """The whole-hand collision term of an optimiser's loss (``optimize(..., hand_term=HandTerm(hand, …))`` of
    ProbabilisticGraspOptimizer, KinGPISGraspOptimizer, KinGraspOptimizer and WCKinGPISGraspOptimizer): per iteration
    and candidate ``loss += weight · hand_collision(hand, q, palm_pose, obj, floor_z, margins and weights)``, formed
    before the best-iterate comparison and the step, its gradient into the joint angles (and, in prob mode, the palm).
    ``obj`` None: the optimiser's own object (its GPIS; KinGraspOptimizer's mesh).  A value type: the optimisers read
    it and keep nothing in it."""

    def __init__(self, hand, weight=1.0, m_obj=0.0, m_self=0.0, m_floor=0.0, w_obj=1.0, w_self=1.0, w_floor=1.0,
                 floor_z=None, obj=None):
        if not isinstance(hand, HandSpheres):
            raise TypeError("HandTerm: hand must be a HandSpheres")
        self.hand, self.weight = hand, float(weight)
        self.m_obj, self.m_self, self.m_floor = float(m_obj), float(m_self), float(m_floor)
        self.w_obj, self.w_self, self.w_floor = float(w_obj), float(w_self), float(w_floor)
        self.floor_z = None if floor_z is None else float(floor_z)
        self.obj = obj
        if not all(math.isfinite(v) for v in (self.weight, *self.kwargs().values(), self.floor_z or 0.0)):
            raise ValueError("HandTerm: weight, margins, weights and floor_z must be finite")

    def key(self, own=None):
        """What a captured loop depends on: the model, the numbers and the object's fitted state (``own``: the
        optimiser's object, taken when ``obj`` is None)."""
        obj = self.object(own)
        st = obj.native_state() if hasattr(obj, "native_state") else obj
        return (id(self.hand), self.weight, self.m_obj, self.m_self, self.m_floor, self.w_obj, self.w_self,
                self.w_floor, self.floor_z, id(st))

    def kwargs(self):
        """hand_collision's margins and weights."""
        return dict(m_obj=self.m_obj, m_self=self.m_self, m_floor=self.m_floor, w_obj=self.w_obj, w_self=self.w_self,
                    w_floor=self.w_floor)

    def params(self):
        p = N.CdxHandParams()
        p.m_obj, p.m_self, p.m_floor = self.m_obj, self.m_self, self.m_floor
        p.w_obj, p.w_self, p.w_floor = self.w_obj, self.w_self, self.w_floor
        p.floor_on = 0 if self.floor_z is None else 1
        p.floor_z = 0.0 if self.floor_z is None else self.floor_z
        return p

    def object(self, own):
        return own if self.obj is None else self.obj

    def check(self, n_dofs, device):
        if self.hand.desc.n_dofs != n_dofs:
            raise ValueError(f"hand_term: the sphere model has {self.hand.desc.n_dofs} joints, the optimiser {n_dofs}")
        if torch.device(self.hand.device).type != torch.device(device).type:
            raise ValueError("hand_term: the sphere model and the optimiser must be on the same device")

    def cost(self, q, palm_pose, own_obj):
        """weight · hand_collision(...) [E] through autograd (the eager loops' term)."""
        cost, _ = hand_collision(self.hand, q, palm_pose, self.object(own_obj), floor_z=self.floor_z, **self.kwargs())
        return self.weight * cost

    def report(self, q, palm_pose, own_obj):
        """penetration_report at the returned joint angles and palm (device tensors, nothing read back)."""
        return penetration_report(self.hand, q.detach().double(), None if palm_pose is None else palm_pose.detach().double(),
                                  self.object(own_obj), floor_z=self.floor_z)


def palm_rows(palm_offset, E):
    """The palm pose [E, 6] float64 a Kin-style optimiser's forward_kinematics applies: its 3-entry ``palm_offset`` is a
    position, the angles are zero."""
    off = palm_offset.detach().to(torch.float64).reshape(-1)
    if off.numel() != 3:
        raise ValueError("hand_term needs a 3-entry palm_offset (the position forward_kinematics adds to the fingertips)")
    return torch.cat([off, torch.zeros(3, dtype=torch.float64, device=off.device)]).expand(E, 6).contiguous()


class TermLoop:
    """The term inside a fused loop: its buffers, allocated once with the loop state, and per iteration
    ``launch`` = cdx_hand_spheres on the current joint angles and palm, the GPIS mean and ∇mean at the S·E centres
    (``query``; a loop whose own cdx_gpis_mean launch carries the centres passes ``dist`` / ``gdist`` views instead)
    and cdx_hand_term with accumulate = 1 into the loop's loss and gradient buffers.  No allocation, no host sync."""

    def __init__(self, term, E, gpis, device, centers=None):
        from .gpis import GPIS
        hs = term.hand
        self.term, self.hs, self.E = term, hs, E
        self.params = term.params()
        f64 = dict(dtype=torch.float64, device=device)
        S = hs.n_spheres
        self.poses = torch.empty(E, hs.desc.n_bodies, 12, dtype=torch.float32, device=device)
        self.centers = torch.empty(E * S, 3, **f64) if centers is None else centers
        self.depth = torch.empty(E, 3, **f64)
        self.worst = torch.empty(E, 3, dtype=torch.int32, device=device)
        self.state = None
        if centers is None:
            obj = term.object(gpis)
            if not isinstance(obj, GPIS):
                raise ValueError("hand_term: a fused loop takes a GPIS object (use fused=False for a mesh or a callable)")
            self.state = obj.native_state()
            self.dist, self.gdist = torch.empty(E * S, **f64), torch.empty(E * S, 3, **f64)
        hs.native()  # (the tables are built before any capture)

    def place(self, lib, q, pp, po, stream):
        N.check(lib.cdx_hand_spheres(C.byref(self.hs.desc), C.byref(self.hs.native()), self.E, N.ptr(q), N.ptr(pp),
                                     N.ptr(po), N.ptr(self.poses), N.ptr(self.centers), stream), "cdx_hand_spheres")

    def query(self, lib, stream):
        N.check(lib.cdx_gpis_mean(self.state.desc, N.ptr(self.centers), self.E * self.hs.n_spheres, N.ptr(self.dist),
                                  N.ptr(self.gdist), None, stream), "cdx_gpis_mean")

    def add(self, lib, po, loss, g_q, g_pp, g_po, stream, dist=None, gdist=None):
        N.check(lib.cdx_hand_term(C.byref(self.hs.desc), C.byref(self.hs.native()), C.byref(self.params), self.E,
                                  N.ptr(self.poses), N.ptr(self.centers), N.ptr(self.dist if dist is None else dist),
                                  N.ptr(self.gdist if gdist is None else gdist), N.ptr(po), self.term.weight, 1,
                                  N.ptr(loss), N.ptr(g_q), N.ptr(g_pp), N.ptr(g_po), N.ptr(self.depth),
                                  N.ptr(self.worst), stream), "cdx_hand_term")


class _Report(dict):
    """penetration_report's dict; ``worst_links`` is resolved on the host (a read-back) only when asked for."""

    def __missing__(self, key):
        if key != "worst_links":
            raise KeyError(key)
        self[key] = self.hs.names(self["worst"])
        return self[key]


def penetration_report(hs, q, palm_pose, obj, floor_z=None, allow=0.0):
    """dict(depth [E, 3] the largest penetration per class (object, self, floor) at zero margin — positive means
    intersecting, −inf a class that is off —, worst [E, 3] the sphere / pair that attains it, clear [E] bool: every
    depth ≤ allow, and, on request, worst_links: names per row as ``HandSpheres.names`` gives them).  Nothing is read
    back unless the caller reads."""
    with torch.no_grad():
        _, rep = hand_collision(hs, q, palm_pose, obj, floor_z)
    out = _Report(depth=rep["depth"], worst=rep["worst"], clear=(rep["depth"] <= float(allow)).all(1))
    out.hs = hs
    return out
