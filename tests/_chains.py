"""Synthetic kinematic chains for the FK family of kernels, and a float64 statement of what they compute.

The three packaged robots reach a small corner of what a ``cdx_chain`` may describe (no −x / −y axis, no sign-0 joint,
no tip on the root or an inner body, never more than 4 tips or 23 DOFs, depths 4, 6 and 13 only).  ``bodies(case)``
generates chains in the packaged-robot JSON form that cover the rest: every axis with either sign, a joint whose axis is
(0, 0, 0), fixed joints, tips on the root and on inner bodies, the depths 8 | 9 where the kernels change their register
bound, the depth limit 16, and the largest chain the descriptor holds.

``statement(desc, q, gpos)`` restates FK from the descriptor in torch float64: positions, quaternions and the
vector-Jacobian product with the reference's semantics (the quaternion branch of spatial_vector_algebra.py:108-136 with
the DETACHED scale, then quat_rotate; autograd with the scale taken out of the graph does exactly this).  The geometric
Jacobian's statement stays tests/_ik.np_fk_jac.

Tolerances.  They come from the float32 restatement of the reference (oracle.cdx_oracle.OracleChain, autograd for the
gradient) measured against the float64 statement on the same inputs — per quantity max|a − b| / max|b|, maximised over
the family (both offset variants, B = 257; ``measure_oracle`` recomputes it, test_chains_cpu pins it):

    quantity                     oracle vs float64    tolerance = 4 ×
    pos   (positions)                 6.1e-7               2.5e-6
    quat  (quaternions)               3.7e-7               1.5e-6
    grad  (vector-Jacobian product)   5.0e-7               2.0e-6

(With offsets the position is mostly quat_rotate(quat, offset), quadratic in a quaternion that carries up to 16
levels of rounded rotation products: its figure is the largest of the three.)

A kernel and the oracle round the same number of float32 operations in different orders (the device has its own
sin / cos, fk_tip_bwd2 / bwd3 associate the products differently), which a small factor covers; a wrong term, sign,
axis or branch shows at 1e-3 or more.
"""
import functools
import json
import math
import os

import numpy as np
import torch

from tests import _ik

PI = math.pi
B_MAX = 257
BATCHES = (1, 63, 65, 257)
CASES = ("line8", "line9", "line16", "tree8", "hand8", "hand9", "hand16")
HANDS = ("hand8", "hand9", "hand16")
NEAR = 1e-3        # rows this close to a quaternion branch decision are left out of the branch-dependent comparisons
MAX_EXCLUDED = 0.05
MIN_PER_BRANCH = 8
REACH = 0.15       # every tip stays this close to the origin (the packaged GPIS states are usable there)
OFFSET = 0.05

# OracleChain (float32) against the float64 statement, measured by measure_oracle() over CASES × {offsets, none} at
# B = 257, and the tolerances derived from it (4 ×, see the module docstring).
ORACLE_ERR = dict(pos=6.2e-7, quat=3.8e-7, grad=5.0e-7)  # measured 6.11e-7, 3.73e-7, 4.95e-7
TOL = {k: 4.0 * v for k, v in ORACLE_ERR.items()}
TOL_JAC = 2e-5     # the project's bound on the geometric Jacobian (test_jacobian_vs_numpy)


# ------------------------------------------------------------------ the chain family
def _topology(case):
    """→ (parent [n], fixed body indices, tip body indices)."""
    if case.startswith("line"):
        depth = int(case[4:])
        parent = [-1] + list(range(depth))
        if depth == 8:
            return parent, [], [8, 3]
        if depth == 9:
            return parent, [4], [9, 0]  # a fixed joint on the path; a tip on the root (empty path)
        return parent, [7], [16]
    if case == "tree8":
        parent = [-1] + list(range(12))          # spine 1..12 (depth = index)
        parent += [4, 13, 14, 15]                # 13..16 off body 4: depths 5..8
        parent += [8, 17, 18]                    # 17..19 off body 8: depths 9..11
        parent += [0, 20]                        # 20, 21 off the root: depths 1, 2
        parent += [9, 22, 23]                    # 22..24 off body 9: depths 10..12
        parent += [13, 25, 26]                   # 25..27 off body 13: depths 6..8
        parent += [3, 28, 29, 30]                # 28..31 off body 3: depths 4..7
        return parent, [], [12, 1, 16, 19, 21, 24, 26, 31]  # body 1 and body 26 are inner bodies
    arm = int(case[4:]) - 4                      # hands: an arm, then four fingers of 4, 3, 4 and 2 bodies
    parent, tips = [-1] + list(range(arm)), []
    for n in (4, 3, 4, 2):
        last = arm
        for _ in range(n):
            parent.append(last)
            last = len(parent) - 1
        tips.append(last)
    return parent, [2], tips


def _depth(parent, b):
    d = 0
    while b > 0:
        d, b = d + 1, parent[b]
    return d


@functools.lru_cache(None)
def bodies(case):
    """→ (bodies in the packaged-robot JSON form, tip link names).  Fixed seed per case."""
    parent, fixed, tips = _topology(case)
    n = len(parent)
    rng = np.random.default_rng(1000 + CASES.index(case))
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    moving = [i for i in range(1, n) if i not in fixed]
    order = [axes[j % 6] for j in rng.permutation(len(moving))]
    zero = moving[len(moving) // 2]  # the joint whose axis is (0, 0, 0): sign 0, it has a DOF and never moves
    xyz = rng.standard_normal((n, 3))
    xyz *= (0.5 + 0.5 * rng.random((n, 1))) / np.linalg.norm(xyz, axis=1, keepdims=True)
    xyz[0] = 0.0

    def path_len(b):
        s = 0.0
        while b > 0:
            s, b = s + float(np.linalg.norm(xyz[b])), parent[b]
        return s
    xyz *= (REACH - OFFSET * math.sqrt(3.0)) * 0.98 / max(path_len(t) for t in tips)
    out = []
    for i in range(n):
        if i == 0 or i in fixed:
            joint, axis = "fixed", [0.0, 0.0, 0.0]
        else:
            joint = "revolute"
            axis = [0.0, 0.0, 0.0] if i == zero else [float(v) for v in order[moving.index(i)]]
        out.append(dict(name=f"b{i}", parent=parent[i], joint=joint, joint_name=f"j{i}",
                        xyz=[0.0] * 3 if i == 0 else [float(v) for v in xyz[i]],
                        rpy=[0.0] * 3 if i == 0 else [float(v) for v in rng.uniform(-PI, PI, 3)],
                        axis=axis, lower=-PI, upper=PI))
    return out, [f"b{t}" for t in tips]


def tip_offsets(case):
    _, links = bodies(case)
    rng = np.random.default_rng(2000 + CASES.index(case))
    return rng.uniform(-OFFSET, OFFSET, (len(links), 3)).tolist()


def depths(case):
    parent, _, tips = _topology(case)
    return [_depth(parent, t) for t in tips]


def robot_dict(case, config=None):
    b, links = bodies(case)
    cfg = dict(ee_link_name=links, ee_link_offset=tip_offsets(case),
               ref_q=[0.0] * sum(x["joint"] != "fixed" for x in b[1:]))
    cfg.update(config or {})  # (may replace the fingertips: a subset of the tips)
    return dict(name=case, bodies=b, config=cfg)


def write_json(case, tmp_path, config=None):
    """The chain as a packaged-robot JSON file: Chain(load_robot(path)), OracleChain(load_robot(path)["bodies"]) and
    every optimiser's ``robot`` argument accept the path."""
    path = os.path.join(str(tmp_path), f"{case}.json")
    with open(path, "w") as f:
        json.dump(robot_dict(case, config), f)
    return path


def chain_of(robot):
    from compliancedex_amd.chain import Chain
    return Chain(robot)


def chain(case):
    return chain_of(robot_dict(case))


@functools.lru_cache(None)
def descriptor(case, offsets=True):
    _, links = bodies(case)
    return chain(case).descriptor(links, tip_offsets(case) if offsets else None)


def line(depth, fixed=()):
    """A line of bodies with unit F, t = (0.1, 0, 0) and z joints, the tip `depth` levels deep (the depth-limit cases;
    any depth the descriptor holds, so also chains the library must refuse)."""
    out = [dict(name="b0", parent=-1, joint="fixed", xyz=[0.0] * 3, rpy=[0.0] * 3, axis=[0.0] * 3, lower=0.0, upper=0.0)]
    for i in range(1, depth + 1):
        fx = i in fixed
        out.append(dict(name=f"b{i}", parent=i - 1, joint="fixed" if fx else "revolute", xyz=[0.1, 0.0, 0.0],
                        rpy=[0.0] * 3, axis=[0.0] * 3 if fx else [0.0, 0.0, 1.0], lower=-PI, upper=PI))
    return dict(name=f"line{depth}", bodies=out)


def raw_descriptor(robot, tip_links, offsets=None):
    """The cdx_chain of `robot` without Chain.descriptor's depth check (what a C caller can hand the library)."""
    from compliancedex_amd._native import MAX_TIPS
    ch = chain_of(robot)
    d = ch.descriptor([robot["bodies"][0]["name"]] * len(tip_links), offsets)
    assert len(tip_links) <= MAX_TIPS
    for k, name in enumerate(tip_links):
        d.tip_body[k] = ch.index[name]
    return d


@functools.lru_cache(None)
def joint_rows(case, B=B_MAX):
    """q [B, D] uniform in [−π, π], rounded to float32, and a cotangent gpos [B, T, 3] (float32 standard normal)."""
    d = descriptor(case)
    rng = np.random.default_rng(3000 + CASES.index(case))
    q = rng.uniform(-PI, PI, (B, d.n_dofs)).astype(np.float32)
    gpos = rng.standard_normal((B, d.n_tips, 3)).astype(np.float32)
    return q, gpos


# ------------------------------------------------------------------ the float64 statement
def _axis_rot(axis, th):
    c, s = torch.cos(th), torch.sin(th)
    A = torch.zeros(th.shape[0], 3, 3, dtype=torch.float64)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    A[:, axis, axis] = 1.0
    A[:, i, i] = c
    A[:, j, j] = c
    A[:, i, j] = -s
    A[:, j, i] = s
    return A


def _quaternion(R):
    """xyzw [B, 4] with the reference's branches and its detached scale; → (quat, branch [B] (−1 = trace, else the
    pivot), distance [B] of the row from the nearest branch decision)."""
    d0, d1, d2 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    trace = d0 + d1 + d2
    cands = [torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1], trace + 1.0], 1)]
    for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        comp = [None] * 4
        comp[i] = R[:, i, i] - (R[:, j, j] + R[:, k, k]) + 1.0
        comp[j] = R[:, i, j] + R[:, j, i]
        comp[k] = R[:, k, i] + R[:, i, k]
        comp[3] = R[:, k, j] - R[:, j, k]
        cands.append(torch.stack(comp, 1))
    with torch.no_grad():
        pivot = torch.zeros_like(trace, dtype=torch.long)
        pivot = torch.where(d1 > d0, torch.ones_like(pivot), pivot)
        top = torch.where(pivot == 1, d1, d0)
        pivot = torch.where(d2 > top, torch.full_like(pivot, 2), pivot)
        branch = torch.where(trace + 1.0 > 1.0, torch.full_like(pivot, -1), pivot)
        diag = torch.sort(torch.stack([d0, d1, d2], 1), dim=1).values
        gap = diag[:, 2] - diag[:, 1]
        dist = torch.where(branch < 0, trace.abs(), torch.minimum(trace.abs(), gap))
    raw = torch.stack(cands, 1)[torch.arange(R.shape[0]), branch + 1]  # [B, 4] un-scaled components
    tn = torch.where(branch < 0, raw[:, 3], raw[torch.arange(R.shape[0]), branch.clamp(min=0)])
    scale = 0.5 / torch.sqrt(tn.detach())  # math.sqrt on a tensor: a constant for autograd
    return raw * scale[:, None], branch, dist


def _quat_rotate(q, v):
    w, qv = q[:, 3:4], q[:, :3]
    return v * (2.0 * w ** 2 - 1.0) + torch.cross(qv, v.expand_as(qv), dim=-1) * w * 2.0 + \
        qv * (qv * v).sum(-1, keepdim=True) * 2.0


def statement(desc, q, gpos=None):
    """FK of `desc` at q [B, D] in float64 → dict(pos [B, T, 3], quat [B, T, 4], branch [B, T], dist [B, T]) and, with a
    cotangent gpos [B, T, 3], grad [B, D] = (∂pos/∂q)ᵀ·gpos with the reference's detached quaternion scale."""
    qt = torch.tensor(np.array(q, np.float64), requires_grad=gpos is not None)
    B, T = qt.shape[0], desc.n_tips
    pos, quat, branch, dist = [], [], [], []
    for k in range(T):
        path, b = [], desc.tip_body[k]
        while b > 0:
            path.append(b)
            b = desc.bodies[b].parent
        R = torch.eye(3, dtype=torch.float64).expand(B, 3, 3)
        t = torch.zeros(B, 3, dtype=torch.float64)
        for bi in reversed(path):
            body = desc.bodies[bi]
            F = torch.tensor(list(body.F), dtype=torch.float64).view(3, 3)
            t = t + R @ torch.tensor(list(body.t), dtype=torch.float64)
            R = R @ F
            if body.dof >= 0:
                R = R @ _axis_rot(body.axis, float(body.sign) * qt[:, body.dof])
        qk, br, ds = _quaternion(R)
        p = t
        if desc.has_offsets:
            p = t + _quat_rotate(qk, torch.tensor(list(desc.tip_offset[k]), dtype=torch.float64).view(1, 3))
        pos.append(p)
        quat.append(qk)
        branch.append(br)
        dist.append(ds)
    pos = torch.stack(pos, 1)
    out = dict(pos=pos.detach().numpy(), quat=torch.stack(quat, 1).detach().numpy(),
               branch=torch.stack(branch, 1).numpy(), dist=torch.stack(dist, 1).numpy())
    if gpos is not None:
        (pos * torch.tensor(np.array(gpos, np.float64)).view(B, T, 3)).sum().backward()
        out["grad"] = qt.grad.numpy()
    return out


def oracle(case, offsets, q, gpos):
    """The float32 restatement of the reference on the same inputs → dict(pos, quat, grad)."""
    from oracle.cdx_oracle import OracleChain
    b, links = bodies(case)
    ch = OracleChain(b)
    qt = torch.tensor(np.array(q, np.float32), requires_grad=True)
    pos, quat = ch.forward_kinematics(qt, links, tip_offsets(case) if offsets else None)
    T = len(links)
    (pos.view(-1, T, 3) * torch.tensor(np.array(gpos, np.float32)).view(-1, T, 3)).sum().backward()
    return dict(pos=pos.detach().numpy().reshape(-1, T, 3), quat=quat.detach().numpy().reshape(-1, T, 4),
                grad=qt.grad.numpy())


@functools.lru_cache(None)
def reference(case, offsets=True):
    """The float64 statement of a case at its 257 rows, computed once and shared (read-only), with the conditions that
    keep a comparison from passing on thin data checked here:
      * with offsets, each of the four quaternion branches holds at least MIN_PER_BRANCH (row, tip) pairs;
      * at most MAX_EXCLUDED of the rows lie within NEAR of a branch decision (``keep`` marks the others)."""
    desc = descriptor(case, offsets)
    q, gpos = joint_rows(case)
    ref = statement(desc, q, gpos)
    ref["q"], ref["gpos"] = q, gpos
    ref["keep"] = (ref["dist"] >= NEAR).all(1)  # [B]: no tip of the row is near a decision
    ref["keep_tip"] = ref["dist"] >= NEAR        # [B, T]
    if offsets:
        counts = {br: int((ref["branch"] == br).sum()) for br in (-1, 0, 1, 2)}
        assert min(counts.values()) >= MIN_PER_BRANCH, (case, counts)
    assert 1.0 - ref["keep"].mean() <= MAX_EXCLUDED, (case, 1.0 - ref["keep"].mean())
    for v in ref.values():
        v.setflags(write=False)
    return ref


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def compare(got, case, offsets, B):
    """rel. errors of dict(pos [B, T·3], quat [B, T·4] | None, grad [B, D] | None) against the statement's first B
    rows: positions on every row; quaternions on the (row, tip) pairs and offset gradients on the rows away from a
    branch decision; no-offset gradients on every row (they do not see the quaternion)."""
    ref = reference(case, offsets)
    T = ref["pos"].shape[1]
    out = dict(pos=rel(np.reshape(got["pos"], (B, T, 3)), ref["pos"][:B]))
    if got.get("quat") is not None:
        kt = ref["keep_tip"][:B]
        out["quat"] = rel(np.reshape(got["quat"], (B, T, 4))[kt], ref["quat"][:B][kt]) if kt.any() else 0.0
    if got.get("grad") is not None:
        rows = ref["keep"][:B] if offsets else np.ones(B, bool)
        out["grad"] = rel(got["grad"][rows], ref["grad"][:B][rows]) if rows.any() else 0.0
    return out


def check_primitives(case, offsets, fk, bwd, jac):
    """The assertions of section 2, shared with the device file: fk(desc, q, B) → (pos, quat), bwd(desc, q, gpos, B) →
    grad, jac(desc, q, B, ang) → (lin, ang | None)."""
    desc = descriptor(case, offsets)
    ref = reference(case, offsets)
    q, gpos = ref["q"], ref["gpos"]
    _, lin_ref, ang_ref = _ik.np_fk_jac(desc, q)
    off = ~np.broadcast_to(_ik.on_path(desc)[None, :, None, :], lin_ref.shape)
    for B in BATCHES:
        pos, quat = fk(desc, q, B)
        e = compare(dict(pos=pos, quat=quat, grad=bwd(desc, q, gpos, B)), case, offsets, B)
        lin, ang = jac(desc, q, B, True)
        e["lin"], e["ang"] = rel(lin, lin_ref[:B]), rel(ang, ang_ref[:B])
        print(case, "offsets" if offsets else "no offsets", B, {k: f"{v:.2e}" for k, v in e.items()})
        for k in ("pos", "quat", "grad"):
            assert e[k] < TOL[k], (case, offsets, B, k, e[k])
        assert e["lin"] < TOL_JAC and e["ang"] < TOL_JAC, (case, offsets, B, e)
        assert (lin[off[:B]] == 0).all() and (ang[off[:B]] == 0).all()
        only, none = jac(desc, q, B, False)
        assert none is None and _ik.same_bits(only, lin)
        assert _ik.same_bits(fk(desc, q, B)[0], pos)


def measure_oracle():
    """→ dict(pos, quat, grad): OracleChain against the float64 statement, maximised over the family."""
    worst = dict(pos=0.0, quat=0.0, grad=0.0)
    for case in CASES:
        for offsets in (True, False):
            q, gpos = joint_rows(case)
            e = compare({k: v for k, v in oracle(case, offsets, q, gpos).items()}, case, offsets, B_MAX)
            for k in worst:
                worst[k] = max(worst[k], e[k])
    return worst


# ------------------------------------------------------------------ shared pipeline inputs
COLLISION_PAIRS = [[0, 1], [2, 3], [4, 5], [6, 7], [0, 5], [1, 4]]  # over tree8's eight tips as anchors
COLLISION_THRESHOLD = 0.05  # (tips within 0.15 m of the origin: a share of the pairs is closer than this)


@functools.lru_cache(None)
def collision_rows(E=65):
    """q [E, D] and palm [E, 6] (float64) for the collision loss on tree8, and the oracle's cost and gradients.  Rows
    whose masks (pair distance against the threshold, anchor and palm height against the 0.02 m floor) are decided by
    less than 1e-3, or with an anchor within 1e-3 of z = 0 (where 1/z amplifies the float32 FK's last bit without
    bound), are redrawn: the comparison is then one of values, not of mask decisions."""
    from oracle.cdx_oracle import OracleChain, collision_loss, euler_xyz
    b, links = bodies("tree8")
    ch, offs = OracleChain(b), tip_offsets("tree8")
    D = descriptor("tree8").n_dofs
    rng = np.random.default_rng(77)
    q, palm = np.zeros((0, D)), np.zeros((0, 6))
    pr = np.asarray(COLLISION_PAIRS)
    while len(q) < E:
        qn = rng.uniform(-PI, PI, (E, D))
        pn = np.concatenate([rng.uniform(-0.05, 0.05, (E, 2)), rng.uniform(0.0, 0.12, (E, 1)),
                             rng.uniform(-PI, PI, (E, 3))], 1)
        a = ch.forward_kinematics(torch.from_numpy(qn).float(), links, offs)[0].double().view(E, -1, 3)
        a = (torch.bmm(euler_xyz(torch.from_numpy(pn[:, 3:])), a.transpose(1, 2)).transpose(1, 2)
             + torch.from_numpy(pn[:, None, :3])).numpy()
        d = np.linalg.norm(a[:, pr[:, 0]] - a[:, pr[:, 1]], axis=2)
        z = np.concatenate([a[:, :, 2], pn[:, 2:3]], 1)
        ok = ((np.abs(d - COLLISION_THRESHOLD) > 1e-3).all(1) & (np.abs(z - 0.02) > 1e-3).all(1)
              & (np.abs(z) > 1e-3).all(1))
        q, palm = np.concatenate([q, qn[ok]]), np.concatenate([palm, pn[ok]])
    q, palm = q[:E].copy(), palm[:E].copy()
    qt = torch.from_numpy(q).requires_grad_(True)
    pt = torch.from_numpy(palm).requires_grad_(True)
    cost = collision_loss(ch, links, offs, COLLISION_PAIRS, qt, pt, threshold=COLLISION_THRESHOLD)
    cost.sum().backward()
    out = dict(q=q, palm=palm, cost=cost.detach().numpy(), grad_q=qt.grad.numpy(), grad_palm=pt.grad.numpy())
    # row 0 is the E = 1 case: a row with a floor term (a row with pair terms only has a palm gradient of exactly 0 —
    # the pair distances do not see the palm — and its computed value is rounding noise)
    first = int(np.flatnonzero((np.abs(out["grad_palm"]).max(1) > 1.0) & (np.abs(out["grad_q"]).max(1) > 1.0))[0])
    for v in out.values():
        v[[0, first]] = v[[first, 0]]
    assert (out["cost"] != 0).mean() > 0.5  # the terms are live …
    assert np.abs(out["grad_palm"][0]).max() > 1.0 and np.abs(out["grad_q"][0]).max() > 1.0  # … in the first row too
    for v in out.values():
        v.setflags(write=False)
    return out


def collision_descriptor():
    from compliancedex_amd.problem import build_collision
    return build_collision(descriptor("tree8"), COLLISION_PAIRS, threshold=COLLISION_THRESHOLD)


def closure_inputs(case, E=5):
    """(q, comp, target, palm, noise [3·E, 3, 3]) of a prob-mode closure on a synthetic hand: workloads.prob_inputs
    around the banana with the joints spread over ±0.3 rad and a replayed Kabsch noise draw."""
    from compliancedex_amd.workloads import prob_inputs
    D = descriptor(case).n_dofs
    q, comp, target, palm = prob_inputs([0.0] * D, E, seed=2, spread=True)
    rng = np.random.default_rng(3)
    q = q + 0.3 * rng.standard_normal(q.shape)
    return q, comp, target, palm, rng.random((3 * E, 3, 3))


def oracle_closure(case, q, comp, target, palm, noise):
    from oracle.cdx_oracle import OracleChain, OracleProblem, closure_with_grads
    from tests._helpers import oracle_gpis
    b, links = bodies(case)
    prob = OracleProblem(OracleChain(b), links, tip_offsets(case), [0.0] * q.shape[1], oracle_gpis("banana"))
    return closure_with_grads(prob, q, comp, target, palm, noise)


def hand_kin_inputs(case, E, q_scale=0.3, seed=44):
    """workloads.config4_kin_inputs for a synthetic hand: (links, offsets, palm_offset [3], q [E, D], target [E, 4, 3],
    comp [E, 4]) in float32 — joints q_scale·randn, the q = 0 fingertips' centre moved onto the banana's."""
    from compliancedex_amd.workloads import DATA
    from tests import _host
    _, links = bodies(case)
    desc = descriptor(case)
    center = np.load(os.path.join(DATA, "banana_center.npy"))
    tips0 = _host.fk_forward(desc, np.zeros((1, desc.n_dofs), np.float32))[0].reshape(4, 3).astype(np.float64).mean(0)
    rng = np.random.default_rng(seed)
    q = (q_scale * rng.standard_normal((E, desc.n_dofs))).astype(np.float32)
    target = (np.tile(center, (E, 4, 1)) + 0.01 * rng.standard_normal((E, 4, 3))).astype(np.float32)
    comp = np.tile(np.array([10.0, 10.0, 10.0, 20.0], np.float32), (E, 1))
    return links, tip_offsets(case), (center - tips0).astype(np.float32), q, target, comp


@functools.lru_cache(None)
def ik_rows(case, E=67, seed=9):
    """IK inputs on a synthetic chain and the host build's answers: q* uniform in the inner 80 % of the joint box
    [−π, π], targets FK_f32(q*) widened, starts q* + 0.05·randn → dict(params(max_iters), q0, target, one, full) with
    `one` / `full` the host's solve after one iteration / to the end (50 iterations at most)."""
    from compliancedex_amd.ik import ik_params
    from tests import _host
    desc = descriptor(case)
    D = desc.n_dofs
    rng = np.random.default_rng(seed)
    qs = 0.8 * PI * (2.0 * rng.random((E, D)) - 1.0)
    q0 = qs + 0.05 * rng.standard_normal((E, D))
    target = _host.fk_forward(desc, qs)[0].astype(np.float64).reshape(E, desc.n_tips, 3)

    def params(max_iters):
        return ik_params([-PI] * D, [PI] * D, [0.0] * D, 0.0, max_iters, _ik.TOL)
    return dict(params=params, q0=q0, target=target, one=_ik.ik_solve_host(desc, params(1), q0, target),
                full=_ik.ik_solve_host(desc, params(_ik.MAX_ITERS), q0, target))


def ik_mem_bytes(T, D):
    """csrc/cdx_ik.h's per-row storage, restated: doubles A n(n+1)/2, g D, y n, dv 2n; floats J n·D, q D, qn D."""
    n = 3 * T
    return 8 * (n * (n + 1) // 2 + D + n + 2 * n) + 4 * (n * D + 2 * D)


def ik_rows_per_block(T, D):
    """… and the launch's rows per workgroup: the largest power of two ≤ 64 whose rows fit 40 KB of LDS."""
    lanes = 64
    while lanes > 1 and ik_mem_bytes(T, D) * lanes > 40960:
        lanes //= 2
    return lanes
