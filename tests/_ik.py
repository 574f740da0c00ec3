"""Test helpers of the fingertip Jacobians and the IK solve: ctypes wrappers of the host build's two entries, a float64
numpy statement of chain FK, of the geometric Jacobian and of the palm transform, and the shared cases."""
import ctypes as C
import functools
import math

import numpy as np

from compliancedex_amd._native import CdxChain, CdxIkParams
from compliancedex_amd.ik import ik_params, joint_box
from tests._helpers import golden, product_chain
from tests._host import host, p

F32, F64 = 0, 1  # CDX_DTYPE_*


# ------------------------------------------------------------------ host build
def fk_jacobian_host(desc: CdxChain, q, ang=True):
    q = np.ascontiguousarray(q, np.float32)
    B, T, D = q.shape[0], desc.n_tips, desc.n_dofs
    lin = np.full((B, T, 3, D), 7.0, np.float32)
    a = np.full((B, T, 3, D), 7.0, np.float32) if ang else None
    rc = host().cdxh_fk_jacobian(C.byref(desc), p(q), B, p(lin), p(a))
    assert rc == 0, rc
    return lin, a


def ik_solve_host(desc: CdxChain, params: CdxIkParams, q0, target, palm=None, palm_offset=None, w=None):
    """→ dict(q, err, iters, status); q0 float32 or float64 [E, D]."""
    q0 = np.ascontiguousarray(q0)
    assert q0.dtype in (np.float32, np.float64)
    E, T, D = q0.shape[0], desc.n_tips, desc.n_dofs
    target = np.ascontiguousarray(target, np.float64).reshape(E, T, 3)
    palm = None if palm is None else np.ascontiguousarray(palm, np.float64).reshape(E, 6)
    w = None if w is None else np.ascontiguousarray(w, np.float64).reshape(E, T)
    po = None if palm_offset is None else (C.c_double * 3)(*[float(v) for v in palm_offset])
    q = np.full_like(q0, 7.0)
    err = np.full((E, T), 7.0)
    iters = np.full(E, -7, np.int32)
    status = np.full(E, -7, np.int32)
    rc = host().cdxh_ik_solve(C.byref(desc), C.byref(params), E, p(q0), F64 if q0.dtype == np.float64 else F32,
                              p(target), p(palm), po, p(w), p(q), p(err), p(iters), p(status))
    assert rc == 0, rc
    return dict(q=q, err=err, iters=iters, status=status)


# ------------------------------------------------------------------ numpy statement (float64)
def _axis_rot(axis, th):
    c, s = np.cos(th), np.sin(th)
    A = np.zeros(th.shape + (3, 3))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    A[..., axis, axis] = 1.0
    A[..., i, i] = c
    A[..., j, j] = c
    A[..., i, j] = -s
    A[..., j, i] = s
    return A


def _paths(desc):
    for k in range(desc.n_tips):
        path, b = [], desc.tip_body[k]
        while b > 0:
            path.append(b)
            b = desc.bodies[b].parent
        yield k, path[::-1]


def np_fk_jac(desc: CdxChain, q):
    """→ pos [B, T, 3], lin [B, T, 3, D], ang [B, T, 3, D] in float64 from the descriptor's bodies: world poses by
    R' = R·F·A(sign·q), t' = R·t_b + t; p = t + R·offset; lin[:, dof] = sign·ω × (p − o), ang[:, dof] = sign·ω with
    ω = R_parent·F·e_axis and o the joint's world origin."""
    q = np.asarray(q, np.float64)
    B, T, D = q.shape[0], desc.n_tips, desc.n_dofs
    pos, lin, ang = np.zeros((B, T, 3)), np.zeros((B, T, 3, D)), np.zeros((B, T, 3, D))
    for k, path in _paths(desc):
        R, t = np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3))
        joints = []
        for bi in path:
            b = desc.bodies[bi]
            F = np.array(list(b.F), np.float64).reshape(3, 3)
            t = t + R @ np.array(list(b.t), np.float64)
            M = R @ F
            if b.dof >= 0:
                joints.append((b.dof, float(b.sign), M[:, :, b.axis].copy(), t.copy()))
                R = M @ _axis_rot(b.axis, float(b.sign) * q[:, b.dof])
            else:
                R = M
        pt = t
        if desc.has_offsets:
            pt = t + R @ np.array(list(desc.tip_offset[k]), np.float64)
        pos[:, k] = pt
        for dof, sign, om, o in joints:
            lin[:, k, :, dof] = sign * np.cross(om, pt - o)
            ang[:, k, :, dof] = sign * om
    return pos, lin, ang


def on_path(desc):
    """[T, D] bool: joint d moves tip k."""
    m = np.zeros((desc.n_tips, desc.n_dofs), bool)
    for k, path in _paths(desc):
        for bi in path:
            if desc.bodies[bi].dof >= 0:
                m[k, desc.bodies[bi].dof] = True
    return m


def _mm(a, b):
    """[N, 3, 3] products with the rule's order: (a_i0·b_0j + a_i1·b_1j) + a_i2·b_2j, each operation rounded."""
    c = np.empty_like(a)
    for i in range(3):
        for j in range(3):
            c[:, i, j] = (a[:, i, 0] * b[:, 0, j] + a[:, i, 1] * b[:, 1, j]) + a[:, i, 2] * b[:, 2, j]
    return c


def host_sincos(ang):
    """sin and cos of a float64 array through the C library (math.sin / math.cos), as the host build takes them."""
    ang = np.asarray(ang, np.float64)
    s = np.array([math.sin(v) for v in ang.reshape(-1)]).reshape(ang.shape)
    c = np.array([math.cos(v) for v in ang.reshape(-1)]).reshape(ang.shape)
    return s, c


def palm_rotation(sin, cos):
    """R = (Rx(a)·Ry(b))·Rz(c) [N, 3, 3] from the sines / cosines [N, 3] of the XYZ Euler angles."""
    N = sin.shape[0]
    mats = []
    for axis in range(3):
        A = np.zeros((N, 3, 3))
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        A[:, axis, axis] = 1.0
        A[:, i, i] = cos[:, axis]
        A[:, j, j] = cos[:, axis]
        A[:, i, j] = -sin[:, axis]
        A[:, j, i] = sin[:, axis]
        mats.append(A)
    return _mm(_mm(mats[0], mats[1]), mats[2])


def world_tips(pos32, palm=None, palm_offset=None, sincos=None):
    """The rule's fingertips from float32 FK positions [E, T, 3]: (Rp·double(pos) + palm_pos) + palm_offset, in the
    rule's order of operations.  ``sincos``: (sin, cos) [E, 3] of the palm angles (default: the C library's)."""
    v = np.asarray(pos32, np.float32).astype(np.float64)
    E = v.shape[0]
    if palm is None:
        R, pp = np.broadcast_to(np.eye(3), (E, 3, 3)), np.zeros((E, 3))
    else:
        palm = np.asarray(palm, np.float64)
        s, c = sincos if sincos is not None else host_sincos(palm[:, 3:])
        R, pp = palm_rotation(s, c), palm[:, :3]
    po = np.zeros(3) if palm_offset is None else np.asarray(palm_offset, np.float64)
    out = np.empty_like(v)
    for i in range(3):
        x = (R[:, None, i, 0] * v[:, :, 0] + R[:, None, i, 1] * v[:, :, 1]) + R[:, None, i, 2] * v[:, :, 2]
        out[:, :, i] = (x + pp[:, None, i]) + po[i]
    return out


def tip_errors(tips, target):
    d = np.asarray(target, np.float64).reshape(tips.shape) - tips
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def ik_cost(err, q, w=None, ref_q=None, rho=0.0):
    """½·Σ (w·e)² + ½·ρ·‖q − ref_q‖² per row (plain float64; for comparisons of costs, not of bits)."""
    we = err if w is None else err * w
    c = 0.5 * (we * we).sum(1)
    if rho:
        c = c + 0.5 * rho * ((np.asarray(q, np.float64) - np.asarray(ref_q)) ** 2).sum(1)
    return c


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ shared cases
TOL = 1e-5
MAX_ITERS = 50


@functools.lru_cache(None)
def hand(robot="allegro"):
    """(Chain, fingertip descriptor, lower, upper, ref_q, links, offsets) of a packaged robot; iiwa7_allegro takes the
    fingertip links and offsets of its FK fixture and ref_q = the middle of the limits."""
    ch = product_chain(robot)
    lower, upper = joint_box([dict(lower=b["lower"], upper=b["upper"]) for i, b in enumerate(ch.bodies) if ch.dof[i] >= 0])
    if robot == "iiwa7_allegro":
        d = golden("fk_iiwa7_allegro_eeoff_nonrec.npz")
        links, offsets = [str(s) for s in d["links"]], d["offsets"].tolist()
        ref_q = [0.5 * (a + b) for a, b in zip(lower, upper)]
    else:
        links, offsets, ref_q = ch.config["ee_link_name"], ch.config["ee_link_offset"], list(ch.config["ref_q"])
    return ch, ch.descriptor(links, offsets), lower, upper, ref_q, links, offsets


def params(robot="allegro", rho=0.0, max_iters=MAX_ITERS, tol=TOL, **lm):
    _, _, lower, upper, ref_q, _, _ = hand(robot)
    return ik_params(lower, upper, ref_q, rho, max_iters, tol, **lm)


@functools.lru_cache(None)
def case_results():
    """3(a): the nine rows of results_{lego,realsense}.npz from ref_q with the stored wrist."""
    _, _, _, _, ref_q, _, _ = hand("allegro")
    target, palm = [], []
    for exp in ("lego", "realsense"):
        d = golden(f"results_{exp}.npz")
        target.append(d["contact"])
        palm.append(d["wrist"])
    target, palm = np.concatenate(target), np.concatenate(palm)
    q0 = np.tile(np.asarray(ref_q, np.float64), (len(target), 1))
    return dict(q0=q0, target=target, palm=palm)


@functools.lru_cache(None)
def case_inner(robot="allegro", rows=128, spread=0.3, seed=0):
    """3(b) / GPU 5: q* uniform in the inner 80 % of every joint range, targets FK_f32(q*) widened, start q* ± spread
    clamped to the limits."""
    from tests import _host
    _, desc, lower, upper, _, _, _ = hand(robot)
    lo, hi = np.asarray(lower), np.asarray(upper)
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    rng = np.random.default_rng(seed)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    qs = mid + 0.8 * half * (2.0 * rng.random((rows, len(lo))) - 1.0)
    q0 = np.clip(qs + spread * (2.0 * rng.random(qs.shape) - 1.0), lo, hi)
    target = _host.fk_forward(desc, qs)[0].astype(np.float64).reshape(rows, desc.n_tips, 3)
    return dict(q0=q0, target=target, palm=None, q_star=qs)


def check_converged(out, max_iters=MAX_ITERS, tol=TOL):
    """Every row: status 0, err ≤ tol, iters ≤ max_iters — no row may miss."""
    assert (out["status"] == 0).all(), np.flatnonzero(out["status"] != 0)
    assert (out["err"] <= tol).all(), float(out["err"].max())
    assert (out["iters"] <= max_iters).all() and (out["iters"] >= 0).all()


# ------------------------------------------------------------------ checks shared by the host and the device files
# solve(desc, params, q0, target, palm=None, palm_offset=None, w=None) → dict(q, err, iters, status);
# fk(desc, q32) → float32 positions [E, 3T];  sincos(angles) → (sin, cos) as the build under test takes them.
def recomputed_err(fk, sincos, desc, q, target, palm=None, palm_offset=None):
    E = len(q)
    pos = fk(desc, np.asarray(q).astype(np.float32)).reshape(E, desc.n_tips, 3)
    sc = None if palm is None else sincos(np.asarray(palm, np.float64)[:, 3:])
    return tip_errors(world_tips(pos, palm, palm_offset, sc), target)


def check_box(q, robot="allegro"):
    _, _, lower, upper, _, _, _ = hand(robot)
    q = np.asarray(q, np.float64)
    assert (q >= np.asarray(lower)).all() and (q <= np.asarray(upper)).all()


def check_err_bits(solve, fk, sincos):
    """err is, bit for bit, the distance recomputed from FK(q_out) widened and transformed in float64."""
    _, desc, *_ = hand()
    c = case_results()
    out = solve(desc, params(), c["q0"], c["target"], c["palm"])
    assert same_bits(out["err"], recomputed_err(fk, sincos, desc, out["q"], c["target"], c["palm"]))
    c = case_inner()
    po = [0.01, -0.02, 0.03]
    out = solve(desc, params(max_iters=3), c["q0"][:32], c["target"][:32] + np.asarray(po), palm_offset=po)
    assert same_bits(out["err"], recomputed_err(fk, sincos, desc, out["q"], c["target"][:32] + np.asarray(po), None, po))
    return out


def check_unreachable(solve, fk, sincos):
    """Targets 1 m out of reach: status 1, every output finite, q inside the box, final cost ≤ initial cost."""
    _, desc, lower, upper, *_ = hand()
    c = case_inner()
    q0, target = c["q0"][:16], c["target"][:16] + np.array([1.0, 0.0, 0.0])
    out = solve(desc, params(max_iters=12), q0, target)
    assert (out["status"] == 1).all() and (out["iters"] == 12).all()
    assert np.isfinite(out["q"]).all() and np.isfinite(out["err"]).all()
    check_box(out["q"])
    start = np.clip(q0.astype(np.float32), np.asarray(lower, np.float32), np.asarray(upper, np.float32))
    c0 = ik_cost(recomputed_err(fk, sincos, desc, start, target), start)
    c1 = ik_cost(out["err"], out["q"])
    assert (c1 <= c0).all()
    assert (c1 < c0).any()
    return out


def check_start_on_target(solve, fk):
    _, desc, *_ = hand()
    q0 = case_inner()["q_star"][:24]  # float64 values that are no float32
    assert not same_bits(q0, q0.astype(np.float32).astype(np.float64))
    target = fk(desc, q0.astype(np.float32)).astype(np.float64).reshape(len(q0), desc.n_tips, 3)
    out = solve(desc, params(), q0, target)
    assert (out["iters"] == 0).all() and (out["status"] == 0).all()
    assert same_bits(out["q"], q0.astype(np.float32).astype(np.float64))
    assert (out["err"] == 0).all()
    out32 = solve(desc, params(), q0.astype(np.float32), target)
    assert out32["q"].dtype == np.float32 and same_bits(out32["q"], q0.astype(np.float32))


def check_weight_zero(solve):
    """Weight 0 on one finger (ρ = 0): its four joints stay at the start bit for bit, and the other fingers' result
    does not depend on the dropped finger's target."""
    ch, desc, *_ = hand()
    c = case_inner()
    q0, target = c["q0"][:32], c["target"][:32].copy()
    finger = 1
    joints = np.flatnonzero(on_path(desc)[finger])
    assert len(joints) == 4
    w = np.ones((len(q0), 4))
    w[:, finger] = 0.0
    a = solve(desc, params(), q0, target, w=w)
    assert same_bits(a["q"][:, joints], q0.astype(np.float32).astype(np.float64)[:, joints])
    assert (a["status"] == 0).all()
    target2 = target.copy()
    target2[:, finger] += np.array([0.5, -1.0, 0.25])
    b = solve(desc, params(), q0, target2, w=w)
    others = [k for k in range(4) if k != finger]
    assert same_bits(a["q"], b["q"]) and same_bits(a["iters"], b["iters"]) and same_bits(a["status"], b["status"])
    assert same_bits(a["err"][:, others], b["err"][:, others])
    assert (a["err"][:, others] <= TOL).all()


def check_rest_pose(solve):
    """ρ > 0 with an unreachable target ends nearer ref_q than ρ = 0 does."""
    _, desc, _, _, ref_q, _, _ = hand()
    c = case_inner()
    q0, target = c["q0"][:16], c["target"][:16] + np.array([0.0, 0.0, 1.0])
    a = solve(desc, params(rho=0.0, max_iters=30), q0, target)
    b = solve(desc, params(rho=1.0, max_iters=30), q0, target)
    da = np.linalg.norm(a["q"] - np.asarray(ref_q), axis=1)
    db = np.linalg.norm(b["q"] - np.asarray(ref_q), axis=1)
    assert (db < da).all(), (da, db)
    check_box(b["q"])


def check_bad_rows(solve, group=16):
    """A non-finite q0, target, palm or w gives its row status 2, q = q0, err NaN; every other row is bit-identical
    to the run without bad rows.  Bad rows sit first, last and on both sides of a group boundary."""
    _, desc, *_ = hand()
    c = case_inner("allegro", 257, 0.3, 1)
    E = 2 * group + 5
    rng = np.random.default_rng(3)
    q0, target = c["q0"][:E].copy(), c["target"][:E].copy()
    palm = np.concatenate([0.02 * rng.standard_normal((E, 3)), 0.3 * rng.standard_normal((E, 3))], 1)
    w = 0.5 + rng.random((E, 4))
    par = params(max_iters=6)
    clean = solve(desc, par, q0, target, palm, None, w)
    bad = [0, group - 1, group, E - 1]
    q0b, tb, pb, wb = q0.copy(), target.copy(), palm.copy(), w.copy()
    q0b[0, 3] = np.nan
    tb[group - 1, 2, 1] = np.inf
    pb[group, 4] = np.nan
    wb[E - 1, 0] = -np.inf
    out = solve(desc, par, q0b, tb, pb, None, wb)
    good = np.setdiff1d(np.arange(E), bad)
    assert (out["status"][bad] == 2).all() and (out["iters"][bad] == 0).all()
    assert same_bits(out["q"][bad], q0b[bad])
    assert np.isnan(out["err"][bad]).all()
    for k in ("q", "err", "iters", "status"):
        assert same_bits(out[k][good], clean[k][good]), k
    assert (clean["status"] != 2).all()
