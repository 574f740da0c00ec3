"""Test helpers of the free-wrist IK solve (ik_pose_row in csrc/cdx_ik.h): a ctypes wrapper of the host build's entry, a
numpy statement of one step of the rule, the two input families and the checks shared by the host file
(tests/test_ik_pose_cpu.py) and the device file (tests/test_gpu_ik_pose.py).

solve(desc, params, q0, target, pos0=None, rot0=None, palm_offset=None, w=None)
    → dict(q, palm_pos [E, 3], palm_rot [E, 3, 3], err, iters, status);   fk(desc, q32) → float32 positions [E, 3T].

The families' spreads were fixed on the host build (see pose_inner): every row converges in at most half of MAX_ITERS.
"""
import ctypes as C
import functools

import numpy as np

from tests import _host, _ik
from tests._helpers import rel_err
from tests._host import host, p
from tests._ik import F32, F64, same_bits

TOL = 1e-5
MAX_ITERS = 100  # solve_ik_pose's default
OUTS = ("q", "palm_pos", "palm_rot", "err", "iters", "status")


def params(robot="allegro", rho=0.0, max_iters=MAX_ITERS, tol=TOL, **lm):
    return _ik.params(robot, rho, max_iters, tol, **lm)


# ------------------------------------------------------------------ host build
def ik_pose_host(desc, par, q0, target, pos0=None, rot0=None, palm_offset=None, w=None):
    q0 = np.ascontiguousarray(q0)
    assert q0.dtype in (np.float32, np.float64)
    E, T = q0.shape[0], desc.n_tips
    target = np.ascontiguousarray(target, np.float64).reshape(E, T, 3)
    pos0 = None if pos0 is None else np.ascontiguousarray(pos0, np.float64).reshape(E, 3)
    rot0 = None if rot0 is None else np.ascontiguousarray(rot0, np.float64).reshape(E, 3, 3)
    w = None if w is None else np.ascontiguousarray(w, np.float64).reshape(E, T)
    po = None if palm_offset is None else (C.c_double * 3)(*[float(v) for v in palm_offset])
    out = dict(q=np.full_like(q0, 7.0), palm_pos=np.full((E, 3), 7.0), palm_rot=np.full((E, 3, 3), 7.0),
               err=np.full((E, T), 7.0), iters=np.full(E, -7, np.int32), status=np.full(E, -7, np.int32))
    rc = host().cdxh_ik_solve_pose(C.byref(desc), C.byref(par), E, p(q0), F64 if q0.dtype == np.float64 else F32,
                                   p(target), p(pos0), p(rot0), po, p(w), *[p(out[k]) for k in OUTS])
    assert rc == 0, rc
    return out


def host_fk(desc, q32):
    return _host.fk_forward(desc, q32)[0]


# ------------------------------------------------------------------ numpy statement
def euler_rot(ang):
    """(Rx(a)·Ry(b))·Rz(c) [N, 3, 3] of XYZ angles [N, 3] (numpy's sin / cos: these build inputs, not expectations)."""
    ang = np.asarray(ang, np.float64)
    return _ik.palm_rotation(np.sin(ang), np.cos(ang))


def axis_angle_rot(axis, angle):
    """Rodrigues: I + sin θ·[k]× + (1 − cos θ)·[k]ײ [N, 3, 3] for unit axes [N, 3]."""
    k = axis / np.linalg.norm(axis, axis=1, keepdims=True)
    K = np.zeros((len(k), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    s, c = np.sin(angle)[:, None, None], np.cos(angle)[:, None, None]
    return np.eye(3) + s * K + (1.0 - c) * (K @ K)


def rule_tips(pos32, rot, pos, palm_offset=None):
    """The rule's fingertips (Rp·double(FK_f32) + pp) + palm_offset, products summed left to right."""
    v = np.asarray(pos32, np.float32).astype(np.float64).reshape(len(rot), -1, 3)
    R, pp = np.asarray(rot, np.float64).reshape(-1, 3, 3), np.asarray(pos, np.float64)
    po = np.zeros(3) if palm_offset is None else np.asarray(palm_offset, np.float64)
    out = np.empty_like(v)
    for i in range(3):
        x = (R[:, None, i, 0] * v[:, :, 0] + R[:, None, i, 1] * v[:, :, 1]) + R[:, None, i, 2] * v[:, :, 2]
        out[:, :, i] = (x + pp[:, None, i]) + po[i]
    return out


def recomputed_err(fk, desc, out, target, palm_offset=None):
    pos = fk(desc, np.asarray(out["q"]).astype(np.float32))
    return _ik.tip_errors(rule_tips(pos, out["palm_rot"], out["palm_pos"], palm_offset), target)


def cayley(om):
    """C = ((1 − a·a)·I + 2·a·aᵀ + 2·[a]×)/(1 + a·a), a = ½·ω [N, 3]."""
    a = 0.5 * np.asarray(om, np.float64)
    s = (a * a).sum(1)[:, None, None]
    A = np.zeros((len(a), 3, 3))
    A[:, 0, 1], A[:, 0, 2], A[:, 1, 0] = -a[:, 2], a[:, 1], a[:, 2]
    A[:, 1, 2], A[:, 2, 0], A[:, 2, 1] = -a[:, 0], -a[:, 1], a[:, 0]
    return ((1.0 - s) * np.eye(3) + 2.0 * a[:, :, None] * a[:, None, :] + 2.0 * A) / (1.0 + s)


def np_pose_step(desc, q0, target, pos0, rot0, lower, upper, mu=1e-3):
    """One iteration of the rule (unit weights, ρ = 0, no palm_offset) in float64 numpy, dense: the joint columns from
    _ik.np_fk_jac at float32(q), the pose columns I₃ and −[v]×, the residual in the palm frame, joints on a bound with
    the gradient pointing out fixed, δ = (JᵀJ + κI)⁻¹·g, the trial point by clamp / Rp·t_b / Rp·Cayley(ω_b), kept if its
    cost is lower.  → (q, palm_pos, palm_rot)."""
    lo, hi = np.asarray(lower, np.float32).astype(np.float64), np.asarray(upper, np.float32).astype(np.float64)
    q = np.clip(np.asarray(q0).astype(np.float32).astype(np.float64), lo, hi)
    E, T, D = len(q), desc.n_tips, desc.n_dofs
    target = np.asarray(target, np.float64).reshape(E, T, 3)

    def cost(qq, R, pp):
        v = _ik.np_fk_jac(desc, qq)[0]
        d = target - (np.einsum("eij,etj->eti", R, v) + pp[:, None])
        return 0.5 * (d * d).sum((1, 2)), d, v
    c0, d, v = cost(q, rot0, pos0)
    J = np.zeros((E, T, 3, D + 6))
    J[..., :D] = _ik.np_fk_jac(desc, q)[1]
    J[..., D:D + 3] = np.eye(3)
    J[:, :, 0, D + 4], J[:, :, 0, D + 5] = v[:, :, 2], -v[:, :, 1]
    J[:, :, 1, D + 3], J[:, :, 1, D + 5] = -v[:, :, 2], v[:, :, 0]
    J[:, :, 2, D + 3], J[:, :, 2, D + 4] = v[:, :, 1], -v[:, :, 0]
    J = J.reshape(E, 3 * T, D + 6)
    u = np.einsum("eji,etj->eti", rot0, d).reshape(E, 3 * T)
    g = np.einsum("erd,er->ed", J, u)
    fixed = np.zeros((E, D + 6), bool)
    fixed[:, :D] = ((q <= lo) & (g[:, :D] < 0)) | ((q >= hi) & (g[:, :D] > 0))
    g[fixed] = 0.0
    J = J * ~fixed[:, None, :]
    step = np.linalg.solve(np.einsum("erd,erf->edf", J, J) + mu * np.eye(D + 6), g[:, :, None])[:, :, 0]
    qn = np.clip(q + step[:, :D], lo, hi).astype(np.float32).astype(np.float64)
    pn = pos0 + np.einsum("eij,ej->ei", rot0, step[:, D:D + 3])
    Rn = rot0 @ cayley(step[:, D + 3:])
    ok = cost(qn, Rn, pn)[0] < c0
    return (np.where(ok[:, None], qn, q), np.where(ok[:, None], pn, pos0), np.where(ok[:, None, None], Rn, rot0))


# ------------------------------------------------------------------ families
@functools.lru_cache(None)
def pose_inner(robot="allegro", rows=128, seed=0, dq=0.3, dpos=0.05, drot=0.3):
    """q* uniform in the inner 80 % of the joint box, palm* position uniform in a ±0.2 m box, palm* rotation from XYZ
    angles with |b| ≤ 1.2 (a, c in ±π), targets the rule's tips of (q*, palm*); the start q0 = q* ± dq rad clamped, the
    start pose palm* displaced by ≤ dpos m per axis and rotated by ≤ drot rad about a random axis.  The issue's proposed
    spreads (0.3 rad, 0.05 m, 0.3 rad) hold on the host build: every row of the families the tests use converges in at
    most MAX_ITERS / 2 iterations, with and without the start pose (test_ik_pose_cpu.py asserts it)."""
    _, desc, lower, upper, *_ = _ik.hand(robot)
    lo, hi = np.asarray(lower), np.asarray(upper)
    rng = np.random.default_rng(seed)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    qs = mid + 0.8 * half * (2.0 * rng.random((rows, len(lo))) - 1.0)
    q0 = np.clip(qs + dq * (2.0 * rng.random(qs.shape) - 1.0), lo, hi)
    pos = 0.2 * (2.0 * rng.random((rows, 3)) - 1.0)
    ang = (2.0 * rng.random((rows, 3)) - 1.0) * np.array([np.pi, 1.2, np.pi])
    rot = euler_rot(ang)
    target = rule_tips(host_fk(desc, qs.astype(np.float32)), rot, pos)
    pos0 = pos + dpos * (2.0 * rng.random((rows, 3)) - 1.0)
    rot0 = rot @ axis_angle_rot(rng.standard_normal((rows, 3)), drot * (2.0 * rng.random(rows) - 1.0))
    return dict(q_star=qs, q0=q0, target=target, pos_star=pos, rot_star=rot, pos0=pos0, rot0=rot0)


def pose_rigid(robot="allegro", rows=128, seed=0):
    """pose_inner with q0 = float32(q*) exactly and no start pose: the Kabsch start alone is the solution."""
    c = dict(pose_inner(robot, rows, seed))
    c["q0"] = c["q_star"].astype(np.float32)
    c["pos0"] = c["rot0"] = None
    return c


# ------------------------------------------------------------------ checks
def check_rotation(out):
    """(e) every row that has a pose: max|R·Rᵀ − I| ≤ 1e-12 and det > 0."""
    R = out["palm_rot"][out["status"] != 2]
    assert np.isfinite(R).all()
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(initial=0.0) <= 1e-12
    assert (np.linalg.det(R) > 0).all()


def check_converged(out, robot="allegro", w=None, max_iters=MAX_ITERS):
    assert (out["status"] == 0).all(), np.flatnonzero(out["status"] != 0)
    werr = out["err"] if w is None else out["err"] * w
    assert (werr <= TOL).all(), float(werr.max())
    assert (out["iters"] <= max_iters).all() and (out["iters"] >= 0).all()
    _ik.check_box(out["q"], robot)
    check_rotation(out)


def check_start_on_solution(solve):
    """(a) q0 = q* and the start pose = pose*: status 0, 0 iterations, the pose is the input bit for bit."""
    _, desc, *_ = _ik.hand()
    c = pose_inner()
    out = solve(desc, params(), c["q_star"], c["target"], c["pos_star"], c["rot_star"])
    assert (out["status"] == 0).all() and (out["iters"] == 0).all()
    assert same_bits(out["palm_pos"], c["pos_star"]) and same_bits(out["palm_rot"], c["rot_star"])
    assert same_bits(out["q"], c["q_star"].astype(np.float32).astype(np.float64))
    check_rotation(out)


def check_kabsch_start(solve):
    """(b) on pose_rigid the Kabsch fit is the answer: status 0 with 0 iterations everywhere (a transposed or reflected
    fit misses by centimetres), also with one finger's weight 0; a row with two positive weights takes the fallback."""
    _, desc, *_ = _ik.hand()
    c = pose_rigid()
    out = solve(desc, params(), c["q0"], c["target"])
    assert (out["status"] == 0).all() and (out["iters"] == 0).all(), (out["status"], out["iters"])
    # (the fit is palm* itself up to the FK under test: the targets hold the host build's float32 FK, the device's may
    # differ in the last bits, ~1e-8 m over fingertips ≥ 3 cm apart and ≤ 0.4 m from the origin)
    assert np.abs(out["palm_rot"] - c["rot_star"]).max() < 1e-5 and np.abs(out["palm_pos"] - c["pos_star"]).max() < 1e-5
    check_rotation(out)
    E = len(c["q0"])
    w = np.ones((E, 4))
    w[5, 2] = 0.0
    w[9, 0] = w[9, 3] = 0.0
    target = c["target"].copy()
    target[5, 2] += 0.5  # (the dropped finger's target is nowhere near)
    out = solve(desc, params(), c["q0"], target, w=w)
    three = np.arange(E) != 9
    assert (out["status"][three] == 0).all() and (out["iters"][three] == 0).all()
    assert out["status"][9] in (0, 1)
    for k in OUTS:
        assert np.isfinite(out[k][9]).all(), k
    check_rotation(out)
    return out


def check_convergence(solve, half=False):
    """(c) pose_inner with the given start and with the Kabsch start: every row converges.  ``half``: in at most half
    of MAX_ITERS (the host build's own requirement of the families)."""
    _, desc, *_ = _ik.hand()
    c = pose_inner()
    outs = [solve(desc, params(), c["q0"], c["target"], c["pos0"], c["rot0"]), solve(desc, params(), c["q0"], c["target"])]
    for out in outs:
        check_converged(out, max_iters=MAX_ITERS // 2 if half else MAX_ITERS)
    return outs


def check_err_bits(solve, fk):
    """(d) err is the distance recomputed from the outputs, bit for bit — converged rows, rows cut at 3 iterations,
    with a palm_offset and weights."""
    _, desc, *_ = _ik.hand()
    c = pose_inner()
    out = solve(desc, params(), c["q0"], c["target"], c["pos0"], c["rot0"])
    assert same_bits(out["err"], recomputed_err(fk, desc, out, c["target"]))
    po = [0.01, -0.02, 0.03]
    w = 0.5 + np.random.default_rng(5).random((32, 4))
    out = solve(desc, params(max_iters=3), c["q0"][:32], c["target"][:32], None, None, po, w)
    assert same_bits(out["err"], recomputed_err(fk, desc, out, c["target"][:32], po))
    assert (out["status"] == 1).any()
    check_rotation(out)


def pair_reach(desc):
    """[T, T] upper bounds of the distance between two fingertips over ALL joint angles: tip k stays within r_k of the
    origin b_k of its first moving joint (r_k: the lengths of the links after it, plus the tip offset), b_k is fixed in
    the palm frame, so |tip_i − tip_j| ≤ |b_i − b_j| + r_i + r_j whatever the rigid pose."""
    base, reach = [], []
    for k, path in _ik._paths(desc):
        R, t, r, moving = np.eye(3), np.zeros(3), 0.0, False
        for bi in path:
            b = desc.bodies[bi]
            bt = np.array(list(b.t), np.float64)
            if moving:
                r += np.linalg.norm(bt)
                continue
            t = t + R @ bt
            R = R @ np.array(list(b.F), np.float64).reshape(3, 3)
            moving = b.dof >= 0
        assert moving
        if desc.has_offsets:
            r += np.linalg.norm(np.array(list(desc.tip_offset[k]), np.float64))
        base.append(t)
        reach.append(r)
    base, reach = np.array(base), np.array(reach)
    return np.linalg.norm(base[:, None] - base[None], axis=2) + reach[:, None] + reach[None]


def check_unreachable(solve, fk):
    """(g) targets scaled by 3 about their centroid: status 1, every output finite, q in the box, cost not risen.
    The scaling alone does not put every row out of reach — two of pose_inner's 128 rows have fingertips so close
    together that the hand does reach their threefold spread (the host build converges there to 2e-6 m) — so the rows
    taken are the first 32 with a certificate: a pair of scaled targets farther apart than pair_reach allows."""
    _, desc, lower, upper, *_ = _ik.hand()
    c = pose_inner()
    t = c["target"]
    cen = t.mean(1, keepdims=True)
    scaled = cen + 3.0 * (t - cen)
    gap = np.linalg.norm(scaled[:, :, None] - scaled[:, None], axis=3) - pair_reach(desc)
    rows = np.flatnonzero(gap.max((1, 2)) > 1e-3)[:32]
    n = len(rows)
    assert n == 32
    q0, target, pos0, rot0 = c["q0"][rows], scaled[rows], c["pos0"][rows], c["rot0"][rows]
    out = solve(desc, params(), q0, target, pos0, rot0)
    assert (out["status"] == 1).all() and (out["iters"] == MAX_ITERS).all()
    for k in OUTS:
        assert np.isfinite(out[k]).all(), k
    _ik.check_box(out["q"])
    check_rotation(out)
    start = dict(q=np.clip(q0.astype(np.float32), np.asarray(lower, np.float32), np.asarray(upper, np.float32)),
                 palm_pos=pos0, palm_rot=rot0)
    c0 = _ik.ik_cost(recomputed_err(fk, desc, start, target), start["q"])
    c1 = _ik.ik_cost(out["err"], out["q"])
    assert (c1 <= c0).all() and (c1 < c0).any()


def check_bad_rows(solve, group):
    """(h) a non-finite q0, target, w, palm0_pos or palm0_rot: status 2, q = q0, NaN pose and err, 0 iterations; every
    other row bit-identical to the run without bad rows.  Bad rows first, last, on both sides of a ``group`` boundary
    and of a wave boundary."""
    _, desc, *_ = _ik.hand()
    c = pose_inner("allegro", 257, 1)
    E = max(2 * group, 64) + 5
    rng = np.random.default_rng(3)
    q0, target, pos0, rot0 = (c[k][:E].copy() for k in ("q0", "target", "pos0", "rot0"))
    w = 0.5 + rng.random((E, 4))
    par = params(max_iters=6)
    clean = solve(desc, par, q0, target, pos0, rot0, None, w)
    assert (clean["status"] != 2).all()
    bad = sorted({0, group - 1, group, 63, 64, E - 1})
    b = [a.copy() for a in (q0, target, w, pos0, rot0)]
    spots = [(0, (3,)), (1, (2, 1)), (2, (0,)), (3, (1,)), (4, (2, 0))]
    vals = [np.nan, np.inf, -np.inf]
    for i, row in enumerate(bad):
        which, at = spots[i % len(spots)]
        b[which][(row,) + at] = vals[i % len(vals)]
    out = solve(desc, par, b[0], b[1], b[3], b[4], None, b[2])
    good = np.setdiff1d(np.arange(E), bad)
    assert (out["status"][bad] == 2).all() and (out["iters"][bad] == 0).all()
    assert same_bits(out["q"][bad], b[0][bad])
    for k in ("palm_pos", "palm_rot", "err"):
        assert np.isnan(out[k][bad]).all(), k
    for k in OUTS:
        assert same_bits(out[k][good], clean[k][good]), k
    check_rotation(out)


def check_iiwa7(solve, half=False):
    """(j) D = 23, D′ = 29: 64 rows with a start pose, q* ± 0.2 rad (the fixed-palm test's arm spread), the pose spreads
    of pose_inner."""
    _, desc, *_ = _ik.hand("iiwa7_allegro")
    assert desc.n_dofs == 23
    c = pose_inner("iiwa7_allegro", 64, 0, 0.2)
    par = params("iiwa7_allegro")
    out = solve(desc, par, c["q0"], c["target"], c["pos0"], c["rot0"])
    check_converged(out, "iiwa7_allegro", max_iters=MAX_ITERS // 2 if half else MAX_ITERS)
    return out


def one_iteration_case():
    _, desc, lower, upper, *_ = _ik.hand()
    c = pose_inner()
    return desc, c, lower, upper


def check_one_iteration(out, ref):
    """(f) q, palm_pos, palm_rot after max_iters = 1 against ``ref`` (the numpy statement or the host build)."""
    assert (out["iters"] == 1).all()
    for k, r in zip(("q", "palm_pos", "palm_rot"), ref):
        assert rel_err(out[k], r) < 2e-5, k
    check_rotation(out)
