"""Test helpers of the rigid-body dynamics: a float64 numpy statement of the rule (csrc/cdx_dyn.h) from the two
descriptors' constants, ctypes wrappers of the host build's three entries, seeded inertials for the synthetic chains of
tests/_chains.py, and the shared cases.

The statement: Featherstone's recursive Newton–Euler algorithm in body coordinates (``inverse``), H by unit
accelerations (``inertia``), and ``solve(H, f − damping·q̇ − nle)`` (``forward``).  With ``exact=False`` the joint angles
are rounded to float32 and their sines / cosines are float32 (the rule's convention); with ``exact=True`` everything is
float64 and every fixed rotation F (a float32 matrix, orthogonal to 1e-7 only) is replaced by the nearest orthogonal
matrix — the form the physics checks of tests/test_dyn_cpu.py differentiate: a rigid-body identity holds to float64
accuracy only between rigid frames.

Tolerances against the reference (tests/golden/dyn_*.npz, float32).  The measure is tests/_chains.rel, per quantity
max|a − b| / max|b| over the batch.  ``ORACLE_ERR`` is the reference's own float32 error against this statement on the
stored inputs (B = 16), measured on the CPU (``measure_oracle`` recomputes it, test_dyn_cpu pins it); a kernel is held to
``TOL`` = 4 × that, the factor covering the reordering of float32 roundings as in _chains.py:

    quantity   allegro (measured)   leap (measured)      iiwa7_allegro (measured)
    tau        1.8e-7  (1.70e-7)    2.0e-7  (1.91e-7)    2.4e-7  (2.34e-7)
    H          1.1e-5  (1.09e-5)    2.9e-5  (2.86e-5)    2.3e-6  (2.21e-6)
    fd         1.0e-7  (9.57e-8)    5.5e-8  (5.42e-8)    1.7e-7  (1.61e-7)

(The reference's H is the difference of two float32 inverse-dynamics passes that both carry the gravity torque, a
thousand times the hands' inertia terms: its own error is the loosest of the three.  Its forward dynamics is the
articulated-body sweep, which never forms H, so iiwa7_allegro's cond(H) ≈ 2·10⁶ does not show in its figure; the rule here
solves H in float64, and the physics checks and the host-against-statement check carry that conditioning.)
"""
import ctypes as C
import functools
import math

import numpy as np

from compliancedex_amd._native import CdxChain, CdxDyn
from tests import _chains
from tests._helpers import golden
from tests._host import host, p

F32, F64 = 0, 1  # CDX_DTYPE_*
ROBOTS = ("allegro", "leap", "iiwa7_allegro")
SYNTH = ("line9", "tree8", "hand16")
GUARD = 3
G0 = (0.0, 0.0, -9.81)

ORACLE_ERR = dict(
    allegro=dict(tau=1.8e-7, H=1.1e-5, fd=1.0e-7),
    leap=dict(tau=2.0e-7, H=2.9e-5, fd=5.5e-8),
    iiwa7_allegro=dict(tau=2.4e-7, H=2.3e-6, fd=1.7e-7),
)
TOL = {r: {k: 4.0 * v for k, v in e.items()} for r, e in ORACLE_ERR.items()}
TOL_HOST = 1e-10  # inverse dynamics and H, host or device against the statement (fewer than 1e4 float64 roundings per
#                   output leave 1e-12; two decades of room for cancellation; a wrong term shows at 1e-3)


def tol_tips(desc):
    """Tip forces against tests/_ik.np_fk_jac (float64 trigonometry on the float32 F): per level of the deepest tip a
    float32 F that is orthogonal to 2⁻²³ only — the rule takes forces up with E where the Jacobian takes positions down
    with it — and two float32 roundings of the sine and cosine."""
    depth = max([_chains._depth([b.parent for b in desc.bodies], desc.tip_body[k]) for k in range(desc.n_tips)] + [1])
    return 4.0 * depth * 2.0 ** -23


def tol_forward(cond):
    """Forward dynamics per row against the statement: the n·ε·κ bound at n ≤ 32."""
    return 1e3 * 2.2e-16 * cond


# ------------------------------------------------------------------ chains
def with_inertials(bodies, seed):
    """The bodies of a synthetic chain with seeded inertials: mass 0.01 … 1, com within 0.05, a small SPD inertia,
    damping 0 … 0.1 and an effort limit on the moving joints."""
    rng = np.random.default_rng(seed)
    out = []
    for b in bodies:
        A = rng.standard_normal((3, 3))
        I = 1e-4 * (A @ A.T + 0.5 * np.eye(3))
        moving = b["joint"] != "fixed"
        out.append(dict(b, mass=float(rng.uniform(0.01, 1.0)), com=[float(v) for v in rng.uniform(-0.05, 0.05, 3)],
                        inertia=[float(I[0, 0]), float(I[0, 1]), float(I[0, 2]), float(I[1, 1]), float(I[1, 2]),
                                 float(I[2, 2])],
                        damping=float(rng.uniform(0.0, 0.1)) if moving else 0.0, effort=1.0 if moving else 0.0,
                        velocity=1.0 if moving else 0.0))
    return out


def widest_line():
    """The largest chain the descriptor holds: 32 bodies in a line (31 levels), x / y / z joints in turn, two fixed."""
    robot = _chains.line(31, fixed=(5, 20))
    axes = ([1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0])
    rng = np.random.default_rng(31)
    for i, b in enumerate(robot["bodies"][1:], 1):
        if b["joint"] != "fixed":
            b["axis"] = list(axes[i % 3])
        b["rpy"] = [float(v) for v in rng.uniform(-1.0, 1.0, 3)]
        b["xyz"] = [float(v) for v in rng.uniform(-0.03, 0.03, 3)]
    return robot


@functools.lru_cache(None)
def chain(name, live=False):
    """(Chain, tip links, tip offsets) of a packaged robot, a synthetic case of tests/_chains.py with seeded inertials,
    or "line31".  ``live``: the family's sign-0 joint gets a z axis (the forward dynamics refuses a dead joint)."""
    if name in ROBOTS:
        from tests import _ik
        ch, _, _, _, _, links, offsets = _ik.hand(name)
        return ch, list(links), [list(o) for o in offsets]
    if name == "line31":
        robot = widest_line()
        robot["bodies"] = with_inertials(robot["bodies"], 931)
        return _chains.chain_of(robot), ["b31", "b7"], [[0.01, -0.02, 0.03], [0.0, 0.02, 0.0]]
    b, links = _chains.bodies(name)
    b = with_inertials(b, 900 + _chains.CASES.index(name))
    if live:
        b = [dict(x, axis=[0.0, 0.0, 1.0]) if x["joint"] != "fixed" and x["axis"] == [0.0, 0.0, 0.0] else x for x in b]
    return _chains.chain_of(dict(name=name, bodies=b)), list(links), _chains.tip_offsets(name)


@functools.lru_cache(None)
def descriptors(name, live=False, tips=True):
    """(cdx_chain, cdx_dyn) of ``chain(name)``, with its tips (and offsets) or with none."""
    ch, links, offsets = chain(name, live)
    desc = ch.descriptor(links, offsets, check_depth=False) if tips else ch.descriptor([], None)
    return desc, ch.dynamics_descriptor()


@functools.lru_cache(None)
def rows(name, B=_chains.B_MAX, live=False):
    """Seeded inputs of a chain: q uniform in the joint box (±π where the box is empty), q̇, q̈, f ~ N(0, 1), a gravity
    per row, tip forces — all float64 values that are float32 too, so both I/O dtypes see the same numbers."""
    ch, links, _ = chain(name, live)
    lo = np.array([b["lower"] for i, b in enumerate(ch.bodies) if ch.dof[i] >= 0])
    hi = np.array([b["upper"] for i, b in enumerate(ch.bodies) if ch.dof[i] >= 0])
    lo, hi = np.where(hi > lo, lo, -math.pi), np.where(hi > lo, hi, math.pi)
    rng = np.random.default_rng(700 + sum(ord(ch_) for ch_ in name) + int(live))
    D = ch.n_dofs
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    out = dict(q=f32(lo + (hi - lo) * rng.random((B, D))), qd=f32(rng.standard_normal((B, D))),
               qdd=f32(rng.standard_normal((B, D))), f=f32(rng.standard_normal((B, D))),
               gravity=f32(9.81 * rng.standard_normal((B, 3)) / math.sqrt(3.0)),
               tipF=f32(rng.standard_normal((B, len(links), 3))))
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------ the float64 statement
def _cross(a, b):
    return np.cross(a, b)


def _mv(M, v):
    return np.einsum("bij,bj->bi", M, v)


def _mtv(M, v):
    return np.einsum("bji,bj->bi", M, v)


def _c_trig32(th32):
    """float32 cos / sin of a float32 array the way the builds take them: the C library's double functions, rounded."""
    flat = th32.reshape(-1)
    c = np.array([math.cos(float(v)) for v in flat]).astype(np.float32).astype(np.float64).reshape(th32.shape)
    s = np.array([math.sin(float(v)) for v in flat]).astype(np.float32).astype(np.float64).reshape(th32.shape)
    return c, s


def joint_poses(desc: CdxChain, q, exact=False):
    """E [n, B, 3, 3]: the joint poses F·A(axis, sign·q) of every body."""
    q = np.asarray(q, np.float64)
    B, n = q.shape[0], desc.n_bodies
    E = np.zeros((n, B, 3, 3))
    for i in range(n):
        b = desc.bodies[i]
        F = np.array(list(b.F), np.float64).reshape(3, 3)
        if exact:
            U, _, Vt = np.linalg.svd(F)
            F = U @ Vt
        if i > 0 and b.dof >= 0:
            if exact:
                th = float(b.sign) * q[:, b.dof]
                c, s = np.cos(th), np.sin(th)
            else:
                c, s = _c_trig32(np.float32(b.sign) * q[:, b.dof].astype(np.float32))
            A = np.zeros((B, 3, 3))
            u, v = [(1, 2), (2, 0), (0, 1)][b.axis]
            A[:, b.axis, b.axis] = 1.0
            A[:, u, u] = c
            A[:, v, v] = c
            A[:, u, v] = -s
            A[:, v, u] = s
            E[i] = F @ A
        else:
            E[i] = F
    return E


def _constants(desc, dyn: CdxDyn):
    n = desc.n_bodies
    m = np.array(list(dyn.mass))[:n]
    mc = np.array([list(r) for r in dyn.mcom])[:n]
    I6 = np.array([list(r) for r in dyn.inertia])[:n]
    I = np.stack([np.array([[x[0], x[1], x[2]], [x[1], x[3], x[4]], [x[2], x[4], x[5]]]) for x in I6])
    damping = np.array(list(dyn.damping))[:desc.n_dofs]
    return m, mc, I, damping


def world_poses(desc, E):
    """(R [n, B, 3, 3], t [n, B, 3]) of every body in the base frame."""
    n, B = E.shape[:2]
    R, t = np.zeros((n, B, 3, 3)), np.zeros((n, B, 3))
    R[0] = np.eye(3)
    for i in range(1, n):
        b = desc.bodies[i]
        R[i] = R[b.parent] @ E[i]
        t[i] = t[b.parent] + _mv(R[b.parent], np.broadcast_to(np.array(list(b.t), np.float64), (B, 3)))
    return R, t


def inverse(desc, dyn, q, qd=None, qdd=None, include_gravity=True, use_damping=True, gravity=None, tipF=None,
            exact=False, E=None):
    """tau [B, D] of the rule (see csrc/cdx_dyn.h), float64."""
    q = np.asarray(q, np.float64)
    B, n, D = q.shape[0], desc.n_bodies, desc.n_dofs
    qd = np.zeros((B, D)) if qd is None else np.asarray(qd, np.float64)
    qdd = np.zeros((B, D)) if qdd is None else np.asarray(qdd, np.float64)
    g = np.zeros((B, 3))
    if include_gravity:
        g = np.broadcast_to(np.asarray(G0 if gravity is None else gravity, np.float64), (B, 3))
    m, mc, I, damping = _constants(desc, dyn)
    E = joint_poses(desc, q, exact) if E is None else E
    w, v, al, a = (np.zeros((n, B, 3)) for _ in range(4))
    a[0] = -g
    S = np.zeros((n, 3))
    for i in range(1, n):
        b = desc.bodies[i]
        pr, pos = b.parent, np.array(list(b.t), np.float64)
        if b.dof >= 0:
            S[i, b.axis] = float(b.sign)
        wj = S[i] * qd[:, b.dof, None] if b.dof >= 0 else np.zeros((B, 3))
        zj = S[i] * qdd[:, b.dof, None] if b.dof >= 0 else np.zeros((B, 3))
        w[i] = _mtv(E[i], w[pr]) + wj
        v[i] = _mtv(E[i], v[pr] + _cross(w[pr], pos))
        al[i] = _mtv(E[i], al[pr]) + zj + _cross(w[i], wj)
        a[i] = _mtv(E[i], a[pr] + _cross(al[pr], pos)) + _cross(v[i], wj)
    nn, ff = np.zeros((n, B, 3)), np.zeros((n, B, 3))
    for i in range(1, n):
        na = al[i] @ I[i].T + _cross(mc[i], a[i])
        fa = m[i] * a[i] - _cross(mc[i], al[i])
        hn = w[i] @ I[i].T + _cross(mc[i], v[i])
        hf = m[i] * v[i] - _cross(mc[i], w[i])
        nn[i] = na + _cross(w[i], hn) + _cross(v[i], hf)
        ff[i] = fa + _cross(w[i], hf)
    if tipF is not None and desc.n_tips:
        R, _ = world_poses(desc, E)
        tipF = np.asarray(tipF, np.float64).reshape(B, desc.n_tips, 3)
        for k in range(desc.n_tips):
            body = desc.tip_body[k]
            if body <= 0:
                continue
            fl = _mtv(R[body], tipF[:, k])
            ff[body] -= fl
            if desc.has_offsets:
                nn[body] -= _cross(np.array(list(desc.tip_offset[k]), np.float64), fl)
    tau = np.zeros((B, D))
    for i in range(n - 1, 0, -1):
        b = desc.bodies[i]
        if b.dof >= 0:
            tau[:, b.dof] = float(b.sign) * nn[i][:, b.axis]
        if b.parent > 0:
            Ef = _mv(E[i], ff[i])
            nn[b.parent] += _mv(E[i], nn[i]) + _cross(np.array(list(b.t), np.float64), Ef)
            ff[b.parent] += Ef
    if use_damping:
        tau = tau + damping * qd
    return tau


def inertia(desc, dyn, q, exact=False):
    """H [B, D, D] by unit accelerations: column j = inverse(q, 0, e_j) without gravity and damping."""
    q = np.asarray(q, np.float64)
    B, D = q.shape[0], desc.n_dofs
    E = joint_poses(desc, q, exact)
    H = np.zeros((B, D, D))
    for j in range(D):
        e = np.zeros((B, D))
        e[:, j] = 1.0
        H[:, :, j] = inverse(desc, dyn, q, None, e, False, False, E=E)
    return H


def forward(desc, dyn, q, qd, f, include_gravity=True, use_damping=False, gravity=None, exact=False):
    """(qdd [B, D], cond(H) [B]) = solve(H, f − damping·q̇ − nle)."""
    qd = np.asarray(qd, np.float64)
    nle = inverse(desc, dyn, q, qd, None, include_gravity, False, gravity, exact=exact)
    H = inertia(desc, dyn, q, exact)
    rhs = np.asarray(f, np.float64) - nle
    if use_damping:
        rhs = rhs - _constants(desc, dyn)[3] * qd
    return np.linalg.solve(H, rhs[:, :, None])[:, :, 0], np.linalg.cond(H)


def potential_energy(desc, dyn, q, gravity=G0):
    """−Σ_i m_i·gᵀ·p_com,i [B] from the statement's own FK, float64 trigonometry."""
    m, mc, _, _ = _constants(desc, dyn)
    R, t = world_poses(desc, joint_poses(desc, q, exact=True))
    g = np.asarray(gravity, np.float64)
    U = np.zeros(len(q))
    for i in range(desc.n_bodies):
        U -= (m[i] * t[i] + _mv(R[i], np.broadcast_to(mc[i], t[i].shape))) @ g
    return U


# ------------------------------------------------------------------ host build
def _io(a, dtype):
    return None if a is None else np.ascontiguousarray(a, np.float64 if dtype == F64 else np.float32)


def _guarded(B, shape, dtype):
    """An output of B rows with GUARD more rows behind it, all 7."""
    return np.full((B + GUARD,) + shape, 7.0, np.float64 if dtype == F64 else np.float32)


def inverse_host(desc, dyn, q, qd=None, qdd=None, dtype=F64, include_gravity=True, use_damping=True, gravity=None,
                 tipF=None, expect=0):
    B = len(q)
    q, qd, qdd = _io(q, dtype), _io(qd, dtype), _io(qdd, dtype)
    g = None if gravity is None else np.ascontiguousarray(gravity, np.float64)
    tf = None if tipF is None else np.ascontiguousarray(tipF, np.float64)
    tau = _guarded(B, (desc.n_dofs,), dtype)
    rc = host().cdxh_dyn_inverse(C.byref(desc), C.byref(dyn), B, p(q), p(qd), p(qdd), dtype, int(include_gravity),
                                 int(use_damping), p(g), int(g is not None and g.ndim == 2), p(tf), p(tau))
    assert rc == expect, rc
    assert (tau[B:] == 7.0).all()
    return tau[:B]


def inertia_host(desc, dyn, q, dtype=F64):
    B, D = len(q), desc.n_dofs
    q = _io(q, dtype)
    H = _guarded(B, (D, D), dtype)
    rc = host().cdxh_dyn_inertia(C.byref(desc), C.byref(dyn), B, p(q), dtype, p(H))
    assert rc == 0, rc
    assert (H[B:] == 7.0).all()
    return H[:B]


def forward_host(desc, dyn, q, qd, f, dtype=F64, include_gravity=True, use_damping=False, gravity=None, expect=0):
    B = len(q)
    q, qd, f = _io(q, dtype), _io(qd, dtype), _io(f, dtype)
    g = None if gravity is None else np.ascontiguousarray(gravity, np.float64)
    qdd = _guarded(B, (desc.n_dofs,), dtype)
    rc = host().cdxh_dyn_forward(C.byref(desc), C.byref(dyn), B, p(q), p(qd), p(f), dtype, int(include_gravity),
                                 int(use_damping), p(g), int(g is not None and g.ndim == 2), p(qdd))
    assert rc == expect, rc
    assert (qdd[B:] == 7.0).all()
    return qdd[:B]


# ------------------------------------------------------------------ the reference's figures
def rel(a, b):
    return _chains.rel(a, b)


def against_golden(robot, inverse_fn, inertia_fn, forward_fn):
    """→ dict(tau, H, fd): the three entries (signatures of the statement's, float32 I/O allowed) against the
    reference's stored results, each the worst of its variants."""
    d = golden(f"dyn_{robot}.npz")
    desc, dyn = descriptors(robot)
    e = dict(tau=0.0, H=0.0, fd=0.0)
    for g in (0, 1):
        for dm in (0, 1):
            tau = inverse_fn(desc, dyn, d["q"], d["qd"], d["qdd"], include_gravity=bool(g), use_damping=bool(dm))
            e["tau"] = max(e["tau"], rel(tau, d[f"tau_g{g}_d{dm}"]))
    e["H"] = rel(inertia_fn(desc, dyn, d["q"]), d["H"])
    for dm in (0, 1):
        qdd = forward_fn(desc, dyn, d["q"], d["qd"], d["f"], include_gravity=True, use_damping=bool(dm))
        e["fd"] = max(e["fd"], rel(qdd, d[f"fd_d{dm}"]))
    return e


def measure_oracle(robot):
    """The reference (float32, as stored) against the statement on the stored inputs."""
    return against_golden(robot, inverse, inertia, lambda *a, **k: forward(*a, **k)[0])
