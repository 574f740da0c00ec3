"""Rigid-body dynamics on an MI355X (cdx_dyn_inverse, cdx_dyn_inertia, cdx_dyn_forward): every entry against the host
build bit for bit and against the float64 statement and the reference's stored results (tests/_dyn.py), the
independence of rows and of the launch shape, the argument checks, and the Python layer on top
(DifferentiableRobotModel's dynamics methods, holding_torques, impedance_torques)."""
import functools

import numpy as np
import pytest
import torch

from tests import _chains, _dyn, _ik
from tests._helpers import golden, product_chain
from tests._ik import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = _dyn.GUARD
ALL = _dyn.ROBOTS + _dyn.SYNTH + ("line31",)
BATCHES = _chains.BATCHES  # 1, 63, 65, 257
B_MAX = _chains.B_MAX


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)  # (a writable copy)


def _np_dtype(dtype):
    return np.float64 if dtype == _dyn.F64 else np.float32


@functools.lru_cache(None)
def _dyn_dev(name, live=False):
    """The cdx_dyn of a chain in device memory (the entries read it there)."""
    _, dyn = _dyn.descriptors(name, live)
    return torch.frombuffer(bytearray(bytes(dyn)), dtype=torch.uint8).to(DEV)


def _out(B, shape, dtype):
    return torch.full((B + GUARD,) + shape, 7.0, dtype=torch.float64 if dtype == _dyn.F64 else torch.float32, device=DEV)


def _take(t, B):
    a = t.cpu().numpy()
    assert (a[B:] == 7.0).all()  # the GUARD rows past the output are untouched
    return a[:B]


def inverse_dev(name, desc, q, qd=None, qdd=None, dtype=_dyn.F64, include_gravity=True, use_damping=True, gravity=None,
                tipF=None, live=False):
    from compliancedex_amd import _native as N
    B, nd = len(q), _np_dtype(dtype)
    tq, tqd, tqdd = _dev(q, nd), _dev(qd, nd), _dev(qdd, nd)
    g, tf = _dev(gravity, np.float64), _dev(tipF, np.float64)
    tau = _out(B, (desc.n_dofs,), dtype)
    N.check(N.load().cdx_dyn_inverse(desc, N.ptr(_dyn_dev(name, live)), B, N.ptr(tq), N.ptr(tqd), N.ptr(tqdd), dtype,
                                     int(include_gravity), int(use_damping), N.ptr(g),
                                     int(g is not None and g.ndim == 2), N.ptr(tf), N.ptr(tau), N.stream_ptr()),
            "cdx_dyn_inverse")
    return _take(tau, B)


def inertia_dev(name, desc, q, dtype=_dyn.F64, live=False):
    from compliancedex_amd import _native as N
    B, D = len(q), desc.n_dofs
    tq = _dev(q, _np_dtype(dtype))
    H = _out(B, (D, D), dtype)
    N.check(N.load().cdx_dyn_inertia(desc, N.ptr(_dyn_dev(name, live)), B, N.ptr(tq), dtype, N.ptr(H), N.stream_ptr()),
            "cdx_dyn_inertia")
    return _take(H, B)


def forward_dev(name, desc, q, qd, f, dtype=_dyn.F64, include_gravity=True, use_damping=False, gravity=None, live=False):
    from compliancedex_amd import _native as N
    B, nd = len(q), _np_dtype(dtype)
    tq, tqd, tf = _dev(q, nd), _dev(qd, nd), _dev(f, nd)
    g = _dev(gravity, np.float64)
    keep = tf.clone()
    qdd = _out(B, (desc.n_dofs,), dtype)
    N.check(N.load().cdx_dyn_forward(desc, N.ptr(_dyn_dev(name, live)), B, N.ptr(tq), N.ptr(tqd), N.ptr(tf), dtype,
                                     int(include_gravity), int(use_damping), N.ptr(g),
                                     int(g is not None and g.ndim == 2), N.ptr(qdd), N.stream_ptr()), "cdx_dyn_forward")
    assert torch.equal(tf, keep)  # the caller's f is not written
    return _take(qdd, B)


@functools.lru_cache(None)
def _host(name):
    """The host build's answers at the chain's 257 rows, computed once and shared (read-only)."""
    desc, dyn = _dyn.descriptors(name)
    x = _dyn.rows(name)
    out = dict(tau=_dyn.inverse_host(desc, dyn, x["q"], x["qd"], x["qdd"], gravity=x["gravity"], tipF=x["tipF"]),
               H=_dyn.inertia_host(desc, dyn, x["q"]))
    live = name in _dyn.SYNTH
    ldesc, ldyn = _dyn.descriptors(name, live)
    lx = _dyn.rows(name, B_MAX, live)
    out["fd"] = _dyn.forward_host(ldesc, ldyn, lx["q"], lx["qd"], lx["f"], use_damping=True, gravity=lx["gravity"])
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------ 1. the host build, bit for bit; rows and shapes
@pytest.mark.parametrize("name", ALL)
def test_entries_equal_the_host_build(name):
    """float64 I/O at every batch shape: row r of any batch has the bits of row r of the host build (so a row's bits do
    not depend on the batch it sits in); float32 I/O is the same result rounded once."""
    desc, _ = _dyn.descriptors(name)
    x, ref = _dyn.rows(name), _host(name)
    live = name in _dyn.SYNTH
    ldesc, _ = _dyn.descriptors(name, live)
    lx = _dyn.rows(name, B_MAX, live)
    for B in BATCHES:
        tau = inverse_dev(name, desc, x["q"][:B], x["qd"][:B], x["qdd"][:B], gravity=x["gravity"][:B], tipF=x["tipF"][:B])
        assert same_bits(tau, ref["tau"][:B]), (B, "tau")
        H = inertia_dev(name, desc, x["q"][:B])
        assert same_bits(H, ref["H"][:B]), (B, "H")
        assert same_bits(H, np.ascontiguousarray(H.transpose(0, 2, 1)))
        fd = forward_dev(name, ldesc, lx["q"][:B], lx["qd"][:B], lx["f"][:B], use_damping=True, gravity=lx["gravity"][:B],
                         live=live)
        assert same_bits(fd, ref["fd"][:B]), (B, "fd")
    # rows of the B = 257 run again alone (B = 1) and as a block of 63 that starts inside a workgroup
    for rows_ in ([15], [16], [64], [256], list(range(100, 163))):
        r = np.asarray(rows_)
        tau = inverse_dev(name, desc, x["q"][r], x["qd"][r], x["qdd"][r], gravity=x["gravity"][r], tipF=x["tipF"][r])
        assert same_bits(tau, ref["tau"][r]) and same_bits(inertia_dev(name, desc, x["q"][r]), ref["H"][r])
        fd = forward_dev(name, ldesc, lx["q"][r], lx["qd"][r], lx["f"][r], use_damping=True, gravity=lx["gravity"][r],
                         live=live)
        assert same_bits(fd, ref["fd"][r]), rows_
    B = 65
    tau = inverse_dev(name, desc, x["q"][:B], x["qd"][:B], x["qdd"][:B], dtype=_dyn.F32, gravity=x["gravity"][:B],
                      tipF=x["tipF"][:B])
    assert tau.dtype == np.float32 and same_bits(tau, ref["tau"][:B].astype(np.float32))
    assert same_bits(inertia_dev(name, desc, x["q"][:B], dtype=_dyn.F32), ref["H"][:B].astype(np.float32))
    fd = forward_dev(name, ldesc, lx["q"][:B], lx["qd"][:B], lx["f"][:B], dtype=_dyn.F32, use_damping=True,
                     gravity=lx["gravity"][:B], live=live)
    assert same_bits(fd, ref["fd"][:B].astype(np.float32))


def test_rows_per_block_follow_the_lds_a_row_needs():
    from compliancedex_amd import _native as N
    lib = N.load()
    for name in ALL:
        desc, _ = _dyn.descriptors(name)
        n, D = desc.n_bodies, desc.n_dofs
        for entry in (0, 1, 2):
            row = 8 * (12 * n + (D * (D + 1) // 2 + D if entry == 2 else 0)) + 4 * 2 * n
            lanes = 64
            while lanes > 1 and row * lanes > 40960:
                lanes //= 2
            assert lib.cdx_dyn_rows_per_block(n, D, entry) == lanes
            assert lanes < 65 <= B_MAX  # (BATCHES straddle a workgroup and a wave of every entry)
    assert lib.cdx_dyn_rows_per_block(33, 4, 0) == 0 and lib.cdx_dyn_rows_per_block(4, 4, 3) == 0


@pytest.mark.parametrize("name", ("allegro", "tree8"))
def test_a_nan_row_stays_in_its_row(name):
    live = name in _dyn.SYNTH
    desc, _ = _dyn.descriptors(name, live)
    x = _dyn.rows(name, B_MAX, live)
    B = 65
    bad = [0, 15, 16, 63, 64]
    q, qd, qdd = x["q"][:B].copy(), x["qd"][:B].copy(), x["qdd"][:B].copy()
    q[bad] = np.nan
    qd[bad[1]] = np.inf
    good = np.setdiff1d(np.arange(B), bad)
    kw = dict(gravity=x["gravity"][:B], live=live)
    clean = inverse_dev(name, desc, x["q"][:B], x["qd"][:B], x["qdd"][:B], tipF=x["tipF"][:B], **kw)
    dirty = inverse_dev(name, desc, q, qd, qdd, tipF=x["tipF"][:B], **kw)
    assert same_bits(dirty[good], clean[good]) and np.isnan(dirty[bad]).all()
    assert same_bits(inertia_dev(name, desc, q, live=live)[good], inertia_dev(name, desc, x["q"][:B], live=live)[good])
    assert same_bits(forward_dev(name, desc, q, qd, x["f"][:B], **kw)[good],
                     forward_dev(name, desc, x["q"][:B], x["qd"][:B], x["f"][:B], **kw)[good])


# ------------------------------------------------------------------ 2. the statement and the reference
@pytest.mark.parametrize("name", ALL)
def test_entries_vs_statement(name):
    B = 65
    desc, dyn = _dyn.descriptors(name)
    x = _dyn.rows(name)
    q, qd, qdd = x["q"][:B], x["qd"][:B], x["qdd"][:B]
    for g in (False, True):
        for dm in (False, True):
            kw = dict(include_gravity=g, use_damping=dm)
            assert _dyn.rel(inverse_dev(name, desc, q, qd, qdd, **kw), _dyn.inverse(desc, dyn, q, qd, qdd, **kw)) < _dyn.TOL_HOST
    one = inverse_dev(name, desc, q, gravity=x["gravity"][0])
    assert same_bits(one, inverse_dev(name, desc, q, gravity=np.tile(x["gravity"][0], (B, 1))))
    assert _dyn.rel(one, _dyn.inverse(desc, dyn, q, gravity=x["gravity"][0])) < _dyn.TOL_HOST
    assert _dyn.rel(inertia_dev(name, desc, q), _dyn.inertia(desc, dyn, q)) < _dyn.TOL_HOST
    # tip forces against the Jacobians of tests/_ik.np_fk_jac
    _, lin, _ = _ik.np_fk_jac(desc, q)
    want = -np.einsum("btid,bti->bd", lin, x["tipF"][:B])
    got = inverse_dev(name, desc, q, qd, qdd, tipF=x["tipF"][:B]) - inverse_dev(name, desc, q, qd, qdd)
    assert np.abs(got - want).max() / np.abs(want).max() < _dyn.tol_tips(desc)
    live = name in _dyn.SYNTH
    desc, dyn = _dyn.descriptors(name, live)
    x = _dyn.rows(name, B_MAX, live)
    for dm in (False, True):
        want, cond = _dyn.forward(desc, dyn, x["q"][:B], x["qd"][:B], x["f"][:B], use_damping=dm)
        got = forward_dev(name, desc, x["q"][:B], x["qd"][:B], x["f"][:B], use_damping=dm, live=live)
        assert (np.abs(got - want).max(1) / np.abs(want).max(1) < _dyn.tol_forward(cond)).all()


@pytest.mark.parametrize("dtype", [_dyn.F32, _dyn.F64])
@pytest.mark.parametrize("robot", _dyn.ROBOTS)
def test_entries_vs_reference(robot, dtype):
    e = _dyn.against_golden(
        robot, lambda desc, dyn, *a, **k: inverse_dev(robot, desc, *a, dtype=dtype, **k),
        lambda desc, dyn, q: inertia_dev(robot, desc, q, dtype=dtype),
        lambda desc, dyn, *a, **k: forward_dev(robot, desc, *a, dtype=dtype, **k))
    print(robot, dtype, {k: f"{v:.3e}" for k, v in e.items()})
    for k, v in e.items():
        assert v < _dyn.TOL[robot][k], (k, v)


# ------------------------------------------------------------------ 3. argument checks
def test_bad_arguments_write_nothing():
    from compliancedex_amd import _native as N
    from compliancedex_amd._native import CdxChain
    lib = N.load()
    desc, _ = _dyn.descriptors("allegro")
    dd = N.ptr(_dyn_dev("allegro"))
    q = torch.zeros(4, 16, dtype=torch.float64, device=DEV)
    out = torch.full((4, 16, 16), 7.0, dtype=torch.float64, device=DEV)
    s = N.stream_ptr()
    inv = lambda c, d, B, qq, dt, o: lib.cdx_dyn_inverse(c, d, B, qq, None, None, dt, 1, 1, None, 0, None, o, s)  # noqa: E731
    assert inv(None, dd, 4, N.ptr(q), 1, N.ptr(out)) == -3
    assert inv(desc, None, 4, N.ptr(q), 1, N.ptr(out)) == -3
    assert inv(desc, dd, 4, None, 1, N.ptr(out)) == -3 and inv(desc, dd, 4, N.ptr(q), 1, None) == -3
    assert inv(desc, dd, -1, N.ptr(q), 1, N.ptr(out)) == -1 and inv(desc, dd, 4, N.ptr(q), 7, N.ptr(out)) == -1
    assert inv(desc, dd, 0, None, 1, None) == 0
    bad = CdxChain.from_buffer_copy(desc)
    bad.bodies[3].parent = 5
    assert inv(bad, dd, 4, N.ptr(q), 1, N.ptr(out)) == -3
    assert lib.cdx_dyn_inertia(bad, dd, 4, N.ptr(q), 1, N.ptr(out), s) == -3
    assert lib.cdx_dyn_inertia(desc, dd, 4, None, 1, N.ptr(out), s) == -3
    assert lib.cdx_dyn_inertia(desc, dd, 0, None, 1, None, s) == 0
    big = CdxChain.from_buffer_copy(desc)
    big.n_dofs = 33
    assert lib.cdx_dyn_forward(big, dd, 4, N.ptr(q), None, N.ptr(q), 1, 1, 0, None, 0, N.ptr(out), s) == -1
    assert lib.cdx_dyn_forward(desc, dd, 4, N.ptr(q), None, None, 1, 1, 0, None, 0, N.ptr(out), s) == -3
    # a moving joint with sign 0: the forward dynamics refuses the chain before it launches
    dead, _ = _dyn.descriptors("tree8")
    q31 = torch.zeros(4, dead.n_dofs, dtype=torch.float64, device=DEV)
    assert lib.cdx_dyn_forward(dead, N.ptr(_dyn_dev("tree8")), 4, N.ptr(q31), None, N.ptr(q31), 1, 1, 0, None, 0,
                               N.ptr(out), s) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------ 4. the Python layer
@functools.lru_cache(None)
def _model(robot):
    from compliancedex_amd import DifferentiableRobotModel
    return DifferentiableRobotModel(robot, device=DEV)


@pytest.mark.parametrize("robot", ("allegro", "iiwa7_allegro"))
def test_model_methods_are_the_c_entries(robot):
    m = _model(robot)
    desc, _ = _dyn.descriptors(robot)
    _, links, offsets = _dyn.chain(robot)
    x = _dyn.rows(robot)
    B = 33
    q, qd, qdd, f, g, tf = (x[k][:B] for k in ("q", "qd", "qdd", "f", "gravity", "tipF"))
    for nd, dt in ((np.float64, _dyn.F64), (np.float32, _dyn.F32)):
        tq, tqd, tqdd, tf_ = _dev(q, nd), _dev(qd, nd), _dev(qdd, nd), _dev(f, nd)
        tq.requires_grad_(True)
        tau = m.compute_inverse_dynamics(tq, tqd, tqdd)
        assert tau.dtype == tq.dtype and not tau.requires_grad
        assert same_bits(tau.cpu().numpy(), inverse_dev(robot, desc, q, qd, qdd, dtype=dt))
        tau = m.compute_inverse_dynamics(tq, tqd, tqdd, False, False, gravity=_dev(g), tip_forces=_dev(tf),
                                         link_names=links, offsets=offsets)
        assert same_bits(tau.cpu().numpy(), inverse_dev(robot, desc, q, qd, qdd, dtype=dt, include_gravity=False,
                                                        use_damping=False, gravity=g, tipF=tf))
        assert same_bits(m.compute_non_linear_effects(tq, tqd).cpu().numpy(), inverse_dev(robot, desc, q, qd, None, dtype=dt))
        assert same_bits(m.gravity_compensation(tq, gravity=g[0].tolist()).cpu().numpy(),
                         inverse_dev(robot, desc, q, dtype=dt, use_damping=False, gravity=g[0]))
        H = m.compute_lagrangian_inertia_matrix(tq, False, True)
        assert same_bits(H.cpu().numpy(), inertia_dev(robot, desc, q, dtype=dt))
        keep = tf_.clone()
        qdd_out = m.compute_forward_dynamics(tq, tqd, tf_, use_damping=True)
        assert torch.equal(tf_, keep)
        assert same_bits(qdd_out.cpu().numpy(), forward_dev(robot, desc, q, qd, f, dtype=dt, use_damping=True))
        assert same_bits(m.compute_forward_dynamics(tq, tqd, tf_).cpu().numpy(), forward_dev(robot, desc, q, qd, f, dtype=dt))
        assert same_bits(m.compute_inverse_dynamics(tq[0], tqd[0], tqdd[0]).cpu().numpy(),
                         inverse_dev(robot, desc, q[:1], qd[:1], qdd[:1], dtype=dt)[0])
    assert m.get_joint_effort_limits() == _dyn.chain(robot)[0].effort_limits()
    assert m.get_joint_limits()[0].keys() == {"lower", "upper"}


@functools.lru_cache(None)
def _results():
    """The nine stored results of tests/golden/results_*.npz: q by the device IK, and the statement's torques."""
    from compliancedex_amd.results import joint_angles_from_contacts
    m, cfg = _model("allegro"), product_chain("allegro").config
    d = {k: np.concatenate([golden(f"results_{e}.npz")[k] for e in ("lego", "realsense")])
         for k in ("contact", "target", "wrist", "compliance")}
    q, status = joint_angles_from_contacts(m, cfg, d["contact"], d["wrist"])
    assert len(q) == 9 and (status == 0).all()
    d["q"] = q
    return m, cfg, d


def _by_hand(m, cfg, q, contact, target, comp, wrist, gravity_world):
    """compute_fingertip_jacobiansᵀ·F + gravity_compensation with the rotation applied here, float64 numpy."""
    from compliancedex_amd.ik import euler_xyz_matrix
    E = len(q)
    Rp = np.broadcast_to(np.eye(3), (E, 3, 3)) if wrist is None else euler_xyz_matrix(torch.from_numpy(wrist[:, 3:])).numpy()
    F = np.einsum("eji,etj->eti", Rp, comp[:, :, None] * (target - contact))
    g = np.einsum("eji,j->ei", Rp, np.asarray(gravity_world, np.float64))
    J = m.compute_fingertip_jacobians(_dev(q), cfg["ee_link_name"], cfg["ee_link_offset"])[0].double().cpu().numpy()
    return np.einsum("etid,eti->ed", J, F) + m.gravity_compensation(_dev(q), gravity=_dev(g)).cpu().numpy()


def test_holding_torques_on_the_stored_results():
    from compliancedex_amd import holding_torques
    m, cfg, d = _results()
    q, contact, target, comp, wrist = d["q"], d["contact"], d["target"], d["compliance"], d["wrist"]
    for w in (None, wrist):  # the identity wrist, and the stored (rotated) one
        rep = holding_torques(m, cfg, _dev(q), contact, target, comp, wrist=w)
        want = _by_hand(m, cfg, q, contact, target, comp, w, (0.0, 0.0, -9.81))
        tau = rep.tau.cpu().numpy()
        assert np.abs(want).max() > 1e-2
        assert _dyn.rel(tau, want) < _chains.TOL_JAC  # (the float32 Jacobian's bound: the torques are linear in it)
        limit = np.asarray(m.get_joint_effort_limits())
        assert same_bits(rep.margin.cpu().numpy(), limit - np.abs(tau))
        assert rep.feasible.cpu().numpy().tolist() == ((limit - np.abs(tau)) >= 0).all(1).tolist()
        assert rep.worst_joint.cpu().numpy().tolist() == (limit - np.abs(tau)).argmin(1).tolist()
    assert np.abs(wrist[:, 3:]).max() > 0.1  # (the stored wrists do rotate)
    # a rotated wrist is forces and gravity rotated by hand
    from compliancedex_amd.ik import euler_xyz_matrix
    Rp = euler_xyz_matrix(torch.from_numpy(wrist[:, 3:])).numpy()
    gb = np.einsum("eji,j->ei", Rp, np.array([0.0, 0.0, -9.81]))
    tf = np.einsum("eji,etj->eti", Rp, -comp[:, :, None] * (target - contact))
    direct = m.compute_inverse_dynamics(_dev(q), None, None, True, False, gravity=_dev(gb), tip_forces=_dev(tf),
                                        link_names=cfg["ee_link_name"], offsets=cfg["ee_link_offset"]).cpu().numpy()
    assert _dyn.rel(holding_torques(m, cfg, _dev(q), contact, target, comp, wrist=wrist).tau.cpu().numpy(), direct) < 1e-12
    # an effort override flips `feasible` on the row chosen for it
    rep = holding_torques(m, cfg, _dev(q), contact, target, comp, wrist=wrist)
    peak = rep.tau.abs().max(1).values.cpu().numpy()
    row = int(np.argmax(peak))
    cut = 0.5 * (np.sort(peak)[-1] + np.sort(peak)[-2])
    assert rep.feasible.all()
    low = holding_torques(m, cfg, _dev(q), contact, target, comp, wrist=wrist, effort=float(cut))
    assert low.feasible.cpu().numpy().tolist() == [i != row for i in range(9)]
    assert int(low.worst_joint[row]) == int(rep.tau[row].abs().argmax())


def test_impedance_torques_vs_numpy():
    """The control law of os_impedance_ctrl.py:32-63 restated in numpy on Allegro (four joints a finger)."""
    from compliancedex_amd import impedance_torques
    m, cfg, d = _results()
    q = d["q"]
    E = len(q)
    rng = np.random.default_rng(5)
    qd = rng.standard_normal((E, 16))
    kP, kD = rng.uniform(50, 200, (4, 3)), rng.uniform(0.1, 1.0, (4, 3))
    links, offsets = cfg["ee_link_name"], cfg["ee_link_offset"]
    pos = m.compute_forward_kinematics(_dev(q), links, offsets=offsets)[0].double().cpu().numpy().reshape(E, 4, 3)
    goal = pos + 0.01 * rng.standard_normal((E, 4, 3))
    J = m.compute_fingertip_jacobians(_dev(q), links, offsets)[0].double().cpu().numpy()
    on = _ik.on_path(m._descriptor(links, offsets))
    ref_q = np.asarray(cfg["ref_q"], np.float64)
    want = np.zeros((E, 16))
    for e in range(E):
        Jall = J[e].reshape(12, 16)
        F = (kP.reshape(-1) * (goal[e] - pos[e]).reshape(-1)) - kD.reshape(-1) * (Jall @ qd[e])
        for i in range(4):
            cols = np.flatnonzero(on[i])
            assert len(cols) == 4
            Js = Jall[3 * i:3 * i + 3][:, cols]
            want[e, cols] = Js.T @ F[3 * i:3 * i + 3]
            want[e, cols] += (np.eye(4) - Js.T @ np.linalg.pinv(Js).T) @ (1.0 * (ref_q[cols] - q[e, cols]))
    want += m.gravity_compensation(_dev(q)).cpu().numpy()
    got = impedance_torques(m, cfg, _dev(q), qd, goal, kP, kD).cpu().numpy()
    assert np.abs(want).max() > 1e-2 and _dyn.rel(got, want) < 1e-9
