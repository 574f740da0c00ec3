"""Rigid-body dynamics on the CPU: the float64 statement of tests/_dyn.py anchored three ways — against the reference's
stored results, against physics with no reference involved, and the host build (libcdx_host.so) against it — plus the
chain data the descriptors are packed from.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from compliancedex_amd._native import CdxChain, CdxDyn
from tests import _chains, _dyn, _ik
from tests._host import host, p
from tests.conftest import REPO

ALL = _dyn.ROBOTS + _dyn.SYNTH + ("line31",)
B = 33


# ------------------------------------------------------------------ 0. chain data
def test_packaged_robots_carry_the_inertials():
    """Every link of the three URDFs has an <inertial>; the table of the feature's triage (limits, damping)."""
    effort = {"allegro": {15.0}, "leap": {0.95}, "iiwa7_allegro": {300.0, 15.0}}
    for robot in _dyn.ROBOTS:
        ch, _, _ = _dyn.chain(robot)
        assert ch.has_dynamics and ch.no_inertial == []
        assert set(ch.effort_limits()) == effort[robot]
        damping = {b["damping"] for i, b in enumerate(ch.bodies) if ch.dof[i] >= 0}
        assert (damping == {0.0}) == (robot != "iiwa7_allegro")
        d = ch.dynamics_descriptor()
        assert C.sizeof(d) == C.sizeof(CdxDyn) == 8 * (32 + 96 + 192 + 32)
        for i, b in enumerate(ch.bodies):
            m, c = np.float32(b["mass"]).astype(np.float64), np.float32(b["com"]).astype(np.float64)
            I6 = np.float32(b["inertia"]).astype(np.float64)
            I = np.array([[I6[0], I6[1], I6[2]], [I6[1], I6[3], I6[4]], [I6[2], I6[4], I6[5]]])
            cx = np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]])
            full = I + m * (cx @ cx.T)
            got = list(d.inertia[i])
            want = [full[0, 0], full[0, 1], full[0, 2], full[1, 1], full[1, 2], full[2, 2]]
            assert d.mass[i] == m and np.allclose(list(d.mcom[i]), m * c, rtol=1e-15, atol=0)
            assert np.allclose(got, want, rtol=1e-12, atol=1e-18)


def test_urdf_parser_reads_inertials(tmp_path):
    from compliancedex_amd.chain import Chain
    from compliancedex_amd.urdf import parse_urdf
    path = os.path.join(str(tmp_path), "two.urdf")
    with open(path, "w") as f:
        f.write("""<robot name="two"><link name="base"/>
<link name="arm"><inertial><origin xyz="0.1 0.2 0.3" rpy="1 2 3"/><mass value="0.7"/>
<inertia ixx="1e-3" ixy="2e-4" ixz="3e-4" iyy="4e-3" iyz="5e-4" izz="6e-3"/></inertial></link>
<joint name="j" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0 0 0.1"/><axis xyz="0 0 1"/>
<limit lower="-1" upper="1" effort="2.5" velocity="3"/><dynamics damping="0.25"/></joint></robot>""")
    robot = parse_urdf(path)
    assert robot["no_inertial"] == ["base"]
    base, arm = robot["bodies"]
    assert (base["mass"], base["com"], base["inertia"]) == (1.0, [0.0] * 3, [1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
    assert (arm["mass"], arm["com"]) == (0.7, [0.1, 0.2, 0.3])  # (the inertial origin's rpy is ignored)
    assert arm["inertia"] == [1e-3, 2e-4, 3e-4, 4e-3, 5e-4, 6e-3]
    assert (arm["damping"], arm["effort"], arm["velocity"]) == (0.25, 2.5, 3.0)
    ch = Chain(robot)
    assert ch.no_inertial == ["base"] and ch.effort_limits() == [2.5]
    assert ch.dynamics_descriptor().damping[0] == 0.25


def test_chain_without_inertials_still_loads_and_says_so(tmp_path):
    from compliancedex_amd.chain import Chain
    from compliancedex_amd.urdf import DYNAMICS_KEYS, load_robot
    robot = json.load(open(os.path.join(REPO, "compliancedex_amd", "robots", "allegro.json")))
    for b in robot["bodies"]:
        for k in DYNAMICS_KEYS:
            del b[k]
    del robot["no_inertial"]
    path = os.path.join(str(tmp_path), "old.json")
    json.dump(robot, open(path, "w"))
    ch = Chain(load_robot(path))
    assert ch.n_dofs == 16 and not ch.has_dynamics
    ch.descriptor(ch.config["ee_link_name"], ch.config["ee_link_offset"])
    with pytest.raises(ValueError, match="no inertial data"):
        ch.dynamics_descriptor()


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("robot", _dyn.ROBOTS)
def test_oracle_error_is_the_pinned_one(robot):
    """The reference (float32) against the statement: the figures of tests/_dyn.py, neither above them nor far below."""
    e = _dyn.measure_oracle(robot)
    print(robot, {k: f"{v:.3e}" for k, v in e.items()})
    for k, v in e.items():
        assert 0.5 * _dyn.ORACLE_ERR[robot][k] < v <= _dyn.ORACLE_ERR[robot][k], (k, v)


@pytest.mark.parametrize("dtype", [_dyn.F32, _dyn.F64])
@pytest.mark.parametrize("robot", _dyn.ROBOTS)
def test_host_build_vs_reference(robot, dtype):
    e = _dyn.against_golden(
        robot, lambda *a, **k: _dyn.inverse_host(*a, dtype=dtype, **k), lambda *a: _dyn.inertia_host(*a, dtype=dtype),
        lambda *a, **k: _dyn.forward_host(*a, dtype=dtype, **k))
    print(robot, dtype, {k: f"{v:.3e}" for k, v in e.items()})
    for k, v in e.items():
        assert v < _dyn.TOL[robot][k], (k, v)


# ------------------------------------------------------------------ 2. against physics
@pytest.mark.parametrize("name", ALL)
def test_gravity_torque_is_the_gradient_of_the_potential(name):
    desc, dyn = _dyn.descriptors(name)
    x = _dyn.rows(name, B)
    g = x["gravity"][0]
    tau = _dyn.inverse(desc, dyn, x["q"], use_damping=False, gravity=g, exact=True)
    h, num = 1e-6, np.zeros_like(tau)
    for d in range(desc.n_dofs):
        dq = np.zeros_like(x["q"])
        dq[:, d] = h
        num[:, d] = (_dyn.potential_energy(desc, dyn, x["q"] + dq, g) -
                     _dyn.potential_energy(desc, dyn, x["q"] - dq, g)) / (2 * h)
    assert np.abs(tau).max() > 1e-4
    assert _dyn.rel(tau, num) < 1e-7  # (central difference: h² · third derivative, and ε/h of cancellation)


@pytest.mark.parametrize("name", ALL)
def test_equation_of_motion_and_positive_definite_inertia(name):
    live = name in _dyn.SYNTH
    desc, dyn = _dyn.descriptors(name, live)
    x = _dyn.rows(name, B, live)
    for exact in (True, False):
        H = _dyn.inertia(desc, dyn, x["q"], exact)
        nle = _dyn.inverse(desc, dyn, x["q"], x["qd"], None, gravity=x["gravity"], exact=exact)
        tau = _dyn.inverse(desc, dyn, x["q"], x["qd"], x["qdd"], gravity=x["gravity"], exact=exact)
        assert _dyn.rel(np.einsum("bij,bj->bi", H, x["qdd"]) + nle, tau) < 1e-10
        assert _dyn.rel(H, H.transpose(0, 2, 1)) < 1e-12
        np.linalg.cholesky(H)  # raises unless every H is positive definite
        qdd, _ = _dyn.forward(desc, dyn, x["q"], x["qd"], tau, use_damping=False, gravity=x["gravity"], exact=exact)
        # (τ carries damping·q̇: forward dynamics without its damping term takes it as applied torque)
        damped = _dyn.inverse(desc, dyn, x["q"], x["qd"], x["qdd"], use_damping=False, gravity=x["gravity"], exact=exact)
        qdd2, cond = _dyn.forward(desc, dyn, x["q"], x["qd"], damped, gravity=x["gravity"], exact=exact)
        assert (np.abs(qdd2 - x["qdd"]).max(1) / np.abs(x["qdd"]).max(1) < _dyn.tol_forward(cond)).all()
        del qdd


def test_dead_joint_has_a_zero_row_and_column():
    for name in _dyn.SYNTH:
        desc, dyn = _dyn.descriptors(name)
        dead = [desc.bodies[i].dof for i in range(1, desc.n_bodies) if desc.bodies[i].dof >= 0 and desc.bodies[i].sign == 0]
        assert len(dead) == 1
        x = _dyn.rows(name, B)
        for H in (_dyn.inertia(desc, dyn, x["q"]), _dyn.inertia_host(desc, dyn, x["q"])):
            assert (H[:, dead[0], :] == 0).all() and (H[:, :, dead[0]] == 0).all()
        for f in (_dyn.inverse, _dyn.inverse_host):
            tau = f(desc, dyn, x["q"], x["qd"], x["qdd"], gravity=x["gravity"], tipF=x["tipF"])
            assert np.array_equal(tau[:, dead[0]], dyn.damping[dead[0]] * x["qd"][:, dead[0]])
        _dyn.forward_host(desc, dyn, x["q"], x["qd"], x["f"], expect=-1)


@pytest.mark.parametrize("name", ALL)
def test_tip_forces_are_minus_jacobian_transpose(name):
    desc, dyn = _dyn.descriptors(name)
    x = _dyn.rows(name, B)
    _, lin, _ = _ik.np_fk_jac(desc, x["q"].astype(np.float32).astype(np.float64))
    want = -np.einsum("btid,bti->bd", lin, x["tipF"])
    for f in (_dyn.inverse, _dyn.inverse_host):
        a = f(desc, dyn, x["q"], x["qd"], x["qdd"], gravity=x["gravity"], tipF=x["tipF"])
        b = f(desc, dyn, x["q"], x["qd"], x["qdd"], gravity=x["gravity"])
        err = np.abs((a - b) - want).max() / np.abs(want).max()
        print(name, f"{err:.2e}", f"{_dyn.tol_tips(desc):.2e}")
        assert err < _dyn.tol_tips(desc), err


# ------------------------------------------------------------------ 3. the host build against the statement
@pytest.mark.parametrize("name", ALL)
def test_host_build_vs_statement(name):
    desc, dyn = _dyn.descriptors(name)
    x = _dyn.rows(name, B)
    for g in (False, True):
        for dm in (False, True):
            kw = dict(include_gravity=g, use_damping=dm)
            assert _dyn.rel(_dyn.inverse_host(desc, dyn, x["q"], x["qd"], x["qdd"], **kw),
                            _dyn.inverse(desc, dyn, x["q"], x["qd"], x["qdd"], **kw)) < _dyn.TOL_HOST
    full = dict(gravity=x["gravity"], tipF=x["tipF"])
    got = _dyn.inverse_host(desc, dyn, x["q"], x["qd"], x["qdd"], **full)
    assert _dyn.rel(got, _dyn.inverse(desc, dyn, x["q"], x["qd"], x["qdd"], **full)) < _dyn.TOL_HOST
    one = dict(gravity=x["gravity"][0])
    a = _dyn.inverse_host(desc, dyn, x["q"], None, None, **one)
    assert _ik.same_bits(a, _dyn.inverse_host(desc, dyn, x["q"], None, None, gravity=np.tile(x["gravity"][0], (B, 1))))
    assert _ik.same_bits(a, _dyn.inverse_host(desc, dyn, x["q"], np.zeros_like(x["qd"]), np.zeros_like(x["qdd"]), **one))
    assert _dyn.rel(a, _dyn.inverse(desc, dyn, x["q"], **one)) < _dyn.TOL_HOST
    H = _dyn.inertia_host(desc, dyn, x["q"])
    assert _dyn.rel(H, _dyn.inertia(desc, dyn, x["q"])) < _dyn.TOL_HOST
    assert _ik.same_bits(H, np.ascontiguousarray(H.transpose(0, 2, 1)))
    # float32 I/O: the same numbers in (the rows are float32 values), the float64 result rounded once
    t32 = _dyn.inverse_host(desc, dyn, x["q"], x["qd"], x["qdd"], dtype=_dyn.F32, **full)
    assert t32.dtype == np.float32 and _ik.same_bits(t32, got.astype(np.float32))
    assert _ik.same_bits(_dyn.inertia_host(desc, dyn, x["q"], dtype=_dyn.F32), H.astype(np.float32))


@pytest.mark.parametrize("name", ALL)
def test_host_forward_dynamics_vs_statement(name):
    live = name in _dyn.SYNTH
    desc, dyn = _dyn.descriptors(name, live)
    x = _dyn.rows(name, B, live)
    for dm in (False, True):
        want, cond = _dyn.forward(desc, dyn, x["q"], x["qd"], x["f"], use_damping=dm, gravity=x["gravity"])
        f = x["f"].copy()
        got = _dyn.forward_host(desc, dyn, x["q"], x["qd"], f, use_damping=dm, gravity=x["gravity"])
        assert np.array_equal(f, x["f"])  # (the caller's f is not written)
        err = np.abs(got - want).max(1) / np.abs(want).max(1)
        assert (err < _dyn.tol_forward(cond)).all(), float((err / _dyn.tol_forward(cond)).max())
        back = _dyn.inverse_host(desc, dyn, x["q"], x["qd"], got, use_damping=dm, gravity=x["gravity"])
        assert (np.abs(back - x["f"]).max(1) / np.abs(x["f"]).max(1) < _dyn.tol_forward(cond)).all()


def test_host_argument_checks():
    desc, dyn = _dyn.descriptors("allegro")
    q = np.zeros((2, 16))
    out = np.full((2, 16), 7.0)
    h = host()
    args = (p(q), None, None, _dyn.F64, 1, 1, None, 0, None, p(out))
    assert h.cdxh_dyn_inverse(None, C.byref(dyn), 2, *args) == -3
    assert h.cdxh_dyn_inverse(C.byref(desc), None, 2, *args) == -3
    assert h.cdxh_dyn_inverse(C.byref(desc), C.byref(dyn), -1, *args) == -1
    assert h.cdxh_dyn_inverse(C.byref(desc), C.byref(dyn), 2, p(q), None, None, 5, 1, 1, None, 0, None, p(out)) == -1
    assert h.cdxh_dyn_inverse(C.byref(desc), C.byref(dyn), 2, None, None, None, 1, 1, 1, None, 0, None, p(out)) == -3
    assert h.cdxh_dyn_inverse(C.byref(desc), C.byref(dyn), 0, None, None, None, 1, 1, 1, None, 0, None, None) == 0
    bad = CdxChain.from_buffer_copy(desc)
    bad.bodies[3].parent = 5
    assert h.cdxh_dyn_inverse(C.byref(bad), C.byref(dyn), 2, *args) == -3
    assert h.cdxh_dyn_inertia(C.byref(bad), C.byref(dyn), 2, p(q), _dyn.F64, p(out)) == -3
    bad = CdxChain.from_buffer_copy(desc)
    bad.n_bodies = 33
    assert h.cdxh_dyn_forward(C.byref(bad), C.byref(dyn), 2, p(q), None, p(q), 1, 1, 0, None, 0, p(out)) == -1
    assert (out == 7.0).all()
    # a chain deeper than the FK's 16 levels is a chain like any other here
    deep, ddyn = _dyn.descriptors("line31")
    assert _chains.chain_of(_dyn.widest_line()).n_dofs == 29 and deep.n_bodies == 32
    assert max(_chains._depth([b.parent for b in deep.bodies], t) for t in deep.tip_body[:deep.n_tips]) == 31
