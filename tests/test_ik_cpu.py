"""Fingertip Jacobians and the IK rule (csrc/cdx_ik.h) on the host build: the numpy statement against the golden FK
fixtures, the host Jacobian against it, convergence with no row allowed to miss, the rule's properties and the
independence of rows.  CPU only; tests/test_gpu_ik.py asserts the same on the device."""
import ctypes as C

import numpy as np
import pytest

from tests import _host, _ik
from tests._helpers import golden, golden_names, product_chain, rel_err
from tests._ik import same_bits

FK_CASES = golden_names("fk_")


def fixture_chain(name):
    d = golden(name)
    robot = "iiwa7_allegro" if name.startswith("fk_iiwa7") else name.split("_")[1]
    return d, product_chain(robot)


def host_fk(desc, q32):
    return _host.fk_forward(desc, q32)[0]


def solve(desc, params, q0, target, palm=None, palm_offset=None, w=None):
    return _ik.ik_solve_host(desc, params, q0, target, palm, palm_offset, w)


@pytest.mark.parametrize("name", FK_CASES)
def test_numpy_fk_is_a_sound_yardstick(name):
    d, ch = fixture_chain(name)
    desc = ch.descriptor([str(s) for s in d["links"]], d["offsets"].tolist())
    pos, _, _ = _ik.np_fk_jac(desc, d["q"])
    assert rel_err(pos.reshape(len(pos), -1), d["pos"]) < 2e-6


@pytest.mark.parametrize("offsets", [True, False])
@pytest.mark.parametrize("name", ["fk_allegro_eeoff_nonrec.npz", "fk_iiwa7_allegro_eeoff_nonrec.npz"])
def test_host_jacobian_vs_numpy(name, offsets):
    d, ch = fixture_chain(name)
    desc = ch.descriptor([str(s) for s in d["links"]], d["offsets"].tolist() if offsets else None)
    assert desc.n_dofs == (23 if "iiwa7" in name else 16)
    q = d["q"].astype(np.float32)
    _, lin, ang = _ik.np_fk_jac(desc, q)
    hl, ha = _ik.fk_jacobian_host(desc, q)
    assert rel_err(hl, lin) < 2e-5
    assert rel_err(ha, ang) < 2e-5
    on = np.broadcast_to(_ik.on_path(desc)[None, :, None, :], hl.shape)
    assert (hl[~on] == 0).all() and (ha[~on] == 0).all()
    norms = np.linalg.norm(ha.astype(np.float64), axis=2)  # [B, T, D]
    assert np.abs(norms[np.broadcast_to(_ik.on_path(desc)[None], norms.shape)] - 1.0).max() < 1e-6
    hl_only, none = _ik.fk_jacobian_host(desc, q, ang=False)
    assert none is None and same_bits(hl_only, hl)
    if "iiwa7" in name:  # the seven arm joints move all four tips; the deepest path has 13 bodies
        assert _ik.on_path(desc)[:, :7].all() and max(len(p) for _, p in _ik._paths(desc)) == 13


@pytest.mark.parametrize("name", ["fk_allegro_eeoff_nonrec.npz", "fk_iiwa7_allegro_eeoff_nonrec.npz"])
def test_numpy_jacobian_vs_central_differences(name):
    """Pins the formula itself, offset included: central differences of the float64 numpy FK, h = 1e-6."""
    d, ch = fixture_chain(name)
    desc = ch.descriptor([str(s) for s in d["links"]], d["offsets"].tolist())
    q = d["q"][:8].astype(np.float64)
    _, lin, _ = _ik.np_fk_jac(desc, q)
    h = 1e-6
    for j in range(desc.n_dofs):
        dq = np.zeros(desc.n_dofs)
        dq[j] = h
        fd = (_ik.np_fk_jac(desc, q + dq)[0] - _ik.np_fk_jac(desc, q - dq)[0]) / (2 * h)
        assert np.abs(fd - lin[..., j]).max() < 1e-7


def test_converges_on_reference_results():
    _, desc, *_ = _ik.hand()
    c = _ik.case_results()
    out = solve(desc, _ik.params(), c["q0"], c["target"], c["palm"])
    _ik.check_converged(out)
    _ik.check_box(out["q"])


def test_converges_on_inner_box():
    _, desc, *_ = _ik.hand()
    c = _ik.case_inner()
    out = solve(desc, _ik.params(), c["q0"], c["target"])
    _ik.check_converged(out)
    _ik.check_box(out["q"])


def test_converges_iiwa7_allegro():
    """The input set of the device test, checked on the host build first: D = 23, 64 rows, ±0.2 rad."""
    _, desc, *_ = _ik.hand("iiwa7_allegro")
    c = _ik.case_inner("iiwa7_allegro", 64, 0.2)
    out = solve(desc, _ik.params("iiwa7_allegro"), c["q0"], c["target"])
    _ik.check_converged(out)
    _ik.check_box(out["q"], "iiwa7_allegro")


def test_err_is_the_recomputed_distance():
    _ik.check_err_bits(solve, host_fk, _ik.host_sincos)


def test_unreachable_targets():
    _ik.check_unreachable(solve, host_fk, _ik.host_sincos)


def test_start_on_target():
    _ik.check_start_on_target(solve, host_fk)


def test_weight_zero():
    _ik.check_weight_zero(solve)


def test_rest_pose_weight():
    _ik.check_rest_pose(solve)


def test_bad_rows_stay_in_their_row():
    _ik.check_bad_rows(solve)


def test_argument_errors():
    _, desc, *_ = _ik.hand()
    fn = _host.host().cdxh_ik_solve
    c = _ik.case_results()
    E = len(c["q0"])
    q, err = np.zeros((E, 16)), np.zeros((E, 4))
    it, st = np.zeros(E, np.int32), np.zeros(E, np.int32)
    p = _host.p

    def call(par, E=E, q0=p(c["q0"]), desc=desc):
        return fn(C.byref(desc), C.byref(par), E, q0, _ik.F64, p(c["target"]), None, None, None,
                  p(q), p(err), p(it), p(st))

    assert call(_ik.params()) == 0
    assert call(_ik.params(), E=0, q0=None) == 0
    assert call(_ik.params(), q0=None) == -3
    assert call(_ik.params(), E=-1) == -1
    assert call(_ik.params(max_iters=-1)) == -1
    for bad in (dict(tol=0.0), dict(tol=float("nan")), dict(mu0=float("inf")), dict(mu_min=-1.0), dict(nu=0.0),
                dict(rho=-1.0)):
        assert call(_ik.params(**bad)) == -1, bad
    par = _ik.params()
    par.lower[2], par.upper[2] = 1.0, 0.5
    assert call(par) == -1
    big = type(desc)()
    C.memmove(C.byref(big), C.byref(desc), C.sizeof(big))
    big.n_tips = 9
    assert call(_ik.params(), desc=big) == -1
    big.n_tips, big.n_dofs = 4, 33
    assert call(_ik.params(), desc=big) == -1
