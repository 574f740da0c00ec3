"""Fingertip Jacobians (cdx_fk_jacobian) and the batched IK solve (cdx_ik_solve) on an MI355X: the Jacobian against the
numpy statement, one iteration against the host build, convergence with no row allowed to miss, the rule's properties
and the independence of rows and of the launch shape — the assertions of tests/test_ik_cpu.py on the device — and the
Python entry points on top."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _ik
from tests._helpers import golden, product_chain, rel_err
from tests._ik import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4  # output rows past the last, preset and found untouched


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def device_fk(desc, q32):
    from compliancedex_amd import _native as N
    lib = N.load()
    q = _dev(q32, np.float32)
    pos = torch.empty(q.shape[0], 3 * desc.n_tips, dtype=torch.float32, device=DEV)
    N.check(lib.cdx_fk_forward(desc, N.ptr(q), q.shape[0], N.ptr(pos), None, N.stream_ptr()), "cdx_fk_forward")
    return pos.cpu().numpy()


def device_sincos(ang):
    """sin / cos of float64 angles as the device's math library gives them."""
    a = _dev(ang, np.float64)
    return torch.sin(a).cpu().numpy(), torch.cos(a).cpu().numpy()


def device_jacobian(desc, q, ang=True):
    from compliancedex_amd import _native as N
    lib = N.load()
    q = _dev(q, np.float32)
    B, T, D = q.shape[0], desc.n_tips, desc.n_dofs
    lin = torch.full((B + GUARD, T, 3, D), -7.0, dtype=torch.float32, device=DEV)
    a = torch.full((B + GUARD, T, 3, D), -9.0, dtype=torch.float32, device=DEV) if ang else None
    N.check(lib.cdx_fk_jacobian(desc, N.ptr(q), B, N.ptr(lin), N.ptr(a), N.stream_ptr()), "cdx_fk_jacobian")
    lin = lin.cpu().numpy()
    assert (lin[B:] == -7.0).all()
    if ang:
        a = a.cpu().numpy()
        assert (a[B:] == -9.0).all()
        a = a[:B]
    return lin[:B], a


def solve(desc, params, q0, target, palm=None, palm_offset=None, w=None):
    """cdx_ik_solve through the C ABI on host arrays; GUARD rows past each output are checked to be untouched."""
    from compliancedex_amd import _native as N
    lib = N.load()
    q0 = np.ascontiguousarray(q0)
    E, T, D = q0.shape[0], desc.n_tips, desc.n_dofs
    tq0 = _dev(q0)
    tt, tp, tw = _dev(np.reshape(target, (E, T, 3)), np.float64), _dev(palm, np.float64), _dev(w, np.float64)
    q = torch.full((E + GUARD, D), -7.0, dtype=tq0.dtype, device=DEV)
    err = torch.full((E + GUARD, T), -7.0, dtype=torch.float64, device=DEV)
    iters = torch.full((E + GUARD,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((E + GUARD,), -7, dtype=torch.int32, device=DEV)
    po = None if palm_offset is None else (C.c_double * 3)(*[float(v) for v in palm_offset])
    assert lib.cdx_ik_workspace(E, T, D) == 0
    N.check(lib.cdx_ik_solve(desc, C.byref(params), E, N.ptr(tq0), N.DTYPE_F64 if q0.dtype == np.float64 else N.DTYPE_F32,
                             N.ptr(tt), N.ptr(tp), po, N.ptr(tw), None, N.ptr(q), N.ptr(err), N.ptr(iters),
                             N.ptr(status), N.stream_ptr()), "cdx_ik_solve")
    out = dict(q=q.cpu().numpy(), err=err.cpu().numpy(), iters=iters.cpu().numpy(), status=status.cpu().numpy())
    for k, v in out.items():
        assert (v[E:] == -7).all(), k
        out[k] = v[:E]
    return out


def rows_per_block(desc):
    from compliancedex_amd import _native as N
    return N.load().cdx_ik_rows_per_block(desc.n_tips, desc.n_dofs)


# ------------------------------------------------------------------ 1. Jacobian
_JAC = {}


def _jac_case(robot, T):
    """257 rows over the whole joint box and their numpy Jacobians, computed once."""
    key = (robot, T)
    if key not in _JAC:
        ch, _, lower, upper, _, links, offsets = _ik.hand(robot)
        desc = ch.descriptor(links[:T], offsets[:T])
        rng = np.random.default_rng(11)
        lo, hi = np.asarray(lower), np.asarray(upper)
        q = (lo + (hi - lo) * rng.random((257, len(lo)))).astype(np.float32)
        _JAC[key] = (desc, q) + _ik.np_fk_jac(desc, q)[1:]
    return _JAC[key]


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("robot", ["allegro", "iiwa7_allegro"])
def test_jacobian_vs_numpy(robot, T):
    desc, q, lin, ang = _jac_case(robot, T)
    assert desc.n_dofs == (16 if robot == "allegro" else 23)
    on = _ik.on_path(desc)[None, :, None, :]
    for B in (1, 63, 64, 65, 257):
        dl, da = device_jacobian(desc, q[:B])
        assert rel_err(dl, lin[:B]) < 2e-5
        assert rel_err(da, ang[:B]) < 2e-5
        assert (dl[~np.broadcast_to(on, dl.shape)] == 0).all() and (da[~np.broadcast_to(on, da.shape)] == 0).all()
        only, none = device_jacobian(desc, q[:B], ang=False)
        assert none is None and same_bits(only, dl)


# ------------------------------------------------------------------ 2. one iteration against the host build
@pytest.mark.parametrize("case", ["results", "inner", "iiwa7"])
def test_single_iteration_vs_host(case):
    robot = "iiwa7_allegro" if case == "iiwa7" else "allegro"
    _, desc, *_ = _ik.hand(robot)
    c = {"results": _ik.case_results, "inner": _ik.case_inner,
         "iiwa7": lambda: _ik.case_inner("iiwa7_allegro", 64, 0.2)}[case]()
    par = _ik.params(robot, max_iters=1)
    dev = solve(desc, par, c["q0"], c["target"], c["palm"])
    ref = _ik.ik_solve_host(desc, par, c["q0"], c["target"], c["palm"])
    assert rel_err(dev["q"], ref["q"]) < 2e-5
    assert (dev["iters"] == 1).all() and same_bits(dev["iters"], ref["iters"])


# ------------------------------------------------------------------ 3. convergence and properties
def _allegro_opt(palm):
    from compliancedex_amd import ProbabilisticGraspOptimizer
    cfg = product_chain("allegro").config
    return ProbabilisticGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"], palm_offset=palm,
                                       ref_q=cfg["ref_q"], optimize_target=True, optimize_palm=True, device=DEV,
                                       num_iters=1, seed=0)


def test_converges_on_reference_results_through_public_fk():
    _, desc, *_ = _ik.hand()
    c = _ik.case_results()
    out = solve(desc, _ik.params(), c["q0"], c["target"], c["palm"])
    _ik.check_converged(out)
    _ik.check_box(out["q"])
    opt = _allegro_opt(c["palm"])
    tips = opt.forward_kinematics(_dev(out["q"]), _dev(c["palm"])).cpu().numpy()
    assert np.linalg.norm(tips - c["target"], axis=2).max() <= _ik.TOL + 1e-7


def test_converges_on_inner_box():
    _, desc, *_ = _ik.hand()
    c = _ik.case_inner()
    out = solve(desc, _ik.params(), c["q0"], c["target"])
    _ik.check_converged(out)
    _ik.check_box(out["q"])
    tips = device_fk(desc, out["q"].astype(np.float32)).astype(np.float64).reshape(c["target"].shape)
    assert np.linalg.norm(tips - c["target"], axis=2).max() <= _ik.TOL + 1e-7


def test_err_is_the_recomputed_distance():
    _ik.check_err_bits(solve, device_fk, device_sincos)


def test_unreachable_targets():
    _ik.check_unreachable(solve, device_fk, device_sincos)


def test_start_on_target():
    _ik.check_start_on_target(solve, device_fk)


def test_weight_zero():
    _ik.check_weight_zero(solve)


def test_rest_pose_weight():
    _ik.check_rest_pose(solve)


def test_launch_shapes():
    """Group, wave and workgroup edges, and the workgroup's own row count: a row's result does not depend on E nor on
    how the rows are split over calls."""
    _, desc, *_ = _ik.hand()
    L = rows_per_block(desc)
    assert L in (1, 2, 4, 8, 16, 32, 64)
    c = _ik.case_inner("allegro", 257, 0.3, 1)
    par = _ik.params()
    full = solve(desc, par, c["q0"], c["target"])
    _ik.check_converged(full)
    for E in sorted({1, 15, 16, 17, 64, 65, L - 1, L, L + 1} - {0}):
        part = solve(desc, par, c["q0"][:E], c["target"][:E])
        for k in full:
            assert same_bits(part[k], full[k][:E]), (E, k)
    a = solve(desc, par, c["q0"][:100], c["target"][:100])
    b = solve(desc, par, c["q0"][100:], c["target"][100:])
    for k in full:
        assert same_bits(np.concatenate([a[k], b[k]]), full[k]), k


# ------------------------------------------------------------------ 4. rows
def test_bad_rows_stay_in_their_row():
    _, desc, *_ = _ik.hand()
    _ik.check_bad_rows(solve, group=rows_per_block(desc))
    _ik.check_bad_rows(solve, group=64)


# ------------------------------------------------------------------ 5. arm + hand
def test_converges_iiwa7_allegro():
    _, desc, *_ = _ik.hand("iiwa7_allegro")
    assert desc.n_dofs == 23
    c = _ik.case_inner("iiwa7_allegro", 64, 0.2)
    out = solve(desc, _ik.params("iiwa7_allegro"), c["q0"], c["target"])
    _ik.check_converged(out)
    _ik.check_box(out["q"], "iiwa7_allegro")


# ------------------------------------------------------------------ 6. ABI
def test_abi_return_codes():
    from compliancedex_amd import _native as N
    lib = N.load()
    for name in ("cdx_fk_jacobian", "cdx_ik_solve", "cdx_ik_workspace"):
        assert hasattr(lib, name)
    _, desc, *_ = _ik.hand()
    c = _ik.case_results()
    E = len(c["q0"])
    q0, target = _dev(c["q0"]), _dev(c["target"])
    q, err = torch.zeros(E, 16, dtype=torch.float64, device=DEV), torch.zeros(E, 4, dtype=torch.float64, device=DEV)
    it, st = (torch.zeros(E, dtype=torch.int32, device=DEV) for _ in range(2))

    def call(par, E=E, q0p=N.ptr(q0), desc=desc):
        return lib.cdx_ik_solve(desc, C.byref(par) if par is not None else None, E, q0p, N.DTYPE_F64, N.ptr(target),
                                None, None, None, None, N.ptr(q), N.ptr(err), N.ptr(it), N.ptr(st), N.stream_ptr())

    assert call(_ik.params()) == 0
    assert call(_ik.params(), E=0, q0p=None) == 0
    assert call(_ik.params(), q0p=None) == -3
    assert call(None) == -3
    assert lib.cdx_ik_solve(None, C.byref(_ik.params()), E, N.ptr(q0), N.DTYPE_F64, N.ptr(target), None, None, None,
                            None, N.ptr(q), N.ptr(err), N.ptr(it), N.ptr(st), N.stream_ptr()) == -3
    assert call(_ik.params(), E=-1) == -1
    assert call(_ik.params(max_iters=-1)) == -1
    for bad in (dict(tol=0.0), dict(tol=float("nan")), dict(mu0=float("inf")), dict(mu_min=-1.0), dict(nu=0.0)):
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
    qf = torch.zeros(2, 16, dtype=torch.float32, device=DEV)
    lin = torch.zeros(2, 4, 3, 16, dtype=torch.float32, device=DEV)
    assert lib.cdx_fk_jacobian(desc, N.ptr(qf), 2, N.ptr(lin), None, N.stream_ptr()) == 0
    assert lib.cdx_fk_jacobian(desc, None, 0, None, None, N.stream_ptr()) == 0
    assert lib.cdx_fk_jacobian(desc, None, 2, N.ptr(lin), None, N.stream_ptr()) == -3
    assert lib.cdx_fk_jacobian(desc, N.ptr(qf), 2, None, None, N.stream_ptr()) == -3
    assert lib.cdx_fk_jacobian(None, N.ptr(qf), 2, N.ptr(lin), None, N.stream_ptr()) == -3
    assert lib.cdx_fk_jacobian(big, N.ptr(qf), 2, N.ptr(lin), None, N.stream_ptr()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 7. Python
def test_python_jacobians():
    from compliancedex_amd import DifferentiableRobotModel
    rm = DifferentiableRobotModel("allegro", device=DEV)
    cfg = rm.chain.config
    links = cfg["ee_link_name"]
    offsets = [[0.01, 0.0, 0.02], [0.0, -0.015, 0.01], [0.005, 0.005, 0.0], [0.0, 0.0, 0.03]]
    q64 = _dev(_ik.case_inner()["q_star"][:9])
    lin, ang = rm.compute_fingertip_jacobians(q64, links, offsets)
    assert lin.shape == ang.shape == (9, 4, 3, 16) and lin.dtype == ang.dtype == torch.float32
    lin32, ang32 = rm.compute_fingertip_jacobians(q64.float(), links, offsets)  # a float64 q is rounded like FK's
    assert torch.equal(lin, lin32) and torch.equal(ang, ang32)
    for k in (0, 2):
        l1, a1 = rm.compute_endeffector_jacobian(q64, links[k], offsets[k])
        assert l1.shape == a1.shape == (9, 3, 16) and l1.dtype == torch.float32
        assert torch.equal(l1, lin[:, k]) and torch.equal(a1, ang[:, k])
    l0, _ = rm.compute_endeffector_jacobian(q64, links[1])
    assert l0.shape == (9, 3, 16) and not torch.equal(l0, lin[:, 1])
    desc = rm.chain.descriptor(links, offsets)
    assert rel_err(lin.cpu().numpy(), _ik.np_fk_jac(desc, q64.float().cpu().numpy())[1]) < 2e-5


def test_python_inverse_kinematics_and_result_files(tmp_path):
    from compliancedex_amd import DifferentiableRobotModel, IKResult, solve_ik
    from compliancedex_amd.results import NAMES, joint_angles_from_contacts, load_results, save_results
    rm = DifferentiableRobotModel("allegro", device=DEV)
    cfg = rm.chain.config
    c = _ik.case_results()
    _, desc, *_ = _ik.hand()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res = rm.inverse_kinematics(_dev(c["target"]), cfg["ee_link_name"], cfg["ee_link_offset"],
                                    palm_pose=_dev(c["palm"]), ref_q=cfg["ref_q"])
    side.synchronize()
    assert isinstance(res, IKResult) and res.q.is_cuda and res.q.shape == (9, 16) and res.q.dtype == torch.float64
    assert res.err.shape == (9, 4) and res.iters.dtype == res.status.dtype == torch.int32
    raw = solve(desc, _ik.params(), c["q0"], c["target"], c["palm"])  # q0 None starts at ref_q
    for k in raw:
        assert same_bits(getattr(res, k).cpu().numpy(), raw[k]), k
    free = solve_ik(rm, _dev(c["target"]), cfg["ee_link_name"], cfg["ee_link_offset"], palm_pose=_dev(c["palm"]),
                    ref_q=cfg["ref_q"], q0=_dev(c["q0"]).float())
    assert free.q.dtype == torch.float32 and torch.equal(free.q.double(), res.q)
    d = golden("results_lego.npz")
    ja, status = joint_angles_from_contacts(rm, cfg, d["contact"], d["wrist"])
    assert ja.shape == (3, 16) and ja.dtype == np.float64 and (status == 0).all()
    save_results("lego_ik", d["contact"], d["target"], d["wrist"], d["compliance"], ja, data_dir=str(tmp_path))
    back = load_results("lego_ik", data_dir=str(tmp_path))
    for n in NAMES:
        assert back[n].dtype == d[n].dtype == np.float64 and back[n].shape == d[n].shape, n
