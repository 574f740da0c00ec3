"""The free-wrist IK solve (cdx_ik_solve_pose) on an MI355X: the assertions of tests/test_ik_pose_cpu.py on the device
through the C ABI with guard rows past every output, one iteration against the host build, the independence of rows
and of the launch shape, and the Python entry points on top (solve_ik_pose, inverse_kinematics(solve_palm=True),
results.hand_pose_from_contacts)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import _hand, _ik, _ik_pose as P
from tests._helpers import golden, product_chain
from tests._ik import same_bits
from tests.test_gpu_ik import DEV, GUARD, _dev, device_fk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def solve(desc, params, q0, target, pos0=None, rot0=None, palm_offset=None, w=None):
    """cdx_ik_solve_pose through the C ABI on host arrays; GUARD rows past each output are checked to be untouched."""
    from compliancedex_amd import _native as N
    lib = N.load()
    q0 = np.ascontiguousarray(q0)
    E, T, D = q0.shape[0], desc.n_tips, desc.n_dofs
    tq0 = _dev(q0)
    tt, tw = _dev(np.reshape(target, (E, T, 3)), np.float64), _dev(w, np.float64)
    tp, tr = _dev(pos0, np.float64), _dev(rot0, np.float64)
    shapes = dict(q=((D,), tq0.dtype), palm_pos=((3,), torch.float64), palm_rot=((3, 3), torch.float64),
                  err=((T,), torch.float64), iters=((), torch.int32), status=((), torch.int32))
    dev = {k: torch.full((E + GUARD, *s), -7, dtype=t, device=DEV) for k, (s, t) in shapes.items()}
    po = None if palm_offset is None else (C.c_double * 3)(*[float(v) for v in palm_offset])
    N.check(lib.cdx_ik_solve_pose(desc, C.byref(params), E, N.ptr(tq0),
                                  N.DTYPE_F64 if q0.dtype == np.float64 else N.DTYPE_F32, N.ptr(tt), N.ptr(tp), N.ptr(tr),
                                  po, N.ptr(tw), None, *[N.ptr(dev[k]) for k in P.OUTS], N.stream_ptr()),
            "cdx_ik_solve_pose")
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    for k, v in out.items():
        assert (v[E:] == -7).all(), k
        out[k] = v[:E]
    return out


def rows_per_block(desc):
    from compliancedex_amd import _native as N
    return N.load().cdx_ik_pose_rows_per_block(desc.n_tips, desc.n_dofs)


# ------------------------------------------------------------------ the shared checks
def test_start_on_the_solution():
    P.check_start_on_solution(solve)


def test_kabsch_start_alone():
    P.check_kabsch_start(solve)


def _allegro_opt(palm):
    from compliancedex_amd import ProbabilisticGraspOptimizer
    cfg = product_chain("allegro").config
    return ProbabilisticGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"], palm_offset=palm,
                                       ref_q=cfg["ref_q"], optimize_target=True, optimize_palm=True, device=DEV,
                                       num_iters=1, seed=0)


def test_converges_and_public_fk_reproduces_the_targets():
    P.check_convergence(solve)
    from compliancedex_amd import DifferentiableRobotModel, IKPoseResult, solve_ik_pose
    rm = DifferentiableRobotModel("allegro", device=DEV)
    cfg = rm.chain.config
    c = P.pose_inner()
    for start in (None, (_dev(c["pos0"]), _dev(c["rot0"]))):
        res = solve_ik_pose(rm, _dev(c["target"]), cfg["ee_link_name"], cfg["ee_link_offset"], q0=_dev(c["q0"]),
                            palm_pose0=start, ref_q=cfg["ref_q"])
        assert isinstance(res, IKPoseResult) and res.palm_pose.shape == (128, 6) and res.palm_rot.shape == (128, 3, 3)
        assert (res.status == 0).all()
        tips = _allegro_opt(res.palm_pose.cpu().numpy()).forward_kinematics(res.q, res.palm_pose).cpu().numpy()
        assert np.linalg.norm(tips - c["target"], axis=2).max() <= P.TOL + 1e-7 + 1e-12
    raw = solve(P_desc(), P.params(), c["q0"], c["target"], c["pos0"], c["rot0"])  # the last call: the pair start
    for k in ("q", "palm_pos", "palm_rot", "err", "iters", "status"):
        assert same_bits(getattr(res, k).cpu().numpy(), raw[k]), k


def P_desc():
    return _ik.hand()[1]


def test_err_is_the_recomputed_distance():
    P.check_err_bits(solve, device_fk)


def test_single_iteration_vs_host():
    desc, c, _, _ = P.one_iteration_case()
    par = P.params(max_iters=1)
    dev = solve(desc, par, c["q0"], c["target"], c["pos0"], c["rot0"])
    ref = P.ik_pose_host(desc, par, c["q0"], c["target"], c["pos0"], c["rot0"])
    P.check_one_iteration(dev, (ref["q"], ref["palm_pos"], ref["palm_rot"]))
    assert same_bits(dev["iters"], ref["iters"])


def test_unreachable_targets():
    P.check_unreachable(solve, device_fk)


def test_bad_rows_stay_in_their_row():
    L = rows_per_block(P_desc())
    assert L == 16
    P.check_bad_rows(solve, group=L)


def test_launch_shapes():
    """Group, wave and workgroup edges: a row's result does not depend on E nor on how the rows are split over calls."""
    desc = P_desc()
    L = rows_per_block(desc)
    c = P.pose_inner("allegro", 257, 1)
    par = P.params()
    full = solve(desc, par, c["q0"], c["target"], c["pos0"], c["rot0"])
    P.check_converged(full)
    for E in sorted({1, 15, 16, 17, 64, 65, L - 1, L, L + 1} - {0}):
        part = solve(desc, par, c["q0"][:E], c["target"][:E], c["pos0"][:E], c["rot0"][:E])
        for k in full:
            assert same_bits(part[k], full[k][:E]), (E, k)
    a = solve(desc, par, c["q0"][:100], c["target"][:100], c["pos0"][:100], c["rot0"][:100])
    b = solve(desc, par, c["q0"][100:], c["target"][100:], c["pos0"][100:], c["rot0"][100:])
    for k in full:
        assert same_bits(np.concatenate([a[k], b[k]]), full[k]), k


def test_converges_iiwa7_allegro():
    P.check_iiwa7(solve)
    desc = _ik.hand("iiwa7_allegro")[1]
    assert rows_per_block(desc) == 8 and rows_per_block(P_desc()) in (1, 2, 4, 8, 16, 32, 64)


# ------------------------------------------------------------------ ABI
def test_abi_return_codes():
    from compliancedex_amd import _native as N
    lib = N.load()
    desc = P_desc()
    c = P.pose_inner()
    E = 9
    q0, target = _dev(c["q0"][:E]), _dev(c["target"][:E])
    pos0, rot0 = _dev(c["pos0"][:E]), _dev(c["rot0"][:E])
    outs = [torch.full((E + GUARD, n), -7.0, dtype=torch.float64, device=DEV) for n in (16, 3, 9, 4)]
    outs += [torch.full((E + GUARD,), -7, dtype=torch.int32, device=DEV) for _ in range(2)]

    def call(par, E=E, q0p=N.ptr(q0), pos=N.ptr(pos0), rot=N.ptr(rot0), dtype=N.DTYPE_F64, outs=outs, desc=desc):
        return lib.cdx_ik_solve_pose(desc, C.byref(par) if par is not None else None, E, q0p, dtype, N.ptr(target), pos,
                                     rot, None, None, None, *[N.ptr(o) for o in outs], N.stream_ptr())

    assert call(P.params(), E=0, q0p=None) == 0
    assert call(P.params(), E=-1) == -1
    assert call(P.params(), dtype=5) == -1
    assert call(P.params(max_iters=-1)) == -1
    for bad in (dict(tol=0.0), dict(tol=float("nan")), dict(mu0=float("inf")), dict(nu=0.0), dict(rho=-1.0)):
        assert call(P.params(**bad)) == -1, bad
    assert call(None) == -3
    assert call(P.params(), desc=None) == -3
    assert call(P.params(), q0p=None) == -3
    assert call(P.params(), pos=None) == -3
    assert call(P.params(), rot=None) == -3
    for i in range(len(outs)):
        assert call(P.params(), outs=[None if j == i else o for j, o in enumerate(outs)]) == -3, i
    big = type(desc)()
    C.memmove(C.byref(big), C.byref(desc), C.sizeof(big))
    big.n_tips = 9
    assert call(P.params(), desc=big) == -1
    assert lib.cdx_ik_pose_rows_per_block(9, 16) == 0 and lib.cdx_ik_pose_rows_per_block(4, 33) == 0
    torch.cuda.synchronize()
    for o in outs:  # nothing was launched so far
        assert (o == -7).all()
    assert call(P.params()) == 0 and call(P.params(), pos=None, rot=None) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert (o[E:] == -7).all() and not (o[:E] == -7).any()


# ------------------------------------------------------------------ Python
def test_euler_helpers_on_the_device():
    from compliancedex_amd.ik import euler_xyz_matrix, matrix_to_euler_xyz
    g = torch.Generator().manual_seed(1)
    x = ((2.0 * torch.rand(257, 3, generator=g, dtype=torch.float64) - 1.0) * torch.tensor([np.pi, 1.4, np.pi])).to(DEV)
    R = euler_xyz_matrix(x)
    assert R.is_cuda and (matrix_to_euler_xyz(R) - x).abs().max() < 1e-12
    assert (euler_xyz_matrix(matrix_to_euler_xyz(R)) - R).abs().max() < 1e-12
    for sign in (1.0, -1.0):
        lock = torch.tensor([[0.0, 0.0, sign], [0.6 * sign, 0.8, 0.0], [-0.8 * sign, 0.6, 0.0]], dtype=torch.float64, device=DEV)
        ang = matrix_to_euler_xyz(lock)
        assert float(ang[2]) == 0.0 and (euler_xyz_matrix(ang) - lock).abs().max() < 1e-15


def test_inverse_kinematics_solve_palm_switch():
    """solve_palm=False is today's call bit for bit; True routes to solve_ik_pose with palm_pose as the start."""
    from compliancedex_amd import DifferentiableRobotModel, IKPoseResult, IKResult, solve_ik, solve_ik_pose
    rm = DifferentiableRobotModel("allegro", device=DEV)
    cfg = rm.chain.config
    c = _ik.case_results()
    args = (_dev(c["target"]), cfg["ee_link_name"], cfg["ee_link_offset"])
    old = solve_ik(rm, *args, palm_pose=_dev(c["palm"]), ref_q=cfg["ref_q"])
    for res in (rm.inverse_kinematics(*args, palm_pose=_dev(c["palm"]), ref_q=cfg["ref_q"]),
                rm.inverse_kinematics(*args, palm_pose=_dev(c["palm"]), ref_q=cfg["ref_q"], solve_palm=False)):
        assert isinstance(res, IKResult)
        for a, b in zip(res, old):
            assert torch.equal(a, b)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        free = rm.inverse_kinematics(*args, palm_pose=_dev(c["palm"]), ref_q=cfg["ref_q"], solve_palm=True)
    side.synchronize()
    assert isinstance(free, IKPoseResult) and (free.status == 0).all()
    want = solve_ik_pose(rm, *args, palm_pose0=_dev(c["palm"]), ref_q=cfg["ref_q"])
    for a, b in zip(free, want):
        assert torch.equal(a, b)


def _golden_hand():
    from compliancedex_amd.hand import HandSpheres
    with open(_hand.GOLDEN) as f:
        d = json.load(f)
    spheres = {}
    for link, c, r in zip(d["links"], d["centers"], d["radii"]):
        spheres.setdefault(link, []).append((c, r))
    return HandSpheres("allegro", spheres, device=DEV)


def test_hand_pose_from_contacts_and_result_files(tmp_path):
    """The nine stored results with their wrist withheld: a hand for every row, contacts reproduced through the public
    FK (the wrist found need not be the stored one: the pose is not unique), the five files written."""
    from compliancedex_amd import DifferentiableRobotModel
    from compliancedex_amd.results import NAMES, hand_pose_from_contacts, load_results, save_results
    rm = DifferentiableRobotModel("allegro", device=DEV)
    cfg = rm.chain.config
    contact = _ik.case_results()["target"]
    ja, wrist, status, info = hand_pose_from_contacts(rm, cfg, contact)
    assert ja.shape == (9, 16) and wrist.shape == (9, 6) and ja.dtype == wrist.dtype == np.float64
    assert (status == 0).all() and status.dtype == np.int32
    assert info["start"].shape == (9,) and (info["n_converged"] >= 1).all() and (info["n_clear"] == 8).all()
    assert "depth" not in info and info["all"]["status"].shape == (9, 8)
    _ik.check_box(ja)
    tips = _allegro_opt(wrist).forward_kinematics(_dev(ja), _dev(wrist)).cpu().numpy()
    assert np.linalg.norm(tips - contact, axis=2).max() <= P.TOL + 1e-7 + 1e-12
    again = hand_pose_from_contacts(rm, cfg, contact)
    assert same_bits(again[0], ja) and same_bits(again[1], wrist)  # seeded
    d = golden("results_lego.npz")
    save_results("lego_free", d["contact"], d["target"], wrist[:3], d["compliance"], ja[:3], data_dir=str(tmp_path))
    back = load_results("lego_free", data_dir=str(tmp_path))
    for n in NAMES:
        assert back[n].dtype == d[n].dtype == np.float64 and back[n].shape == d[n].shape, n


def test_hand_pose_from_contacts_prefers_a_clear_start():
    """With the hand's spheres and the banana GPIS: info carries depth / clear of the kept rows, and a grasp that has a
    converged clear start and a converged non-clear start with a smaller error keeps the clear one.  The case is built
    from the all-rows report: ``allow`` is set between the depths of two converged starts of one grasp."""
    from compliancedex_amd import DifferentiableRobotModel
    from compliancedex_amd.results import hand_pose_from_contacts
    from compliancedex_amd.workloads import stored_gpis
    rm = DifferentiableRobotModel("allegro", device=DEV)
    cfg = rm.chain.config
    hs = _golden_hand()
    obj = stored_gpis("banana", torch.device(DEV))
    contact = _ik.case_results()["target"]
    ja, wrist, status, info = hand_pose_from_contacts(rm, cfg, contact, hand=hs, obj=obj)
    assert info["depth"].shape == (9, 3) and info["clear"].shape == (9,) and info["clear"].dtype == np.bool_
    every = {k: v.cpu().numpy() for k, v in info["all"].items()}
    rows = np.arange(9)
    assert same_bits(info["depth"], every["depth"][rows, info["start"]])
    assert same_bits(info["clear"], every["clear"][rows, info["start"]])
    assert same_bits(info["clear"], (info["depth"] <= 0.0).all(1))
    deep = every["depth"].max(2)  # [9, 8]: the worst class per start
    ok = every["status"] == 0
    case = None
    for g in range(9):
        conv = np.flatnonzero(ok[g])
        if len(conv) < 2:
            continue
        by_err = conv[np.argmin(every["werr"][g, conv])]  # what the error alone would keep
        shallower = conv[deep[g, conv] < deep[g, by_err]]
        if len(shallower):
            j = shallower[np.argmin(deep[g, shallower])]
            case = (g, by_err, 0.5 * (deep[g, j] + deep[g, by_err]))
            break
    assert case is not None, "no grasp whose least-error start is not also its shallowest"
    g, by_err, allow = case
    ja2, wrist2, status2, info2 = hand_pose_from_contacts(rm, cfg, contact, hand=hs, obj=obj, allow=allow)
    clear2 = info2["all"]["clear"].cpu().numpy()
    assert not clear2[g, by_err] and (clear2[g] & ok[g]).any()
    assert info2["start"][g] != by_err and info2["clear"][g] and status2[g] == 0
    assert same_bits(info2["all"]["q"].cpu().numpy(), every["q"])  # the same solves: only the ranking changed
    assert info2["n_clear"][g] == clear2[g].sum()
