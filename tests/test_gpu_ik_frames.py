"""The pose-target IK solve (cdx_ik_solve_frames) on an MI355X: the assertions of tests/test_ik_frames_cpu.py on the
device through the C ABI with guard rows past every output — and every one of those device runs is held to the host
build bit for bit on q, err, rot_err, iters and status —, the independence of rows and of the launch shape, the return
codes, and the Python layers on top: solve_ik_frames, inverse_kinematics(target_rot=…), results.arm_goal_for_results
and results.arm_approach_for_results."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _ik, _ik_frames as F
from tests._helpers import golden
from tests._ik import same_bits
from tests.test_gpu_ik import DEV, GUARD, _dev
from tests.test_gpu_ik import solve as plain_solve

pytestmark = pytest.mark.gpu

# the reference's arm stands here (verify_grasp_robot.py:135-138: basePosition, and a base quaternion that is a turn of
# −π/4 about z)
REFERENCE_BASE = [-0.14134081, 0.50142033, -0.15, 0.0, 0.0, -np.pi / 4]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def device_solve(desc, params, q0, target, rot=None, palm=None, palm_offset=None, w=None, wr=None, rot_mask=0,
                 dof_mask=None):
    """cdx_ik_solve_frames through the C ABI on host arrays; GUARD rows past each output are checked to be untouched."""
    from compliancedex_amd import _native as N
    lib = N.load()
    q0 = np.ascontiguousarray(q0)
    E, T, D = q0.shape[0], desc.n_tips, desc.n_dofs
    tq0 = _dev(q0)
    tt = _dev(np.reshape(target, (E, T, 3)), np.float64)
    tr = None if rot is None else _dev(np.reshape(rot, (E, T, 3, 3)), np.float64)
    tp, tw, twr = _dev(palm, np.float64), _dev(w, np.float64), _dev(wr, np.float64)
    shapes = dict(q=((D,), tq0.dtype), err=((T,), torch.float64), rot_err=((T,), torch.float64), iters=((), torch.int32),
                  status=((), torch.int32))
    dev = {k: torch.full((E + GUARD, *s), -7, dtype=t, device=DEV) for k, (s, t) in shapes.items()}
    po = None if palm_offset is None else (C.c_double * 3)(*[float(v) for v in palm_offset])
    N.check(lib.cdx_ik_solve_frames(desc, C.byref(params), E, N.ptr(tq0),
                                    N.DTYPE_F64 if q0.dtype == np.float64 else N.DTYPE_F32, N.ptr(tt), N.ptr(tr),
                                    N.ptr(tp), po, N.ptr(tw), N.ptr(twr), rot_mask,
                                    F.all_dofs(desc) if dof_mask is None else dof_mask, None,
                                    *[N.ptr(dev[k]) for k in F.OUTS], N.stream_ptr()), "cdx_ik_solve_frames")
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    for k, v in out.items():
        assert (v[E:] == -7).all(), k
        out[k] = v[:E]
    return out


def solve(desc, params, q0, target, rot=None, palm=None, palm_offset=None, w=None, wr=None, rot_mask=0, dof_mask=None):
    """The device run, held to the host build's bits — the host build taking the FK's float32 sines as the device does
    (F.frames_host, device_trig).  No base pose in these cases: its sines and cosines are the only float64 library
    calls of the rule, and the two libraries may round them differently."""
    out = device_solve(desc, params, q0, target, rot, palm, palm_offset, w, wr, rot_mask, dof_mask)
    if palm is None:
        ref = F.frames_host(desc, params, q0, target, rot, palm, palm_offset, w, wr, rot_mask, dof_mask, device_trig=1)
        for k in F.OUTS:
            differ = np.flatnonzero((out[k] != ref[k]).reshape(len(ref[k]), -1).any(1) &
                                    ~(np.isnan(out[k]) & np.isnan(ref[k])).reshape(len(ref[k]), -1).all(1))
            assert same_bits(out[k], ref[k]), (k, "rows that differ from the host build:", differ[:8], len(differ))
    return out


def rows_per_block(desc, rot_mask):
    from compliancedex_amd import _native as N
    return N.load().cdx_ik_frames_rows_per_block(desc.n_tips, desc.n_dofs, rot_mask)


# ------------------------------------------------------------------ the shared checks
def test_same_bits_without_the_additions():
    F.check_same_bits_without_additions(device_solve, plain_solve)


def test_start_on_the_solution():
    F.check_start_on_solution(solve)


def test_single_iteration_vs_numpy():
    F.check_one_iteration(solve)


def test_converges_on_the_arm():
    F.check_convergence(solve)


def test_multi_start_reaches_every_goal():
    F.check_multi_start(solve)


def test_half_turns():
    F.check_half_turns(solve)


def test_held_joints_keep_their_bits():
    F.check_held_joints(solve)


def test_bad_rows_stay_in_their_row():
    desc, _, _ = F.arm()
    L = rows_per_block(desc, 1)
    assert L == 16
    F.check_bad_rows(solve, group=L)


def test_launch_shapes():
    """E = 0, 1, lanes − 1, lanes, lanes + 1 and a split over two calls: a row's result does not depend on the launch."""
    desc, _, _ = F.arm()
    L = rows_per_block(desc, 1)
    c = F.arm_case(2 * 64 + 5, 1)
    par = F.arm_params()
    full = solve(desc, par, c["q0"], c["target"], c["rot"], rot_mask=1)
    F.check_converged(full)
    for E in (0, 1, L - 1, L, L + 1):
        part = device_solve(desc, par, c["q0"][:E], c["target"][:E], c["rot"][:E], rot_mask=1)
        for k in full:
            assert same_bits(part[k], full[k][:E]), (E, k)
    a = device_solve(desc, par, c["q0"][:50], c["target"][:50], c["rot"][:50], rot_mask=1)
    b = device_solve(desc, par, c["q0"][50:], c["target"][50:], c["rot"][50:], rot_mask=1)
    for k in full:
        assert same_bits(np.concatenate([a[k], b[k]]), full[k]), k


def test_packed_rows_on_the_synthetic_chain():
    desc, lower, upper = F.tree3()
    c = F.tree3_case()
    assert rows_per_block(desc, 0b101) in (1, 2, 4, 8, 16, 32, 64)
    for mask in (0b101, 0b010):
        out = solve(desc, F.tree3_params(), c["q0"], c["target"], c["rot"], rot_mask=mask)
        assert (out["status"] == 0).all()
        off = [k for k in range(3) if not (mask >> k) & 1]
        assert (out["rot_err"][:, off] == 0).all()


# ------------------------------------------------------------------ ABI
def test_abi_return_codes():
    from compliancedex_amd import _native as N
    lib = N.load()
    desc, _, _ = F.arm()
    c = F.arm_case()
    E = 9
    q0, target, rot = _dev(c["q0"][:E]), _dev(c["target"][:E]), _dev(c["rot"][:E])
    outs = [torch.full((E + GUARD, n), -7.0, dtype=torch.float64, device=DEV) for n in (23, 1, 1)]
    outs += [torch.full((E + GUARD,), -7, dtype=torch.int32, device=DEV) for _ in range(2)]

    def call(par, E=E, q0p=N.ptr(q0), tp=N.ptr(target), rp=N.ptr(rot), dtype=N.DTYPE_F64, outs=outs, desc=desc,
             rot_mask=1, dof_mask=(1 << 23) - 1):
        return lib.cdx_ik_solve_frames(desc, C.byref(par) if par is not None else None, E, q0p, dtype, tp, rp, None, None,
                                       None, None, rot_mask, dof_mask, None, *[N.ptr(o) for o in outs], N.stream_ptr())

    ok = F.arm_params()
    for rot_mask, dof_mask in ((2, 1), (1 << 8, 1), (1, 0), (1, 1 << 23), (1, 1 << 40), (1 << 33, 1)):
        assert call(ok, rot_mask=rot_mask, dof_mask=dof_mask) == -1, (rot_mask, dof_mask)
    assert call(ok, E=0, q0p=None) == 0
    assert call(ok, E=-1) == -1 and call(ok, dtype=5) == -1 and call(F.arm_params(max_iters=-1)) == -1
    for bad in (dict(tol=0.0), dict(tol=float("nan")), dict(mu0=float("inf")), dict(nu=0.0), dict(rho=-1.0)):
        assert call(F.arm_params(**bad)) == -1, bad
    assert call(None) == -3 and call(ok, desc=None) == -3
    assert call(ok, q0p=None) == -3 and call(ok, tp=None) == -3 and call(ok, rp=None) == -3
    for i in range(len(outs)):
        assert call(ok, outs=[None if j == i else o for j, o in enumerate(outs)]) == -3, i
    big = type(desc)()
    C.memmove(C.byref(big), C.byref(desc), C.sizeof(big))
    big.n_tips = 9
    assert call(ok, desc=big) == -1
    # (a row over 64 KB of LDS cannot be described: the largest valid one, 8 oriented tips and 32 joints, needs 18 KB)
    assert lib.cdx_ik_frames_rows_per_block(8, 32, 0xff) == 2
    assert lib.cdx_ik_frames_rows_per_block(9, 16, 0) == 0 and lib.cdx_ik_frames_rows_per_block(4, 33, 0) == 0
    assert lib.cdx_ik_frames_rows_per_block(4, 16, 1 << 4) == 0
    assert lib.cdx_ik_frames_rows_per_block(4, 16, 0) == lib.cdx_ik_rows_per_block(4, 16) == 16
    torch.cuda.synchronize()
    for o in outs:  # nothing was launched so far
        assert (o == -7).all()
    assert call(ok) == 0 and call(ok, rp=None, rot_mask=0) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert (o[E:] == -7).all() and not (o[:E] == -7).any()


# ------------------------------------------------------------------ Python
@pytest.fixture(scope="module")
def models():
    from compliancedex_amd import DifferentiableRobotModel
    return DifferentiableRobotModel("iiwa7_allegro", device=DEV), DifferentiableRobotModel("allegro", device=DEV)


def test_solve_ik_frames_and_the_dispatch(models):
    """solve_ik_frames has the C ABI's bits (rot_err turned into radians), takes matrices or xyzw quaternions, runs on
    the current stream; inverse_kinematics(target_rot=…) is the same call."""
    from compliancedex_amd import IKFrameResult, solve_ik_frames
    arm, _ = models
    desc, _, _ = F.arm()
    c = F.arm_case()
    raw = device_solve(desc, F.arm_params(), c["q0"], c["target"], c["rot"], rot_mask=1, dof_mask=(1 << 7) - 1)
    joints = [b["name"] for i, b in enumerate(arm.chain.bodies) if 0 <= arm.chain.dof[i] < 7]
    res = solve_ik_frames(arm, _dev(c["target"]), _dev(c["rot"]), ["palm_link"], q0=_dev(c["q0"]), joints=joints)
    assert isinstance(res, IKFrameResult) and res.rot_err.shape == (128, 1)
    for k in ("q", "err", "iters", "status"):
        assert same_bits(getattr(res, k).cpu().numpy(), raw[k]), k
    assert np.abs(res.rot_err.cpu().numpy() - 2.0 * np.arcsin(np.minimum(1.0, 0.5 * raw["rot_err"]))).max() < 1e-15
    assert (res.status == 0).all() and float(res.rot_err.max()) <= F.TOL / F.WR * 1.001
    # quaternions of the public FK at q* are the same targets
    pos, quat = arm.compute_forward_kinematics(_dev(c["q_star"], np.float32), ["palm_link"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        viaq = arm.inverse_kinematics(pos.double().view(-1, 1, 3), ["palm_link"], q0=_dev(c["q0"]),
                                      target_rot=quat.view(-1, 1, 4), joints=list(range(7)))
    side.synchronize()
    assert isinstance(viaq, IKFrameResult) and (viaq.status == 0).all()
    back, _ = arm.compute_forward_kinematics(viaq.q.float(), ["palm_link"])
    assert float((back - pos).norm(dim=1).max()) <= F.TOL + 1e-6
    # a position-only link next to an oriented one
    both = solve_ik_frames(arm, torch.cat([_dev(c["target"])] * 2, 1), torch.cat([_dev(c["rot"])] * 2, 1),
                           ["palm_link", "palm_link"], q0=_dev(c["q0"]), oriented=[False, True])
    assert (both.status == 0).all() and (both.rot_err[:, 0] == 0).all()


def _hand_tips(hand_model, q, wrist):
    """The hand-only model's world fingertips: Rp·FK(q) + palm_pos, as forward_kinematics(q, wrist) places them."""
    from compliancedex_amd.ik import euler_xyz_matrix
    cfg = hand_model.chain.config
    pos, _ = hand_model.compute_forward_kinematics(q.float(), cfg["ee_link_name"], offsets=cfg["ee_link_offset"])
    R = euler_xyz_matrix(wrist[:, 3:])
    return torch.einsum("eij,etj->eti", R, pos.double().view(len(q), -1, 3)) + wrist[:, None, :3]


def _arm_tips(arm_model, hand_model, q):
    cfg = hand_model.chain.config
    pos, _ = arm_model.compute_forward_kinematics(q.float(), cfg["ee_link_name"], offsets=cfg["ee_link_offset"])
    return pos.double().view(len(q), -1, 3)


def _stored():
    d = [golden(f"results_{exp}.npz") for exp in ("lego", "realsense")]
    return {k: np.concatenate([x[k] for x in d]) for k in ("wrist", "joint_angle", "contact")}


def _within_limits(hand_model, fingers):
    """The stored finger rows clamped to the hand's joint limits.  One stored row (results_realsense) holds a joint
    0.006 rad past its upper limit; the IK holds a joint at clamp(q0), as a robot would, so the hand it is compared with
    is the hand-only model at the clamped angles — 0.006 rad at 0.1 m from the joint would otherwise show as 7e-4 m.
    Every other entry is compared as stored."""
    from compliancedex_amd.ik import joint_box
    lower, upper = joint_box(hand_model.get_joint_limits())
    inside = np.clip(fingers, lower, upper)
    assert np.abs(inside - fingers).max() < 0.01 and (inside != fingers).mean() < 0.01
    return inside


def test_arm_goals_of_a_synthetic_result_set(models):
    """Arm q* in the inner 80 % of the limits, the wrist rows derived from the palm link's pose through the mount, the
    finger rows from the stored fixtures: every row's 23-joint fingertips at q_goal lie within 5e-5 m of the hand-only
    model's (1e-5 m of position tolerance + 1e-4 rad × at most 0.2 m from palm to tip + the float32 slack of two
    chains)."""
    from compliancedex_amd.ik import matrix_to_euler_xyz, quaternion_matrix
    from compliancedex_amd.results import arm_goal_for_results, hand_mount
    arm, hand = models
    cfg = hand.chain.config
    R_x, t_x, jmap = hand_mount(arm, hand, cfg)
    fingers = np.tile(_stored()["joint_angle"], (2, 1))  # 18 rows
    E = len(fingers)
    _, lower, upper = F.arm()
    qs = F._inner(lower, upper, E, 21, 0.0)[0]
    qs[:, jmap] = fingers
    pos, quat = arm.compute_forward_kinematics(_dev(qs, np.float32), ["palm_link"])
    R_l = quaternion_matrix(quat.view(E, 4))
    Rp = R_l @ _dev(R_x)
    wrist = torch.cat([pos.double() + torch.einsum("eij,j->ei", R_l, _dev(t_x)), matrix_to_euler_xyz(Rp)], 1)
    stored = dict(wrist=wrist.cpu().numpy(), joint_angle=fingers)
    q_goal, status, info = arm_goal_for_results(arm, hand, cfg, stored, lift=(0.0, 0.0, 0.1))
    assert q_goal.shape == (E, 23) and q_goal.dtype == np.float64 and status.dtype == np.int32
    print("starts that reach their goal per grasp:", info["n_converged"].tolist())
    assert (status == 0).all(), np.flatnonzero(status != 0)
    lo32, hi32 = F.box32(lower, upper)
    assert same_bits(q_goal[:, jmap], np.clip(fingers.astype(np.float32), lo32[jmap], hi32[jmap]).astype(np.float64))
    inside = _dev(_within_limits(hand, fingers))
    gap = (_arm_tips(arm, hand, _dev(q_goal)) - _hand_tips(hand, inside, wrist)).norm(dim=2)
    print("largest fingertip gap", float(gap.max()))
    assert float(gap.max()) <= 5e-5
    assert info["start"].shape == (E,) and info["all"]["q"].shape == (E, 8, 23) and (info["n_clear"] == 8).all()
    assert info["lift_goal"].shape == (E, 23) and info["lift_status"].shape == (E,)
    up = info["lift_status"] == 0
    lifted = _arm_tips(arm, hand, _dev(info["lift_goal"]))[_dev(up)]
    want = _hand_tips(hand, inside, wrist)[_dev(up)] + _dev(np.array([0.0, 0.0, 0.1]))
    assert up.any() and float((lifted - want).norm(dim=2).max()) <= 5e-5
    again = arm_goal_for_results(arm, hand, cfg, stored)
    assert same_bits(again[0], q_goal)  # seeded


def test_stored_grasps_at_the_reference_base(models):
    """The nine stored rows of results_lego / results_realsense with the arm where the reference stands it.  How many
    are reachable is a finding (DESIGN records it), not a pass condition: the call has to answer for every row, and a
    row it calls reached has to be reached."""
    from compliancedex_amd.results import arm_goal_for_results
    arm, hand = models
    cfg = hand.chain.config
    stored = _stored()
    q_goal, status, info = arm_goal_for_results(arm, hand, cfg, stored, base_pose=REFERENCE_BASE)
    print("stored grasps at the reference's base pose: status", status.tolist(), "starts converged",
          info["n_converged"].tolist(), "err", info["err"].tolist(), "rot_err", info["rot_err"].tolist())
    assert q_goal.shape == (9, 23) and np.isfinite(q_goal).all() and set(status.tolist()) <= {0, 1}
    ok = status == 0
    if ok.any():
        from compliancedex_amd.ik import euler_xyz_matrix
        base = _dev(np.asarray(REFERENCE_BASE))
        tips = torch.einsum("ij,etj->eti", euler_xyz_matrix(base[3:]), _arm_tips(arm, hand, _dev(q_goal))) + base[:3]
        gap = (tips - _hand_tips(hand, _dev(_within_limits(hand, stored["joint_angle"])), _dev(stored["wrist"]))).norm(dim=2)
        assert float(gap[_dev(ok)].max()) <= 5e-5


def test_arm_approach_for_results_ends_on_the_goals(models):
    """G = 2 grasps, 2 seeds, T = 8, 5 iterations, no obstacle: each path ends on its goal bit for bit; a goal forced
    out of reach has success False."""
    from compliancedex_amd.ik import matrix_to_euler_xyz, quaternion_matrix
    from compliancedex_amd.results import arm_approach_for_results, hand_mount
    from tests import _traj as J
    arm, hand = models
    cfg = hand.chain.config
    hs = J.scene()["hs"]
    R_x, t_x, jmap = hand_mount(arm, hand, cfg)
    fingers = _stored()["joint_angle"][:2]
    _, lower, upper = F.arm()
    qs = F._inner(lower, upper, 2, 33, 0.0)[0]
    qs[:, jmap] = fingers
    pos, quat = arm.compute_forward_kinematics(_dev(qs, np.float32), ["palm_link"])
    R_l = quaternion_matrix(quat.view(2, 4))
    wrist = torch.cat([pos.double() + torch.einsum("eij,j->ei", R_l, _dev(t_x)), matrix_to_euler_xyz(R_l @ _dev(R_x))], 1)
    wrist = wrist.cpu().numpy()
    far = torch.tensor([10.0, 10.0, 10.0], dtype=torch.float64, device=DEV)

    def nothing(X):
        v = X - far
        n = v.norm(dim=-1)
        return n - 0.01, v / n[:, None]
    q_start = 0.5 * (np.asarray(lower) + np.asarray(upper))
    plan, q_goal, status, _ = arm_approach_for_results(arm, hand, cfg, hs, q_start, dict(wrist=wrist, joint_angle=fingers),
                                                       nothing, seeds=2, T=8, iters=5)
    assert (status == 0).all() and plan.trajectory.shape == (2, 8, 23)
    assert same_bits(plan.trajectory[:, -1].cpu().numpy(), q_goal)
    assert same_bits(plan.trajectory[:, 0].cpu().numpy(), np.tile(q_start, (2, 1)))
    wrist[1, :3] += 5.0  # five metres away: out of the arm's reach
    plan, q_goal, status, _ = arm_approach_for_results(arm, hand, cfg, hs, q_start, dict(wrist=wrist, joint_angle=fingers),
                                                       nothing, seeds=2, T=8, iters=5)
    assert status.tolist() == [0, 1] and not bool(plan.success[1])
    assert same_bits(plan.trajectory[:, -1].cpu().numpy(), q_goal)
