"""The pose-target IK rule (frame_ik_row in csrc/cdx_ik.h) on the host build: the bits of the fixed-palm rule without
the additions, the start on the solution, one iteration against the numpy statement, convergence with no row allowed
to miss, half turns, held joints, the independence of rows, the argument checks, and the Python helpers that need no
GPU.  CPU only; tests/test_gpu_ik_frames.py asserts the same on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _chains, _host, _ik, _ik_frames as F

solve = F.frames_host


def test_same_bits_without_the_additions():
    F.check_same_bits_without_additions(solve, _ik.ik_solve_host)


def test_start_on_the_solution():
    F.check_start_on_solution(solve)


def test_single_iteration_vs_numpy():
    F.check_one_iteration(solve)


def test_packed_rows_follow_the_mask():
    """tree3 with rot_mask 0b101, 0b010 and 0b111 against the numpy statement: the orientation rows of a tip sit where
    its rank in the mask says, not where its index does."""
    desc, lower, upper = F.tree3()
    c = F.tree3_case()
    for mask in (0b010, 0b111, 0b100):
        out = solve(desc, F.tree3_params(1), c["q0"], c["target"], c["rot"], rot_mask=mask)
        ref = F.np_frames_step(desc, c["q0"], c["target"], c["rot"], lower, upper, mask)
        assert F.rel_err(out["q"], ref) < 2e-5, mask
        off = [k for k in range(3) if not (mask >> k) & 1]
        assert (out["rot_err"][:, off] == 0).all()


def test_converges_on_the_arm():
    F.check_convergence(solve)


def test_converges_on_the_synthetic_chain():
    desc, lower, upper = F.tree3()
    c = F.tree3_case()
    out = solve(desc, F.tree3_params(), c["q0"], c["target"], c["rot"], rot_mask=0b101)
    F.check_converged(out)
    F.check_box(out["q"], lower, upper)


def test_multi_start_reaches_every_goal():
    F.check_multi_start(solve)


def test_half_turns():
    F.check_half_turns(solve)


def test_held_joints_keep_their_bits():
    F.check_held_joints(solve)


def test_bad_rows_stay_in_their_row():
    F.check_bad_rows(solve, group=32)


def test_weights_and_base_pose():
    """wr = 0 drops the orientation (the row is the position-only solve with rot_err reported as it is); a base pose
    moves targets and solution together."""
    desc, lower, upper = F.arm()
    c = F.arm_case()
    n = 32
    q0, target, rot = c["q0"][:n], c["target"][:n], c["rot"][:n]
    free = solve(desc, F.arm_params(), q0, target, rot, wr=np.zeros((n, 1)), rot_mask=1)
    assert (free["status"] == 0).all() and (free["err"] <= F.TOL).all()
    plain = solve(desc, F.arm_params(), q0, target)
    assert F.same_bits(free["q"], plain["q"]) and F.same_bits(free["iters"], plain["iters"])
    base = np.tile(np.array([0.3, -0.2, 0.1, 0.4, -0.3, 1.1]), (n, 1))
    from tests._ik_pose import euler_rot
    Rb = euler_rot(base[:, 3:])
    moved = np.einsum("eij,etj->eti", Rb, target) + base[:, None, :3]
    out = solve(desc, F.arm_params(), q0, moved, Rb[:, None] @ rot, palm=base, rot_mask=1)
    F.check_converged(out)
    still = solve(desc, F.arm_params(), q0, target, rot, rot_mask=1)
    assert np.abs(out["q"] - still["q"]).max() < 1e-3  # (the same solve up to the rounding of the moved targets)


def test_argument_errors():
    desc, _, _ = F.arm()
    raw = _host.host().cdxh_ik_solve_frames

    def fn(*a):
        return raw(*a, 0)
    c = F.arm_case()
    E, G, p = 9, 4, _host.p
    q0, target, rot = (np.ascontiguousarray(c[k][:E]) for k in ("q0", "target", "rot"))
    outs = [np.full((E + G, 23), 7.0), np.full((E + G, 1), 7.0), np.full((E + G, 1), 7.0),
            np.full(E + G, -7, np.int32), np.full(E + G, -7, np.int32)]

    def call(par, E=E, q0p=p(q0), tp=p(target), rp=p(rot), dtype=_ik.F64, outs=outs, desc=desc, rot_mask=1,
             dof_mask=(1 << 23) - 1):
        return fn(C.byref(desc), C.byref(par) if par is not None else None, E, q0p, dtype, tp, rp, None, None, None,
                  None, rot_mask, dof_mask, *[None if o is None else p(o) for o in outs])

    ok = F.arm_params()
    for rot_mask, dof_mask in ((2, 1), (1 << 8, 1), (1, 0), (1, 1 << 23), (1, 1 << 40), (1 << 33, 1)):
        assert call(ok, rot_mask=rot_mask, dof_mask=dof_mask) == -1, (rot_mask, dof_mask)
    assert call(ok, E=0, q0p=None) == 0
    assert call(ok, E=-1) == -1 and call(ok, dtype=5) == -1 and call(F.arm_params(max_iters=-1)) == -1
    for bad in (dict(tol=0.0), dict(mu0=float("inf")), dict(nu=0.0), dict(rho=-1.0)):
        assert call(F.arm_params(**bad)) == -1, bad
    assert call(None) == -3 and call(ok, q0p=None) == -3 and call(ok, tp=None) == -3
    assert call(ok, rp=None) == -3             # target_rot is required where a tip is oriented …
    for i in range(len(outs)):
        assert call(ok, outs=[None if j == i else o for j, o in enumerate(outs)]) == -3, i
    preset = [7.0, 7.0, 7.0, -7, -7]
    for o, v in zip(outs, preset):
        assert (o == v).all()                    # nothing was written so far
    assert call(ok, rp=None, rot_mask=0) == 0  # … and only there
    assert call(ok) == 0
    for o, v in zip(outs, preset):
        assert (o[E:] == v).all() and not (o[:E] == v).any()


def test_device_sines_change_last_bits_only():
    """device_trig = 1 (the form the kernel is held to) is the same solve up to the FK's last bit."""
    desc, _, _ = F.arm()
    c = F.arm_case()
    a = solve(desc, F.arm_params(), c["q0"], c["target"], c["rot"], rot_mask=1)
    b = solve(desc, F.arm_params(), c["q0"], c["target"], c["rot"], rot_mask=1, device_trig=1)
    F.check_converged(b)
    assert not F.same_bits(a["q"], b["q"]) and np.abs(a["q"] - b["q"]).max() < 1e-3
    again = solve(desc, F.arm_params(), c["q0"], c["target"], c["rot"], rot_mask=1)
    assert F.same_bits(a["q"], again["q"])  # (the switch lasts for its call only)


def test_largest_row_fits():
    """The 64 KB refusal cannot be reached through a valid descriptor: the largest row there is — eight oriented tips,
    32 joints — needs 18 KB.  tree8 (eight tips, 31 joints) with every tip oriented solves."""
    desc = _chains.descriptor("tree8")
    assert desc.n_tips == 8 and desc.n_dofs == 31
    rng = np.random.default_rng(2)
    qs = 0.8 * np.pi * (2.0 * rng.random((5, 31)) - 1.0)
    pos, rot = F.host_fk(desc, qs.astype(np.float32))
    par = F.ik_params([-np.pi] * 31, [np.pi] * 31, [0.0] * 31, 0.0, F.MAX_ITERS, F.TOL)
    out = solve(desc, par, qs + 0.02 * rng.standard_normal(qs.shape), pos, rot, rot_mask=0xff)
    F.check_converged(out)


# ------------------------------------------------------------------ Python helpers (any device)
def test_quaternion_matrix():
    from compliancedex_amd.ik import quaternion_matrix
    q = torch.randn(5, 3, 4, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    R = quaternion_matrix(q)
    assert R.shape == (5, 3, 3, 3) and R.dtype == torch.float64
    assert np.abs(R.numpy() - F.quat_matrix(q.numpy())).max() < 1e-15
    assert (R @ R.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-14
    assert (quaternion_matrix(torch.tensor([0.0, 0.0, np.sin(0.35), np.cos(0.35)])) -
            torch.from_numpy(F.rot_z(0.7))).abs().max() < 1e-7  # (a float32 quaternion: xyzw, z by 0.7 rad)


def test_joint_indices_and_dispatch_errors():
    from compliancedex_amd import DifferentiableRobotModel
    from compliancedex_amd.ik import joint_indices
    rm = DifferentiableRobotModel("iiwa7_allegro", device="cpu")
    moving = [b["name"] for i, b in enumerate(rm.chain.bodies) if rm.chain.dof[i] >= 0]
    assert joint_indices(rm, moving[:7]) == list(range(7)) and joint_indices(rm, [3, moving[10]]) == [3, 10]
    with pytest.raises(KeyError):
        joint_indices(rm, ["no_such_joint"])
    with pytest.raises(ValueError):
        joint_indices(rm, [23])
    t = torch.zeros(1, 1, 3)
    with pytest.raises(ValueError):
        rm.inverse_kinematics(t, ["palm_link"], target_rot=torch.eye(3).view(1, 1, 3, 3), solve_palm=True)
    with pytest.raises(ValueError):
        rm.inverse_kinematics(t, ["palm_link"], joints=[0])


def test_hand_mount_of_the_packaged_pair():
    """The two packaged models are one hand: the fit's residual is ≤ 1e-6 m, the mount a quarter turn without
    translation, the joint map a permutation of the arm model's 16 finger joints; a hand that differs raises."""
    from compliancedex_amd.chain import Chain
    from compliancedex_amd.results import hand_mount
    from compliancedex_amd.urdf import load_robot
    arm_chain, hand_chain = Chain(load_robot("iiwa7_allegro")), Chain(load_robot("allegro"))
    R, t, jmap, resid = hand_mount(arm_chain, hand_chain, hand_chain.config, residual=True)
    assert resid <= 1e-6, resid
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0
    # (a quarter turn, trace = 1 + 2·cos θ — to the four decimals the URDF writes π/2 with)
    assert np.abs(t).max() < 1e-6 and abs(np.trace(R) - 1.0) < 1e-4
    assert sorted(jmap) == list(range(7, 23)) and list(jmap) != list(range(7, 23))
    import copy
    bent = copy.deepcopy(load_robot("allegro"))
    tip = bent["bodies"][hand_chain.index[hand_chain.config["ee_link_name"][0]]]
    tip["xyz"] = [tip["xyz"][0] + 0.01, tip["xyz"][1], tip["xyz"][2]]
    with pytest.raises(ValueError):
        hand_mount(arm_chain, Chain(bent), hand_chain.config)
