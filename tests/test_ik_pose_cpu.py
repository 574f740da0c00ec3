"""The free-wrist IK rule (ik_pose_row in csrc/cdx_ik.h) on the host build: the start, convergence with no row allowed
to miss and within half of the iteration budget, one iteration against the numpy statement, the rule's properties,
the independence of rows, the argument checks, and the Euler helpers of ik.py.  CPU only;
tests/test_gpu_ik_pose.py asserts the same on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _host, _ik, _ik_pose as P

solve = P.ik_pose_host


def test_start_on_the_solution():
    P.check_start_on_solution(solve)


def test_kabsch_start_alone():
    P.check_kabsch_start(solve)


def test_converges_within_half_the_budget():
    P.check_convergence(solve, half=True)


def test_err_is_the_recomputed_distance():
    P.check_err_bits(solve, P.host_fk)


def test_single_iteration_vs_numpy():
    desc, c, lower, upper = P.one_iteration_case()
    out = solve(desc, P.params(max_iters=1), c["q0"], c["target"], c["pos0"], c["rot0"])
    P.check_one_iteration(out, P.np_pose_step(desc, c["q0"], c["target"], c["pos0"], c["rot0"], lower, upper))
    assert not P.same_bits(out["palm_rot"], c["rot0"])  # (the step was taken)


def test_unreachable_targets():
    P.check_unreachable(solve, P.host_fk)


def test_bad_rows_stay_in_their_row():
    P.check_bad_rows(solve, group=16)


def test_converges_iiwa7_allegro():
    P.check_iiwa7(solve, half=True)


def test_fixed_palm_entry_is_unchanged_by_the_pose_entry():
    """The pose rule started on a converged fixed-palm answer returns it: the two entries agree on tips and err."""
    _, desc, *_ = _ik.hand()
    c = _ik.case_results()
    fixed = _ik.ik_solve_host(desc, _ik.params(), c["q0"], c["target"], c["palm"])
    rot = P.euler_rot(c["palm"][:, 3:])
    out = solve(desc, P.params(), fixed["q"], c["target"], c["palm"][:, :3], rot)
    assert (out["iters"] == 0).all() and (out["status"] == 0).all()
    assert P.same_bits(out["q"], fixed["q"]) and np.abs(out["err"] - fixed["err"]).max() < 1e-12


def test_argument_errors():
    _, desc, *_ = _ik.hand()
    fn = _host.host().cdxh_ik_solve_pose
    c = P.pose_inner()
    E = 9
    p = _host.p
    q0, target = np.ascontiguousarray(c["q0"][:E]), np.ascontiguousarray(c["target"][:E])
    pos0, rot0 = np.ascontiguousarray(c["pos0"][:E]), np.ascontiguousarray(c["rot0"][:E])
    G = 4
    outs = [np.full((E + G, 16), 7.0), np.full((E + G, 3), 7.0), np.full((E + G, 9), 7.0), np.full((E + G, 4), 7.0),
            np.full(E + G, -7, np.int32), np.full(E + G, -7, np.int32)]

    def call(par, E=E, q0p=p(q0), pos=p(pos0), rot=p(rot0), dtype=_ik.F64, outs=outs, desc=desc):
        return fn(C.byref(desc), C.byref(par) if par is not None else None, E, q0p, dtype, p(target), pos, rot, None,
                  None, *[None if o is None else p(o) for o in outs])

    assert call(P.params()) == 0
    for o in outs:
        assert (np.abs(o[E:]) == 7).all() and not (np.abs(o[:E]) == 7).any()  # (guard rows untouched, the rest written)
    assert call(P.params(), pos=None, rot=None) == 0
    assert call(P.params(), E=0, q0p=None) == 0
    assert call(P.params(), E=-1) == -1
    assert call(P.params(), dtype=5) == -1
    assert call(P.params(max_iters=-1)) == -1
    for bad in (dict(tol=0.0), dict(mu0=float("inf")), dict(nu=0.0), dict(rho=-1.0)):
        assert call(P.params(**bad)) == -1, bad
    assert call(None) == -3
    assert call(P.params(), q0p=None) == -3
    assert call(P.params(), pos=None) == -3
    assert call(P.params(), rot=None) == -3
    for i in range(len(outs)):
        assert call(P.params(), outs=[None if j == i else o for j, o in enumerate(outs)]) == -3, i


# ------------------------------------------------------------------ Python: the Euler helpers (any device)
def test_euler_round_trip():
    from compliancedex_amd.ik import euler_xyz_matrix, matrix_to_euler_xyz
    g = torch.Generator().manual_seed(0)
    x = (2.0 * torch.rand(7, 64, 3, generator=g, dtype=torch.float64) - 1.0) * torch.tensor([np.pi, 1.4, np.pi])
    R = euler_xyz_matrix(x)
    assert R.shape == (7, 64, 3, 3) and R.dtype == torch.float64
    assert np.abs(R.reshape(-1, 3, 3).numpy() - P.euler_rot(x.reshape(-1, 3).numpy())).max() < 1e-15
    back = matrix_to_euler_xyz(R)
    assert back.shape == x.shape and (back - x).abs().max() < 1e-12
    assert (euler_xyz_matrix(back) - R).abs().max() < 1e-12


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_euler_gimbal_branch(sign):
    """b = ±π/2 with R00 = R01 = 0 exactly: c = 0 and a carries the whole rotation about the shared axis."""
    from compliancedex_amd.ik import euler_xyz_matrix, matrix_to_euler_xyz
    a = 0.7
    sa, ca = np.sin(a), np.cos(a)
    R = torch.tensor([[0.0, 0.0, sign], [sa * sign, ca, 0.0], [-ca * sign, sa, 0.0]], dtype=torch.float64)
    ang = matrix_to_euler_xyz(R)
    assert float(ang[2]) == 0.0 and abs(float(ang[1]) - sign * np.pi / 2) < 1e-15 and abs(float(ang[0]) - a) < 1e-15
    assert (euler_xyz_matrix(ang) - R).abs().max() < 1e-15
    other = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)  # (the branch is taken per row)
    batch = matrix_to_euler_xyz(torch.stack([R, euler_xyz_matrix(other)]))
    assert float(batch[0, 2]) == 0.0 and (batch[1] - other).abs().max() < 1e-12


def test_pick_start_order():
    """results.pick_start: status before clearance before error, NaN errors last."""
    from compliancedex_amd.results import pick_start
    status = torch.tensor([[0, 0, 1, 2], [1, 1, 0, 0], [1, 1, 1, 2], [0, 0, 0, 0]], dtype=torch.int32)
    clear = torch.tensor([[False, True, True, True], [True, True, False, False], [False, False, True, True],
                          [True, True, True, True]])
    nan = float("nan")
    werr = torch.tensor([[1e-7, 9e-6, 0.0, nan], [0.0, 0.0, 5e-6, 4e-6], [0.3, 0.2, 0.4, nan], [2e-6, 1e-6, 1.5e-6, 3e-6]],
                        dtype=torch.float64)
    assert pick_start(status, clear, werr).tolist() == [1, 3, 2, 1]
