"""The trajectory rule on the host build (libcdx_host.so compiles csrc/cdx_traj.h as the kernels do) and the Python
layer's host-side pieces.  CPU only.

Kernel level: tests/_traj.py's checks — the seed bit for bit against numpy's Philox and polynomial, the cost parts, the
gradient (against torch autograd) and the stepped trajectory (against a dense solve) at the issue's bounds, the one-step
fixed point, best-iterate tracking, rows, guard rows, refusals.

Loop level: the issue's scenario on the host hand entries — iiwa7_allegro with 29 spheres of radius 0.03, T = 24, a
sphere of radius 0.06 in the way, 150 iterations from the straight line.
"""
import numpy as np
import pytest
import torch

from tests import _hand as H, _hand_term as HT, _traj as J


class Host(J.HostBackend):
    spheres = staticmethod(H.host_spheres)
    model = staticmethod(H.host_model)
    term = staticmethod(HT.host_term)


@pytest.mark.parametrize("T,D,E", J.SHAPES, ids=J.IDS)
def test_seed_is_philox_and_a_polynomial(T, D, E):
    J.check_seed(Host, T, D, E)


def test_seed_refusals():
    J.check_seed_refusals(Host)


@pytest.mark.parametrize("T,D,E", J.SHAPES, ids=J.IDS)
def test_step_against_the_statement(T, D, E):
    J.check_step_statement(Host, T, D, E)


@pytest.mark.parametrize("T,D,E", J.SHAPES, ids=J.IDS)
def test_gradient_against_autograd(T, D, E):
    J.check_gradient(T, D, E)


@pytest.mark.parametrize("T,D,E", J.SHAPES, ids=J.IDS)
def test_one_step_fixed_point(T, D, E):
    J.check_fixed_point(Host, T, D, E)


@pytest.mark.parametrize("T,D,E", J.SHAPES[1:], ids=J.IDS[1:])
def test_best_iterate_is_strict(T, D, E):
    J.check_best(Host, T, D, E)


@pytest.mark.parametrize("T,D", [(3, 1), (6, 32), (64, 23)])
def test_rows_stay_in_their_row(T, D):
    J.check_rows(Host, T, D)


def test_step_refusals():
    J.check_step_refusals(Host)


def test_smoothness_matrix_and_factor():
    """A_T is [6] at T = 3 and [[6, −4], [−4, 6]] at T = 4, the outer band appears at T = 5, it is symmetric positive
    definite, and the host build's LDLᵀ solve of it matches a dense solve (through one step with w_c = w_l = 0)."""
    from compliancedex_amd.trajectory import smoothness_matrix, step_size
    assert np.array_equal(smoothness_matrix(3), [[6.0]])
    assert np.array_equal(smoothness_matrix(4), [[6.0, -4.0], [-4.0, 6.0]])
    assert np.array_equal(smoothness_matrix(5)[0], [6.0, -4.0, 1.0]) and smoothness_matrix(4)[0, 1] == -4.0
    for T in (3, 4, 5, 6, 32, 64):
        A = smoothness_matrix(T)
        assert np.array_equal(A, A.T) and np.linalg.eigvalsh(A)[0] > 0
    assert abs(np.linalg.cond(smoothness_matrix(32)) / 3.3e4 - 1) < 0.02
    assert abs(np.linalg.cond(smoothness_matrix(64)) / 5.4e5 - 1) < 0.02
    lam = np.linalg.eigvalsh(smoothness_matrix(24))[0]
    assert step_size(24, 1.0, 100.0, 0.5) == 0.5 / (1.0 + 100.0 / lam)


@pytest.fixture(scope="module")
def scenario():
    sc = J.scene()
    obj = J.obstacle(sc["center"])
    out = J.loop(Host, sc["hs"], J.scene_params(sc), J.hand_params(), sc["line"], obj, J.SCENE["iters"])
    return sc, obj, out


def test_scenario_precondition(scenario):
    sc, obj, _ = scenario
    depth = J.host_depth(sc["hs"], sc["line"], obj)
    print("the line's depth", depth)
    assert depth[0] > 0.05
    clipped = np.abs(sc["q_goal"][7:] - 0.3) > 1e-9  # (the clip into the limits moves the thumb's first joint alone)
    assert clipped.sum() == 1 and abs(sc["q_goal"][7:][clipped][0] - 0.303) < 1e-3


def test_scenario_seed_0_ends_clear(scenario):
    sc, obj, out = scenario
    best = out["best_traj"]
    way, fine = J.host_depth(sc["hs"], best, obj)[0], J.host_depth(sc["hs"], best, obj, refine=4)[0]
    a = J.accelerations(best)
    print("best iteration", out["best_iter"], "depth at waypoints", way, "refined", fine, "U_s", 0.5 * (a * a).sum())
    assert fine <= 0.0  # clear at allow = 0 with refine = 4
    assert ((best >= sc["lower"]) & (best <= sc["upper"])).all()  # within limits
    assert H.same_bits(best[:, 0], sc["line"][:, 0]) and H.same_bits(best[:, -1], sc["line"][:, -1])
    assert H.same_bits(out["traj"][:, 0], sc["line"][:, 0]) and H.same_bits(out["traj"][:, -1], sc["line"][:, -1])
    assert out["best_cost"][0] <= out["first_cost"][0] and np.isfinite(out["best_cost"]).all()
    assert out["best_iter"][0] > 0  # the line itself is not the best


def test_scenario_rows_do_not_depend_on_the_batch(scenario):
    """Four iterations on the line and two seeded rows: row 0 has the bits of the line optimised alone."""
    sc, obj, _ = scenario
    three = J.numpy_seed(1, 3, J.SCENE["T"], 23, sc["q_start"][None], sc["q_goal"][None], 0.3, 0)
    assert H.same_bits(three[:1], sc["line"])
    a = J.loop(Host, sc["hs"], J.scene_params(sc), J.hand_params(), three, obj, 4)
    b = J.loop(Host, sc["hs"], J.scene_params(sc), J.hand_params(), sc["line"], obj, 4)
    for k in J.OUTS:
        assert H.same_bits(a[k][:1], b[k]), k


# ------------------------------------------------------------------ the Python layer's host-side pieces
def test_interpolate_against_numpy():
    from compliancedex_amd.trajectory import interpolate
    rng = np.random.default_rng(2)
    q = rng.standard_normal((3, 7, 5))
    for n in (2, 7, 13, 50):
        got = interpolate(torch.from_numpy(q), n).numpy()
        s = np.linspace(0.0, 6.0, n)
        want = np.stack([np.stack([np.interp(s, np.arange(7.0), q[e, :, d]) for d in range(5)], 1) for e in range(3)])
        assert got.shape == (3, n, 5) and np.abs(got - want).max() <= 1e-14
        assert H.same_bits(got[:, 0], q[:, 0]) and H.same_bits(got[:, -1], q[:, -1])
    assert H.same_bits(interpolate(torch.from_numpy(q), 7).numpy(), q)
    assert interpolate(torch.from_numpy(q[0]), 4).shape == (4, 5)


def test_retime_against_numpy():
    from compliancedex_amd.chain import Chain
    from compliancedex_amd.trajectory import retime
    from compliancedex_amd.urdf import load_robot
    rng = np.random.default_rng(3)
    q = rng.standard_normal((4, 9, 23))
    v = Chain(load_robot("iiwa7_allegro")).velocity_limits()
    assert len(v) == 23 and max(v) > 0
    vv = np.where(np.array(v) > 0, v, np.inf)
    want = (np.abs(np.diff(q, axis=1)) / vv).max((1, 2))
    got = retime(torch.from_numpy(q), v_max=v).numpy()
    assert np.abs(got - want).max() <= 1e-15 * want.max()
    dt = got[:, None, None]
    assert (np.abs(np.diff(q, axis=1)) / dt <= vv * (1 + 1e-12)).all()

    class Model:
        chain = Chain(load_robot("iiwa7_allegro"))
    assert H.same_bits(retime(torch.from_numpy(q), robot_model=Model).numpy(), got)
    with pytest.raises(ValueError):
        retime(torch.from_numpy(q))


def test_path_samples_and_pick_seed():
    from compliancedex_amd.trajectory import path_samples, pick_seed, smoothness
    rng = np.random.default_rng(4)
    q = torch.from_numpy(rng.standard_normal((2, 5, 3)))
    assert path_samples(q, 1) is q
    x = path_samples(q, 4)
    assert x.shape == (2, 17, 3) and H.same_bits(x[:, ::4].numpy(), q.numpy())
    assert np.abs(x[:, 2].numpy() - 0.5 * (q[:, 0] + q[:, 1]).numpy()).max() < 1e-15
    a = J.accelerations(q.numpy())
    assert np.abs(smoothness(q).numpy() - 0.5 * (a * a).sum((1, 2))).max() < 1e-12
    clear = torch.tensor([[True, True, False], [False, False, False], [True, False, True]])
    lim = torch.tensor([[True, False, True], [True, True, True], [True, True, True]])
    smooth = torch.tensor([[3.0, 1.0, 0.5], [1.0, 2.0, 3.0], [float("nan"), 1.0, 2.0]], dtype=torch.float64)
    depth = torch.tensor([[0.0, 0.0, 0.1], [0.3, 0.1, 0.2], [-0.1, 0.2, -0.2]], dtype=torch.float64)
    pick, ok = pick_seed(clear, lim, smooth, depth)
    assert pick.tolist() == [0, 1, 2] and ok.tolist() == [True, False, True]


def test_along_links_fills_the_arm():
    from compliancedex_amd.hand import HandSpheres
    hs = HandSpheres.along_links("iiwa7_allegro", 0.03, pairs=np.zeros((0, 2), np.int32))
    assert 29 < hs.n_spheres <= 256 and set(hs.links) == {b["name"] for b in hs.chain.bodies}
    c = hs.rest_centers()
    for i, b in enumerate(hs.chain.bodies):  # along every parent–child segment no gap exceeds a diameter
        if i == 0:
            continue
        mine = np.concatenate([c[hs.body == b["parent"]], c[hs.body == i][:1]])
        v = np.linalg.norm(np.array(b["xyz"], float))
        if v > 0.06:
            gaps = np.sort(np.linalg.norm(mine - c[hs.body == b["parent"]][0], axis=1))
            assert np.diff(gaps[gaps <= v + 1e-9]).max() <= 0.06 + 1e-6, b["name"]
    with pytest.raises(ValueError):
        HandSpheres.along_links("iiwa7_allegro", 0.0)
