"""cdx_traj_seed / cdx_traj_step on an MI355X through the C ABI and the Python layer of compliancedex_amd.trajectory.

Kernel level: tests/_traj.py's checks on the device (the numpy statement at the issue's bounds, fixed point, best
iterate, rows, guard rows, refusals) and the device against the host build, bit for bit on every output of the seed
and of the step.

Loop level.  The loop of tests/_traj.py on the device against the same loop on the host build for 4 iterations, bit
for bit on every output of every iteration — in lock-step: the host loop takes each iteration's poses and centres from
the device's cdx_hand_spheres launch, as tests/test_gpu_hand_term.py hands "the device's own poses" to the host term.
Two free-running loops cannot agree bit for bit: the FK rounds float32 sines and cosines, glibc's sinf on the host and
the rounded float64 sine on the device, and the two differ in the last place for 1.3 % of arguments (517 774 of
4·10⁷ uniform draws in ±π measured on the host) — tests/test_gpu_hand.py compares the centres to a tolerance for that
reason.  Everything this feature adds is downstream of those centres and is held to the host's bits.

Then the issue's scenario through ``plan_approach`` with a callable object on the device, the Allegro hand on the
packaged banana GPIS (the cdx_gpis_mean launch), and the report / selection identities.
"""
import numpy as np
import pytest
import torch

from tests import _hand as H, _hand_term as HT, _traj as J
from tests import test_gpu_hand as GH
from tests import test_gpu_hand_term as GT

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def _up(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


class Dev:
    spheres = staticmethod(GH.dev_spheres)
    model = staticmethod(lambda hs: hs.native())
    term = staticmethod(GT.dev_term)

    @staticmethod
    def seed(G, seeds, T, D, qs, qg, amp, seed, out):
        from compliancedex_amd import _native as N
        a, b, o = _up(qs), _up(qg), _up(out)
        rc = N.load().cdx_traj_seed(G, seeds, T, D, N.ptr(a), N.ptr(b), amp, seed, N.ptr(o), N.stream_ptr())
        torch.cuda.synchronize()
        if out is not None:
            out[...] = o.cpu().numpy()
        return rc

    @staticmethod
    def step(par, E, traj, g_c, cost_t, iteration, cost, best_cost, best_iter, best_traj):
        from compliancedex_amd import _native as N
        host = (traj, cost, best_cost, best_iter, best_traj)
        t, c, bc, bi, bt = (_up(a) for a in host)
        g, ct = _up(g_c), _up(cost_t)  # (named: an unnamed tensor's memory is free again before the launch reads it)
        rc = N.load().cdx_traj_step(par, E, N.ptr(t), N.ptr(g), N.ptr(ct), iteration, N.ptr(c), N.ptr(bc), N.ptr(bi),
                                    N.ptr(bt), N.stream_ptr())
        torch.cuda.synchronize()
        for a, d in zip(host, (t, c, bc, bi, bt)):
            if a is not None:
                a[...] = d.cpu().numpy()
        return rc


class Host(J.HostBackend):
    spheres = staticmethod(H.host_spheres)
    model = staticmethod(H.host_model)
    term = staticmethod(HT.host_term)


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("T,D,E", J.SHAPES, ids=J.IDS)
def test_seed(T, D, E):
    J.check_seed(Dev, T, D, E)
    G, seeds, qs, qg = J.seed_inputs(T, D, E)
    a = J.run_seed(Dev, G, seeds, T, D, qs, qg, 0.3, J.SEED_KEY)
    b = J.run_seed(Host, G, seeds, T, D, qs, qg, 0.3, J.SEED_KEY)
    assert a[0] == b[0] == 0 and H.same_bits(a[1], b[1])


def test_seed_refusals():
    J.check_seed_refusals(Dev)


@pytest.mark.parametrize("T,D,E", J.SHAPES, ids=J.IDS)
def test_step_against_the_statement(T, D, E):
    J.check_step_statement(Dev, T, D, E)


@pytest.mark.parametrize("T,D,E", J.SHAPES, ids=J.IDS)
def test_step_device_equals_host_build(T, D, E):
    """Every output, its guard rows included: a first step (every row wins) and a step on random best presets of which
    about half win; with and without the collision term."""
    f = J.family(T, D)
    par = J.params(f["lower"], f["upper"], T)
    a = J.run_step(Dev, par, E, f["q"], f["g_c"], f["cost_t"], iteration=2)
    b = J.run_step(Host, par, E, f["q"], f["g_c"], f["cost_t"], iteration=2)
    assert a[0] == b[0] == 0
    J.same(a[1], b[1], tag="first step")
    best = np.array(b[1]["best_cost"][:E]) * np.random.default_rng(1).choice([0.5, 2.0], E)
    a = J.run_step(Dev, par, E, f["q"], f["g_c"], f["cost_t"], iteration=9, best=best, seed=3)
    b = J.run_step(Host, par, E, f["q"], f["g_c"], f["cost_t"], iteration=9, best=best, seed=3)
    assert a[0] == b[0] == 0
    J.same(a[1], b[1], tag="presets")
    if E > 1:
        assert 0 < (b[1]["best_iter"][:E] == 9).sum() < E
    a = J.run_step(Dev, par, E, f["q"], None, None)
    b = J.run_step(Host, par, E, f["q"], None, None)
    assert a[0] == b[0] == 0
    J.same(a[1], b[1], tag="no collision term")


@pytest.mark.parametrize("T,D,E", J.SHAPES, ids=J.IDS)
def test_one_step_fixed_point(T, D, E):
    J.check_fixed_point(Dev, T, D, E)


@pytest.mark.parametrize("T,D,E", J.SHAPES[1:], ids=J.IDS[1:])
def test_best_iterate_is_strict(T, D, E):
    J.check_best(Dev, T, D, E)


@pytest.mark.parametrize("T,D", [(3, 1), (6, 32), (64, 23)])
def test_rows_stay_in_their_row(T, D):
    J.check_rows(Dev, T, D)


def test_step_refusals():
    J.check_step_refusals(Dev)


# ------------------------------------------------------------------ the loop
def test_loop_device_equals_host_build():
    """The scenario's line and two seeded rows, 4 iterations, in lock-step (module docstring): every iteration's
    outputs, hence the final ones, bit for bit."""
    sc = J.scene()
    obj = J.obstacle(sc["center"])
    traj = J.numpy_seed(1, 3, J.SCENE["T"], 23, sc["q_start"][None], sc["q_goal"][None], 0.3, 0)
    tape = []
    dev = J.loop(Dev, sc["hs"], J.scene_params(sc), J.hand_params(), traj, obj, 4, record=tape)
    assert len(tape) == 4
    host = J.loop(Host, sc["hs"], J.scene_params(sc), J.hand_params(), traj, obj, 4, replay=tape)
    J.same(dev, host, tag="4 iterations")
    assert H.same_bits(dev["first_cost"], host["first_cost"])
    assert not H.same_bits(dev["traj"], traj) and H.same_bits(dev["traj"][:, 0], traj[:, 0])
    for it in (1, 3):  # each prefix as well
        J.same(J.loop(Dev, sc["hs"], J.scene_params(sc), J.hand_params(), traj, obj, it, replay=tape),
               J.loop(Host, sc["hs"], J.scene_params(sc), J.hand_params(), traj, obj, it, replay=tape), tag=f"{it}")
    # free-running, the two agree to the FK's float32 last place: 1e-6 on joint angles of order 1 after 4 steps
    free = J.loop(Host, sc["hs"], J.scene_params(sc), J.hand_params(), traj, obj, 4)
    print("free-running host vs device, max |Δq|", np.abs(free["traj"] - dev["traj"]).max())


def _sphere_on_device(center, radius):
    c = torch.tensor(center, device=DEV)

    def f(X):
        v = X - c
        n = v.norm(dim=-1)
        return n - radius, v / n[:, None]
    return f


@pytest.fixture(scope="module")
def planned():
    from compliancedex_amd import DifferentiableRobotModel, TrajectoryOptimizer, plan_approach
    sc = J.scene()
    S = J.SCENE
    rm = DifferentiableRobotModel("iiwa7_allegro", device=DEV)
    opt = TrajectoryOptimizer(rm, sc["hs"], T=S["T"], w_smooth=S["w_smooth"], w_col=S["w_col"], w_lim=S["w_lim"],
                              m_lim=S["m_lim"], gain=S["gain"], m_obj=S["m_obj"], w_obj=S["w_obj"])
    assert opt.step == sc["step"] and np.array_equal(opt.lower, sc["lower"]) and np.array_equal(opt.upper, sc["upper"])
    obj = _sphere_on_device(sc["center"], S["obstacle"])
    plan = plan_approach(rm, sc["hs"], _up(sc["q_start"]), _up(sc["q_goal"]), obj, seeds=8, amp=0.3, seed=0, refine=4,
                         allow=0.0, iters=S["iters"], optimizer=opt)
    return sc, opt, obj, plan


def test_scenario_through_plan_approach(planned):
    from compliancedex_amd import trajectory_report
    sc, opt, obj, plan = planned
    T = J.SCENE["T"]
    line = _up(sc["line"])
    rep0 = trajectory_report(sc["hs"], line, obj, refine=1)
    print("the line's depth", rep0["depth"][0].tolist())
    assert rep0["depth"][0, 0] > 0.05 and not rep0["clear"][0]
    assert plan.trajectory.shape == (1, T, 23) and plan.all_trajectories.shape == (1, 8, T, 23)
    assert plan.seed.shape == (1,) and plan.success.shape == (1,) and plan.success.dtype == torch.bool
    rep = plan.all_report
    print("refined depth per seed", rep["depth"][:, 0].tolist(), "U_s", rep["smoothness"].tolist(), "kept", plan.seed.tolist())
    assert H.same_bits(plan.all_trajectories[0, 0, 0].cpu().numpy(), sc["q_start"])
    assert H.same_bits(plan.all_trajectories[0, 0, -1].cpu().numpy(), sc["q_goal"])
    assert bool(rep["clear"][0]) and bool(rep["within_limits"][0])  # seed 0's best iterate, refine = 4, allow = 0
    first = opt.optimize(line, obj, iters=1)
    assert H.same_bits(first.trajectory.cpu().numpy(), sc["line"]) and (first.iteration == 0).all()
    assert float(plan.all_cost[0, 0]) <= float(first.cost[0])
    assert plan.success.all() and plan.report["clear"].all() and plan.report["within_limits"].all()
    k = int(plan.seed[0])
    assert torch.equal(plan.trajectory[0], plan.all_trajectories[0, k])
    ok = rep["clear"] & rep["within_limits"]
    assert ok[k] and float(rep["smoothness"][k]) == float(rep["smoothness"][ok].min())
    for key, v in plan.report.items():
        assert torch.equal(v[0], rep[key][k]), key


def test_plan_with_one_seed_is_optimize_on_the_line(planned):
    from compliancedex_amd import plan_approach
    sc, opt, obj, _ = planned
    res = opt.optimize(_up(sc["line"]), obj, iters=6)
    plan = plan_approach(None, sc["hs"], _up(sc["q_start"]), _up(sc["q_goal"]), obj, seeds=1, iters=6, optimizer=opt)
    assert torch.equal(plan.trajectory, res.trajectory) and torch.equal(plan.cost, res.cost)
    assert (plan.seed == 0).all() and int(res.iteration[0]) >= 0


def test_approach_for_results_plans_to_the_stored_grasps(planned):
    """results.approach_for_results: the goals are the stored joint angles, the root stands at the stored wrist (the
    identity here, so the plan has the bits of plan_approach without a palm pose)."""
    from compliancedex_amd import plan_approach
    from compliancedex_amd.results import approach_for_results
    sc, opt, obj, _ = planned
    goals = np.stack([sc["q_goal"], 0.5 * (sc["q_start"] + sc["q_goal"])])
    stored = dict(joint_angle=goals, wrist=np.zeros((2, 6)))
    a = approach_for_results(None, sc["hs"], sc["q_start"], stored, obj, seeds=2, iters=5, optimizer=opt)
    b = plan_approach(None, sc["hs"], _up(sc["q_start"]), _up(goals), obj, seeds=2, iters=5, optimizer=opt)
    assert a.trajectory.shape == (2, J.SCENE["T"], 23) and torch.equal(a.trajectory, b.trajectory)
    assert torch.equal(a.seed, b.seed) and torch.equal(a.success, b.success)
    assert H.same_bits(a.trajectory[:, -1].cpu().numpy(), goals)


def test_report_at_refine_1_is_the_waypoints_report(planned):
    from compliancedex_amd import penetration_report, trajectory_report
    sc, _, obj, plan = planned
    traj = plan.all_trajectories[0]
    E, T, D = traj.shape
    rep = trajectory_report(sc["hs"], traj, obj, refine=1, floor_z=-0.2)
    way = penetration_report(sc["hs"], traj.reshape(E * T, D).contiguous(), None, obj, floor_z=-0.2)
    depth = way["depth"].view(E, T, 3)
    assert torch.equal(rep["depth"], depth.amax(1)) and torch.equal(rep["at"], depth.argmax(1))
    assert torch.equal(rep["clear"], (depth.amax(1) <= 0).all(1))
    for k, shape in (("depth", (E, 3)), ("at", (E, 3)), ("clear", (E,)), ("within_limits", (E,)), ("max_step", (E,)),
                     ("smoothness", (E,))):
        assert tuple(rep[k].shape) == shape and rep[k].is_cuda, k
    q = traj.cpu().numpy()
    a = J.accelerations(q)
    assert np.abs(rep["smoothness"].cpu().numpy() - 0.5 * (a * a).sum((1, 2))).max() < 1e-12
    assert H.same_bits(rep["max_step"].cpu().numpy(), np.abs(np.diff(q, axis=1)).max((1, 2)))
    fine = trajectory_report(sc["hs"], traj, obj, refine=4, floor_z=-0.2)
    assert (fine["depth"] >= rep["depth"]).all()  # the sub-steps include the waypoints


def test_allegro_on_the_banana_gpis():
    """The cdx_gpis_mean path: 8 goals × 4 seeds, T = 16, a fixed palm pose per goal, 10 iterations."""
    from compliancedex_amd import DifferentiableRobotModel, TrajectoryOptimizer, seed_trajectories, trajectory_report
    hs = GH.golden_hand()
    gpis, center = GH.banana("gpis")
    rm = DifferentiableRobotModel("allegro", device=DEV)
    G, S, T, D = 8, 4, 16, hs.desc.n_dofs
    opt = TrajectoryOptimizer(rm, hs, T=T, m_obj=0.005, m_self=0.002, m_floor=0.01)
    rng = np.random.default_rng(31)
    lo, hi = np.array(opt.lower) + 0.04, np.array(opt.upper) - 0.04
    qs = np.clip(hs.rest_q[None], lo, hi).repeat(G, 0)
    qg = np.clip(hs.rest_q[None] + 0.3 * rng.standard_normal((G, D)), lo, hi)
    palm = np.concatenate([center[None] + rng.uniform(-0.1, 0.1, (G, 3)), rng.uniform(-H.PI, H.PI, (G, 3))], 1)
    palm = _up(np.repeat(palm, S, 0))
    floor_z = float(center[2]) - 0.05
    traj = seed_trajectories(_up(qs), _up(qg), T, S, amp=0.2, seed=4)
    assert traj.shape == (G * S, T, D)
    first = opt.optimize(traj, gpis, palm, floor_z, iters=1)
    res = opt.optimize(traj, gpis, palm, floor_z, iters=10)
    for t in (res.trajectory, res.cost, res.last, res.parts):
        assert torch.isfinite(t).all()
    assert (first.parts[:, 1] > 0).float().mean() >= 0.25  # U_c: the hand does meet the banana, itself or the floor
    assert (res.cost <= first.cost).all() and (res.cost < first.cost).any() and (res.iteration >= 0).all()
    for t in (res.trajectory, res.last):
        assert torch.equal(t[:, 0], traj[:, 0]) and torch.equal(t[:, -1], traj[:, -1])
    assert torch.equal(traj[::S, 0], _up(qs)) and torch.equal(traj[::S, -1], _up(qg))
    again = opt.optimize(traj, gpis, palm, floor_z, iters=10)
    assert torch.equal(again.trajectory, res.trajectory) and torch.equal(again.cost, res.cost)
    rep = trajectory_report(hs, res.trajectory, gpis, palm, floor_z, refine=2)
    assert rep["depth"].shape == (G * S, 3) and rep["at"].shape == (G * S, 3) and rep["clear"].dtype == torch.bool
    assert rep["within_limits"].shape == (G * S,) and rep["within_limits"].dtype == torch.bool
    assert 0 <= int(rep["at"].min()) and int(rep["at"].max()) <= (T - 1) * 2


def test_mesh_object_and_python_refusals():
    from compliancedex_amd import DifferentiableRobotModel, TrajectoryOptimizer, seed_trajectories
    hs = GH.golden_hand()
    mesh, center = GH.banana("mesh")
    rm = DifferentiableRobotModel("allegro", device=DEV)
    opt = TrajectoryOptimizer(rm, hs, T=8)
    lo, hi = np.array(opt.lower) + 0.04, np.array(opt.upper) - 0.04
    qg = np.clip(hs.rest_q + 0.3, lo, hi)
    traj = seed_trajectories(_up(hs.rest_q[None]), _up(qg[None]), 8, 3)
    palm = _up(np.concatenate([center, np.zeros(3)]))
    res = opt.optimize(traj, mesh, palm, None, iters=3)
    assert torch.isfinite(res.trajectory).all() and torch.isfinite(res.cost).all()
    none = opt.optimize(traj, None, palm, None, iters=3)
    assert torch.isfinite(none.cost).all()
    with pytest.raises(ValueError):
        opt.optimize(traj[:, :5], mesh)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.optimize(traj.cpu(), mesh)
    with pytest.raises(ValueError):
        TrajectoryOptimizer(rm, hs, T=65)
    with pytest.raises(ValueError):
        TrajectoryOptimizer(rm, hs, T=2)
