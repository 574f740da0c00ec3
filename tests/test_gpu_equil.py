"""The disturbance-load test (cdx_grasp_equilibrium, cdx_equil_reduce, compliancedex_amd.stability) on an MI355X: the
assertions of tests/test_equil_cpu.py on the device through the C ABI with guard items past every output, the device
against the host build bit for bit on every output, and the Python entry points on top."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _equil as Q
from tests._equil import same_bits
from tests._helpers import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4  # output items (rows, for the reduction) past the last, preset and found untouched


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def solve(contact, target, k, normal, f, c, **kw):
    """cdx_grasp_equilibrium through the C ABI on host arrays → item-major dict of Q.FIELDS."""
    from compliancedex_amd import _native as N
    lib = N.load()
    a, E, W, T, shared = Q.as_inputs(contact, target, k, normal, f, c)
    n = E * W
    preset = Q.outputs(n + GUARD, T)
    dev = {name: _dev(v, v.dtype) for name, v in preset.items()}
    ins = [_dev(x) for x in a]  # (named: a temporary would be freed, and its block reused, before the launch)
    par = Q.params(T, **kw)
    N.check(lib.cdx_grasp_equilibrium(C.byref(par), E, W, *[N.ptr(x) for x in ins], int(shared),
                                      *[N.ptr(dev[name]) for name in Q.FIELDS], N.stream_ptr()), "cdx_grasp_equilibrium")
    out = {name: v.cpu().numpy() for name, v in dev.items()}
    for name, v in out.items():
        assert same_bits(v[n:], preset[name][n:]), name
        out[name] = v[:n]
    return out


def reduce(out, E, W, T, **lim):
    """cdx_equil_reduce through the C ABI on item-major host arrays → dict of Q.RED_FIELDS."""
    from compliancedex_amd import _native as N
    lib = N.load()
    preset = Q.reduce_outputs(E + GUARD)
    dev = {name: _dev(v, v.dtype) for name, v in preset.items()}
    ins = [_dev(out[name], out[name].dtype) for name in ("margin", "normal_force", "shift", "chord", "stable", "status")]
    lm = Q.limits(**lim)
    N.check(lib.cdx_equil_reduce(C.byref(lm), E, W, T, *[N.ptr(x) for x in ins],
                                 *[N.ptr(dev[name]) for name in Q.RED_FIELDS], N.stream_ptr()), "cdx_equil_reduce")
    red = {name: v.cpu().numpy() for name, v in dev.items()}
    for name, v in red.items():
        assert same_bits(v[E:], preset[name][E:]), name
        red[name] = v[:E]
    return red


# ------------------------------------------------------------------ 1. certificate
def test_certificate_from_the_outputs_alone():
    out = Q.check_certificate(solve, report="device")
    pts, tgt, k, nrm = Q.family("shallow", 37, 4)
    ref = Q.solve_host(pts, tgt, k, nrm, *Q.loads(pts, k, 26, 1.0))
    for name in Q.FIELDS:
        assert same_bits(out[name], ref[name]), name


# ------------------------------------------------------------------ 2. closed forms
def test_closed_form_tetrahedron():
    got = Q.closed_a_error(solve)
    print("tetrahedron: device", got, "allowed", Q.CLOSED_A_TOL)
    assert got <= Q.CLOSED_A_TOL


def test_closed_form_weighted_kabsch():
    got = Q.closed_b_error(solve, "device")
    print("Kabsch: device", got, "allowed", Q.CLOSED_B_TOL)
    assert got <= Q.CLOSED_B_TOL


# ------------------------------------------------------------------ 3. one iteration against numpy
def test_one_iteration_against_numpy():
    Q.check_one_iteration(solve, report="device to numpy, one iteration:")


def test_converged_against_numpy():
    Q.check_converged_against_numpy(solve)


def test_no_stall_at_the_default_tolerance():
    Q.check_no_stall(solve)


# ------------------------------------------------------------------ 4. the device equals the host build
SHAPES = [(1, 1), (3, 26), (5, 64), (2, 129)]  # items below a wave, across a wave, across several workgroups


@pytest.mark.parametrize("T", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("name", ["shallow", "deep"])
def test_device_equals_host_bit_for_bit(name, T):
    rejected = 0
    for E, W in SHAPES:
        pts, tgt, k, nrm = Q.family(name, E, T)
        for shared in (False, True):
            f, c = Q.loads(pts, k, W, (0.0, 4.0), shared=shared)
            dev, ref = solve(pts, tgt, k, nrm, f, c), Q.solve_host(pts, tgt, k, nrm, f, c)
            for fld in Q.FIELDS:
                assert same_bits(dev[fld], ref[fld]), (E, W, shared, fld)
            assert np.isin(dev["status"], (0, 1)).all()
            rejected += int((dev["iters"] > 8).sum())
    print(name, T, "items beyond 8 iterations", rejected)


# ------------------------------------------------------------------ 5. independence
def test_independence():
    Q.check_independence(solve)


# ------------------------------------------------------------------ 6. statuses
def test_statuses():
    Q.check_statuses(solve)


# ------------------------------------------------------------------ 7. reduction
def test_reduction():
    Q.check_reduction(reduce)


def test_reduction_across_workgroups():
    """More rows than one workgroup of the reduction, from a real solve whose loads make both verdicts occur."""
    E, W, T = 131, 6, 4
    pts, tgt, k, nrm = Q.family("firm", E, T)
    f, c = Q.loads(pts, k, W, (0.1, 4.0))
    out = solve(pts, tgt, k, nrm, f, c)
    red, ref = reduce(out, E, W, T), Q.np_reduce(out, E, W, T)
    for name in Q.RED_FIELDS:
        assert same_bits(red[name], ref[name]), name
    assert 0 < red["n_failed"].sum() < E * W


# ------------------------------------------------------------------ 8. the Python layer
def _case(E=9, W=None, mag=(0.1, 4.0)):
    pts, tgt, k, nrm = Q.family("firm", E, 4)
    f, c = Q.loads(pts, k, W or 7, mag)
    return pts, tgt, k, nrm, f, c


def test_disturbance_report_against_the_c_abi():
    from compliancedex_amd import DisturbanceReport, EquilibriumResult, disturbance_report, grasp_equilibrium
    pts, tgt, k, nrm, f, c = _case()
    E, W, T = 9, 7, 4
    raw = solve(pts, tgt, k, nrm, f, c)
    lim = dict(max_shift=0.01, margin_min=0.05)
    red = reduce(raw, E, W, T, **lim)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rep = disturbance_report(_dev(pts), _dev(tgt), _dev(k), _dev(nrm), Q.MU, _dev(f), _dev(c), **lim)
    side.synchronize()
    assert isinstance(rep, DisturbanceReport) and isinstance(rep.result, EquilibriumResult)
    assert rep.holds.dtype == torch.bool and rep.result.stable.dtype == torch.bool and rep.result.rot.shape == (E, W, 3, 3)
    for name in Q.FIELDS:
        got = getattr(rep.result, name)
        got = got.to(torch.uint8) if name == "stable" else got
        assert same_bits(got.cpu().numpy().reshape(raw[name].shape), raw[name]), name
    for name in Q.RED_FIELDS:
        got = getattr(rep, name)
        got = got.to(torch.uint8) if name == "holds" else got
        assert same_bits(got.cpu().numpy(), red[name]), name
    assert 0 < int(rep.n_failed.sum()) < E * W
    # loads shared by every row, placed at a centre of mass, and float32 inputs widened rather than refused
    fs, _ = Q.loads(pts, k, 5, 2.0, shared=True)
    com = np.array([0.004, -0.002, 0.001])
    res = grasp_equilibrium(_dev(pts, np.float32), _dev(tgt, np.float32), _dev(k, np.float32), _dev(nrm, np.float32),
                            Q.MU, fs, com=com)
    pts32, tgt32, k32, nrm32 = (x.astype(np.float32).astype(np.float64) for x in (pts, tgt, k, nrm))
    raw = solve(pts32, tgt32, k32, nrm32, fs, np.tile(com, (5, 1)))
    assert res.force.dtype == torch.float64 and same_bits(res.force.cpu().numpy().reshape(raw["force"].shape), raw["force"])
    # no load point and no centre of mass: the stiffness centre of each grasp
    res = grasp_equilibrium(_dev(pts), _dev(tgt), _dev(k), _dev(nrm), Q.MU, fs)
    raw = solve(pts, tgt, k, nrm, np.tile(fs, (E, 1, 1)), np.tile(Q.centre(pts, k)[:, None], (1, 5, 1)))
    assert np.abs(res.trans.cpu().numpy().reshape(-1, 3) - raw["trans"]).max() <= 1e-12  # (torch's own sum for the centre)
    assert not res.force.requires_grad


def test_load_directions_on_the_device_path():
    from compliancedex_amd import gravity_loads, load_directions
    d = load_directions(26)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-15
    assert (d @ d.T - 2.0 * np.eye(26)).max() < 1.0 - 1e-6  # distinct
    force, point = gravity_loads(0.4, directions=26, com=(0.0, 0.0, 0.01))
    assert force.shape == (26, 3) and point == (0.0, 0.0, 0.01)


def test_max_payload():
    """Eight grasps that hold 1 N and not 8 N in 14 directions, then four that do not hold unloaded."""
    from compliancedex_amd import disturbance_report, load_directions, max_payload
    firm, loose = Q.family("firm", 8, 4), Q.family("shallow", 12, 4)
    a = [_dev(np.concatenate([x, y[:4]])) for x, y in zip(firm, loose)]
    hi, steps = 16.0, 6
    res = max_payload(*a, Q.MU, directions=14, hi=hi, steps=steps)
    payload, upper = res.payload.cpu().numpy(), res.upper.cpu().numpy()
    d = load_directions(14)
    live = ~np.isnan(payload)
    assert live.tolist() == [True] * 8 + [False] * 4 and (upper[~live] == 0).all()
    assert (payload[live] >= 1.0).all() and (payload[live] < 8.0).all()
    assert same_bits((upper - payload)[live], np.full(8, hi / 2 ** steps))
    at = disturbance_report(*a, Q.MU, _dev(np.nan_to_num(payload)[:, None, None] * d[None])).holds.cpu().numpy()
    above = disturbance_report(*a, Q.MU, _dev(upper[:, None, None] * d[None])).holds.cpu().numpy()
    assert at[live].all()  # the returned magnitude holds
    assert not above[live].any()  # one bisection interval above it fails
    assert not at[~live].any()  # (those loads are zero: the rows do not hold unloaded)
    # a ceiling below what they hold: the answer is the ceiling, and it holds
    low = max_payload(*a, Q.MU, directions=d, hi=1.0, steps=3)
    assert (low.payload.cpu().numpy()[:8] == 1.0).all() and (low.upper.cpu().numpy()[:8] == 1.0).all()
    assert disturbance_report(*a, Q.MU, _dev(d)).holds.cpu().numpy()[:8].all()


def test_robustness_for_results_on_the_stored_lego_grasps(tmp_path):
    from compliancedex_amd.results import load_results, robustness_for_results, save_results
    from compliancedex_amd.workloads import stored_gpis
    d = golden("results_lego.npz")
    save_results("lego", d["contact"], d["target"], d["wrist"], d["compliance"], d["joint_angle"], data_dir=str(tmp_path))
    gpis = stored_gpis("lego", DEV)
    rep = robustness_for_results(None, gpis, 1.0, 0.1, exp_name="lego", data_dir=str(tmp_path), device=DEV)
    E, T = d["contact"].shape[:2]
    assert rep.holds.shape == (E,) and rep.result.margin.shape == (E, 26, T)
    status = rep.result.status.cpu().numpy()
    assert np.isin(status, (0, 1)).all()
    # the same numbers from the pieces: the normals of the GPIS at the contacts, 26 weights of 0.1 kg
    nrm = gpis.compute_normal(_dev(d["contact"]).reshape(-1, 3)).reshape(E, T, 3).cpu().numpy().astype(np.float64)
    from compliancedex_amd import gravity_loads
    f, _ = gravity_loads(0.1)
    raw = solve(d["contact"], d["target"], d["compliance"], nrm, np.tile(f, (E, 1, 1)),
                np.tile(Q.centre(d["contact"], d["compliance"])[:, None], (1, 26, 1)))
    assert same_bits(status.reshape(-1), raw["status"])
    assert np.abs(rep.result.margin.cpu().numpy().reshape(-1, T) - raw["margin"]).max() <= 1e-9
    same = robustness_for_results(load_results("lego", str(tmp_path)), gpis, 1.0, 0.1, com=None, device=DEV)
    assert same_bits(same.worst_margin.cpu().numpy(), rep.worst_margin.cpu().numpy())
    print("lego, 0.1 kg:", "holds", rep.holds.cpu().numpy().tolist(), "worst margin",
          rep.worst_margin.cpu().numpy().round(3).tolist(), "max shift", rep.max_shift.cpu().numpy().round(4).tolist())


def test_cpu_tensors_and_bad_arguments():
    from compliancedex_amd import _native as N, disturbance_report, grasp_equilibrium, max_payload
    lib = N.load()
    pts, tgt, k, nrm, f, c = _case(E=2)
    E, W, T = 2, 7, 4
    preset = Q.outputs(E * W, T)
    dev = {name: _dev(v, v.dtype) for name, v in preset.items()}
    ins = [_dev(x) for x in (pts, tgt, k, nrm, f, c)]

    def call(par, E=E, W=W, drop_in=None, drop_out=None):
        a = [None if i == drop_in else N.ptr(x) for i, x in enumerate(ins)]
        o = [None if n == drop_out else N.ptr(dev[n]) for n in Q.FIELDS]
        return lib.cdx_grasp_equilibrium(C.byref(par) if par is not None else None, E, W, *a, 0, *o, N.stream_ptr())
    assert call(None) == -1 and call(Q.params(T), E=-1) == -1 and call(Q.params(T), W=-1) == -1
    for i in range(6):
        assert call(Q.params(T), drop_in=i) == -1, i
    for n in Q.FIELDS[3:]:
        assert call(Q.params(T), drop_out=n) == -1, n
    for bad in (dict(T=0), dict(T=9), dict(mu=0.0), dict(mu=float("nan")), dict(tol=0.0), dict(tol=float("inf")),
                dict(max_iters=-1), dict(mu0=0.0), dict(mu_min=-1.0), dict(mu_max=float("nan")), dict(nu=0.0)):
        assert call(Q.params(**{"T": T, **bad})) == -1, bad
    assert call(Q.params(T), E=0, drop_in=0) == 0 and call(Q.params(T), W=0, drop_in=4) == 0
    assert call(Q.params(T), E=1 << 40, W=1 << 40) == -1
    red = {n: _dev(v, v.dtype) for n, v in Q.reduce_outputs(E).items()}
    items = [dev[n] for n in ("margin", "normal_force", "shift", "chord", "stable", "status")]

    def red_call(lim=Q.limits(), E=E, W=W, T=T, drop=None):
        a = [None if i == drop else N.ptr(x) for i, x in enumerate(items + [red[n] for n in Q.RED_FIELDS])]
        return lib.cdx_equil_reduce(C.byref(lim) if lim is not None else None, E, W, T, *a, N.stream_ptr())
    assert red_call(None) == -1 and red_call(E=-1) == -1 and red_call(W=-1) == -1 and red_call(T=0) == -1
    assert red_call(T=9) == -1 and red_call(E=0, drop=0) == 0 and red_call(W=0, drop=0) == 0
    for i in range(13):
        assert red_call(drop=i) == -1, i
    torch.cuda.synchronize()
    for n, v in preset.items():
        assert same_bits(dev[n].cpu().numpy(), v), n  # nothing was launched
    for n, v in Q.reduce_outputs(E).items():
        assert same_bits(red[n].cpu().numpy(), v), n
    for n in Q.FIELDS[:3]:  # rot, trans, force are optional: skipped, the others written
        assert call(Q.params(T), drop_out=n) == 0
    torch.cuda.synchronize()
    full = solve(pts, tgt, k, nrm, f, c)
    for n in Q.FIELDS[3:]:
        assert same_bits(dev[n].cpu().numpy(), full[n]), n
    sizes = (C.c_size_t * 2)()
    lib.cdx_equil_abi_sizes(sizes)
    assert list(sizes) == [C.sizeof(N.CdxEquilParams), C.sizeof(N.CdxEquilLimits)]
    a = [_dev(x) for x in (pts, tgt, k, nrm)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        grasp_equilibrium(*[torch.from_numpy(x.copy()) for x in (pts, tgt, k, nrm)], 1.0, f)
    with pytest.raises(ValueError):
        grasp_equilibrium(a[0][:, :, :2], *a[1:], 1.0, f)
    with pytest.raises(ValueError):
        grasp_equilibrium(*a, 1.0, f[:1])  # loads of another row count
    with pytest.raises(ValueError):
        grasp_equilibrium(*a, 1.0, f, c[:, :3])
    with pytest.raises(RuntimeError, match="invalid argument"):
        grasp_equilibrium(*a, -1.0, f)
    with pytest.raises(RuntimeError, match="invalid argument"):
        disturbance_report(*a, 1.0, f, tol=0.0)
    with pytest.raises(TypeError):
        disturbance_report(*a, 1.0, f, max_tilt=0.1)
    with pytest.raises(ValueError):
        max_payload(*a, 1.0, hi=-1.0)
