"""The minimum-wrench solve (cdx_min_wrench, compliancedex_amd.wrench) and WCKinGPISGraspOptimizer on an MI355X: the
duality-gap certificate with no row allowed to miss, the closed forms, the device against the host build, the
independence of rows and of the launch shape, status 1 and 2, the gradient, the argument checks — the assertions of
tests/test_wrench_cpu.py on the device — and the Python entry points and the optimiser on top."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _wrench as W
from tests._helpers import golden
from tests._wrench import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4  # output rows past the last, preset and found untouched


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def solve(tips, normals, **kw):
    """cdx_min_wrench through the C ABI on host arrays [E, T, 3]; GUARD rows past each output are checked to be
    untouched."""
    from compliancedex_amd import _native as N
    lib = N.load()
    tips, normals = np.ascontiguousarray(tips, np.float64), np.ascontiguousarray(normals, np.float64)
    E, T = tips.shape[:2]
    preset = W.outputs(E + GUARD, T)
    dev = {k: _dev(v, v.dtype) for k, v in preset.items()}
    par = W.params(T, **kw)
    dt, dn = _dev(tips), _dev(normals)  # (named: a temporary would be freed, and its block reused, before the launch)
    N.check(lib.cdx_min_wrench(C.byref(par), E, N.ptr(dt), N.ptr(dn),
                               *[N.ptr(dev[k]) for k in W.FIELDS], N.stream_ptr()), "cdx_min_wrench")
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    for k, v in out.items():
        assert same_bits(v[E:], preset[k][E:]), k
        out[k] = v[:E]
    return out


def rows_per_block(T=4):
    from compliancedex_amd import _native as N
    return N.load().cdx_wrench_rows_per_block(T)


_FULL = {}


def full_E():
    """Family E solved once in one call."""
    if "E" not in _FULL:
        _FULL["E"] = solve(*W.family("E"))
    return _FULL["E"]


# ------------------------------------------------------------------ 1. certificate
@pytest.mark.parametrize("name,T,kw", W.CERT_CASES, ids=[f"{n}{t}{'-'.join(map(str, k.values()))}" for n, t, k in W.CERT_CASES])
def test_certificate_every_row(name, T, kw):
    if (name, T, kw) == ("E", 4, {}):
        tips, normals = W.family("E")
        W.check_certificate(full_E(), tips, normals, report=("E", 4, {}))
    else:
        W.run_cert_case(solve, name, T, kw)


# ------------------------------------------------------------------ 2. closed forms
def test_closed_forms():
    W.check_closed_forms(solve)


# ------------------------------------------------------------------ 3. device against the host build
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_device_vs_host(name):
    """Both carry a certificate, so each is within sqrt(2·tol·max(1, P)/reg) of the unique optimum."""
    tips, normals = W.family(name)
    dev, ref = solve(tips, normals), W.solve_host(tips, normals)
    assert (dev["status"] == 0).all() and (ref["status"] == 0).all()
    P = np.maximum(W.np_primal(dev["forces"], tips, W.REG), W.np_primal(ref["forces"], tips, W.REG))
    bound = 2.0 * np.sqrt(2.0 * W.TOL * np.maximum(1.0, P) / W.REG)
    d = np.linalg.norm((dev["forces"] - ref["forces"]).reshape(len(tips), -1), axis=1)
    print(name, "largest distance / bound", float((d / bound).max()))
    assert (d <= bound).all()
    one_d = solve(tips, normals, max_iters=1, check_every=1)
    one_h = W.solve_host(tips, normals, max_iters=1, check_every=1)
    assert (one_d["iters"] == 1).all() and same_bits(one_d["iters"], one_h["iters"])
    assert same_bits(one_d["status"], one_h["status"])
    for k in ("forces", "wrench", "margin", "dual", "gap", "grad"):
        assert np.abs(one_d[k] - one_h[k]).max() <= 1e-12, k


# ------------------------------------------------------------------ 4. rows and launch shape
def test_launch_shapes():
    """A row's outputs do not depend on E nor on how the rows are split over calls."""
    L = rows_per_block()
    assert L in (1, 2, 4, 8, 16, 32, 64) and rows_per_block(8) in (1, 2, 4, 8, 16, 32, 64)
    assert rows_per_block(0) == 0 and rows_per_block(9) == 0
    tips, normals = W.family("E")
    full = full_E()
    again = solve(tips, normals)
    for k in W.FIELDS:
        assert same_bits(again[k], full[k]), k
    for E in sorted({1, 15, 16, 17, 63, 64, 65, L - 1, L, L + 1} - {0}):
        part = solve(tips[:E], normals[:E])
        for k in W.FIELDS:
            assert same_bits(part[k], full[k][:E]), (E, k)
    a, b = solve(tips[:100], normals[:100]), solve(tips[100:], normals[100:])
    for k in W.FIELDS:
        assert same_bits(np.concatenate([a[k], b[k]]), full[k]), k


def test_launch_shapes_eight_tips():
    """The 32-lane workgroup of T > 4: the same independence across its boundary."""
    L = rows_per_block(8)
    tips, normals = W.family("C", 8)
    full = solve(tips, normals)
    for E in sorted({1, L - 1, L, L + 1, 63} & set(range(1, len(tips) + 1))):
        part = solve(tips[:E], normals[:E])
        for k in W.FIELDS:
            assert same_bits(part[k], full[k][:E]), (E, k)


def test_bad_rows_stay_in_their_row():
    W.check_bad_rows(solve, group=rows_per_block())
    W.check_bad_rows(solve, group=16)


# ------------------------------------------------------------------ 5. status 1
def test_status_one():
    W.check_status_one(solve)


# ------------------------------------------------------------------ 6. gradient
def test_gradient():
    out = W.check_gradient(solve)
    from compliancedex_amd import minimum_wrench_reward, solve_minimum_wrench
    tips, normals = W.family("B")
    t = _dev(tips).requires_grad_(True)
    n = _dev(normals).requires_grad_(True)
    forces, wrench = solve_minimum_wrench(t, n, W.MU, W.FMIN)
    assert forces.shape == tips.shape and wrench.shape == (len(tips),)
    assert not forces.requires_grad and wrench.requires_grad
    coef = _dev(np.linspace(0.5, 2.0, len(tips)))
    (wrench * coef).sum().backward()
    assert n.grad is None
    assert same_bits(t.grad.cpu().numpy(), out["grad"] * coef.cpu().numpy()[:, None, None])
    assert same_bits(forces.cpu().numpy(), out["forces"]) and same_bits(wrench.detach().cpu().numpy(), out["wrench"])
    # the reference's shapes for one candidate: (forces [T, 3], scalar) and (wrench, margin [1, T], forces)
    t1 = _dev(tips[3]).requires_grad_(True)
    f1, w1 = solve_minimum_wrench(t1, _dev(normals[3]), W.MU)
    assert f1.shape == (4, 3) and w1.shape == ()
    w1.backward()
    assert same_bits(t1.grad.cpu().numpy(), out["grad"][3])
    wr, mg, fr = minimum_wrench_reward(_dev(tips[3]), _dev(normals[3]), W.MU, W.FMIN)
    assert wr.shape == () and mg.shape == (1, 4) and fr.shape == (4, 3)
    assert np.abs(mg.cpu().numpy()[0] - out["margin"][3]).max() <= 1e-12
    wr, mg, fr = minimum_wrench_reward(_dev(tips), _dev(normals), W.MU, W.FMIN)
    assert wr.shape == (len(tips),) and mg.shape == (len(tips), 4) and fr.shape == tips.shape
    assert np.abs(mg.cpu().numpy() - out["margin"]).max() <= 1e-12


def test_python_result():
    from compliancedex_amd import MinWrenchResult, min_wrench
    tips, normals = W.family("A")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res = min_wrench(_dev(tips), _dev(normals), W.MU)
    side.synchronize()
    assert isinstance(res, MinWrenchResult) and all(v.is_cuda for v in res)
    assert res.iters.dtype == res.status.dtype == torch.int32 and res.dual.shape == (len(tips), 6)
    raw = solve(tips, normals)
    for k in MinWrenchResult._fields:
        assert same_bits(getattr(res, k).detach().cpu().numpy(), raw[k]), k
    r32 = min_wrench(_dev(tips, np.float32), _dev(normals, np.float32), W.MU)  # widened, not refused
    assert r32.forces.dtype == torch.float64 and (r32.status == 0).all()


# ------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments():
    from compliancedex_amd import _native as N, min_wrench
    lib = N.load()
    tips, normals = W.family("A")
    E = len(tips)
    preset = W.outputs(E, 4)
    dev = {k: _dev(v, v.dtype) for k, v in preset.items()}
    t, n = _dev(tips), _dev(normals)

    def call(par, E=E, tips_p=N.ptr(t), drop=None):
        args = [None if k == drop else N.ptr(dev[k]) for k in W.FIELDS]
        return lib.cdx_min_wrench(C.byref(par) if par is not None else None, E, tips_p, N.ptr(n), *args, N.stream_ptr())

    assert call(None) == -1
    assert call(W.params(), E=-1) == -1
    assert call(W.params(), tips_p=None) == -1
    for k in W.FIELDS[:-1]:
        assert call(W.params(), drop=k) == -1, k
    for bad in (dict(T=0), dict(T=9), dict(mu=0.0), dict(mu=-1.0), dict(mu=float("nan")), dict(min_force=-1.0),
                dict(reg=0.0), dict(rho=0.0), dict(rho=float("inf")), dict(tol=0.0), dict(max_iters=-1),
                dict(check_every=0)):
        assert call(W.params(**bad)) == -1, bad
    assert call(W.params(), E=0, tips_p=None) == 0
    torch.cuda.synchronize()
    for k, v in preset.items():
        assert same_bits(dev[k].cpu().numpy(), v), k  # nothing was launched
    assert call(W.params(), drop="grad") == 0  # grad_tips is optional
    torch.cuda.synchronize()
    assert same_bits(dev["grad"].cpu().numpy(), preset["grad"])
    assert lib.cdx_wrench_abi_size() == C.sizeof(N.CdxWrenchParams)
    with pytest.raises(RuntimeError, match="no CPU path"):
        min_wrench(torch.from_numpy(tips), torch.from_numpy(normals), 1.0)
    with pytest.raises(ValueError):
        min_wrench(t[:, :, :2], n[:, :, :2], 1.0)
    with pytest.raises(RuntimeError, match="invalid argument"):
        min_wrench(t, n, -1.0)


# ------------------------------------------------------------------ 8. the optimiser
def _wc(iters):
    from compliancedex_amd import WCKinGPISGraspOptimizer
    from compliancedex_amd.urdf import load_robot
    cfg = load_robot("allegro")["config"]
    palm3 = golden("mode_kingpis.npz")["palm3"].tolist()
    return WCKinGPISGraspOptimizer("allegro", list(cfg["ee_link_name"]), list(cfg["ee_link_offset"]), palm_offset=palm3,
                                   num_iters=iters, ref_q=cfg["ref_q"], uncertainty=3.0), cfg


def _wc_inputs(E=3, comp=(45.0, 60.0, 80.0, 50.0)):
    from compliancedex_amd.urdf import load_robot
    rng = np.random.default_rng(0)
    q = np.asarray(load_robot("allegro")["config"]["ref_q"], np.float64) + 0.05 * rng.standard_normal((E, 16))
    center = golden("mode_gpis.npz")["center"]
    target = np.tile(center, (E, 4, 1)) + 0.003 * rng.standard_normal((E, 4, 3))
    return _dev(q), _dev(target), _dev(np.tile(np.asarray(comp), (E, 1)))


def test_wc_optimizer():
    from compliancedex_amd import min_wrench
    from compliancedex_amd.workloads import stored_gpis
    gpis = stored_gpis("banana", DEV)
    o, _ = _wc(4)
    q, target, comp = _wc_inputs()
    keep = [x.clone() for x in (q, target, comp)]
    oq, ocomp, otarget, flag = o.optimize(q, target, comp, 1.0, gpis, verbose=False, trace_rows=True)
    for x, y in zip((q, target, comp), keep):
        assert torch.equal(x, y)  # the caller's tensors are unchanged
    rows = torch.stack(o.loss_rows).cpu().numpy()
    assert rows.shape == (4, 3) and np.isfinite(rows).all() and len(o.loss_history) == 4
    assert np.allclose(torch.stack(o.loss_history).cpu().numpy(), rows.sum(1), rtol=1e-12)
    # iteration 0's losses from the public pieces
    tips = o.forward_kinematics(q).view(3, 4, 3)
    dist, var = gpis.pred(tips.reshape(-1, 3))
    tar_dist, _ = gpis.pred(target.reshape(-1, 3))
    normal = gpis.compute_normal(tips.reshape(-1, 3)).view(3, 4, 3)
    res = min_wrench(tips, normal, 1.0, min_force=5.0)
    assert (res.status == 0).all()
    fn = res.forces.norm(dim=2)
    force_cost = -(fn * torch.softmax(-fn, dim=1)).clamp(max=1.0).sum(dim=1)
    l0 = (5.0 * res.wrench + 1000 * dist.abs().view(3, 4).sum(1) + 10 * tar_dist.view(3, 4).sum(1) +
          10.0 * (tips.mean(1) - target.mean(1)).norm(dim=1) + force_cost + 20.0 * (q - o.ref_q).norm(dim=1) +
          (20 * torch.log(100 * var)).view(3, 4).max(dim=1)[0])
    l0 = l0.cpu().numpy()
    assert (np.abs(rows[0] - l0) <= 1e-9 * np.abs(l0)).all(), (rows[0], l0)
    # the best iterate: target = tip + forces / compliance of that iteration; compliance ≥ 40; the flag
    best_it = rows.argmin(0)
    assert same_bits(o.best_loss.cpu().numpy(), rows.min(0))
    for e in range(3):
        r = o.wrench_rows[best_it[e]]
        assert int(r.status[e]) == 0
        assert torch.equal(oq[e], q[e]) == (best_it[e] == 0)
        tips_best = o.forward_kinematics(oq[e:e + 1]).view(4, 3)
        assert torch.equal(otarget[e], tips_best + r.forces[e] / ocomp[e].unsqueeze(1))
        assert torch.equal(ocomp[e], comp[e])  # (≥ 40 as given, and no gradient reaches the compliance)
    assert (ocomp >= 40.0).all()
    before = np.minimum.accumulate(np.vstack([np.full(3, np.inf), rows]), 0)  # the best losses before iteration s
    improved = [s for s in range(4) if (rows[s] < before[s]).any()]
    assert bool(flag) == bool((o.wrench_rows[improved[-1]].margin > 0).all())
    # E = 1 against the same row inside E = 3: no coupling between candidates
    for e in (0, 2):
        o1, _ = _wc(4)
        q1, c1, t1, _ = o1.optimize(q[e:e + 1], target[e:e + 1], comp[e:e + 1], 1.0, gpis, verbose=False, trace_rows=True)
        assert torch.equal(q1[0], oq[e]) and torch.equal(c1[0], ocomp[e]) and torch.equal(t1[0], otarget[e])
        assert same_bits(torch.stack(o1.loss_rows).cpu().numpy()[:, 0], rows[:, e])


def test_wc_optimizer_keeps_a_low_compliance_of_iteration_zero():
    """The reference's clamp acts after the step, so a best iterate found at iteration 0 returns the compliance as
    given, and any later one a compliance ≥ 40 (:603-607)."""
    from compliancedex_amd.workloads import stored_gpis
    gpis = stored_gpis("banana", DEV)
    o, _ = _wc(3)
    q, target, comp = _wc_inputs(comp=(10.0, 10.0, 10.0, 20.0))
    _, ocomp, _, _ = o.optimize(q, target, comp, 1.0, gpis, verbose=False, trace_rows=True)
    best_it = torch.stack(o.loss_rows).argmin(0)
    for e in range(3):
        assert torch.equal(ocomp[e], comp[e] if best_it[e] == 0 else comp[e].clamp(min=40.0))
