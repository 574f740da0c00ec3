"""cdx_hand_term on an MI355X and the ``hand_term=`` keyword of the joint-space optimisers.

Kernel: tests/_hand_term.py's checks through the C ABI on the device (the term against cdx_hand_cost followed by
cdx_hand_pullback and against numpy's old + (weight · x), bit for bit; batch sizes, positions, non-finite neighbours,
guard rows, refusals) and the device against the host build, bit for bit.

Loops: Allegro (the recorded 87 spheres), the packaged banana GPIS (N = 361), E = 70, 4 iterations on a fixed Kabsch
noise tape.  Iteration 0's loss rows and joint gradient with the term are those without it plus weight ·
hand_collision(...) at the initial pose; fused equals eager at the tolerances of the optimisers' own fused-versus-eager
tests (KinGPIS: test_gpu_gpis_mode.TOL; prob mode: test_gpu_parity.test_optimize_vs_reference's 1e-6 on the losses and
5e-6 on the outputs, which both of its paths meet against the reference); a captured prob loop equals the eager one bit
for bit; a NaN joint row stays in its row; KinGraspOptimizer's fused loop refuses the term.

Tolerance of the iteration-0 identity: |with − (without + term)| ≤ 1e-12·(|without| + |term|), per row for the loss
(the issue's), per row in the max-norm for the gradient rows (a gradient entry is a signed sum over up to 87 spheres
whose rounding scales with the row's terms, not with the entry).  KinGraspOptimizer's loop is float32: its bound is
2⁻²³·(|without| + |term|), one rounding of the term to float32 and one of the sum.
"""
import os

import numpy as np
import pytest
import torch

from tests import _chains, _hand as H, _hand_term as T
from tests import test_gpu_gpis_mode as G
from tests import test_gpu_hand as GH
from tests._helpers import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_LOOP, ITERS = 70, 4
# (penetrations are centimetres, so ½·p² is 1e-4: a weight of 2e4 puts the term at the size of the loops' own terms —
# with a weight near 1 it would sit below the tolerances of the fused-versus-eager comparisons)
KW = dict(weight=2.0e4, m_obj=0.02, m_self=0.01, m_floor=0.01, w_obj=2.0, w_self=3.0, w_floor=0.5)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


# ------------------------------------------------------------------ the kernel
def dev_term(chain, hand, par, E, poses, centers, dist, gdist, po, weight, accumulate, outs):
    from compliancedex_amd import _native as N
    lib = N.load()
    d = lambda a: None if a is None else torch.tensor(a, device=DEV)  # noqa: E731
    ins = [d(a) for a in (poses, centers, dist, gdist, po)]
    dev_outs = {k: d(v) for k, v in outs.items()}
    rc = lib.cdx_hand_term(chain, hand, par, E, *[N.ptr(t) for t in ins], weight, accumulate,
                           *[N.ptr(dev_outs.get(k)) for k in T.OUTS], N.stream_ptr())
    torch.cuda.synchronize()
    for k, t in dev_outs.items():
        outs[k][...] = t.cpu().numpy()
    return rc


class DevBackend:
    spheres = staticmethod(GH.dev_spheres)
    cost = staticmethod(GH.dev_cost)
    pullback = staticmethod(GH.dev_pullback)
    model = staticmethod(lambda hs: hs.native())
    term = staticmethod(dev_term)


@pytest.mark.parametrize("case,S,pairs", T.FAMILIES, ids=T.IDS)
def test_term_is_the_pair_and_the_output_rule(case, S, pairs):
    T.check_values(DevBackend, T.fam(case, S, pairs))


@pytest.mark.parametrize("case,S,pairs", T.FAMILIES, ids=T.IDS)
def test_device_equals_host_build(case, S, pairs):
    """The same poses (the device's own), centres and distances through cdx_hand_term and cdxh_hand_term, at weight 1
    and accumulating at 0.37 on the same random presets: every output bit for bit."""
    f = T.fam(case, S, pairs)
    hs, par, E = f["hs"], H.params_struct(), H.E_MAX
    poses = GH.dev_spheres(hs, f["q"], f["palm"])[0]
    inp = (poses, f["centers"], f["dist"], f["gdist"], f["palm"][:, 3:])
    pre = T.presets(hs, E, seed=9)
    for kw in (dict(), dict(weight=T.WEIGHT, accumulate=1, preset=pre)):
        T.same(T.good(DevBackend, hs, par, E, *inp, **kw), T.good(T.HostBackend, hs, par, E, *inp, **kw), tag=str(kw.keys()))


@pytest.mark.parametrize("case,S,pairs", T.FAMILIES[:3], ids=T.IDS[:3])
def test_rows_stay_in_their_row(case, S, pairs):
    T.check_rows(DevBackend, T.fam(case, S, pairs))


def test_refusals_leave_the_outputs_untouched():
    T.check_refusals(DevBackend, T.fam("hand8", 63, "full"), H.family("tree8", 65, "one")["hs"],
                     _chains.raw_descriptor(_chains.line(17), ["b17"]))


# ------------------------------------------------------------------ the loops
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _hand():
    if "hand" not in _CACHE:
        _CACHE["hand"] = GH.golden_hand()
    return _CACHE["hand"]


def _term(**over):
    from compliancedex_amd import HandTerm
    from compliancedex_amd.workloads import surface_center
    floor_z = float(surface_center(G._banana())[2]) - 0.05
    return HandTerm(_hand(), floor_z=floor_z, **dict(KW, **over))


def _statement(term, q, palm):
    """weight · hand_collision at (q, palm) through autograd → (term [E], ∂/∂q, ∂/∂palm) as numpy float64."""
    qq = q.detach().double().clone().requires_grad_(True)
    pl = palm.detach().double().clone().requires_grad_(True)
    t = term.cost(qq, pl, G._banana())
    t.sum().backward()
    return t.detach().cpu().numpy(), qq.grad.cpu().numpy(), pl.grad.cpu().numpy()


def _identity(tag, with_, without, term, tol=1e-12, rowwise=False):
    a, b = np.asarray(without, np.float64), np.asarray(term, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    if rowwise:
        fin = fin.all(1, keepdims=True) & np.ones_like(fin)
        bound = tol * (np.abs(np.where(fin, a, 0)).max(1, keepdims=True) + np.abs(np.where(fin, b, 0)).max(1, keepdims=True))
        bound = np.broadcast_to(bound, a.shape)
    else:
        bound = tol * (np.abs(a) + np.abs(b))
    err = np.abs(np.asarray(with_, np.float64) - (a + b))
    print(tag, "worst |Δ| / bound", float((err[fin] / np.maximum(bound[fin], 1e-300)).max()), "rows", int(fin.sum()))
    assert fin.sum() >= 0.9 * fin.size and (err[fin] <= bound[fin]).all(), tag
    assert np.array_equal(np.isfinite(np.asarray(with_, np.float64)), np.isfinite(a + b)), tag


def _report_ok(rep, E):
    assert {"depth", "worst", "clear"} <= set(rep)
    assert rep["depth"].shape == (E, 3) and rep["worst"].shape == (E, 3) and rep["clear"].shape == (E,)
    assert rep["depth"].is_cuda and rep["clear"].dtype == torch.bool


def _kingpis(E, iters, term, fused, q=None, keep=True):
    """One KinGPIS call on test_gpu_gpis_mode's inputs → dict(rows, out, best, g, report, q0, palm)."""
    from compliancedex_amd.hand import palm_rows
    o = G._make("kingpis", iters)
    o._keep_loop_state = keep
    pose, target, comp = G._inputs("kingpis", E)
    if q is not None:
        pose = q
    out = o.optimize(pose, target, comp, 1, G._banana(), verbose=False, kabsch_noise=G._noise(E, iters), trace_rows=True,
                     fused=fused, hand_term=term)
    st = getattr(o, "_loop_state", None)
    return dict(rows=torch.stack(o.loss_rows).cpu().numpy(), out=[x.detach().cpu().numpy() for x in out[:3]],
                best=o.best_loss.cpu().numpy(), g=None if st is None else st.g[0].cpu().numpy(),
                report=o.last_hand_report, q0=pose, palm=palm_rows(o.palm_offset, E))


def _kingpis_cached(E, iters, with_term, fused):
    key = ("kingpis", E, iters, with_term, fused)
    if key not in _CACHE:
        _CACHE[key] = _kingpis(E, iters, _term() if with_term else None, fused)
    return _CACHE[key]


def test_kingpis_iteration_0_is_the_sum():
    """Fused, one iteration: the loss rows and the kept joint gradient with the term against those without plus the
    statement; at least a quarter of the rows start with a positive hand cost."""
    a, b = _kingpis_cached(E_LOOP, 1, True, True), _kingpis_cached(E_LOOP, 1, False, True)
    t, gq, _ = _statement(_term(), a["q0"], a["palm"])
    assert (t[np.isfinite(t)] > 0).mean() >= 0.25, (t > 0).mean()
    _identity("kingpis fused loss", a["rows"][0], b["rows"][0], t)
    _identity("kingpis fused g_q", a["g"], b["g"], gq, rowwise=True)
    _report_ok(a["report"], E_LOOP)
    assert b["report"] is None


def test_kingpis_eager_iteration_0_is_the_sum():
    a, b = _kingpis(E_LOOP, 1, _term(), False), _kingpis(E_LOOP, 1, None, False)
    t, _, _ = _statement(_term(), a["q0"], a["palm"])
    _identity("kingpis eager loss", a["rows"][0], b["rows"][0], t)
    _report_ok(a["report"], E_LOOP)


def test_kingpis_fused_equals_eager_with_the_term():
    """E = 70, 4 iterations: test_gpu_gpis_mode._compare_paths' assertions at its KinGPIS tolerance."""
    a, b = _kingpis_cached(E_LOOP, ITERS, True, True), _kingpis(E_LOOP, ITERS, _term(), False)
    tol = G.TOL["kingpis"]
    assert a["rows"].shape == b["rows"].shape == (ITERS, E_LOOP)
    for s in range(ITERS):
        fin = np.isfinite(b["rows"][s])
        assert np.array_equal(np.isfinite(a["rows"][s]), fin) and np.array_equal(fin, G._finite_mask(E_LOOP)), s
        err = np.abs(a["rows"][s][fin] - b["rows"][s][fin]).max() / np.abs(b["rows"][s][fin]).max()
        print("kingpis iteration", s, "loss err", err)
        assert err <= tol, (s, err)
    for i, (x, y) in enumerate(zip(a["out"], b["out"])):
        err = rel_err(x, y)
        print("kingpis out", i, err)
        assert err < tol, i
    fin = np.isfinite(b["best"])
    assert np.array_equal(np.isfinite(a["best"]), fin) and rel_err(a["best"][fin], b["best"][fin]) < tol
    # the term is in the loop: the losses differ from the run without it from iteration 0 on
    assert not np.allclose(a["rows"][0][fin], _kingpis_cached(E_LOOP, 1, False, True)["rows"][0][fin], rtol=1e-9)


def test_kingpis_nan_joint_row_stays_in_its_row():
    """E = 65, one joint of row 5 NaN: every other row's returned q, target and compliance have the clean run's bits."""
    E = 65
    pose = G._inputs("kingpis", E)[0]
    bad = pose.clone()
    bad[5, 2] = float("nan")
    a = _kingpis(E, ITERS, _term(), True, q=pose)
    b = _kingpis(E, ITERS, _term(), True, q=bad)
    rows = np.arange(E) != 5
    for x, y in zip(a["out"], b["out"]):
        assert H.same_bits(x[rows], y[rows])
    assert H.same_bits(a["rows"][:, rows], b["rows"][:, rows])
    assert not np.isfinite(b["rows"][:, 5]).any() and np.isfinite(a["rows"][:, 5]).all()


def _prob(E, iters, term, fused, graph=False, tape=True, calls=1):
    """ProbabilisticGraspOptimizer on workloads.prob_inputs → per call dict(out, total_loss, best, steps, report)."""
    from compliancedex_amd import ProbabilisticGraspOptimizer
    from compliancedex_amd.urdf import load_robot
    from compliancedex_amd.workloads import prob_inputs
    cfg = load_robot("allegro")["config"]
    q, comp, target, palm = prob_inputs(cfg["ref_q"], E, seed=11, spread=True)
    opt = ProbabilisticGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"], ref_q=cfg["ref_q"],
                                      optimize_target=True, optimize_palm=True, num_iters=iters, device=DEV,
                                      palm_offset=palm)
    rng = np.random.default_rng(12)
    noise = [_dev(rng.random((3 * E, 3, 3))) for _ in range(iters)] if tape else None
    res = []
    for call in range(calls):
        steps = []

        def hook(s, out, state):
            steps.append({k: out[k].cpu().numpy().copy() for k in ("total_loss", "g_q", "g_palm_pos", "g_palm_ori")})
        kw = dict(step_hook=hook) if fused and not graph else {}
        out = opt.optimize(_dev(q) + 0.01 * call, _dev(target), _dev(comp), 1, G._banana(), verbose=False, noise_tape=noise,
                           fused=fused, graph=graph, hand_term=term, **kw)
        res.append(dict(out=[x.detach().cpu().numpy() for x in out], total_loss=opt.total_loss.detach().cpu().numpy(),
                        best=opt.best_loss.cpu().numpy(), steps=steps, report=opt.last_hand_report))
    return res, _dev(q), _dev(palm)


def test_prob_iteration_0_is_the_sum():
    """Fused, through step_hook: iteration 0's total_loss, g_q and palm gradients with the term against those without
    plus the statement at the initial joints and palm poses."""
    (a,), q, palm = _prob(E_LOOP, 1, _term(), True)
    (b,), _, _ = _prob(E_LOOP, 1, None, True)
    t, gq, gp = _statement(_term(), q, palm)
    assert (t > 0).mean() >= 0.25, (t > 0).mean()
    sa, sb = a["steps"][0], b["steps"][0]
    _identity("prob loss", sa["total_loss"], sb["total_loss"], t)
    _identity("prob g_q", sa["g_q"], sb["g_q"], gq, rowwise=True)
    _identity("prob g_palm_pos", sa["g_palm_pos"], sb["g_palm_pos"], gp[:, :3], rowwise=True)
    _identity("prob g_palm_ori", sa["g_palm_ori"], sb["g_palm_ori"], gp[:, 3:], rowwise=True)
    _report_ok(a["report"], E_LOOP)
    assert b["report"] is None


def test_prob_fused_equals_eager_with_the_term():
    """4 iterations on one noise tape: the last iteration's per-candidate loss (term included; it depends on every step
    before it) to 1e-6 of the largest, the returned tensors to 5e-6 — test_optimize_vs_reference's bounds."""
    (a,), _, _ = _prob(E_LOOP, ITERS, _term(), True)
    (b,), _, _ = _prob(E_LOOP, ITERS, _term(), False)
    err = np.abs(a["total_loss"] - b["total_loss"]).max() / np.abs(b["total_loss"]).max()
    print("prob last loss err", err)
    assert np.isfinite(b["total_loss"]).all() and err <= 1e-6
    for i, (x, y) in enumerate(zip(a["out"], b["out"])):
        print("prob out", i, rel_err(x, y))
        assert rel_err(x, y) < 5e-6, i
    _report_ok(b["report"], E_LOOP)
    (c,), _, _ = _prob(E_LOOP, ITERS, None, True)
    assert np.abs(a["total_loss"] - c["total_loss"]).max() > 1e-6 * np.abs(c["total_loss"]).max()  # the term acts


def test_prob_graph_equals_eager_with_the_term():
    """The captured loop (on-device noise, so no tape) against the eager launches, on the capturing call and on a
    replay with new inputs: bit for bit; a loop captured without the term is another cache entry."""
    ra, _, _ = _prob(E_LOOP, ITERS, _term(), True, graph=False, tape=False, calls=2)
    rb, _, _ = _prob(E_LOOP, ITERS, _term(), True, graph=True, tape=False, calls=2)
    for a, b in zip(ra, rb):
        for x, y in zip(a["out"] + [a["total_loss"], a["best"]], b["out"] + [b["total_loss"], b["best"]]):
            assert H.same_bits(x, y)
    rc, _, _ = _prob(E_LOOP, ITERS, None, True, graph=True, tape=False, calls=1)
    assert not H.same_bits(rc[0]["total_loss"], rb[0]["total_loss"])


def test_prob_graph_cache_key_includes_the_term():
    from compliancedex_amd import ProbabilisticGraspOptimizer
    from compliancedex_amd.urdf import load_robot
    from compliancedex_amd.workloads import prob_inputs
    cfg = load_robot("allegro")["config"]
    E = 6
    q, comp, target, palm = prob_inputs(cfg["ref_q"], E, seed=3, spread=True)
    opt = ProbabilisticGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"], ref_q=cfg["ref_q"],
                                      num_iters=2, device=DEV, palm_offset=palm)
    for term in (None, _term(), _term(weight=0.5), _term()):
        opt.optimize(_dev(q), _dev(target), _dev(comp), 1, G._banana(), verbose=False, graph=True, hand_term=term)
    assert len(opt._graphs) == 3


def test_kin_fused_refuses_the_term_and_eager_takes_it():
    """KinGraspOptimizer: fused=True with a term raises; fused=False adds it (float32 loop: 2⁻²³·(|a| + |b|))."""
    from compliancedex_amd import KinGraspOptimizer, TriangleMesh
    from compliancedex_amd.hand import palm_rows
    from compliancedex_amd.urdf import load_robot
    from compliancedex_amd.workloads import DATA, prob_inputs
    cfg = load_robot("allegro")["config"]
    E = 6
    q, comp, target, _ = prob_inputs(cfg["ref_q"], E, seed=12, spread=True)
    mesh = TriangleMesh.from_npz(os.path.join(DATA, "meshes", "banana_mesh.npz"))
    center = np.load(os.path.join(DATA, "banana_center.npy"))
    args = [_dev(a).float() for a in (q, target, comp)]
    noise = G._noise(E, 1)
    rows = {}
    for with_term in (True, False):
        o = KinGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"], palm_offset=center.tolist(),
                              num_iters=1, optimize_target=True, ref_q=cfg["ref_q"])
        term = _term() if with_term else None
        if with_term:
            with pytest.raises(ValueError, match="fused=False"):
                o.optimize(*args, 1, TriangleMesh(mesh.vertices, mesh.triangles), verbose=False, fused=True, hand_term=term)
        o.optimize(*args, 1, TriangleMesh(mesh.vertices, mesh.triangles), verbose=False, kabsch_noise=noise,
                   trace_rows=True, fused=False, hand_term=term)
        rows[with_term] = o.loss_rows[0].double().cpu().numpy()
        if with_term:
            _report_ok(o.last_hand_report, E)
            from compliancedex_amd import PreparedMesh, hand_collision
            from compliancedex_amd.optimizers import _face_vertices
            obj = PreparedMesh(_face_vertices(mesh, torch.device(DEV)))
            kw = {k: v for k, v in KW.items() if k != "weight"}
            cost, _ = hand_collision(_hand(), args[0].double(), palm_rows(o.palm_offset, E), obj, floor_z=term.floor_z, **kw)
            t = (KW["weight"] * cost).cpu().numpy()
    _identity("kin eager loss", rows[True], rows[False], t, tol=2.0 ** -23)


def test_wc_takes_the_term():
    """WCKinGPISGraspOptimizer (eager only): iteration 0's loss rows are those without the term plus the statement."""
    from compliancedex_amd import WCKinGPISGraspOptimizer
    from compliancedex_amd.hand import palm_rows
    from compliancedex_amd.urdf import load_robot
    from tests._helpers import golden
    cfg = load_robot("allegro")["config"]
    E = 6
    pose, target, comp = G._inputs("kingpis", E)
    rows = {}
    for with_term in (True, False):
        o = WCKinGPISGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"],
                                    palm_offset=golden("mode_kingpis.npz")["palm3"].tolist(), num_iters=1, ref_q=cfg["ref_q"])
        o.optimize(pose, target, comp, 1, G._banana(), verbose=False, trace_rows=True,
                   hand_term=_term() if with_term else None)
        rows[with_term] = o.loss_rows[0].cpu().numpy()
        if with_term:
            _report_ok(o.last_hand_report, E)
            t, _, _ = _statement(_term(), pose, palm_rows(o.palm_offset, E))
    _identity("wc loss", rows[True], rows[False], t)
