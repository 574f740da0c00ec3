"""Row independence of the per-row kernels on the GPU (tests/_rows.py): a non-finite query or candidate stays in its
own row.

Every case runs a finite batch and the same batch with a set P of rows poisoned through the same entry point at the
same size, and asserts (a) every output row outside P keeps its bytes — each kernel forms a row's sums in an order fixed
by (M, N, tile shape), never by the row's neighbours; the one exception, the screened closure, is named in its test —
(b) the outputs of the rows in P that depend on the poisoned input are non-finite, and on the smallest case of each
family (c) the clean rows meet the oracle evaluated on the clean rows only, at the tolerances test_gpu_edges /
test_gpu_parity already assert for that entry point.  A poisoned row's reference is the oracle on that row alone
(tests/_rows.py says why).

Padding neutrality of the GPIS mean is here too: appending a zero-weight inducing point changes no byte of mean, ∇mean
or normal, which is what lets the kernel pad a partial block of inducing points with a point of the state.
"""
import numpy as np
import pytest
import torch

from tests import _rows
from tests._helpers import golden, oracle_gpis, oracle_gpis_at, oracle_problem, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
E = 67  # one full wave and a 3-lane tail
GRADS = ("grad_q", "grad_comp", "grad_target", "grad_palm_pos", "grad_palm_ori")
QUERY_POISONS = dict(_rows.POISONS, overflow=_rows.OVERFLOW)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def dev(a, **kw):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, **kw)


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- GPIS states and queries
def _gpis(kernel, n):
    """(GPIS, oracle or None): n = an inducing-point count of test_gpu_edges._random_gpis, "banana" (the stored state,
    N = 361) or "banana2000" (workloads.synthetic_banana_gpis)."""
    key = (kernel, n)
    if key not in _CACHE:
        if n == "banana":
            from compliancedex_amd.workloads import stored_gpis
            _CACHE[key] = (stored_gpis("banana", DEV), oracle_gpis("banana"))
        elif n == "banana2000":
            from compliancedex_amd.workloads import synthetic_banana_gpis
            _CACHE[key] = (synthetic_banana_gpis(2000, device=DEV), None)
        else:
            from tests.test_gpu_edges import _random_gpis
            g, ref, _ = _random_gpis(n, seed=n, kernel=kernel)
            _CACHE[key] = (g, ref)
    return _CACHE[key]


def _queries(g, M, seed):
    """M finite queries around the state's inducing points (1 cm jitter), float64 numpy."""
    rng = np.random.default_rng(seed)
    X1 = host(g.X1.double())
    return X1[rng.integers(0, len(X1), M)] + 0.01 * rng.standard_normal((M, 3))


def _dependent(kernel, name):
    """(b) for a GPIS query: every output, except for the RBF kernel at ±inf / 1e200 — there the covariance of an
    infinitely far query is exp(−∞) = 0 and the mean is the bias, in the oracle too: a far query, not a poisoned one."""
    return () if kernel == "rbf" and name != "nan" else None


def _mean(st, X):
    from compliancedex_amd.gpis import gpis_mean
    mean, gmean, normal = gpis_mean(st, dev(X), want_grad=True, want_normal=True)
    return dict(mean=host(mean), gmean=host(gmean), normal=host(normal))


def _std(st, X):
    from compliancedex_amd.gpis import gpis_std
    std, gstd = gpis_std(st, dev(X), want_grad=True)
    return dict(std=host(std), gstd=host(gstd))


MEAN_STATES = [(k, n) for k in ("tps", "rbf", "joint") for n in (255, 256, 257)] + [("tps", "banana")]


@pytest.mark.parametrize("kernel,n", MEAN_STATES)
def test_gpis_mean_rows(kernel, n):
    """cdx_gpis_mean (mean, ∇mean, normal; the TPS moment path, RBF, joint), N around the 256-point staging block and
    the stored banana (N = 361), M = 1, 33, 300 (32 queries per workgroup).  With N = 256 no padding point is staged; at
    the other sizes a padding point placed relative to a query of the workgroup carried a non-finite query into the
    other 31 queries of its workgroup through 0·NaN."""
    g, ref = _gpis(kernel, n)
    st = g.native_state()
    for M in (1, 33, 300):
        X = _queries(g, M, 100 + M)
        clean = _mean(st, X)
        assert all(np.isfinite(v).all() for v in clean.values())
        for P in _rows.query_sets(M):
            for name, v in QUERY_POISONS.items():
                out = _mean(st, _rows.poison(X, P, v))
                _rows.check(clean, out, P, M, _dependent(kernel, name), tag=f"mean {kernel} N={n} M={M} {name}")
                if kernel == "tps" and n in (255, "banana") and M == 33 and name == "nan":  # (c), the smallest case
                    keep = _rows.clean_mask(M, P)
                    r = oracle_gpis_at(ref, X[keep], with_std=False)
                    assert rel_err(out["mean"][keep], r["mean"]) < 1e-8
                    assert rel_err(out["normal"][keep], r["normal"]) < 1e-8
                    assert rel_err(out["gmean"][keep], r["gmean"]) < 1e-7


STD_CASES = [(k, n, 300) for k in ("tps", "rbf") for n in (255, 257)] + \
            [("tps", 300, 4200), ("rbf", 300, 4200), ("tps", "banana2000", 4200)]


@pytest.mark.parametrize("kernel,n,M", STD_CASES)
def test_gpis_std_rows(kernel, n, M):
    """cdx_gpis_std (std and ∇std): the split-K path (M = 300, N = 255 / 257) and the stripe path (M = 4200 ≥ 4096
    queries, N = 300 and the N = 2000 synthetic banana).  A query is one row of the MFMA products; the pad rows of the
    last 128-query tile replicate row M − 1."""
    g, ref = _gpis(kernel, n)
    st = g.native_state()
    X = _queries(g, M, 200)
    clean = _std(st, X)
    assert all(np.isfinite(v).all() for v in clean.values())
    for P in _rows.query_sets(M):
        for name, v in QUERY_POISONS.items():
            out = _std(st, _rows.poison(X, P, v))
            _rows.check(clean, out, P, M, _dependent(kernel, name), tag=f"std {kernel} N={n} M={M} {name}")
            if (kernel, n) == ("tps", 255) and name == "nan":  # (c), the smallest case
                keep = _rows.clean_mask(M, P)
                r = oracle_gpis_at(ref, X[keep], with_std=True)
                assert rel_err(out["std"][keep], r["std"]) < 1e-7
                assert rel_err(out["gstd"][keep], r["gstd"]) < 1e-7


def test_gpis_screen_var_rows():
    """cdx_gpis_screen_var on the N = 2000 synthetic banana, M = 300: a poisoned query's estimate is NaN (as a far
    query's, test_screen_far_queries_are_nan), every other estimate keeps its bits."""
    g, _ = _gpis("tps", "banana2000")
    st = g.native_state()
    M = 300
    X = _queries(g, M, 300)
    clean = dict(est=host(st.screen_var(dev(X))))
    assert np.isfinite(clean["est"]).all()
    for P in _rows.query_sets(M):
        for name, v in QUERY_POISONS.items():
            out = dict(est=host(st.screen_var(dev(_rows.poison(X, P, v)))))
            _rows.assert_clean_rows_keep_bits(clean, out, P, M, f"screen {name}")
            assert np.isnan(out["est"][list(P)]).all(), (name, P, out["est"][list(P)])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gpis_field_rows(axis):
    """cdx_gpis_field through the C ABI, stored banana, 13³ lattice with node 3 of one axis NaN: exactly the nodes of
    that plane are non-finite in mean, std and normal (cell (i, j, k) is at (x[j], y[i], z[k])), every other node
    keeps its bits."""
    from compliancedex_amd import _native as N
    g, _ = _gpis("tps", "banana")
    st = g.native_state()
    lib = N.load()
    d = golden("field_banana_s13.npz")
    steps = 13

    def run(ax):
        ax = dev(ax)
        f64 = dict(dtype=torch.float64, device=DEV)
        mean, sd = torch.empty(steps, steps, steps, **f64), torch.empty(steps, steps, steps, **f64)
        nrm = torch.empty(steps, steps, steps, 3, **f64)
        ws = torch.empty(max(lib.cdx_gpis_field_workspace(st.desc, steps, 0), 1), dtype=torch.uint8, device=DEV)
        N.check(lib.cdx_gpis_field(st.desc, N.ptr(ax[0]), N.ptr(ax[1]), N.ptr(ax[2]), steps, 0, N.ptr(mean), N.ptr(sd),
                                   N.ptr(nrm), N.ptr(ws), N.stream_ptr(torch.device(DEV))), "cdx_gpis_field")
        return dict(mean=host(mean), std=host(sd), normal=host(nrm))
    ax = np.stack([np.linspace(float(d["lb"][k]), float(d["ub"][k]), steps) for k in range(3)])
    clean = run(ax)
    assert all(np.isfinite(v).all() for v in clean.values())
    bad = ax.copy()
    bad[axis, 3] = np.nan
    out = run(bad)
    plane = np.zeros((steps, steps, steps), bool)
    plane[(slice(None), 3, slice(None)) if axis == 0 else (3,) if axis == 1 else (slice(None), slice(None), 3)] = True
    for k in clean:
        a, b = clean[k].reshape(steps ** 3, -1), out[k].reshape(steps ** 3, -1)
        keep = ~plane.reshape(-1)
        assert _rows.same_bits(a[keep], b[keep]), (k, int((a[keep] != b[keep]).any(1).sum()))
        assert not np.isfinite(b[~keep]).any(), k


@pytest.mark.parametrize("kernel", ["tps", "rbf"])
def test_gpis_mean_padding_neutral(kernel):
    """A zero-weight inducing point is neutral to the bit: the N = 255 state against a hand-built C-ABI descriptor with
    one more point (α = 0, at a finite location that is no query's) — N = 256, where the kernel stages no padding point
    at all — gives the same bytes of mean, ∇mean and normal on 300 finite queries.  So the kernel's own padding of a
    partial block changes nothing for finite queries wherever its (finite) padding point lies."""
    from compliancedex_amd import _native as N
    g, _ = _gpis(kernel, 255)
    st = g.native_state()
    assert st.desc.N == 255 and st.desc.N_pad == 256
    X = dev(_queries(g, 300, 400))
    X1 = st.X1.clone()
    X1[255] = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    assert float((X - X1[255]).norm(dim=1).min()) > 0.05
    alpha = st.alpha.clone()
    alpha[255] = 0.0
    more = N.CdxGpis(X1=X1.data_ptr(), alpha=alpha.data_ptr(), N=256, N_pad=256, kernel=st.desc.kernel, R=st.desc.R,
                     sigma=st.desc.sigma, bias=st.desc.bias)
    lib = N.load()
    outs = []
    for desc in (st.desc, more):
        f64 = dict(dtype=torch.float64, device=DEV)
        mean, gmean, nrm = torch.empty(300, **f64), torch.empty(300, 3, **f64), torch.empty(300, 3, **f64)
        N.check(lib.cdx_gpis_mean(desc, N.ptr(X), 300, N.ptr(mean), N.ptr(gmean), N.ptr(nrm),
                                  N.stream_ptr(torch.device(DEV))), "cdx_gpis_mean")
        outs.append((host(mean), host(gmean), host(nrm)))
    assert all(np.isfinite(a).all() for a in outs[0])
    for a, b in zip(*outs):
        assert _rows.same_bits(a, b)


# ---------------------------------------------------------------- FK, ForceEq, collision
@pytest.mark.parametrize("robot", ["allegro", "iiwa7_allegro"])
def test_fk_rows(robot):
    """cdx_fk_forward / cdx_fk_backward (float32), D = 16 and D = 23, B = 67: one joint of the rows in P non-finite —
    the fingertips below that joint and the gradient of every joint on their paths are non-finite, every other row
    keeps its bits."""
    from compliancedex_amd import DifferentiableRobotModel
    from compliancedex_amd.urdf import load_robot
    from compliancedex_amd.workloads import CONFIG4_OFFSETS
    from tests.test_rows_cpu import fk_case, fk_dependent
    desc, q, cot = fk_case(robot)
    links = load_robot(robot)["config"]["ee_link_name"]
    offs = CONFIG4_OFFSETS if robot == "iiwa7_allegro" else load_robot(robot)["config"]["ee_link_offset"]
    m = DifferentiableRobotModel(robot, device=DEV)

    def run(q):
        qt = dev(q).requires_grad_(True)
        pos, quat = m.compute_forward_kinematics(qt, links, offsets=offs)
        (pos * dev(cot)).sum().backward()
        return dict(pos=host(pos), quat=host(quat), grad_q=host(qt.grad))
    clean = run(q)
    assert all(np.isfinite(v).all() for v in clean.values()) and clean["pos"].dtype == np.float32
    for joint in (0, desc.n_dofs - 1):
        dep = fk_dependent(desc, joint)
        for P in _rows.candidate_sets(E):
            for name, v in _rows.POISONS.items():
                out = run(_rows.poison(q, P, v, at=joint))
                _rows.check(clean, out, P, E, {k: np.tile(mk, (len(P), 1)) for k, mk in dep.items()},
                            tag=f"fk {robot} joint {joint} {name}")


def test_force_eq_rows():
    """cdx_force_eq_forward / _backward, B = 67: tip, target, compliance or normal of the rows in P non-finite; a
    poisoned row is non-finite wherever the oracle on that row alone is, every other row keeps its bits."""
    from compliancedex_amd import force_eq_reward
    from tests.test_rows_cpu import FORCE_EQ_FLOAT, force_eq_case, force_eq_cases
    _, a = force_eq_case()

    def run(a):
        t = {k: dev(a[k]).requires_grad_(k in ("tip", "target", "comp")) for k in ("tip", "target", "comp", "normal")}
        reward, margin, fn, flip = force_eq_reward(t["tip"], t["target"], t["comp"], 1, t["normal"], mass=0.1,
                                                   gravity=10.0, COM=[0.0, 0.0, 0.0],
                                                   kabsch_noise=dev(a["noise"].reshape(-1, 3, 3)), return_flip=True)
        ((reward * dev(a["cr"])).sum() + (fn * dev(a["cf"])).sum()).backward()
        return dict(reward=host(reward), margin=host(margin), force_norm=host(fn), flip=host(flip),
                    grad_tip=host(t["tip"].grad), grad_target=host(t["target"].grad), grad_comp=host(t["comp"].grad))
    clean = run(a)
    assert all(np.isfinite(clean[k]).all() for k in FORCE_EQ_FLOAT)
    for tag, P, b, masks in force_eq_cases(a):
        _rows.check(clean, run(b), P, E, masks, tag=tag)


def _prob_opt(palm=None, iters=1, collision=False):
    from compliancedex_amd import ProbabilisticGraspOptimizer
    from compliancedex_amd.urdf import load_robot
    cfg = load_robot("allegro")["config"]
    kw = dict(palm_offset=palm) if palm is not None else {}
    if collision:
        kw.update(anchor_link_names=cfg["collision_links"], anchor_link_offsets=cfg["collision_offsets"],
                  collision_pairs=cfg["collision_pairs"])
    return cfg, ProbabilisticGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"], ref_q=cfg["ref_q"],
                                            optimize_target=True, optimize_palm=True, num_iters=iters, device=DEV, **kw)


def test_collision_rows():
    """cdx_collision_loss, E = 67: a joint, the palm position or the palm orientation of the rows in P non-finite.  The
    reference multiplies a masked term by 0, so a poisoned candidate's cost and gradients are non-finite wherever the
    oracle's are on that row alone — whichever way a comparison with NaN falls."""
    from tests.test_rows_cpu import collision_case, collision_cases
    _, q, palm = collision_case()
    _, opt = _prob_opt(palm, collision=True)

    def run(q, palm):
        qt, pt = dev(q).requires_grad_(True), dev(palm).requires_grad_(True)
        cost = opt.compute_collision_loss(qt, pt)
        cost.sum().backward()
        return dict(cost=host(cost), grad_q=host(qt.grad), grad_palm=host(pt.grad))
    clean = run(q, palm)
    assert all(np.isfinite(v).all() for v in clean.values()) and (clean["cost"] != 0).sum() > 32
    for tag, P, qp, pp, masks in collision_cases(q, palm):
        _rows.check(clean, run(qp, pp), P, E, masks, tag=tag)


# ---------------------------------------------------------------- the closure
CLOSURE_POISON = dict(q=("q", 0), comp=("comp", 1), target=("target", 0), palm_pos=("palm", 0), palm_ori=("palm", 3))
CLOSURE_FLOAT = ("total_loss", "total_margin") + GRADS


def _closure(opt, gpis, inp, noise):
    n = inp["q"].shape[0]
    t = [dev(a).requires_grad_(True) for a in (inp["q"], inp["comp"], inp["target"], inp["palm"][:, :3],
                                               inp["palm"][:, 3:])]
    opt.closure(*t, 1, gpis, n, kabsch_noise=noise)
    torch.cuda.synchronize()
    out = dict(total_loss=host(opt.total_loss), total_margin=host(opt.total_margin),
               pregrasp_tip=host(opt.pregrasp_tip_pose), flip=host(opt.kabsch_flip).reshape(-1, n).T)
    for k, x in zip(GRADS, t):
        out[k] = host(x.grad)
    return out


@pytest.mark.parametrize("n", [67, 1024])
def test_closure_rows(n):
    """cdx_closure, Allegro on the stored banana (N = 361: the mean pads its second block of inducing points), one
    input at a time non-finite in candidate 0 (which closure_combine_kernel's invalid lanes alias), the last one, or 15
    and 16 together: the poisoned candidates' loss, margins and gradients are non-finite.

    E = 67 (268 all-tip rows per level, below the screen's 4096-row threshold): every other candidate keeps its bits.
    E = 1024, the smallest screened size: a poisoned candidate's estimates are NaN, so its group runs the exact pass
    for every fingertip — the exact-row list, and with it the K-split of the refine pass that sums the other rows'
    ‖V‖², depends on the inputs by design (cdx_screen.hip, the exact list's compaction).  The clean candidates are
    therefore compared at the tolerance test_screen.py asserts for that mechanism (TOL_EQ = 1e-10, screened against
    unscreened), with identical finite masks and Kabsch flip bits."""
    from compliancedex_amd.workloads import prob_inputs
    from tests.test_screen import TOL_EQ
    cfg, opt = _prob_opt()
    gpis, _ = _gpis("tps", "banana")
    q, comp, target, palm = prob_inputs(cfg["ref_q"], n, seed=321, spread=True)
    inp = dict(q=q, comp=comp, target=target, palm=palm)
    noise = dev(np.random.default_rng(7).random((3 * n, 3, 3)))
    clean = _closure(opt, gpis, inp, noise)
    assert (opt.screen_stats(gpis, n) is not None) == (n == 1024)
    for P in _rows.candidate_sets(n):
        assert np.isfinite(clean["total_loss"][list(P)]).all()  # (the poisoned candidates are finite in the clean run)
    assert np.isfinite(clean["total_loss"]).sum() > n // 2
    for which, (key, at) in CLOSURE_POISON.items():
        for P in _rows.candidate_sets(n):
            for name, v in _rows.POISONS.items():
                b = dict(inp)
                b[key] = _rows.poison(inp[key], P, v, at)
                out = _closure(opt, gpis, b, noise)
                _rows.check(clean, out, P, n, CLOSURE_FLOAT, tol=TOL_EQ if n == 1024 else None,
                            tag=f"closure E={n} {which} {name}")


def test_closure_rows_vs_oracle():
    """(c) for the closure, the reference's E = 6 vector with candidate 2 poisoned (NaN) in q, comp, target, the palm
    position or the palm orientation: the five clean candidates meet the oracle run on those five alone at
    TOL_CLOSURE_ORACLE, and the poisoned candidate has exactly the finite mask of the oracle run on it alone in every
    output, the pre-grasp fingertips included (no output is exempt)."""
    from oracle.cdx_oracle import closure_with_grads
    from tests.test_gpu_parity import TOL_CLOSURE_ORACLE
    d = golden("closure_allegro_banana_e6.npz")
    n = 6
    _, opt = _prob_opt(d["palm"])
    gpis, _ = _gpis("tps", "banana")
    prob = oracle_problem("allegro", "banana")
    base = {k: d[k] for k in ("q", "comp", "target", "palm")}
    keep = _rows.clean_mask(n, (2,))
    nz = d["noise"][0].reshape(3, n, 3, 3)
    ref = closure_with_grads(prob, *(base[k][keep] for k in ("q", "comp", "target", "palm")),
                             nz[:, keep].reshape(-1, 3, 3))
    for which, (key, at) in CLOSURE_POISON.items():
        b = dict(base)
        b[key] = _rows.poison(base[key], (2,), np.nan, at)
        out = _closure(opt, gpis, b, dev(d["noise"][0]))
        for k in CLOSURE_FLOAT:
            err = rel_err(out[k][keep], ref[k])
            print(which, k, err)
            assert err < TOL_CLOSURE_ORACLE[k], (which, k, err)
        assert np.array_equal(out["flip"][keep].T.reshape(-1).astype(bool), ref["flip"])
        one = closure_with_grads(prob, b["q"][2:3], b["comp"][2:3], b["target"][2:3], b["palm"][2:3],
                                 nz[:, 2:3].reshape(-1, 3, 3))
        assert not np.isfinite(out["total_loss"][2]), which
        for k in CLOSURE_FLOAT + ("pregrasp_tip",):
            assert np.array_equal(np.isfinite(out[k][2]), np.isfinite(one[k][0])), (which, k)


# ---------------------------------------------------------------- the optimiser loops
@pytest.mark.parametrize("fused", [True, False])
def test_prob_optimize_rows(fused):
    """ProbabilisticGraspOptimizer.optimize, E = 67, 5 iterations on a replayed noise tape, candidate 0's first joint
    non-finite: at every step every other candidate's loss, gradients and parameters, and the returned best iterate,
    have the clean run's bits; candidate 0's loss is non-finite at every step."""
    from compliancedex_amd.workloads import prob_inputs
    iters = 5
    gpis, _ = _gpis("tps", "banana")
    cfg, _ = _prob_opt()
    q, comp, target, palm = prob_inputs(cfg["ref_q"], E, seed=11, spread=True)
    rng = np.random.default_rng(12)
    tape = [dev(rng.random((3 * E, 3, 3))) for _ in range(iters)]
    names = ("q", "comp", "target", "pp", "po")

    def run(q):
        _, opt = _prob_opt(palm, iters)
        steps = []
        if fused:
            def hook(s, out, state):
                snap = {k: host(state[k]) for k in names}
                snap.update({k: host(out[k]) for k in ("total_loss", "total_margin", "g_q", "g_comp", "g_target",
                                                       "g_palm_pos", "g_palm_ori")})
                steps.append(snap)
            res = opt.optimize(dev(q), dev(target), dev(comp), 1, gpis, verbose=False, noise_tape=tape, fused=True,
                               step_hook=hook)
        else:
            inner = opt.closure

            def traced(*a, **k):
                r = inner(*a, **k)
                snap = {k_: host(x) for k_, x in zip(names, a[:5])}
                snap.update({"g_" + k_: host(x.grad) for k_, x in zip(names, a[:5])})
                snap.update(total_loss=host(opt.total_loss), total_margin=host(opt.total_margin))
                steps.append(snap)
                return r
            opt.closure = traced
            res = opt.optimize(dev(q), dev(target), dev(comp), 1, gpis, verbose=False, noise_tape=tape, fused=False)
        torch.cuda.synchronize()
        final = {f"opt{i}": host(x) for i, x in enumerate(res)}
        final["best_loss"] = host(opt.best_loss)
        return steps + [final]
    clean = run(q)
    assert len(clean) == iters + 1 and np.isfinite(clean[0]["total_loss"][0])
    for name, v in _rows.POISONS.items():
        out = run(_rows.poison(q, (0,), v))
        for s, (a, b) in enumerate(zip(clean, out)):
            _rows.check(a, b, (0,), E, ("total_loss",) if s < iters else (), tag=f"optimize fused={fused} {name} step {s}")


@pytest.mark.parametrize("mode", ["gpis", "kingpis"])
def test_fused_gpis_loop_rows(mode):
    """The fused GPIS / KinGPIS loop (cdx_gpis_mean over [tips; targets], cdx_gpis_std, cdx_gpis_mode_iteration), E = 67,
    8 iterations on the stored banana: candidate 3 poisoned (test_gpu_gpis_mode's NaN compliance; its fingertips are
    NaN queries from the second iteration on) against candidate 3 clean — every other candidate is bit-identical in the
    per-iteration losses, the returned tensors and best_loss, and candidate 3's loss is NaN at every iteration."""
    from tests import test_gpu_gpis_mode as G
    iters = 8

    def run(clean):
        o = G._make(mode, iters)
        pose, target, comp = G._inputs(mode, E)
        assert bool(torch.isnan(comp[3, 1]))
        if clean:
            comp[3, 1] = 10.0
        res = o.optimize(pose, target, comp, 1, G._banana(), verbose=False, kabsch_noise=G._noise(E, iters),
                         trace_rows=True, fused=True)
        out = dict(loss_rows=host(torch.stack(o.loss_rows)).T, best_loss=host(o.best_loss))
        out.update({f"out{i}": host(x) for i, x in enumerate(res[:3])})
        return out
    clean, bad = run(True), run(False)
    assert np.isfinite(clean["loss_rows"]).all()
    _rows.check(clean, bad, (3,), E, ("loss_rows",), tag=f"fused {mode} loop")
