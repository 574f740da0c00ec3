"""cdx_optimizer_step and cdx_kin_step alone on the device, driven by the scripted tapes of tests/_steps.py: no cost
kernel runs.  After EVERY launch the whole loop state is read back: the best-iterate bookkeeping, the clamps and frozen
groups bit for bit against the models of _steps, the update rule against torch.optim within _steps.TOL, the next
fingertips against tests/_chains.statement, every guard region and read-only buffer untouched.  Then the one-launch
copy of the Kin step (kin_cost4_kernel<…, STEP>) on a loop built to reach the skipped margin commit."""
import numpy as np
import pytest
import torch

from compliancedex_amd import _native as N
from tests import _chains
from tests import _steps as st

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = st.S


def _ids(cases):
    return ["-".join(f"{k}{'+'.join(v) if isinstance(v, tuple) else v}" for k, v in kw.items()) for kw in cases]


def _launch(call):
    rc = call(N.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------ cdx_optimizer_step
def _prob_setup(case):
    E, D, T = case["E"], case["D"], case["T"]
    A = st.Arena()
    for k in case["groups"]:
        x, live = case["init"][k], case["lr"][k] != 0.0
        A.add(k, x)
        A.add("g_" + k, np.zeros_like(x))
        A.add("m_" + k, np.full_like(x, 0.0 if live else st.FROZEN_M))
        A.add("v_" + k, np.full_like(x, 0.0 if live else st.FROZEN_V))
    A.add("total_loss", np.zeros(E))
    A.add("total_margin", np.zeros((E, T)))
    A.add("opt_value", np.full(E, np.inf))
    for k, shape in (("opt_margin", (E, T)), ("opt_q", (E, D)), ("opt_comp", (E, T)), ("opt_target", (E, T, 3)),
                     ("opt_palm", (E, 6))):
        A.add(k, np.full(shape, st.FILL))
    A.add("loop", np.zeros(2, np.int64))
    A.build(DEV)
    cfg = N.CdxAdam()
    for i, k in enumerate(st.PROB_GROUPS):
        cfg.lr[i] = case["lr"][k]
    cfg.beta1, cfg.beta2, cfg.eps = (st.ADAM[k] for k in ("beta1", "beta2", "eps"))
    cfg.comp_min = st.COMP_MIN
    lb, ub = case["box"]
    for j in range(3 * T):
        cfg.target_lb[j], cfg.target_ub[j] = float(lb[j]), float(ub[j])
    cfg.clamp_target, cfg.best_after = int(case["clamp_target"]), case["best_after"]
    buf = N.CdxOptBuffers()
    for name in N.OPT_BUFFER_FIELDS:
        setattr(buf, name, A.ptr(name))
    return A, cfg, buf


PROB_INPUTS = ["g_" + k for k in st.PROB_GROUPS] + ["total_loss", "total_margin", "loop"]


def _run_prob(kw, loop=False):
    case = st.make_case("prob", kw)
    E, D, T = case["E"], case["D"], case["T"]
    lib = N.load()
    A, cfg, buf = _prob_setup(case)
    if loop:
        buf.loop = A.ptr("loop")
    book, ref = st.ProbBook(E, D, T, case["best_after"]), st.trajectory(case)
    worst = {q: 0.0 for q in st.TOL["prob"]}
    improved = []
    for s in range(S):
        A["total_loss"][:], A["total_margin"][:] = case["loss"][s], case["margin"][s]
        for k in case["groups"]:
            A["g_" + k][:] = case["grads"][k][s]
        A["loop"].view(np.int32)[2] = s  # cdx_loop.step, advanced from the host (unused without `loop`)
        before = A.snapshot()
        A.upload()
        arg = (S - 1 - s) if loop else s  # with a loop the argument is wrong on purpose: loop->step must win
        assert _launch(lambda stream: lib.cdx_optimizer_step(cfg, buf, E, D, T, arg, stream)) == 0
        A.download()
        after = A.snapshot()
        assert A.guards_intact(), s
        for name in PROB_INPUTS:
            assert st.same_bits(after[name], before[name]), (name, s)
        improved.append(book.update(s, case["loss"][s], case["margin"][s], before["q"], before["comp"],
                                    before["target"], before["palm_pos"], before["palm_ori"]))
        for name, want in book.state().items():
            assert st.same_bits(after[name], want), (name, s)
        st.check_rule(case, before, after, ref[s], s, worst)
    assert np.array_equal(np.array(improved), st.improvers(case))  # the tape did what it was built to do
    print("cdx_optimizer_step", kw, {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= st.TOL["prob"][k], (k, v, st.TOL["prob"][k])
    return worst


PROB_CASES = st.prob_cases()


@pytest.mark.parametrize("kw", PROB_CASES, ids=_ids(PROB_CASES))
def test_optimizer_step_vs_torch_adam(kw):
    """Sizes E ∈ {1, 63, 64, 65, 130} × (D, T) ∈ {(0, 1), (7, 4), (16, 4), (32, 8)} with best_after 0 | 3 (s =
    best_after must not update, s = best_after + 1 must), then every group frozen in turn and all frozen, with the
    target clamp on and off: compliances driven under comp_min, one under it with its group frozen, one NaN."""
    _run_prob(kw)


def test_optimizer_step_takes_its_iteration_from_the_loop_counter():
    """buf->loop set and a wrong `iteration` argument: the device's loop->step decides the best-iterate gate and Adam's
    bias correction (advanced from the host between the calls)."""
    _run_prob(dict(E=65, D=16, T=4, best_after=3), loop=True)


def test_optimizer_step_no_candidates():
    """E = 0 returns OK and writes nothing."""
    case = st.make_case("prob", dict(E=1, D=7, T=4))
    A, cfg, buf = _prob_setup(case)
    A.upload()
    before = A.host.copy()
    assert _launch(lambda stream: N.load().cdx_optimizer_step(cfg, buf, 0, 7, 4, 0, stream)) == 0
    A.download()
    assert np.array_equal(A.host, before)


# ------------------------------------------------------------------ cdx_kin_step
def _kin_setup(case, tips):
    E, T = case["E"], case["T"]
    f32 = np.float32
    A = st.Arena()
    for k in st.KIN_GROUPS:
        x, live = case["init"][k], case["lr"][k] != 0.0
        A.add(k, x)
        A.add("g_" + k, np.zeros_like(x))
        A.add("m_" + k, np.full_like(x, 0.0 if live and case["rule"] == 0 else st.FROZEN_M))
        A.add("v_" + k, np.full_like(x, 0.0 if live else st.FROZEN_V))
    A.add("loss", np.zeros(E))
    for i in range(2):
        A.add(f"margin{i}", np.full((E, T), st.FILL - 1))
        A.add(f"normal{i}", np.full((E, T, 3), st.FILL - 1, f32))
    A.add("opt_value", np.full(E, np.inf, f32))
    A.add("opt_margin", np.full((E, T), st.FILL))
    A.add("opt_normal", np.full((E, T, 3), st.FILL, f32))
    for k in st.KIN_GROUPS:
        A.add("opt_" + k, np.full_like(case["init"][k], st.FILL))
    A.add("any", np.zeros(3, np.uint32))
    A.add("tips", np.full((E, T, 3), st.FILL, f32))
    A.build(DEV)
    cfg = N.CdxKinOpt()
    cfg.rule, cfg.clamp_box = case["rule"], int(case["clamp_box"])
    for i, k in enumerate(st.KIN_GROUPS):
        cfg.lr[i] = case["lr"][k]
    for k, v in case["hyper"].items():
        setattr(cfg, k, v)
    for i in range(3):
        cfg.palm_offset[i] = st.PALM[i]
    lb, ub = case["box"]
    for j in range(3 * T):
        cfg.box_lb[j], cfg.box_ub[j] = float(lb[j]), float(ub[j])
    buf = N.CdxKinOptBuffers()
    for name in N.KIN_OPT_FIELDS + ["opt_value", "opt_margin", "opt_normal", "any"]:
        setattr(buf, name, A.ptr(name))
    for k in st.KIN_GROUPS:
        setattr(buf, "opt_" + k, A.ptr("opt_" + k))
    for i in range(2):
        buf.margin[i], buf.normal[i] = A.ptr(f"margin{i}"), A.ptr(f"normal{i}")
    if tips:
        buf.tips = A.ptr("tips")
    return A, cfg, buf


KIN_INPUTS = ["g_" + k for k in st.KIN_GROUPS] + ["loss", "margin0", "margin1", "normal0", "normal1"]


def _run_kin(kw, chain=None, tips=False):
    case = st.make_case("kin", kw)
    E, T, kind = case["E"], case["T"], case["kind"]
    lib = N.load()
    desc = _chains.descriptor(chain) if chain else None
    A, cfg, buf = _kin_setup(case, tips)
    book, ref = st.KinBook(E, T, case["init"]["pose"].shape), st.trajectory(case)
    worst = {q: 0.0 for q in st.TOL[kind]}
    improved, tip_err = [], 0.0
    palm = np.asarray(st.PALM, np.float32).astype(np.float64)
    for s in range(S):
        A["loss"][:] = case["loss"][s]
        A[f"margin{s & 1}"][:], A[f"normal{s & 1}"][:] = case["margin"][s], case["normal"][s]
        for k in st.KIN_GROUPS:
            A["g_" + k][:] = case["grads"][k][s]
        before = A.snapshot()
        A.upload()
        assert _launch(lambda stream: lib.cdx_kin_step(desc, cfg, buf, E, T, s, 0, stream)) == 0
        A.download()
        after = A.snapshot()
        assert A.guards_intact(), s
        for name in KIN_INPUTS + ([] if tips else ["tips"]):
            assert st.same_bits(after[name], before[name]), (name, s)
        late = book.state()  # the batch's margin / normal are committed one launch late
        flag = book.update(case["loss"][s], case["margin"][s], case["normal"][s], before["pose"], before["target"],
                           before["comp"])
        improved.append(flag)
        for name, want in book.state(batch=False).items():
            assert st.same_bits(after[name], want), (name, s)
        for name in ("opt_margin", "opt_normal"):
            assert st.same_bits(after[name], late[name]), (name, s)
        # the any[] ring (cdx.h): this iteration's flag is set iff some candidate improved, the next one's is clear
        assert bool(after["any"][s % 3]) == bool(flag.any()) and after["any"][(s + 1) % 3] == 0, (s, after["any"])
        st.check_rule(case, before, after, ref[s], s, worst)
        if tips:
            want = _chains.statement(desc, after["pose"])["pos"] + palm
            tip_err = max(tip_err, _chains.rel(after["tips"], want))
    assert np.array_equal(np.array(improved), st.improvers(case))
    # finalize: only the commit of the last iteration's margin / normal, when it had an improver
    before = A.snapshot()
    assert _launch(lambda stream: lib.cdx_kin_step(desc, cfg, buf, E, T, S, 1, stream)) == 0
    A.download()
    after = A.snapshot()
    assert A.guards_intact()
    final = book.state()
    for name in after:
        assert st.same_bits(after[name], final[name] if name in ("opt_margin", "opt_normal") else before[name]), name
    print("cdx_kin_step", kw, chain, {k: f"{v:.2e}" for k, v in worst.items()}, f"tips {tip_err:.2e}")
    for k, v in worst.items():
        assert v <= st.TOL[kind][k], (k, v, st.TOL[kind][k])
    assert tip_err < _chains.TOL["pos"], tip_err


KIN1_CASES = st.kin1_cases()


@pytest.mark.parametrize("kw", KIN1_CASES, ids=_ids(KIN1_CASES))
def test_kin_step_rmsprop_vs_torch(kw):
    """Rule 1 (no chain): T ∈ {1, 3, 4, 5, 8} — 64 / T leaves idle lanes for 3 and 5 — with E on either side of a
    workgroup's 64 // T candidates, the box clamps on (tips and targets cross their bounds, one target is NaN and
    stays NaN) and off, the target group frozen in half of the unclamped cases."""
    _run_kin(kw)


KIN0_CASES = [(c, kw, tips) for c in st.KIN0_CHAINS for kw in st.kin0_cases() if kw["D"] == st.kin0_dims(c)[0]
              for tips in (True, False)]


@pytest.mark.parametrize("chain,kw,tips", KIN0_CASES,
                         ids=[f"{c}-E{kw['E']}-{'tips' if t else 'notips'}" for c, kw, t in KIN0_CASES])
def test_kin_step_adam_vs_torch(chain, kw, tips):
    """Rule 0 on the synthetic chains: line16 (one tip, D = 15 > 4·T), hand9 (four tips, D = 17: over 4·T — the
    unrolled pose loop's second trip — and no multiple of T), tree8 (eight tips, D = 31), E ∈ {1, 64 // T + 1, 67},
    a non-zero palm offset; with `tips` the next fingertips equal FK(the joint row the device wrote) + offset within
    _chains.TOL["pos"], without it the buffer stays untouched."""
    assert (kw["D"], kw["T"]) == st.kin0_dims(chain)
    _run_kin(kw, chain=chain, tips=tips)


@pytest.mark.parametrize("rule", [0, 1])
def test_kin_step_no_candidates(rule):
    """E = 0 returns OK and writes nothing (step and finalize)."""
    chain = "hand9" if rule == 0 else None
    D, T = st.kin0_dims("hand9")
    case = st.make_case("kin", dict(rule=rule, E=1, T=T, D=D if rule == 0 else 0))
    A, cfg, buf = _kin_setup(case, tips=rule == 0)
    desc = _chains.descriptor(chain) if chain else None
    A.upload()
    before = A.host.copy()
    for fin in (0, 1):
        assert _launch(lambda stream: N.load().cdx_kin_step(desc, cfg, buf, 0, T, 2, fin, stream)) == 0
    A.download()
    assert np.array_equal(A.host, before)


# ------------------------------------------------------------------ the one-launch copy of the Kin step
def test_kin_one_launch_step_skips_the_commit_like_two_launches(monkeypatch):
    """The best-iterate bookkeeping of kin_cost4_kernel<…, STEP> on the loop of _steps.FUSED, which stops improving
    after three iterations (five iterations with NO improver in the batch, the last among them; test_steps_cpu pins
    that on the oracle's tape, every decision clear of the best by 100 × the loss tolerance or more): the one-launch
    and the two-launch loop agree bit for bit on the losses, opt_value, opt_margin, opt_normal and the best parameters,
    and both equal _steps.KinBook run over the losses, margins, normals and parameters the two-launch loop's
    cdx_kin_step calls were handed."""
    import compliancedex_amd.optimizers as opts
    from compliancedex_amd import KinGraspOptimizer
    from compliancedex_amd.workloads import banana_mesh
    from tests._helpers import rel_err
    x = st.fused_inputs()
    E, iters = st.FUSED["E"], st.FUSED["iters"]
    lib = N.load()
    loops, tape = [], []

    class Recorded(opts._FusedLoop):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            loops.append(self)

    real_step = lib.cdx_kin_step

    def step(chain, cfg, buf, n, T, s, finalize, stream):
        if not finalize:  # what this step is handed: iteration s's loss, margin / normal slot and parameters
            loop = loops[-1]
            tape.append([t.detach().clone() for t in (loop.hist[s], loop.margin[s & 1], loop.normal[s & 1], loop.pose,
                                                      loop.target, loop.comp)])
        return real_step(chain, cfg, buf, n, T, s, finalize, stream)

    monkeypatch.setattr(opts, "_FusedLoop", Recorded)
    monkeypatch.setattr(lib, "cdx_kin_step", step, raising=False)
    outs = {}
    for one in ("1", "0"):
        kin = KinGraspOptimizer(st.FUSED["robot"], x["links"], x["offsets"], palm_offset=x["palm"].tolist(),
                                num_iters=iters, optimize_target=True, ref_q=[0.0] * x["q"].shape[1], device=DEV)
        res = kin.optimize(*[torch.from_numpy(x[k]).to(DEV) for k in ("q", "target", "comp")], 1.0, banana_mesh(),
                           verbose=False, kabsch_noise=[torch.from_numpy(n).to(DEV) for n in x["noise"]],
                           trace_rows=True, split_step=one == "0")
        torch.cuda.synchronize()
        loop = kin.last_loop
        outs[one] = dict(opt_pose=res[0], opt_comp=res[1], opt_target=res[2], opt_value=kin.best_loss,
                         opt_margin=loop.opt_margin, opt_normal=loop.opt_normal.view(E, 4, 3),
                         loss=torch.stack(kin.loss_rows))
        outs[one] = {k: v.detach().cpu().numpy() for k, v in outs[one].items()}
    assert len(tape) == iters  # the one-launch loop never called cdx_kin_step but to finalize
    for k, v in outs["1"].items():
        assert st.same_bits(v, outs["0"][k]), k
    # the loop did what it was built to do, on the device as on the oracle
    L = outs["0"]["loss"]
    print("device loss tape", L.tolist(), "vs oracle", rel_err(L, x["oracle_loss"]))
    assert rel_err(L, x["oracle_loss"]) < st.FUSED_LOSS_TOL
    assert np.array_equal(st.decisions(L)[0], st.FUSED_IMPROVERS)
    book = st.KinBook(E, 4, x["q"].shape)
    for s, rec in enumerate(tape):
        loss, margin, normal, pose, target, comp = (t.cpu().numpy() for t in rec)
        assert st.same_bits(loss, L[s])
        flag = book.update(loss, margin, normal.reshape(E, 4, 3), pose, target, comp)
        assert np.array_equal(flag, st.FUSED_IMPROVERS[s])
    want = book.state()
    for k, v in want.items():
        assert st.same_bits(outs["1"][k], v) and st.same_bits(outs["0"][k], v), k
