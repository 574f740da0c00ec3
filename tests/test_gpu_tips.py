"""The closure, the stand-alone force equilibrium and the prob optimise loop off the four-fingertip default, on an
MI355X: the cases of tests/_tips.py (T = 1..8 fingertips, gravity on and off, K = 1..4 levels over Lq = 1..3 query
rows, the palm term on and off) against the oracle, per candidate.

What runs where (csrc/cdx_closure.hip unless said otherwise):
  test_force_eq_vs_oracle          force_eq_forward_kernel<0>, force_eq_backward_kernel<0>
  test_closure_vs_oracle           closure_level_kernel<0,-1,false,VL> (T ≠ 4) and <4,0,false,VL> (t4_nograv_k2);
                                   closure_combine_kernel<8,…> (T = 5, 8) and <4,…> with idle lanes (T = 1..3); the
                                   query layout with Lq > 1 and without the palm row; VarSelect on groups of T rows
  test_screened_closure            closure_kabsch_kernel<0,-1> and the level kernel reading its records, cdx_screen.hip's
                                   screen_select_launch / refine_select_launch on groups of 1, 3, 5 and 8 rows
  test_screened_four_tips_no_gravity   closure_kabsch_kernel<4,0>
  test_loop_fused_equals_eager     cdx_optimizer_step's target clamp on fingertips 4.., both loops at T = 3 and 5
"""
import numpy as np
import pytest
import torch

from tests import _tips as tp
from tests._helpers import assert_rel, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def banana():
    from compliancedex_amd.workloads import stored_gpis
    return stored_gpis("banana", DEV)


def _log(tag, errs):
    print(tag, {k: f"{v:.2e}" for k, v in errs.items()})


# ------------------------------------------------------------------ force equilibrium
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("gravity", [True, False], ids=["gravity", "nogravity"])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 8])
def test_force_eq_vs_oracle(T, gravity, f32):
    """force_eq_reward at a runtime fingertip count, B = 1, 65 and 130 rows, float64 and float32 inputs, against the
    oracle per row at test_force_eq_vs_reference's device bars; flip masks equal.  One fingertip without gravity has
    a residual of rounding noise only (its direction, and with it reward, margin and gradients, is undetermined — NaN
    where the residual is exactly 0): there the flips and the vanishing force norms are compared."""
    from compliancedex_amd import force_eq_reward
    mu = 1 if gravity else 0.5
    d = tp.force_rows(T, gravity, mu, f32)
    dt = torch.float32 if f32 else torch.float64
    for B in (1, 65, 130):
        t = {k: torch.from_numpy(d[k][:B]).to(DEV, dt).requires_grad_(k != "normal")
             for k in ("tip", "target", "comp", "normal")}
        reward, margin, fn, flip = force_eq_reward(
            t["tip"], t["target"], t["comp"], mu, t["normal"], mass=tp.FORCE_MASS, gravity=10.0 if gravity else None,
            COM=list(tp.FORCE_COM), kabsch_noise=torch.from_numpy(d["noise"][:B]).to(DEV), return_flip=True)
        ((reward * torch.from_numpy(d["cr"][:B]).to(DEV)).sum()
         + (fn * torch.from_numpy(d["cf"][:B]).to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        tag = f"force_eq T={T} g={gravity} f32={f32} B={B}"
        assert np.array_equal(flip.cpu().numpy().astype(bool), d["flip"][:B]), tag
        assert t["tip"].grad.dtype == dt and tuple(margin.shape) == (B, T)
        if T == 1 and not gravity:
            assert float(fn.abs().max()) < 1e-12 and float(np.abs(d["force_norm"]).max()) < 1e-12
            continue
        got = dict(reward=reward, margin=margin, force_norm=fn)
        errs = {}
        for k, v in got.items():
            errs[k] = assert_rel(*tp.per_candidate(v.detach().cpu().numpy(), d[k][:B]), 1e-6, f"{tag}:{k}")
        for k, x in (("grad_tip", t["tip"]), ("grad_target", t["target"]), ("grad_comp", t["comp"])):
            errs[k] = assert_rel(*tp.per_candidate(x.grad.cpu().numpy(), d[k][:B]), 2e-5, f"{tag}:{k}")
        _log(tag, errs)


# ------------------------------------------------------------------ closure
def run_closure(opt, gpis, inputs):
    """ProbabilisticGraspOptimizer.closure on numpy inputs with the replayed noise → dict of numpy outputs."""
    q, comp, target, palm, noise = inputs
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(True)
         for a in (q, comp, target, palm[:, :3], palm[:, 3:])]
    opt.closure(*t, 1, gpis, q.shape[0], kabsch_noise=torch.from_numpy(np.ascontiguousarray(noise)).to(DEV))
    torch.cuda.synchronize()
    out = dict(total_loss=opt.total_loss, total_margin=opt.total_margin, pregrasp_tip=opt.pregrasp_tip_pose,
               flip=opt.kabsch_flip)
    out.update(zip(tp.GRADS, (x.grad for x in t)))
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", tp.CASES)
def test_closure_vs_oracle(name, banana, tmp_path):
    """The unscreened closure of every case at its E (67; 35 for two cases) and at E = 1 against closure_with_grads, per candidate: losses,
    margins, pregrasp tips and flips on every candidate, the five gradients on those the oracle keeps."""
    c, ref = tp.case(name), tp.reference(name)
    opt = c.optimizer(tmp_path, DEV, optimize_target=True)
    got = run_closure(opt, banana, ref["inputs"])
    assert opt.screen_stats(banana, c.E) is None
    tp.check_closure(got, ref, f"closure:{name}:E{c.E}", _log)
    row = [tp.single_row(name)]
    one = run_closure(opt, banana, tp.take(ref["inputs"], row, c.K))
    tp.check_closure(one, tp.slice_reference(ref, row, c.K), f"closure:{name}:E1", _log)


def _screened(c, E, inputs, banana, tmp_path):
    """Screened and unscreened closure of a case on the same inputs (test_screen's switch) → (screened, unscreened)."""
    from tests.test_screen import OUTS, TOL_EQ, _closure
    opt = c.optimizer(tmp_path, DEV, optimize_target=True)
    q, comp, target, palm, noise = inputs
    nz = torch.from_numpy(noise).to(DEV)
    a, st = _closure(opt, banana, (q, comp, target, palm), screen=True, noise=nz)
    b, st0 = _closure(opt, banana, (q, comp, target, palm), screen=False, noise=nz)
    b["pregrasp_tip"] = opt.pregrasp_tip_pose.cpu().numpy()
    assert st0 is None and st is not None
    assert st["bound_misses"] == 0 and st["screened_rows"] == c.Lq * E * c.T, st
    assert np.array_equal(a["flip"], b["flip"])
    for k in OUTS:
        e = rel_err(a[k], b[k])
        print(f"screened:{c.name}:E{E}:{k} {e:.2e}")
        assert e <= TOL_EQ, (k, e)
    return a, b


@pytest.mark.parametrize("name,E", [(n, e) for n, e, _ in tp.SCREENED])
def test_screened_closure(name, E, banana, tmp_path):
    """At the smallest screened sizes (Lq·E·T just above 4096 all-tip rows, E no multiple of 64, groups of T rows that
    straddle the 64-row tiles): screened equals unscreened at test_screen.TOL_EQ with identical NaNs and flips, no kept
    estimate outside its bound, every all-tip row screened; the unscreened result against the oracle on 32 candidates
    spread from the first tile to the last."""
    c = tp.case(name)
    ref = tp.screened_reference(name, E)
    _, b = _screened(c, E, ref["inputs"], banana, tmp_path)
    rows = tp.screened_rows(E)
    got = {k: (v.reshape(c.K, E)[:, rows].reshape(-1) if k == "flip" else v[rows]) for k, v in b.items()}
    tp.check_closure(got, ref, f"screened:{name}:E{E}", _log)


def test_screened_four_tips_no_gravity(banana, tmp_path):
    """Four fingertips without the gravity spring at a screened size (E = 520, Lq = 2): the Kabsch records of
    closure_kabsch_kernel<4,0>; screened equals unscreened, and candidates 0..66 — the inputs of the E = 67 case, whose
    rows do not depend on their neighbours (test_gpu_rows) — against that case's oracle reference."""
    c, E = tp.case("t4_nograv_k2"), 520
    ref = tp.reference(c.name)
    big = tp.closure_inputs(c, E)
    q, comp, target, palm, noise = (x.copy() for x in big)
    n = c.E
    for dst, src in zip((q, comp, target, palm), ref["inputs"]):
        dst[:n] = src
    noise.reshape(c.K, E, 3, 3)[:, :n] = ref["inputs"][4].reshape(c.K, n, 3, 3)
    _, b = _screened(c, E, (q, comp, target, palm, noise), banana, tmp_path)
    got = {k: (v.reshape(c.K, E)[:, :n].reshape(-1) if k == "flip" else v[:n]) for k, v in b.items()}
    tp.check_closure(got, ref, f"screened:{c.name}:E{E}", _log)


# ------------------------------------------------------------------ the Python layer and the loop
@pytest.mark.parametrize("name,E", [("t3_k1_nopalm", 4), ("t5_nograv", 7)])
def test_forward_kinematics_vs_oracle(name, E, tmp_path):
    from tests import _chains as ch
    c = tp.case(name)
    opt = c.optimizer(tmp_path, DEV)
    q, _, _, palm, _ = tp.closure_inputs(c, E)
    got = opt.forward_kinematics(torch.from_numpy(q).to(DEV), torch.from_numpy(palm).to(DEV))
    with torch.no_grad():
        ref = c.oracle_problem().forward_kinematics(torch.from_numpy(q), torch.from_numpy(palm))
    assert tuple(got.shape) == (E, c.T, 3)
    assert_rel(got.cpu().numpy(), ref.numpy(), ch.TOL["pos"], f"forward_kinematics:{name}")


@pytest.mark.parametrize("name,single_row", [("t3_nograv_k2", True), ("t5_k4", False)])
def test_loop_fused_equals_eager(name, single_row, banana, tmp_path):
    """optimize over 24 iterations (the best-iterate branch s > 20 runs) at T = 3 and T = 5, E = 67, targets and palm
    optimised, replayed noise: the fused loop's five results equal the eager loop's (test_optimize_vs_reference holds
    each of the two to 5e-6).  The box is tight: T = 3 gets one row for every fingertip, T = 5 a row per fingertip,
    and there the clamp acts on the fifth fingertip's targets (which the fused loop used to clamp to 0)."""
    from compliancedex_amd.workloads import DATA
    import os
    c = tp.case(name)
    E, iters = tp.E_REF, 24
    q, comp, target, palm, _ = tp.closure_inputs(c, E)
    center = np.load(os.path.join(DATA, "banana_center.npy"))
    if single_row:
        lb, ub = (center - 0.012).tolist(), (center + 0.012).tolist()
    else:
        lb = [(center - 0.012 - 0.001 * f).tolist() for f in range(c.T)]
        ub = [(center + 0.012 + 0.001 * f).tolist() for f in range(c.T)]
    g = torch.Generator(device=DEV).manual_seed(5)
    tape = [torch.rand(c.K * E, 3, 3, generator=g, device=DEV, dtype=torch.float64) for _ in range(iters)]
    res = {}
    for fused in (True, False):
        opt = c.optimizer(tmp_path, DEV, optimize_target=True, num_iters=iters, palm_offset=palm,
                          tip_bounding_box=(lb, ub))
        assert opt.optimize_palm
        out = opt.optimize(torch.from_numpy(q).to(DEV), torch.from_numpy(target).to(DEV),
                           torch.from_numpy(comp).to(DEV), 1, banana, verbose=False, noise_tape=tape, fused=fused)
        torch.cuda.synchronize()
        res[fused] = [x.detach().cpu().numpy() for x in out] + [opt.best_loss.cpu().numpy()]
    names = ["opt_q", "opt_comp", "opt_target", "opt_palm", "opt_margin", "best_loss"]
    for k, a, b in zip(names, res[True], res[False]):
        assert a.shape == b.shape, k
        assert_rel(a, b, 5e-6, f"loop:{name}:{k}")
    tgt = res[False][2]
    assert tgt.shape == (E, c.T, 3) and res[False][4].shape == (E, c.T)
    lbt, ubt = opt.tip_bounding_box[0].double().cpu().numpy(), opt.tip_bounding_box[1].double().cpu().numpy()
    fin = np.isfinite(res[False][5])  # (a candidate whose loss is never finite keeps its start)
    assert fin.sum() >= E // 2 and (res[False][0][fin] != q[fin]).any()  # the best-iterate branch ran
    assert (tgt[fin] >= lbt).all() and (tgt[fin] <= ubt).all()
    last = c.T - 1
    hit = (tgt[fin][:, last] == lbt[last]) | (tgt[fin][:, last] == ubt[last])
    assert hit.any() and (lbt[last] != 0).all()  # the clamp acted on the last fingertip, at its own bounds
