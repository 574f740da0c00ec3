"""The closure and the force equilibrium off the four-fingertip default, on the CPU: the host build of the per-candidate
code (libcdx_host.so: ForceEq<0>, closure_candidate at a runtime fingertip count) against the oracle on the cases of
tests/_tips.py, the conditions that keep those comparisons from passing on thin data, the oracle-only criterion that
leaves ill-conditioned candidates out of the gradient comparisons, and the Python layer's handling of a fingertip count
other than four (forward_kinematics, the fingertip box, the coefficient table).  No GPU.
"""
import numpy as np
import pytest
import torch

from tests import _chains as ch
from tests import _host
from tests import _tips as tp
from tests._helpers import assert_rel, oracle_gpis, oracle_gpis_at, rel_err


# ------------------------------------------------------------------ force equilibrium
FORCE_CASES = [(T, g, mu) for T in tp.FORCE_TIPS for g in (True, False) for mu in (1, 0.5) if T > 1 or g]


@pytest.mark.parametrize("T,gravity,mu", FORCE_CASES)
def test_force_eq_host_vs_oracle(T, gravity, mu):
    """ForceEq at a runtime fingertip count against force_eq_reward, per row, at test_force_eq_host_vs_reference's
    tolerances (measured ≤ 1.2e-11); _tips.force_rows asserts the flips and the clamped / unclamped rows."""
    d = tp.force_rows(T, gravity, mu)
    out = _host.force_eq(tp.force_desc(T, gravity, mu), d["tip"], d["target"], d["comp"], d["normal"], d["noise"],
                         d["cr"], d["cf"])
    assert np.array_equal(out["flip"].astype(bool), d["flip"])
    for k in ("reward", "margin", "force_norm"):
        assert_rel(*tp.per_candidate(out[k], d[k]), 1e-9, f"force_eq T={T} g={gravity} mu={mu}:{k}")
    for k in ("grad_tip", "grad_target", "grad_comp"):
        assert_rel(*tp.per_candidate(out[k], d[k]), 1e-6, f"force_eq T={T} g={gravity} mu={mu}:{k}")


def test_force_eq_one_tip_without_gravity_is_undetermined():
    """One point and no gravity spring: the Kabsch fit is exact and the residual is what rounding leaves of 0 — exactly
    0 in some rows (direction 0/0: reward, margin and gradients NaN), 1e-18 in the others (a direction, and with it a
    reward, that no two implementations share).  Neither the values nor the NaN mask can be pinned; the rotation's
    flip (the SVD of the noise alone) and the vanishing force can."""
    d = tp.force_rows(1, False, 1)
    assert np.isnan(d["reward"]).any() and np.isfinite(d["reward"]).any()
    assert np.abs(d["force_norm"]).max() < 1e-12
    out = _host.force_eq(tp.force_desc(1, False, 1), d["tip"], d["target"], d["comp"], d["normal"], d["noise"],
                         d["cr"], d["cf"])
    assert np.array_equal(out["flip"].astype(bool), d["flip"]) and 2 <= d["flip"].sum() <= tp.FORCE_B - 2
    assert np.abs(out["force_norm"]).max() < 1e-12


# ------------------------------------------------------------------ the case table
def test_table_covers_the_settings():
    cases = [tp.case(n) for n in tp.CASES]
    for T in (1, 2, 3, 5, 8):
        mine = [c for c in cases if c.T == T]
        assert T == 1 or any(not c.gravity for c in mine), T
        assert any((c.K, c.Lq) != (3, 1) for c in mine), T
    assert any(c.T == 1 and not c.gravity for c in cases) is False
    assert {(c.K, c.Lq) for c in cases} >= {(1, 1), (2, 2), (3, 1), (4, 3)}
    assert any(c.T == 4 and not c.gravity and c.Lq > 1 for c in cases)
    assert any(not c.optimize_palm for c in cases)
    k4 = tp.case("t8_k4")
    assert len({tuple(r) for r in k4.coeffs}) == 3 and all(len(set(r)) == k4.T for r in k4.coeffs)
    for name, E, _ in tp.SCREENED:
        c = tp.case(name)
        assert c.Lq * E * c.T >= 4096 and E % 64 and c.Lq * (E - 64) * c.T < 4096
        assert tp.screened_rows(E).max() >= E - E % 64 and tp.screened_rows(E).max() < E  # reaches the ragged tile
    assert [tp.case(n).T for n, _, _ in tp.SCREENED if tp.case(n).Lq == 1] == [1, 3, 5, 8]
    assert any(tp.case(n).Lq == 2 for n, _, _ in tp.SCREENED)
    for c in cases:  # the problem descriptor sees what the case says
        p = c.problem()
        assert (p.chain.n_tips, p.n_levels, p.n_query_levels, p.gravity, p.optimize_palm) == \
            (c.T, c.K, c.Lq, int(c.gravity), int(c.optimize_palm))


@pytest.mark.parametrize("name", tp.CASES)
def test_reference_within_the_cap(name):
    """The oracle alone (two evaluations, one float32 ulp of q apart) leaves at most MAX_EXCLUDED of a case's
    candidates out of the gradient comparisons, at the case's E and on the screened cases' slices."""
    ref = tp.reference(name)
    assert len(ref["keep"]) == tp.case(name).E >= 35
    assert 1.0 - ref["keep"].mean() <= ch.MAX_EXCLUDED
    assert ref["keep"][tp.single_row(name)]
    assert np.isfinite(ref["total_loss"]).all()
    for n, E, _ in tp.SCREENED:
        if n == name:
            assert 1.0 - tp.screened_reference(name, E)["keep"].mean() <= ch.MAX_EXCLUDED


def host_closure(c, inputs):
    """The host build's closure of a case: queries (float32 FK), the oracle's GPIS at them, the per-candidate cost."""
    q, comp, target, palm, noise = inputs
    prob = c.problem()
    X = _host.closure_queries(prob, q, target, palm)
    E, T = q.shape[0], c.T
    assert len(X) == (c.Lq + 2) * E * T + (E if c.optimize_palm else 0)
    g = oracle_gpis("banana")
    Ms = c.Lq * E * T
    gp = oracle_gpis_at(g, X, with_std=False)
    gs = oracle_gpis_at(g, X[:Ms], with_std=True)
    gp["std"], gp["gstd"] = gs["std"], gs["gstd"]
    out = _host.closure_cost(prob, q, comp, target, palm, noise, gp)
    out["pregrasp_tip"] = X[(c.Lq + 1) * E * T:(c.Lq + 2) * E * T].reshape(E, T, 3)
    return out


@pytest.mark.parametrize("name", tp.CASES)
def test_closure_host_vs_oracle(name):
    """test_chains_cpu's test_closure_host_vs_oracle per candidate on the case table, E = 67 (35 for two cases)."""
    c, ref = tp.case(name), tp.reference(name)
    out = host_closure(c, ref["inputs"])
    assert rel_err(out["pregrasp_tip"], ref["pregrasp_tip"]) < 1e-6
    errs = tp.check_closure(out, ref, f"host:{name}")
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})


def test_probe_flags_the_large_gradient_candidate():
    """tree8 with its eight tips, levels 0.8 / 0.9 / 0.8 / 0.7, gravity on, E = 5: one candidate's gradient is more
    than ten times its neighbours' (a friction margin next to the −0.9999 clamp, where 0.8 / (margin + 1) multiplies
    the float32 FK's rounding), and in a whole-batch comparison it alone sets the figure.  The probe flags exactly that
    candidate; the host build meets the bar on the other four and on every loss, margin and flip."""
    ref = tp.reference(tp.E5.name, 5)
    big = np.abs(ref["grad_q"]).max(1)
    worst = int(big.argmax())
    assert big[worst] > 10 * np.median(big)
    assert np.array_equal(~ref["keep"], np.arange(5) == worst)
    out = host_closure(tp.E5, ref["inputs"])
    tp.check_closure(out, ref, "host:t8_e5")
    a, b = tp.per_candidate(out["grad_q"], ref["grad_q"])
    per = np.abs(a - b).max(1)
    print("per-candidate grad_q error", per)
    assert per[worst] == per.max() and per[worst] > 10 * np.delete(per, worst).max()


# ------------------------------------------------------------------ the Python layer at T ≠ 4
def cpu_optimizer(c, tmp_path, monkeypatch=None, **kw):
    """The optimiser of a case on the CPU; with ``monkeypatch`` its robot model's FK is the host build's."""
    opt = c.optimizer(tmp_path, "cpu", **kw)
    if monkeypatch is not None:
        def fk(q, link_names, recursive=False, offsets=None):
            pos, quat = _host.fk_forward(opt.robot_model._descriptor(link_names, offsets), q.detach().numpy())
            return torch.from_numpy(pos), torch.from_numpy(quat)
        monkeypatch.setattr(opt.robot_model, "compute_forward_kinematics", fk)
    return opt


@pytest.mark.parametrize("name,E", [("t3_k1_nopalm", 4), ("t5_nograv", 7)])
def test_forward_kinematics_groups_by_fingertip_count(name, E, tmp_path, monkeypatch):
    """forward_kinematics returns [E, T, 3] in the oracle's grouping (3·4 values regroup silently into fours)."""
    c = tp.case(name)
    opt = cpu_optimizer(c, tmp_path, monkeypatch)
    q, _, _, palm, _ = tp.closure_inputs(c, E)
    got = opt.forward_kinematics(torch.from_numpy(q), torch.from_numpy(palm))
    with torch.no_grad():
        ref = c.oracle_problem().forward_kinematics(torch.from_numpy(q), torch.from_numpy(palm))
    assert tuple(got.shape) == (E, c.T, 3) and got.dtype == torch.float64
    assert ch.rel(got.numpy(), ref.numpy()) < ch.TOL["pos"]


@pytest.mark.parametrize("rows", [2, 4, 6])
def test_box_with_the_wrong_row_count_is_rejected(rows, tmp_path):
    c = tp.case("t5_nograv")
    with pytest.raises(ValueError, match="tip_bounding_box"):
        cpu_optimizer(c, tmp_path, tip_bounding_box=([[-0.2, -0.2, 0.0]] * rows, [[0.2, 0.2, 0.2]] * rows))
    with pytest.raises(ValueError, match="tip_bounding_box"):
        cpu_optimizer(c, tmp_path, tip_bounding_box=([-0.2, -0.2, 0.0] * rows, [0.2] * 3))


@pytest.mark.parametrize("name", ["t3_k1_nopalm", "t5_nograv", "t8_k4"])
def test_single_box_row_broadcasts_in_both_loops(name, tmp_path):
    """A [3] row, a [1, 3] row and the default box reach every fingertip: the eager loop clamps with
    ``tip_bounding_box`` [T, 3], the fused loop with adam_config's target_lb / target_ub — the same 3·T numbers."""
    c = tp.case(name)
    lb, ub = [-0.01, -0.02, 0.015], [0.03, 0.04, 0.05]
    per_tip = cpu_optimizer(c, tmp_path, tip_bounding_box=([lb] * c.T, [ub] * c.T))
    for box in ((lb, ub), ([lb], [ub])):
        opt = cpu_optimizer(c, tmp_path, tip_bounding_box=box)
        cfg = opt.adam_config()
        for i, want in enumerate((lb, ub)):
            assert tuple(opt.tip_bounding_box[i].shape) == (c.T, 3)
            assert torch.equal(opt.tip_bounding_box[i], per_tip.tip_bounding_box[i])
            fused = list((cfg.target_lb, cfg.target_ub)[i])[:3 * c.T]
            assert fused == opt.tip_bounding_box[i].double().reshape(-1).tolist()
            assert fused == per_tip.tip_bounding_box[i].double().reshape(-1).tolist()
            assert np.allclose(fused, want * c.T, rtol=1e-7)
    from compliancedex_amd.optimizer import FINGERTIP_LB, FINGERTIP_UB
    opt = cpu_optimizer(c, tmp_path)
    cfg = opt.adam_config()
    assert list(cfg.target_lb)[:3 * c.T] == torch.tensor(FINGERTIP_LB[:3] * c.T).double().tolist()
    assert list(cfg.target_ub)[:3 * c.T] == torch.tensor(FINGERTIP_UB[:3] * c.T).double().tolist()
    assert opt.tip_bounding_box[1].double().reshape(-1).tolist() == list(cfg.target_ub)[:3 * c.T]


def test_four_fingertip_box_is_unchanged(tmp_path):
    """At T = 4 the reference's twelve-entry box and the default give the rows they always gave."""
    from compliancedex_amd.optimizer import FINGERTIP_LB, FINGERTIP_UB
    c = tp.case("t4_nograv_k2")
    a = cpu_optimizer(c, tmp_path, tip_bounding_box=(FINGERTIP_LB, FINGERTIP_UB))
    b = cpu_optimizer(c, tmp_path)
    for i, want in enumerate((FINGERTIP_LB, FINGERTIP_UB)):
        assert torch.equal(a.tip_bounding_box[i], torch.tensor(want).view(-1, 3))
        assert torch.equal(b.tip_bounding_box[i], a.tip_bounding_box[i])


def test_coefficient_table_is_checked_at_construction(tmp_path):
    """A table with another column count than fingertips (the four-wide default handed to three fingertips among
    them), with ragged rows or with too many levels is refused by the constructor, not by the first closure."""
    from compliancedex_amd import ProbabilisticGraspOptimizer
    c = tp.case("t3_k1_nopalm")
    path = ch.write_json(c.chain, tmp_path)

    def make(**kw):
        return ProbabilisticGraspOptimizer(path, c.links, c.offsets, ref_q=[0.0] * c.D, device="cpu", **kw)
    for bad in (((0.8,) * 4,) * 3, ((0.8,) * 2,), ((0.8, 0.8, 0.8), (0.9, 0.9)), ((0.8,) * 3,) * 5):
        with pytest.raises(ValueError, match="pregrasp_coefficients"):
            make(pregrasp_coefficients=bad, pregrasp_weights=[1.0 / len(bad)] * len(bad))
    with pytest.raises(ValueError, match="weight"):
        make(pregrasp_coefficients=((0.8,) * 3,) * 2, pregrasp_weights=(0.1, 0.8, 0.1))
    assert make().pregrasp_coefficients.tolist() == torch.tensor([[0.8] * 3] * 3).tolist()  # the default follows T
