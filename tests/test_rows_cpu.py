"""Row independence on the CPU (tests/_rows.py): the host build of the per-candidate code (FK, ForceEq, collision, the
closure's queries and cost, the GPIS-mode cost and step) under the poison sets of test_gpu_rows.py, and the row-wise
behaviour of the oracle that the GPU tests rely on.  No GPU."""
import numpy as np
import pytest
import torch

from tests import _host, _rows
from tests._helpers import (collision_desc, golden, host_problem, oracle_gpis, oracle_gpis_at, oracle_problem,
                            product_chain)

B = 67  # one full wave and a 3-lane tail on the device; the same batch here
GRADS = ("grad_q", "grad_comp", "grad_target", "grad_palm_pos", "grad_palm_ori")


def grow(a, n, seed, jitter):
    """``a`` [m, ...] extended to n rows: the extra rows are earlier rows plus seeded jitter."""
    a = np.asarray(a, np.float64)
    rng = np.random.default_rng(seed)
    extra = a[np.arange(n - len(a)) % len(a)] + jitter * rng.standard_normal((n - len(a),) + a.shape[1:])
    return np.concatenate([a, extra])


def fk_case(robot):
    """(chain descriptor, q [B, D] float32, cotangent [B, 3·tips] float32)."""
    from compliancedex_amd.urdf import load_robot
    from compliancedex_amd.workloads import CONFIG4_OFFSETS
    cfg = load_robot(robot)["config"]
    offs = CONFIG4_OFFSETS if robot == "iiwa7_allegro" else cfg["ee_link_offset"]
    desc = product_chain(robot).descriptor(cfg["ee_link_name"], offs)
    rng = np.random.default_rng(7)
    ref = np.asarray(cfg.get("ref_q", [0.0] * desc.n_dofs), np.float64)
    if ref.shape != (desc.n_dofs,):
        ref = np.zeros(desc.n_dofs)
    q = (ref + 0.2 * rng.standard_normal((B, desc.n_dofs))).astype(np.float32)
    cot = (1.0 + rng.random((B, 3 * desc.n_tips))).astype(np.float32)  # no zero cotangent
    return desc, q, cot


def fk_dependent(desc, joint):
    """Masks of the elements of pos / quat / grad_q of a row that depend on ``joint``: the fingertips below it, and
    every joint on those fingertips' paths (the Jacobian column of a joint above the poisoned one is axis × (tip − origin)
    with a non-finite tip, that of a joint below it has a non-finite axis)."""
    dep = _rows.chain_dependence(desc)
    tips = dep[:, joint]
    assert tips.any()
    return dict(pos=np.repeat(tips, 3), quat=np.repeat(tips, 4), grad_q=dep[tips].any(0))


@pytest.mark.parametrize("robot", ["allegro", "iiwa7_allegro"])
def test_fk_host_rows(robot):
    """cdxh_fk_forward / cdxh_fk_backward, D = 16 and D = 23: one joint of the rows in P is non-finite."""
    desc, q, cot = fk_case(robot)

    def run(q):
        pos, quat = _host.fk_forward(desc, q)
        return dict(pos=pos, quat=quat, grad_q=_host.fk_backward(desc, q, cot))
    clean = run(q)
    assert all(np.isfinite(v).all() for v in clean.values())
    for joint in (0, desc.n_dofs - 1):
        dep = fk_dependent(desc, joint)
        for P in _rows.candidate_sets(B):
            for name, v in _rows.POISONS.items():
                out = run(_rows.poison(q, P, v, at=joint))
                _rows.check(clean, out, P, B, {k: np.tile(m, (len(P), 1)) for k, m in dep.items()},
                            tag=f"fk {robot} joint {joint} {name}")


def force_eq_case():
    from compliancedex_amd.force_eq import force_eq_descriptor
    d = golden("force_eq_gravity_mu1.npz")
    desc = force_eq_descriptor(4, 1, float(d["mass"]), 10.0, COM=d["com"].tolist())
    a = {k: grow(d[k], B, 11 + i, 1e-3) for i, k in enumerate(("tip", "target", "comp", "normal", "noise", "cr", "cf"))}
    n = a["normal"]
    a["normal"] = n / np.linalg.norm(n, axis=2, keepdims=True)
    return desc, a


FORCE_EQ_FLOAT = ("reward", "margin", "force_norm", "grad_tip", "grad_target", "grad_comp")
FORCE_EQ_ORDER = ("tip", "target", "comp", "normal", "noise", "cr", "cf")


def oracle_force_eq_row(a, r):
    """The oracle's force_eq_reward and its autograd gradients (cotangents cr, cf) on row r alone."""
    from oracle.cdx_oracle import force_eq_reward
    t = {k: torch.from_numpy(a[k][r:r + 1].copy()).requires_grad_(k in ("tip", "target", "comp"))
         for k in ("tip", "target", "comp", "normal")}
    reward, margin, fn, _ = force_eq_reward(t["tip"], t["target"], t["comp"], 1, t["normal"],
                                            torch.from_numpy(a["noise"][r:r + 1].reshape(1, 3, 3)), mass=0.1,
                                            gravity=10.0, COM=(0.0, 0.0, 0.0))
    ((reward * torch.from_numpy(a["cr"][r:r + 1])).sum() + (fn * torch.from_numpy(a["cf"][r:r + 1])).sum()).backward()
    return dict(reward=reward.detach().numpy(), margin=margin.detach().numpy(), force_norm=fn.detach().numpy(),
                grad_tip=t["tip"].grad.numpy(), grad_target=t["target"].grad.numpy(), grad_comp=t["comp"].grad.numpy())


def force_eq_cases(a):
    """(tag, P, poisoned inputs, the oracle's non-finite masks of the rows of P evaluated alone)."""
    for which in ("tip", "target", "comp", "normal"):
        for P in _rows.candidate_sets(B):
            for name, v in _rows.POISONS.items():
                b = dict(a)
                b[which] = _rows.poison(a[which], P, v)
                yield f"force_eq {which} {name}", P, b, _rows.oracle_masks([oracle_force_eq_row(b, r) for r in P])


def test_force_eq_host_rows():
    """cdxh_force_eq (ForceEq forward + backward): tip, target, compliance or normal of the rows in P non-finite; a
    poisoned row is non-finite wherever the oracle on that row alone is."""
    desc, a = force_eq_case()
    clean = _host.force_eq(desc, *(a[k] for k in FORCE_EQ_ORDER))
    assert all(np.isfinite(clean[k]).all() for k in FORCE_EQ_FLOAT)
    for tag, P, b, masks in force_eq_cases(a):
        assert masks["reward"].all(), tag  # (the row's reward is non-finite in the oracle in every case)
        out = _host.force_eq(desc, *(b[k] for k in FORCE_EQ_ORDER))
        _rows.check(clean, out, P, B, masks, tag=tag)


def collision_case():
    d = golden("collision_allegro_e64.npz")
    return collision_desc("allegro"), grow(d["q"], B, 21, 0.02), grow(d["palm"], B, 22, 0.002)


def oracle_collision_row(q, palm, r):
    """The oracle's collision_loss and its autograd gradients on row r alone."""
    from oracle.cdx_oracle import collision_loss
    from tests._helpers import oracle_chain
    chain, c = oracle_chain("allegro")
    cfg = c["config"]
    qt = torch.from_numpy(q[r:r + 1].copy()).requires_grad_(True)
    pt = torch.from_numpy(palm[r:r + 1].copy()).requires_grad_(True)
    cost = collision_loss(chain, cfg["collision_links"], cfg["collision_offsets"], cfg["collision_pairs"], qt, pt)
    cost.sum().backward()
    return dict(cost=cost.detach().numpy(), grad_q=qt.grad.numpy(), grad_palm=pt.grad.numpy())


def collision_cases(q, palm):
    """(tag, P, q, palm, the oracle's non-finite masks of the rows of P evaluated alone)."""
    for which, at in (("q", 0), ("palm_pos", 0), ("palm_ori", 3)):
        for P in _rows.candidate_sets(B):
            for name, v in _rows.POISONS.items():
                qp = _rows.poison(q, P, v, at) if which == "q" else q
                pp = palm if which == "q" else _rows.poison(palm, P, v, at)
                yield (f"collision {which} {name}", P, qp, pp,
                       _rows.oracle_masks([oracle_collision_row(qp, pp, r) for r in P]))


def test_collision_host_rows():
    """cdxh_collision: a joint, the palm position or the palm orientation of the rows in P non-finite.  The reference
    multiplies a masked term by 0 (optimize_pregrasp.py:684-698), so a non-finite candidate's cost and gradients are
    non-finite whichever side of a threshold a comparison with NaN falls: a poisoned row is non-finite wherever the
    oracle on that row alone is."""
    desc, q, palm = collision_case()

    def run(q, palm):
        cost, g_q, g_palm = _host.collision(desc, q, palm)
        return dict(cost=cost, grad_q=g_q, grad_palm=g_palm)
    clean = run(q, palm)
    assert all(np.isfinite(v).all() for v in clean.values())
    for tag, P, qp, pp, masks in collision_cases(q, palm):
        assert masks["cost"].all(), tag  # (the row's cost is non-finite in the oracle in every case)
        _rows.check(clean, run(qp, pp), P, B, masks, tag=tag)


# ---------------------------------------------------------------- closure (queries + cost), GPIS data row by row
@pytest.fixture(scope="module")
def closure_case():
    from compliancedex_amd.urdf import load_robot
    from compliancedex_amd.workloads import prob_inputs
    cfg = load_robot("allegro")["config"]
    q, comp, target, palm = prob_inputs(cfg["ref_q"], B, seed=5, spread=True)
    prob = host_problem("allegro")
    g = oracle_gpis("banana")
    noise = np.random.default_rng(6).random((prob.n_levels * B, 3, 3))
    X = _host.closure_queries(prob, q, target, palm)
    Ms = prob.n_query_levels * B * prob.chain.n_tips
    gp = oracle_gpis_at(g, X, with_std=False)
    gs = oracle_gpis_at(g, X[:Ms], with_std=True)
    gp["std"], gp["gstd"] = gs["std"], gs["gstd"]
    return dict(prob=prob, g=g, inputs=dict(q=q, comp=comp, target=target, palm=palm), noise=noise, X=X, gp=gp)


def query_rows(prob, X, E):
    """The closure's query points regrouped per candidate: [E, (Lq + 2)·T + 1, 3] (cdx_cost.h q_alltip … q_palm)."""
    T, Lq = prob.chain.n_tips, prob.n_query_levels
    tips = X[:(Lq + 2) * E * T].reshape(Lq + 2, E, T, 3).transpose(1, 0, 2, 3).reshape(E, -1, 3)
    return np.concatenate([tips, X[(Lq + 2) * E * T:].reshape(E, 1, 3)], 1)


def closure_outputs(prob, out, E):
    o = {k: out[k] for k in ("total_loss", "total_margin") + GRADS}
    o["flip"] = out["flip"].reshape(prob.n_levels, E).T
    return o


CLOSURE_POISON = dict(q=("q", 0), comp=("comp", 1), target=("target", 0), palm_pos=("palm", 0), palm_ori=("palm", 3))


def test_closure_host_rows(closure_case):
    """cdxh_closure_queries and cdxh_closure_cost, Allegro on the stored banana, E = 67: one input at a time non-finite
    in the rows of P.  The GPIS data of a changed query is the oracle's for that row alone (_rows.gpis_rows).  A poisoned
    candidate's loss, margins and gradients are non-finite in every element, as the oracle's are on that row alone
    (test_gpu_rows.test_closure_rows_vs_oracle compares the masks)."""
    c = closure_case
    prob, inp = c["prob"], c["inputs"]
    clean_q = query_rows(prob, c["X"], B)
    clean = closure_outputs(prob, _host.closure_cost(prob, inp["q"], inp["comp"], inp["target"], inp["palm"], c["noise"],
                                                     c["gp"]), B)

    def row_oracle(x):
        return oracle_gpis_at(c["g"], x, with_std=True)
    for which, (key, at) in CLOSURE_POISON.items():
        for P in _rows.candidate_sets(B):
            for name, v in _rows.POISONS.items():
                b = dict(inp)
                b[key] = _rows.poison(inp[key], P, v, at)
                X = _host.closure_queries(prob, b["q"], b["target"], b["palm"])
                tag = f"closure {which} {name}"
                _rows.assert_clean_rows_keep_bits(dict(X=clean_q), dict(X=query_rows(prob, X, B)), P, B, tag)
                gp = _rows.gpis_rows(c["X"], c["gp"], X, row_oracle)
                out = closure_outputs(prob, _host.closure_cost(prob, b["q"], b["comp"], b["target"], b["palm"],
                                                               c["noise"], gp), B)
                _rows.check(clean, out, P, B, ("total_loss", "total_margin") + GRADS, tag=tag)


# ---------------------------------------------------------------- GPIS-mode cost and step
def _mode_hand():
    """test_gpis_mode_cpu's ``hand`` fixture: the Allegro fingertips of the reference pose around the box."""
    from tests._helpers import oracle_chain
    ochain, c = oracle_chain("allegro")
    cfg = c["config"]
    desc = product_chain("allegro").descriptor(cfg["ee_link_name"], cfg["ee_link_offset"])
    ref_q = np.asarray(cfg["ref_q"], np.float32).astype(np.float64)
    tips0 = _host.fk_forward(desc, ref_q[None].astype(np.float32))[0].reshape(4, 3).astype(np.float64)
    return dict(ochain=ochain, links=cfg["ee_link_name"], offsets=cfg["ee_link_offset"], desc=desc, ref_q=ref_q,
                palm=np.array([0.0, 0.0, 0.03]) - tips0.mean(0), D=desc.n_dofs)


@pytest.mark.parametrize("mode", [0, 1])
def test_gpis_mode_host_rows(mode):
    """cdxh_gpis_mode_cost / cdxh_gpis_mode_step, E = 67, 3 iterations: a non-finite pose, target or compliance in the
    rows of P; after every cost and every step each other candidate's loss, gradients, parameters, RMSprop state and
    best iterate have the clean run's bits, and the poisoned candidates' losses are non-finite."""
    from compliancedex_amd.workloads import box_arrays
    from oracle.cdx_oracle import OracleGPIS
    from tests import test_gpis_mode_cpu as M
    X1, y, nz = box_arrays(n_surface=26)
    g = OracleGPIS.fit(X1[:60], y[:60], nz[:60], bias=1.0)
    hand = _mode_hand()
    pose0, target0, comp0, _ = M._inputs(mode, hand, n=B)
    noise = np.random.default_rng(9).uniform(0, 1, (3, B, 3, 3))
    prm, cfg = M._params(mode, hand), M._opt(M._lrs(mode, True))
    state = ("loss", "g_pose", "g_target", "g_comp", "pose", "target", "comp", "v_pose", "v_target", "v_comp",
             "opt_value", "opt_margin", "opt_pose", "opt_target", "opt_comp")

    def row_oracle(x):
        return oracle_gpis_at(g, x, with_std=True)

    def run(pose, target, comp, ref=None):
        """→ per-phase snapshots; ``ref``: the clean run's (points, data) per iteration, reused row by row."""
        h = M.HostLoop(mode, hand, pose, target, comp)
        snaps, keep = [], []
        for s in range(3):
            pts, tg = h.points().reshape(-1, 3).copy(), h.a["target"].reshape(-1, 3).copy()
            if ref is None:
                at, tt = oracle_gpis_at(g, pts, True), oracle_gpis_at(g, tg, False)
            else:
                at = _rows.gpis_rows(ref[s][0], ref[s][2], pts, row_oracle)
                tt = _rows.gpis_rows(ref[s][1], ref[s][3], tg, row_oracle)
            keep.append((pts, tg, at, tt))
            for k in ("mean", "gmean", "normal", "std", "gstd"):
                h.a[k][:] = at[k].reshape(h.a[k].shape)
            h.a["tmean"][:], h.a["tgmean"][:] = tt["mean"].reshape(-1), tt["gmean"]
            h.cost(prm, noise[s], s)
            snaps.append({k: h.a[k].reshape(B, -1).copy() for k in state})
            h.step(prm, cfg, s)  # (mode 1: the step writes the next fingertips itself)
            snaps.append({k: h.a[k].reshape(B, -1).copy() for k in state})
        h.step(prm, cfg, 3, finalize=1)
        snaps.append({k: h.a[k].reshape(B, -1).copy() for k in state})
        return snaps, keep
    clean, ref = run(pose0, target0, comp0)
    assert np.isfinite(clean[0]["loss"]).all()
    for which in ("pose", "target", "comp"):
        for P in _rows.candidate_sets(B):
            for name, v in _rows.POISONS.items():
                args = dict(pose=pose0, target=target0, comp=comp0)
                args[which] = _rows.poison(args[which], P, v)
                snaps, _ = run(args["pose"], args["target"], args["comp"], ref)
                for i, (a, b) in enumerate(zip(clean, snaps)):
                    _rows.check(a, b, P, B, ("loss",), tag=f"gpis_mode {mode} {which} {name} phase {i}")
                assert np.isinf(snaps[-1]["opt_value"][list(P)]).all()  # a non-finite loss never became a best iterate


# ---------------------------------------------------------------- the oracle, row by row
def _poisoned_queries():
    """40 queries of the reference's banana vector: clean, and with rows poisoned by NaN, +inf, −inf and 1e200."""
    X = golden("gpis_banana.npz")["X"][:40]
    P = {3: np.nan, 11: np.inf, 17: -np.inf, 29: _rows.OVERFLOW}
    Xp = X.copy()
    for r, v in P.items():
        Xp[r, 0] = v
    return X, Xp, P


def test_oracle_gpis_clean_rows_of_a_poisoned_batch():
    """OracleGPIS.pred / compute_normal on 40 queries of which four are poisoned (NaN, ±inf, 1e200) against the same
    oracle on the 36 clean rows alone: mean, ∇mean, normal and std of the clean rows agree.  (∇std is taken from the
    clean subset only: the batched formulation's gradient is not row-wise.)  The two runs differ only in the batch
    size their BLAS calls see, so the bound is f64 summation order: N·ε ≈ 361 · 1.1e-16 = 4e-14, times the
    cancellation of var = k0 − k·E11⁻¹k for std (k0 / var ≤ 1e3 on these rows): 1e-12 and 1e-10."""
    g = oracle_gpis("banana")
    X, Xp, P = _poisoned_queries()
    keep = _rows.clean_mask(len(X), P)
    full = oracle_gpis_at(g, Xp, with_std=False)
    with torch.no_grad():
        full["std"] = g.pred(torch.from_numpy(Xp))[1].numpy()
    sub = oracle_gpis_at(g, X[keep], with_std=True)
    for k, tol in (("mean", 1e-12), ("gmean", 1e-12), ("normal", 1e-12), ("std", 1e-10)):
        a, b = full[k][keep], sub[k]
        assert np.isfinite(a).all(), k
        err = np.abs(a - b).max() / np.abs(b).max()
        print(k, err)
        assert err <= tol, (k, err)


def test_oracle_poisoned_row_alone_is_nan():
    """A poisoned query evaluated alone: mean, ∇mean, normal, std and ∇std are all non-finite (TPS: r = ∞ or NaN reaches
    every term) — what _rows.gpis_rows hands to the host entry points for such a row."""
    g = oracle_gpis("banana")
    _, Xp, P = _poisoned_queries()
    for r in P:
        one = oracle_gpis_at(g, Xp[r:r + 1], with_std=True)
        for k, v in one.items():
            assert not np.isfinite(v).any(), (r, k, v)


def test_oracle_closure_clean_rows_of_a_poisoned_batch():
    """closure_with_grads, Allegro on the stored banana, E = 6 with candidate 2 poisoned in q, comp, target or the palm
    against the five clean candidates alone: total_loss and total_margin of the clean candidates agree (the
    per-candidate cost is f64 on f32 FK; the two runs differ in the GPIS batch size only, as above: 1e-10), and the
    poisoned candidate's total_loss is non-finite.  Gradients come from the clean subset only."""
    from oracle.cdx_oracle import closure_with_grads
    d = golden("closure_allegro_banana_e6.npz")
    prob = oracle_problem("allegro", "banana")
    E = 6
    keep = _rows.clean_mask(E, (2,))
    noise = d["noise"][0].reshape(3, E, 3, 3)
    base = {k: d[k] for k in ("q", "comp", "target", "palm")}
    sub = closure_with_grads(prob, *(base[k][keep] for k in ("q", "comp", "target", "palm")),
                             noise[:, keep].reshape(-1, 3, 3))
    for which, (key, at) in CLOSURE_POISON.items():
        b = dict(base)
        b[key] = _rows.poison(base[key], (2,), np.nan, at)
        full = closure_with_grads(prob, b["q"], b["comp"], b["target"], b["palm"], d["noise"][0])
        assert not np.isfinite(full["total_loss"][2]), which
        for k in ("total_loss", "total_margin"):
            err = np.abs(full[k][keep] - sub[k]).max() / np.abs(sub[k]).max()
            print(which, k, err)
            assert err <= 1e-10, (which, k, err)
