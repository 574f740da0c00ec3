"""The optimiser step kernels alone: scripted tapes, references and the device harness for cdx_optimizer_step
(csrc/cdx_optim.hip) and cdx_kin_step (kin_step_kernel in csrc/cdx_kin.hip).

No cost kernel runs.  Before every call the test writes that iteration's loss, gradients and margin / normal straight
into the buffers, from a tape made here with a fixed seed, and reads the whole loop state back afterwards.

Tapes.  ``loss_tape`` is constructed, not drawn (test_steps_cpu pins its properties): iterations in which no candidate
of the batch improves, an improving one directly after them, a lone improver in the LAST candidate (another workgroup
than the one that rotates the any[] ring), exact ties, a candidate that is NaN from iteration 0 and one that turns NaN
midway, a last iteration with or without an improver and, for the Kin step, the pair 1 + 3e-8 → 1 + 1e-8 (the first is
stored as 1.0f, the second is lower in double and still no improvement).  Margins and normals encode (iteration, row,
component) as 2048·s + row + 0.25·(component + 1) — exact in float32 — so a commit from the wrong iteration, slot or
row is a wrong number.  Gradients span 1e-12 … 1e3 with exact zeros.

References.  The update rule is torch.optim.Adam / RMSprop on CPU tensors of the kernel's dtype with the groups of
optimizer.adam_config / optimizers.py (``TorchRule``); the bookkeeping is ``ProbBook`` / ``KinBook``, a few lines that
follow include/cdx.h's two step sections: copies and compares, so the device must be bit-equal.

Tolerance of the update rule.  ``WideRule`` evaluates the same formulas in a wider type (numpy longdouble for the
float64 step, float64 for the float32 steps); torch's deviation from it over every tape of the case lists below,
relative to |p| + lr·steps for a parameter and to the moment for m / v, is REF_ERR (``measure_reference`` recomputes
it, test_steps_cpu pins it), and the device tolerance is TOL = 4 × REF_ERR: two correct evaluations may each be off
from the wide one by the reference's own error, in rounding orders that differ (the device contracts a·b + c in
cdx_optim.hip, its pow may differ from the host's by an ulp).  The first moment's figure is set by the few entries
where 0.9·m and 0.1·g nearly cancel (the gradients change sign and span fifteen decades): one rounding there is
multiplied by |m before| / |m after|, for torch and for the device alike.
"""
import functools

import numpy as np
import torch

S = 9                       # iterations of every tape: the three any[] flags wrap three times
STRIDE = 2048.0             # margin / normal code: STRIDE·s + row + 0.25·(component + 1)
FILL = -77.0                # initial contents of opt_* (a value no tape or parameter holds)
FROZEN_M, FROZEN_V = 0.5, 0.25  # moments of a frozen group: must come back untouched
GUARD_BYTE = 0xA5
PALM = (0.01, -0.02, 0.03)  # rule 0's palm offset

PROB_LR = dict(q=1e-3, comp=0.2, target=2e-3, palm_pos=1e-4, palm_ori=1e-4)  # optimizer.adam_config
PROB_GROUPS = tuple(PROB_LR)
COMP_MIN = 80.0
KIN_GROUPS = ("pose", "target", "comp")
KIN_LR = {  # optimizers.py: (pose, target, compliance) with / without optimize_target
    (0, True): (2e-3, 1e-5, 0.2), (0, False): (1e-2, 0.0, 0.2),
    (1, True): (1e-3, 1e-3, 0.2), (1, False): (1e-3, 0.0, 0.2)}
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)   # torch.optim.Adam defaults
RMSPROP = dict(alpha=0.99, eps=1e-8)            # torch.optim.RMSprop defaults

# torch.optim against WideRule over the case lists below (measure_reference), and the device tolerance.
REF_ERR = {
    "prob": dict(p=3.5e-15, m=8.7e-13, v=7.3e-16),  # measured 3.43e-15, 8.61e-13, 7.25e-16 (float64 Adam)
    "kin0": dict(p=4.5e-7, m=8.2e-4, v=4.9e-7),     # measured 4.46e-7, 8.10e-4, 4.83e-7 (float32 Adam)
    "kin1": dict(p=1.7e-6, v=3.8e-7),               # measured 1.63e-6 (1.72e-6 on another CPU), 3.74e-7 (f32 RMSprop)
}
TOL = {k: {q: 4.0 * e for q, e in v.items()} for k, v in REF_ERR.items()}


# ------------------------------------------------------------------ tapes
def loss_tape(E, last_improves, kin):
    """losses [S, E] float64, every value exact in float32 except the Kin pair's.

    level of an ordinary candidate c, + 0.125·c − 16 (exact; negative and positive losses):
      s   0   1   2   3   4   5   6   7   8
          10  8   9   8   5   7   6   5   5 (6 with last_improves)
          ↓   ↓   –   tie ↓   –   –   tie tie
    candidate E − 1 alone improves at s = 6 (level 4), candidate 0 alone at s = 8 with last_improves (level 3).  With
    E ≥ 8: candidate 1 is NaN throughout, candidate 2 from s = 4 on, and (kin) candidate 3 holds the double / float
    pair: 10, 1 + 3e-8 (stored as 1.0f), 1 + 1e-8 (lower in double, not lower than 1.0f), 1.0 (tie with the float)."""
    level = np.array([10.0, 8.0, 9.0, 8.0, 5.0, 7.0, 6.0, 5.0, 6.0 if last_improves else 5.0])
    off = 0.125 * np.arange(E) - 16.0
    L = level[:, None] + off[None, :]
    L[6, E - 1] = 4.0 + off[E - 1]
    if last_improves:
        L[8, 0] = 3.0 + off[0]
    if E >= 8:
        L[:, 1] = np.nan
        L[4:, 2] = np.nan
        if kin:
            L[:, 3] = [10.0, 1.0 + 3e-8, 1.0 + 1e-8, 1.0, 0.5, 0.75, 0.75, 0.5, 0.75 if last_improves else 0.5]
    assert L.shape == (S, E)
    return L


def code_tape(E, T, comps):
    """[S, E, T, comps] float64: STRIDE·s + (e·T + f) + 0.25·(component + 1)."""
    s = np.arange(S, dtype=np.float64)[:, None, None, None]
    row = (np.arange(E)[:, None] * T + np.arange(T)[None, :]).astype(np.float64)[None, :, :, None]
    return STRIDE * s + row + 0.25 * (np.arange(comps, dtype=np.float64)[None, None, None, :] + 1.0)


def grad_tape(rng, shape, dtype):
    """[S, *shape]: ±10^U(−12, 3) with a tenth exact zeros; per tensor, element 0 is zero throughout, 1 zero for three
    iterations and then live, 2 live and then zero for good (√v falls under eps), 3 is ±1e-12, 4 is 1e3, and every
    element ≡ 5 (mod 8) is +1 throughout (a steady drive into a clamp)."""
    n = int(np.prod(shape))
    g = 10.0 ** rng.uniform(-12.0, 3.0, (S, n)) * rng.choice([-1.0, 1.0], (S, n))
    g[rng.random((S, n)) < 0.1] = 0.0
    if n > 0:
        g[:, 0] = 0.0
    if n > 1:
        g[:3, 1], g[3:, 1] = 0.0, np.where(g[3:, 1] == 0.0, 1.0, g[3:, 1])
    if n > 2:
        g[:3, 2], g[3:, 2] = 10.0 ** np.array([-3.0, 0.0, 2.0]), 0.0
    if n > 3:
        g[:, 3] = 1e-12 * np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    if n > 4:
        g[:, 4] = 1e3
    g[:, 5::8] = 1.0
    return g.astype(dtype).reshape((S,) + tuple(shape))


def box(T):
    """Per (fingertip, axis) bounds, all different: [−0.03 + j/1000, 0.03 + j/1000] (float32 values)."""
    j = np.arange(3 * T, dtype=np.float64) / 1000.0
    return (j - 0.03).astype(np.float32), (j + 0.03).astype(np.float32)


def _in_box(rng, E, T, dtype):
    """[E, T, 3] inside box(T), within a step or two of a bound in places."""
    lb, ub = box(T)
    x = rng.uniform(lb.astype(np.float64) + 1e-3, ub.astype(np.float64) - 1e-3, (E, 3 * T))
    return x.reshape(E, T, 3).astype(dtype)


# ------------------------------------------------------------------ cases
@functools.lru_cache(None)
def prob_case(E, D, T, best_after=3, frozen=(), clamp_target=True, last_improves=True):
    """One scripted run of cdx_optimizer_step: dict(E, D, T, lr {group: lr}, init {buffer: array}, loss [S, E],
    margin [S, E, T], grads {group: [S, …]}, …), read-only."""
    rng = np.random.default_rng(7000 + 131 * E + 17 * D + T)
    f64 = np.float64
    comp = 80.0 + rng.uniform(0.3, 40.0, (E, T))
    comp.reshape(-1)[5::8] = 80.05   # driven under comp_min by the steady +1 gradient (lr 0.2 a step)
    comp.reshape(-1)[3::7] = 79.0    # under comp_min from the start: clamped even when the group is frozen
    if E * T >= 2:
        comp.reshape(-1)[-1] = np.nan
    init = dict(q=0.3 * rng.standard_normal((E, D)), comp=comp, target=_in_box(rng, E, T, f64),
                palm_pos=0.1 * rng.standard_normal((E, 3)), palm_ori=0.1 * rng.standard_normal((E, 3)))
    grads = {k: grad_tape(rng, init[k].shape, f64) for k in PROB_GROUPS}
    lr = {k: (0.0 if k in frozen else v) for k, v in PROB_LR.items()}
    case = dict(E=E, D=D, T=T, best_after=best_after, clamp_target=bool(clamp_target), lr=lr, init=init, grads=grads,
                loss=loss_tape(E, last_improves, kin=False), margin=code_tape(E, T, 1)[..., 0], box=box(T),
                kind="prob", dtype=f64, groups=PROB_GROUPS, hyper=ADAM, rule=0)
    _freeze(case)
    return case


@functools.lru_cache(None)
def kin_case(rule, E, T, D=0, optimize_target=True, clamp_box=False, last_improves=True, nan_target=False):
    """One scripted run of cdx_kin_step: rule 0 (Adam, pose = q [E, D]) or rule 1 (RMSprop, pose = tips [E, T, 3])."""
    rng = np.random.default_rng(8000 + 1000 * rule + 131 * E + 17 * D + T)
    f32 = np.float32
    pose = (0.3 * rng.standard_normal((E, D))).astype(f32) if rule == 0 else _in_box(rng, E, T, f32)
    target = _in_box(rng, E, T, f32)
    if nan_target and target.size >= 3:
        target.reshape(-1)[-2] = np.nan
    init = dict(pose=pose, target=target, comp=rng.uniform(10.0, 20.0, (E, T)).astype(f32))
    grads = {k: grad_tape(rng, init[k].shape, f32) for k in KIN_GROUPS}
    lr = dict(zip(KIN_GROUPS, KIN_LR[(rule, bool(optimize_target))]))
    case = dict(E=E, D=D, T=T, rule=rule, clamp_box=bool(clamp_box), lr=lr, init=init, grads=grads,
                loss=loss_tape(E, last_improves, kin=True), margin=code_tape(E, T, 1)[..., 0],
                normal=code_tape(E, T, 3).astype(f32), box=box(T), kind="kin%d" % rule, dtype=f32,
                groups=KIN_GROUPS, hyper=ADAM if rule == 0 else RMSPROP)
    _freeze(case)
    return case


def _freeze(case):
    for v in list(case.values()) + list(case["init"].values()) + list(case["grads"].values()) + list(case["box"]):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)


PROB_E = (1, 63, 64, 65, 130)
PROB_DT = ((0, 1), (7, 4), (16, 4), (32, 8))
PROB_FROZEN = tuple((g,) for g in PROB_GROUPS) + (PROB_GROUPS,)
KIN1_T = (1, 3, 4, 5, 8)
KIN0_CHAINS = ("line16", "hand9", "tree8")   # 1, 4 and 8 tips; D = 15 (> 4·T), 17 (> 4·T, no multiple of T), 31


def kin1_E(T):
    return (1, 64 // T, 64 // T + 1, 130)


def kin0_E(T):
    return (1, 64 // T + 1, 67)


def prob_cases():
    """Every cdx_optimizer_step case of the device tests (sizes, then the frozen groups at E = 65, (7, 4))."""
    out = []
    for i, E in enumerate(PROB_E):
        for j, (D, T) in enumerate(PROB_DT):
            out.append(dict(E=E, D=D, T=T, best_after=(0, 3)[(i + j) % 2], last_improves=bool((i + j) % 3)))
    for fz in PROB_FROZEN:
        for clamp in (True, False):
            for ba in (0, 3):
                out.append(dict(E=65, D=7, T=4, best_after=ba, frozen=fz, clamp_target=clamp))
    return out


def kin1_cases():
    out = []
    for T in KIN1_T:
        for i, E in enumerate(kin1_E(T)):
            for clamp in (True, False):
                out.append(dict(rule=1, E=E, T=T, clamp_box=clamp, optimize_target=bool((i + T) % 2) or clamp,
                                last_improves=bool((i + clamp) % 2), nan_target=clamp))
    return out


def kin0_dims(chain):
    from tests import _chains
    d = _chains.descriptor(chain)
    return d.n_dofs, d.n_tips


def kin0_cases():
    out = []
    for chain in KIN0_CHAINS:
        D, T = kin0_dims(chain)
        for i, E in enumerate(kin0_E(T)):
            out.append(dict(rule=0, E=E, T=T, D=D, optimize_target=i != 1, last_improves=i != 2))
    return out


# ------------------------------------------------------------------ the update rule: torch.optim and the wide type
class TorchRule:
    """torch.optim.Adam (rule 0) / RMSprop (rule 1) on CPU tensors of the case's dtype, one param group per live
    group (a frozen group is not handed to the optimiser, as optimizer.py / optimizers.py do), stepped with the tape's
    gradients; then the loop's clamps."""

    def __init__(self, case):
        self.case = case
        self.p = {k: torch.from_numpy(case["init"][k].copy()) for k in case["groups"]}
        groups = [{"params": [self.p[k]], "lr": case["lr"][k]} for k in case["groups"] if case["lr"][k] != 0.0]
        h = case["hyper"]
        self.opt = None
        if groups and case["rule"] == 0:
            self.opt = torch.optim.Adam(groups, betas=(h["beta1"], h["beta2"]), eps=h["eps"])
        elif groups:
            self.opt = torch.optim.RMSprop(groups, alpha=h["alpha"], eps=h["eps"])

    def step(self, s):
        c = self.case
        for k in c["groups"]:
            self.p[k].grad = torch.from_numpy(c["grads"][k][s].copy())
        if self.opt is not None:
            self.opt.step()
        self.unclamped = {k: self.p[k].numpy().copy() for k in c["groups"]}
        lb, ub = (torch.from_numpy(b.astype(c["dtype"])).view(-1, 3) for b in c["box"])
        with torch.no_grad():
            if c["kind"] == "prob":
                self.p["comp"].clamp_(min=COMP_MIN)
                if c["clamp_target"]:
                    self.p["target"].clamp_(min=lb, max=ub)
            elif c["clamp_box"]:
                self.p["target"].clamp_(min=lb, max=ub)
                if c["rule"] == 1:
                    self.p["pose"].clamp_(min=lb, max=ub)

    def state(self):
        """{group: (p, m | None, v | None)} as numpy arrays (m is None for RMSprop, both for a frozen group)."""
        out = {}
        for k in self.case["groups"]:
            st = self.opt.state.get(self.p[k], {}) if self.opt is not None else {}
            m = st["exp_avg"].numpy().copy() if "exp_avg" in st else None
            v = st.get("exp_avg_sq", st.get("square_avg"))
            out[k] = (self.p[k].numpy().copy(), m, None if v is None else v.numpy().copy())
        return out


class WideRule:
    """The same formulas (torch/optim/adam.py, rmsprop.py: single-tensor form) in a wider type, for REF_ERR."""

    def __init__(self, case):
        self.case = case
        self.w = np.longdouble if case["dtype"] == np.float64 else np.float64
        self.p = {k: case["init"][k].astype(self.w) for k in case["groups"]}
        self.m = {k: np.zeros_like(self.p[k]) for k in case["groups"]}
        self.v = {k: np.zeros_like(self.p[k]) for k in case["groups"]}

    def step(self, s):
        c, w, h = self.case, self.w, self.case["hyper"]
        for k in c["groups"]:
            lr = w(c["lr"][k])
            if lr == 0:
                continue
            g = c["grads"][k][s].astype(w)
            if c["rule"] == 0:
                b1, b2, t = w(h["beta1"]), w(h["beta2"]), s + 1
                self.m[k] = self.m[k] + (1 - b1) * (g - self.m[k])
                self.v[k] = self.v[k] * b2 + (1 - b2) * g * g
                denom = np.sqrt(self.v[k]) / np.sqrt(1 - b2 ** t) + w(h["eps"])
                self.p[k] = self.p[k] - (lr / (1 - b1 ** t)) * self.m[k] / denom
            else:
                a = w(h["alpha"])
                self.v[k] = self.v[k] * a + (1 - a) * g * g
                self.p[k] = self.p[k] - lr * g / (np.sqrt(self.v[k]) + w(h["eps"]))
        lb, ub = (b.astype(w).reshape(-1, 3) for b in c["box"])
        if c["kind"] == "prob":
            self.p["comp"] = clamp(self.p["comp"], COMP_MIN, None)
            if c["clamp_target"]:
                self.p["target"] = clamp(self.p["target"], lb, ub)
        elif c["clamp_box"]:
            self.p["target"] = clamp(self.p["target"], lb, ub)
            if c["rule"] == 1:
                self.p["pose"] = clamp(self.p["pose"], lb, ub)

    def state(self):
        live = {k: self.case["lr"][k] != 0.0 for k in self.case["groups"]}
        return {k: (self.p[k], self.m[k] if live[k] and self.case["rule"] == 0 else None,
                    self.v[k] if live[k] else None) for k in self.case["groups"]}


def clamp(x, lo, hi):
    """torch.clamp: a NaN stays NaN (np.fmax / np.fmin would replace it)."""
    if lo is not None:
        x = np.where(x < lo, np.asarray(lo, x.dtype), x)
    if hi is not None:
        x = np.where(x > hi, np.asarray(hi, x.dtype), x)
    return x


def deviation(got, ref, scale=None):
    """max |got − ref| / (|ref| + scale) over the finite entries of ref (scale None: relative to ref itself, and where
    ref is 0 got must be 0); inf when the NaN patterns differ."""
    got, ref = np.asarray(got, np.longdouble), np.asarray(ref, np.longdouble)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    ok = np.isfinite(ref)
    if scale is None:
        zero = ok & (ref == 0)
        if (got[zero] != 0).any():
            return float("inf")
        ok &= ref != 0
    if not ok.any():
        return 0.0
    den = np.abs(ref[ok]) + (0 if scale is None else scale)
    return float((np.abs(got[ok] - ref[ok]) / den).max())


def rule_errors(case, got, ref, s, worst):
    """Folds the deviations of state `got` from `ref` after step s into worst {p, m, v}."""
    for k in case["groups"]:
        lr = case["lr"][k]
        if lr == 0.0:
            continue
        worst["p"] = max(worst["p"], deviation(got[k][0], ref[k][0], lr * (s + 1)))
        if ref[k][1] is not None and "m" in worst:
            worst["m"] = max(worst["m"], deviation(got[k][1], ref[k][1]))
        worst["v"] = max(worst["v"], deviation(got[k][2], ref[k][2]))
    return worst


_TRAJECTORIES = {}


def trajectory(case):
    """torch.optim's (state, unclamped parameters) after every step of a case, computed once and shared (read-only;
    the cases are cached objects)."""
    if id(case) not in _TRAJECTORIES:
        ref, out = TorchRule(case), []
        for s in range(S):
            ref.step(s)
            out.append((ref.state(), ref.unclamped))
        _TRAJECTORIES[id(case)] = (case, out)
    return _TRAJECTORIES[id(case)][1]


def measure_reference():
    """→ {kind: {p, m, v}}: torch.optim against WideRule, maximised over every step of every case."""
    out = {}
    for kind, cases in (("prob", prob_cases()), ("kin0", kin0_cases()), ("kin1", kin1_cases())):
        worst = {q: 0.0 for q in REF_ERR[kind]}
        for kw in cases:
            case = prob_case(**kw) if kind == "prob" else kin_case(**kw)
            wide, tr = WideRule(case), trajectory(case)
            for s in range(S):
                wide.step(s)
                rule_errors(case, tr[s][0], wide.state(), s, worst)
        out[kind] = worst
    return out


# ------------------------------------------------------------------ the bookkeeping (include/cdx.h)
class ProbBook:
    """cdx.h "fused optimizer step": the best-iterate update before the step, only when s > best_after — per candidate,
    total_loss < opt_value copies the loss, the candidate's margins and the parameters the closure saw;
    opt_palm = [palm_pos, palm_ori]."""

    def __init__(self, E, D, T, best_after):
        self.best_after = best_after
        self.value = np.full(E, np.inf)
        self.margin, self.q, self.comp = np.full((E, T), FILL), np.full((E, D), FILL), np.full((E, T), FILL)
        self.target, self.palm = np.full((E, T, 3), FILL), np.full((E, 6), FILL)

    def update(self, s, loss, margin, q, comp, target, palm_pos, palm_ori):
        flag = (loss < self.value) if s > self.best_after else np.zeros(len(loss), bool)  # (NaN < x is False)
        self.value[flag] = loss[flag]
        self.margin[flag], self.q[flag] = margin[flag], q[flag]
        self.comp[flag], self.target[flag] = comp[flag], target[flag]
        self.palm[flag] = np.hstack([palm_pos, palm_ori])[flag]
        return flag

    def state(self):
        return dict(opt_value=self.value, opt_margin=self.margin, opt_q=self.q, opt_comp=self.comp,
                    opt_target=self.target, opt_palm=self.palm)


class KinBook:
    """cdx.h "Kin / SDF optimiser step" 1.: per candidate, loss < opt_value — compared in double, stored as float —
    copies the pose, target and compliance the loss was computed on; margin / normal are the WHOLE batch's of the last
    iteration in which ANY candidate improved.  (The device commits those one launch late: after launch s its
    opt_margin is this model's before update s; after `finalize`, this model's.)"""

    def __init__(self, E, T, pose_shape):
        self.value = np.full(E, np.inf, np.float32)
        self.pose = np.full(pose_shape, FILL, np.float32)
        self.target, self.comp = np.full((E, T, 3), FILL, np.float32), np.full((E, T), FILL, np.float32)
        self.margin, self.normal = np.full((E, T), FILL), np.full((E, T, 3), FILL, np.float32)

    def update(self, loss, margin, normal, pose, target, comp):
        flag = loss < self.value.astype(np.float64)
        self.value[flag] = loss[flag].astype(np.float32)
        self.pose[flag], self.target[flag], self.comp[flag] = pose[flag], target[flag], comp[flag]
        if flag.any():
            self.margin, self.normal = margin.copy(), normal.copy()
        return flag

    def state(self, batch=True):
        out = dict(opt_value=self.value, opt_pose=self.pose, opt_target=self.target, opt_comp=self.comp)
        if batch:
            out.update(opt_margin=self.margin, opt_normal=self.normal)
        return {k: v.copy() for k, v in out.items()}


def improvers(case):
    """[S, E] bool: which candidate improves in which iteration of the case's loss tape, by the model."""
    E, T = case["E"], case["T"]
    out = []
    if case["kind"] == "prob":
        book, i = ProbBook(E, case["D"], T, case["best_after"]), case["init"]
        for s in range(S):
            out.append(book.update(s, case["loss"][s], case["margin"][s], i["q"], i["comp"], i["target"],
                                   i["palm_pos"], i["palm_ori"]))
    else:
        book, i = KinBook(E, T, case["init"]["pose"].shape), case["init"]
        for s in range(S):
            out.append(book.update(case["loss"][s], case["margin"][s], case["normal"][s], i["pose"], i["target"],
                                   i["comp"]))
    return np.array(out)


def same_bits(a, b):
    """Bit equality with NaN patterns compared as patterns (equal_nan): same shape, dtype, NaNs in the same places,
    the same bits elsewhere."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


# ------------------------------------------------------------------ the device harness
class Arena:
    """Every buffer of a run in one byte array: each buffer's rows are followed directly by a guard of the same bytes
    (at least two rows and 64 bytes, GUARD_BYTE), so a write one row — or one element — past a buffer lands in a guard.
    One copy to the device before a launch, one back after it."""

    def __init__(self):
        self.spec, self.size = {}, 0

    def add(self, name, array):
        a = np.ascontiguousarray(array)
        row = a.nbytes // a.shape[0] if a.ndim and a.shape[0] else a.itemsize
        guard = max(64, 2 * row)
        self.spec[name] = (self.size, a.dtype, a.shape, a.nbytes, a)
        self.size += -(-(a.nbytes + guard) // 64) * 64

    def build(self, device=None):
        self.host = np.full(self.size, GUARD_BYTE, np.uint8)
        self.mask = np.ones(self.size, bool)   # True: a guard byte
        for name, (off, _, _, nb, a) in self.spec.items():
            self.host[off:off + nb] = a.reshape(-1).view(np.uint8)
            self.mask[off:off + nb] = False
            self.spec[name] = self.spec[name][:4]
        self.dev = None
        if device is not None:
            self.dev = torch.empty(max(self.size, 64), dtype=torch.uint8, device=device)
        return self

    def __getitem__(self, name):
        off, dt, shape, nb = self.spec[name]
        return self.host[off:off + nb].view(dt).reshape(shape)

    def ptr(self, name):
        return self.dev.data_ptr() + self.spec[name][0]

    def upload(self):
        self.dev[:self.size].copy_(torch.from_numpy(self.host))

    def download(self):
        self.host[:] = self.dev[:self.size].cpu().numpy()

    def guards_intact(self):
        return bool((self.host[self.mask] == GUARD_BYTE).all())

    def snapshot(self):
        return {k: self[k].copy() for k in self.spec}


def check_rule(case, before, after, ref, s, worst):
    """The device's parameters and moments after step s (dicts of arrays by buffer name) against torch's step-s record
    `ref` = (state, unclamped parameters): a frozen group's moments bit-untouched and its parameter the clamp of what
    it was, bit for bit; a live group within TOL, NaN where torch's is, inside its bounds, and exactly ON a bound
    wherever torch's unclamped value passes it by more than the tolerance."""
    kind, tol = case["kind"], TOL[case["kind"]]
    state, unclamped = ref
    lb, ub = (b.astype(case["dtype"]).reshape(-1, 3) for b in case["box"])
    got = {}
    for k in case["groups"]:
        lo = hi = None
        if kind == "prob" and k == "comp":
            lo = np.asarray(COMP_MIN, case["dtype"])
        elif k == "target" and (case["clamp_target"] if kind == "prob" else case["clamp_box"]):
            lo, hi = lb, ub
        elif kind == "kin1" and k == "pose" and case["clamp_box"]:
            lo, hi = lb, ub
        p, m, v = after[k], after["m_" + k], after["v_" + k]
        if case["lr"][k] == 0.0:
            assert same_bits(p, clamp(before[k], lo, hi)), (k, s)
            assert same_bits(m, before["m_" + k]) and same_bits(v, before["v_" + k]), (k, s)
            continue
        got[k] = (p, m if case["rule"] == 0 else None, v)
        if case["rule"] == 1:
            assert same_bits(m, before["m_" + k]), (k, s)  # RMSprop has no first moment
        un = unclamped[k].astype(np.float64)
        assert np.array_equal(np.isnan(p), np.isnan(un)), (k, s)
        slack = tol["p"] * (np.abs(un) + case["lr"][k] * (s + 1))
        with np.errstate(invalid="ignore"):
            if lo is not None:
                assert not (p < lo).any(), (k, s)
                assert (p == lo)[un + slack < lo].all(), (k, s)
            if hi is not None:
                assert not (p > hi).any(), (k, s)
                assert (p == hi)[un - slack > hi].all(), (k, s)
    return rule_errors(case, got, {k: state[k] for k in got}, s, worst)


def make_case(kind, kw):
    """prob_case / kin_case by keyword dict (cached: the same object, trajectory and all, for every user)."""
    return prob_case(**kw) if kind == "prob" else kin_case(**kw)


# ------------------------------------------------------------------ the one-launch copy of the Kin step
# kin_cost4_kernel<…, STEP> cannot be fed a scripted loss, so this loop is BUILT to stop improving: the Allegro hand,
# two candidates about 800 iterations into the oracle's Kin loop on the banana (tests/golden/steps_fused_kin.npz: q,
# target, palm offset and the oracle's loss tape), restarted with fresh Adam moments and every compliance at 1.0 —
# Adam's first 0.2 steps then swing the force-closure reward, the loss falls for three iterations and stays 22 or more
# above the best for the other five, the last included.  test_steps_cpu pins that on oracle.kin_sdf_loop's tape.
FUSED = dict(robot="allegro", E=2, iters=8, comp=1.0, noise_seed=900, fixture="steps_fused_kin.npz")
FUSED_LOSS_TOL = 1e-4  # the project's bound on the Kin loop's per-candidate loss against the oracle (test_gpu_configs)
FUSED_IMPROVERS = np.array([[1, 1]] * 3 + [[0, 0]] * 5, bool)  # [iteration, candidate] on the oracle's tape


def fused_inputs():
    """→ dict(links, offsets, palm [3], q [E, 16], target [E, 4, 3], comp [E, 4] (float32), noise [iters, E, 3, 3] and
    oracle_loss [iters, E] (float64))."""
    from compliancedex_amd.urdf import load_robot
    from tests._helpers import golden
    d, cfg = golden(FUSED["fixture"]), load_robot(FUSED["robot"])["config"]
    E, iters = FUSED["E"], FUSED["iters"]
    return dict(links=cfg["ee_link_name"], offsets=cfg["ee_link_offset"], palm=d["palm"], q=d["q"], target=d["target"],
                comp=np.full((E, 4), FUSED["comp"], np.float32),
                noise=np.random.default_rng(FUSED["noise_seed"]).random((iters, E, 3, 3)), oracle_loss=d["loss"])


def decisions(L):
    """A loss tape [S, E] (float64; the best is kept as float, as the Kin step keeps it) → (improved [S, E] bool,
    gap [S, E] = |loss − best before it|, inf at the first iteration)."""
    best = np.full(L.shape[1], np.inf, np.float32)
    flags, gaps = [], []
    for row in L:
        f = row < best.astype(np.float64)
        gaps.append(np.abs(row - best.astype(np.float64)))
        best[f] = row[f].astype(np.float32)
        flags.append(f)
    return np.array(flags), np.array(gaps)
