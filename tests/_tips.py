"""Prob-mode closure cases off the four-fingertip default: tip subsets of the synthetic chains (tests/_chains.py) with
T = 1..8 fingertips, the gravity spring on and off, K = 1..4 pregrasp levels over Lq = 1..3 distinct query rows, and the
palm term on and off.  A covering list, not a cross product: every T ∈ {1, 2, 3, 5, 8} meets gravity off (T = 1 cannot:
one point without the gravity spring has residual exactly 0 and the reference is NaN) and a non-default level set, T = 4
meets gravity off with Lq > 1, and ``optimize_palm=False`` appears.

Comparisons are per candidate (``per_candidate``): max|a − b| over one candidate's entries of a tensor over max|b| over
the same entries, so that one candidate with a large gradient cannot hide the others.  A candidate is left out of the
gradient comparisons (never out of the loss / margin / flip / NaN comparisons) only when the oracle alone calls it
ill-conditioned (``ill_conditioned``); ``reference`` asserts that this removes at most _chains.MAX_EXCLUDED of a case.
"""
import functools
import os

import numpy as np
import torch

from tests import _chains as ch

E_REF = 67
TOL = 1e-4          # the project's closure-vs-oracle bar
PROBE_EPS = 2.0 ** -23
PROBE_TOL = 1e-5
GRADS = ("grad_q", "grad_comp", "grad_target", "grad_palm_pos", "grad_palm_ori")
VALUES = ("total_loss", "total_margin", "pregrasp_tip")


def _per_finger(base, step, T):
    return [base + step * f for f in range(T)]


def levels(name, T):
    """→ (coefficients [K][T], weights [K]).  default: K = 3, Lq = 1; k1: K = 1; k2: K = 2, Lq = 2; k4: K = 4 over
    Lq = 3 distinct rows (levels 0 and 2 share one) with a different coefficient for every fingertip."""
    if name == "default":
        return [[0.8] * T] * 3, [0.1, 0.8, 0.1]
    if name == "k1":
        return [[0.8] * T], [1.0]
    if name == "k2":
        return [[0.8] * T, [0.9] * T], [0.3, 0.7]
    assert name == "k4"
    a = _per_finger(0.8, -0.01, T)
    return [a, _per_finger(0.9, -0.01, T), a, _per_finger(0.7, 0.02, T)], [0.1, 0.6, 0.2, 0.1]


# The seeds were searched upwards from 2 for one at which the oracle alone leaves at most two of the 67 candidates —
# one of a screened case's 32 — out of the gradient comparisons (``ill_conditioned``; the cap is MAX_EXCLUDED = 5 %).  Two
# cases lose about 13 % of their candidates at a typical seed (many margins per candidate: K·T = 32; three points
# without the gravity spring) and reach the cap at E = 67 for one seed in a thousand at best: they run E = 35 (one
# excluded), still more than one workgroup of every kernel (K·E ≥ 70 level threads, 35·GS ≥ 140 combine threads).
#        name               chain     tips              gravity levels  optimize_palm seed  E
TABLE = (("t1_k2",          "line16", (0,),              True,  "k2",      True,    2, 67),
         ("t1_k1_nopalm",   "line16", (0,),              True,  "k1",      False,    2, 67),
         ("t2_nograv",      "hand16", (1, 2),            False, "default", True,    2, 67),
         ("t2_k4",          "hand16", (1, 2),            True,  "k4",      True,    6, 67),
         ("t3_nograv_k2",   "hand8",  (0, 1, 3),         False, "k2",      True,  411, 35),
         ("t3_k1_nopalm",   "hand8",  (0, 1, 3),         True,  "k1",      False,    2, 67),
         ("t4_nograv_k2",   "hand9",  (0, 1, 2, 3),      False, "k2",      True,  174, 67),
         ("t5_nograv",      "tree8",  (0, 1, 2, 3, 4),   False, "default", True,    7, 67),
         ("t5_k4",          "tree8",  (0, 1, 2, 3, 4),   True,  "k4",      True,  155, 67),
         ("t8_nograv_k1",   "tree8",  tuple(range(8)),   False, "k1",      True,    4, 67),
         ("t8_k4",          "tree8",  tuple(range(8)),   True,  "k4",      True,   36, 35),
         ("t8_k2_nopalm",   "tree8",  tuple(range(8)),   True,  "k2",      False,   81, 67))
CASES = tuple(r[0] for r in TABLE)
# screened closures (name, E, seed): the E of the record — Lq·E·T ≥ 4096 all-tip rows, Lq·(E − 64)·T < 4096, E no
# multiple of 64 — and the 32 candidates of each that the oracle checks
SCREENED = (("t1_k1_nopalm", 4100, 2), ("t3_k1_nopalm", 1400, 3), ("t5_nograv", 830, 2), ("t8_nograv_k1", 520, 2),
            ("t3_nograv_k2", 690, 8))
SLICE = 32


class Case:
    def __init__(self, name, chain, tips, gravity, level_set, optimize_palm, seed=2, E=E_REF):
        _, links = ch.bodies(chain)
        offs = ch.tip_offsets(chain)
        self.name, self.chain, self.gravity, self.optimize_palm = name, chain, gravity, optimize_palm
        self.seed, self.E = seed, E
        self.links = [links[i] for i in tips]
        self.offsets = [offs[i] for i in tips]
        self.T = len(tips)
        self.coeffs, self.weights = levels(level_set, self.T)
        self.K = len(self.coeffs)
        self.Lq = len({tuple(r) for r in self.coeffs})

    def descriptor(self):
        return ch.chain(self.chain).descriptor(self.links, self.offsets)

    @property
    def D(self):
        return ch.descriptor(self.chain).n_dofs

    def problem(self, gpis_desc=None):
        from compliancedex_amd.problem import build_problem
        return build_problem(self.descriptor(), gpis_desc, ref_q=[0.0] * self.D, coeffs=self.coeffs,
                             weights=self.weights, gravity=self.gravity, optimize_palm=self.optimize_palm)

    def oracle_problem(self):
        from oracle.cdx_oracle import OracleChain, OracleProblem
        from tests._helpers import oracle_gpis
        b, _ = ch.bodies(self.chain)
        return OracleProblem(OracleChain(b), self.links, self.offsets, [0.0] * self.D, oracle_gpis("banana"),
                             gravity=self.gravity, optimize_palm=self.optimize_palm, coeffs=self.coeffs,
                             weights=self.weights)

    def optimizer(self, tmp_path, device, **kw):
        """ProbabilisticGraspOptimizer on the chain's JSON file with the subset as its fingertips."""
        from compliancedex_amd import ProbabilisticGraspOptimizer
        path = ch.write_json(self.chain, tmp_path, config=dict(ee_link_name=self.links, ee_link_offset=self.offsets))
        return ProbabilisticGraspOptimizer(path, self.links, self.offsets, ref_q=[0.0] * self.D,
                                           pregrasp_coefficients=self.coeffs, pregrasp_weights=self.weights,
                                           gravity=self.gravity, optimize_palm=self.optimize_palm, device=device, **kw)


@functools.lru_cache(None)
def case(name):
    return Case(*TABLE[CASES.index(name)])


# the case of the record: tree8's eight tips, uniform levels 0.8 / 0.9 / 0.8 / 0.7, E = 5, whose candidate 3 has a
# gradient 80 × its neighbours' (a margin just above the −0.9999 clamp) and misses a whole-batch comparison
E5 = Case("t8_e5", "tree8", tuple(range(8)), True, "default", True)
E5.coeffs, E5.weights = [[0.8] * 8, [0.9] * 8, [0.8] * 8, [0.7] * 8], [0.1, 0.6, 0.2, 0.1]
E5.K, E5.Lq = 4, 3


def closure_inputs(c, E=None, seed=None):
    """(q [E, D], comp [E, T], target [E, T, 3], palm [E, 6], noise [K·E, 3, 3]) as _chains.closure_inputs draws them
    (workloads.prob_inputs around the banana centre, joints spread over ±0.3 rad, a replayed Kabsch noise draw), with
    T targets and compliances per candidate and one noise matrix per (level, candidate)."""
    from compliancedex_amd.workloads import DATA, prob_inputs
    seed = c.seed if seed is None else seed
    E = c.E if E is None else E
    q, _, _, palm = prob_inputs([0.0] * c.D, E, seed=seed, spread=False)
    center = np.load(os.path.join(DATA, "banana_center.npy"))
    rng = np.random.default_rng(seed)
    if E > 6:  # (prob_inputs' draws for q and the palm come first: at T = 4, K = 3 these are _chains' inputs)
        rng.standard_normal((E, c.D + 6))
    target = np.tile(center, (E, c.T, 1)).astype(np.float64) + 0.01 * rng.standard_normal((E, c.T, 3))
    comp = np.tile(np.resize(np.array([10.0, 10.0, 10.0, 20.0]), c.T), (E, 1))
    rng = np.random.default_rng(seed + 1)
    q = q + 0.3 * rng.standard_normal(q.shape)
    return q, comp, target, palm, rng.random((c.K * E, 3, 3))


def take(inputs, rows, K):
    """The inputs of the candidates `rows` alone (their noise matrices at every level)."""
    q, comp, target, palm, noise = inputs
    E = q.shape[0]
    rows = np.asarray(rows)
    nz = noise.reshape(K, E, 3, 3)[:, rows].reshape(-1, 3, 3)
    return q[rows], comp[rows], target[rows], palm[rows], nz


def oracle_closure(c, inputs, q_scale=1.0):
    from oracle.cdx_oracle import closure_with_grads
    q, comp, target, palm, noise = inputs
    return closure_with_grads(c.oracle_problem(), q * q_scale, comp, target, palm, noise)


def _scale(b):
    """max|b| over each candidate's entries, [E, 1, …] (1 where a candidate has no finite entry or is all zero)."""
    b = np.asarray(b, np.float64)
    flat = np.abs(b.reshape(b.shape[0], -1))
    with np.errstate(invalid="ignore"):
        s = np.where(np.isnan(flat), 0.0, flat).max(1)
    s = np.where(s > 0, s, 1.0)
    return s.reshape((-1,) + (1,) * (b.ndim - 1))


def per_candidate(a, b):
    """(a, b) each divided by max|b| of its candidate: rel_err / assert_rel of the pair is then the largest
    per-candidate error max|a_e − b_e| / max|b_e| (and still demands NaNs at the same positions)."""
    s = _scale(b)
    return np.asarray(a, np.float64) / s, np.asarray(b, np.float64) / s


def ill_conditioned(ref, *probes):
    """[E] bool from oracle evaluations alone: `ref` and the `probes`, the same closure with q scaled by 1 + 2⁻²³ and
    by 1 − 2⁻²³ (every joint moves by one or two float32 ulps, the size of the rounding any float32 FK commits).  A
    candidate is ill-conditioned when in either probe one of its five gradients moves by more than PROBE_TOL relative
    to that gradient's largest entry for the candidate: it amplifies the last bit of the joint angles by more than
    1e-5 / 1.2e-7 ≈ 80, and no float32 FK can meet 1e-4 there.  What makes such candidates is a friction margin next
    to the −0.9999 clamp, where the reward's 0.8 / (margin + 1) reaches 8e3.  Both signs are needed: a candidate with
    a margin within an ulp's reach of the clamp itself answers on one side only (clamped, the term's gradient is 0) —
    t4_nograv_k2's candidate 15, |g_q| = 1e5, moves by 3e-6 upwards and 4e-5 downwards.  A candidate whose gradient is
    not finite in an evaluation is not excluded for it (its NaN mask is compared)."""
    bad = np.zeros(len(ref["total_loss"]), bool)
    for probe in probes:
        for k in GRADS:
            a, b = per_candidate(probe[k], ref[k])
            with np.errstate(invalid="ignore"):
                d = np.abs(a - b).reshape(len(bad), -1)
            bad |= np.where(np.isfinite(d), d, 0.0).max(1) > PROBE_TOL
    return bad


def keep_mask(c, inputs, ref):
    return ~ill_conditioned(ref, oracle_closure(c, inputs, 1.0 + PROBE_EPS), oracle_closure(c, inputs, 1.0 - PROBE_EPS))


@functools.lru_cache(None)
def reference(name, E=None):
    """The oracle's closure of a case at its E candidates, computed once and shared (read-only), with ``keep`` [E] marking
    the candidates that stay in the gradient comparisons; at most _chains.MAX_EXCLUDED of them are left out."""
    c = E5 if name == E5.name else case(name)
    E = c.E if E is None else E
    inputs = closure_inputs(c, E)
    ref = oracle_closure(c, inputs)
    ref["keep"] = keep_mask(c, inputs, ref)
    ref["inputs"] = inputs
    if c is not E5:  # (E5 is there for its one ill-conditioned candidate of five)
        assert 1.0 - ref["keep"].mean() <= ch.MAX_EXCLUDED, (name, E, 1.0 - ref["keep"].mean())
    for v in ref.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return ref


def single_row(name):
    """The candidate that stands alone in the E = 1 closures: the first that stays in the gradient comparisons."""
    return int(np.flatnonzero(reference(name)["keep"])[0])


def screened_rows(E):
    """32 fixed candidates of a screened case, spread over its 64-candidate tiles, from the first to the last."""
    return np.unique(np.linspace(0, E - 1, SLICE).round().astype(np.int64))


@functools.lru_cache(None)
def screened_reference(name, E):
    """The inputs of a screened case at its E and the oracle's closure of screened_rows(E) alone."""
    c = case(name)
    seed = [s for n, e, s in SCREENED if (n, e) == (name, E)][0]
    inputs = closure_inputs(c, E, seed)
    part = take(inputs, screened_rows(E), c.K)
    ref = oracle_closure(c, part)
    ref["keep"] = keep_mask(c, part, ref)
    ref["inputs"] = inputs
    assert 1.0 - ref["keep"].mean() <= ch.MAX_EXCLUDED, (name, E, 1.0 - ref["keep"].mean())
    return ref


def slice_reference(ref, rows, K):
    """Rows `rows` of a reference (its flips at every level)."""
    rows = np.asarray(rows)
    E = len(ref["total_loss"])
    out = {k: ref[k][rows] for k in VALUES + GRADS + ("keep",)}
    out["flip"] = ref["flip"].reshape(K, E)[:, rows].reshape(-1)
    return out


def check_closure(got, ref, tag, log=None):
    """The closure-vs-oracle comparison of one case: flips equal, losses / margins / pregrasp tips per candidate on
    every candidate, the five gradients per candidate on ref["keep"].  → dict of the measured errors."""
    from tests._helpers import assert_rel
    assert np.array_equal(np.asarray(got["flip"]).astype(bool), ref["flip"]), tag
    keep = ref["keep"]
    errs = {}
    for k in VALUES:
        if k in got:
            errs[k] = assert_rel(*per_candidate(got[k], ref[k]), TOL, f"{tag}:{k}")
    for k in GRADS:
        # NaN masks on every candidate, values on the kept ones
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (tag, k)
        errs[k] = assert_rel(*per_candidate(np.asarray(got[k])[keep], ref[k][keep]), TOL, f"{tag}:{k}") \
            if keep.any() else 0.0
    errs["excluded"] = float(1.0 - keep.mean())
    if log is not None:
        log(tag, errs)
    return errs


# ------------------------------------------------------------------ force equilibrium rows
FORCE_TIPS = (1, 2, 3, 4, 5, 8)
FORCE_B = 130
FORCE_COM = (0.0, 0.01, -0.02)
FORCE_MASS = 0.1


@functools.lru_cache(None)
def force_rows(T, gravity, mu, f32=False):
    """B = 130 generic rows of force_eq_reward (tips 0.03·randn from their targets, compliances in U(10, 200), unit
    normals, random in two thirds of the rows, the COM off the origin) and the oracle's outputs and gradients of Σ cr·reward + Σ cf·force_norm, with the
    conditions that keep a comparison from passing on thin data: at least 2 flipped rows, at least 8 rows with a
    clamped margin and at least 8 without (T = 1 without gravity: the residual is rounding noise, nothing to count).
    ``f32``: the inputs rounded to float32 (what the op computes on when handed float32 tensors)."""
    from oracle.cdx_oracle import force_eq_reward
    B = FORCE_B
    rng = np.random.default_rng(500 + 10 * T + (1 if gravity else 0) + (2 if mu == 1 else 0))
    target = 0.05 * rng.standard_normal((B, T, 3))
    tip = target + 0.03 * rng.standard_normal((B, T, 3))
    comp = rng.uniform(10.0, 200.0, (B, T))
    normal = rng.standard_normal((B, T, 3))
    # (random normals leave a row of many fingertips no chance of staying off the −0.9999 clamp: in the first third
    # of the rows the normals lean towards the fingertips' displacement)
    lean = (tip - target) / np.linalg.norm(tip - target, axis=2, keepdims=True)
    normal[:B // 3] = lean[:B // 3] + 0.3 * normal[:B // 3]
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    noise = rng.random((B, 3, 3))
    cr, cf = rng.standard_normal(B), rng.standard_normal((B, T))
    if f32:
        tip, target, comp, normal = (x.astype(np.float32).astype(np.float64) for x in (tip, target, comp, normal))
    tt, gt, ct = (torch.from_numpy(x).clone().requires_grad_(True) for x in (tip, target, comp))
    reward, margin, fn, flip = force_eq_reward(tt, gt, ct, mu, torch.from_numpy(normal), torch.from_numpy(noise),
                                               mass=FORCE_MASS, gravity=10.0 if gravity else None, COM=FORCE_COM)
    ((reward * torch.from_numpy(cr)).sum() + (fn * torch.from_numpy(cf)).sum()).backward()
    out = dict(tip=tip, target=target, comp=comp, normal=normal, noise=noise, cr=cr, cf=cf,
               reward=reward.detach().numpy(), margin=margin.detach().numpy(), force_norm=fn.detach().numpy(),
               flip=flip.numpy(), grad_tip=tt.grad.numpy(), grad_target=gt.grad.numpy(), grad_comp=ct.grad.numpy())
    if T > 1 or gravity:
        clamped = (out["margin"] == -0.9999).any(1)
        assert out["flip"].sum() >= 2, (T, gravity, mu, int(out["flip"].sum()))
        assert clamped.sum() >= 8 and (~clamped).sum() >= 8, (T, gravity, mu, int(clamped.sum()))
        assert np.isfinite(out["reward"]).all()
    for v in out.values():
        v.setflags(write=False)
    return out


def force_desc(T, gravity, mu):
    from compliancedex_amd.force_eq import force_eq_descriptor
    return force_eq_descriptor(T, mu, FORCE_MASS, 10.0 if gravity else None, COM=list(FORCE_COM))
