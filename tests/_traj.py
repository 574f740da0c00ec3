"""Shared inputs, a numpy float64 statement and the checks of the trajectory rule (csrc/cdx_traj.h), run by
test_traj_cpu.py on libcdx_host.so and by test_gpu_traj.py on the GPU.

A backend is an object with ``seed(G, seeds, T, D, qs, qg, amp, seed, out) → rc`` and ``step(par, E, traj, g_c, cost_t,
iteration, cost, best_cost, best_iter, best_traj) → rc`` on numpy arrays written in place (None: NULL), and, for the
loop, ``spheres`` / ``model`` / ``term`` of tests/_hand_term.py's backends.

Shapes (T, D, E): SHAPES holds every T ∈ {3, 4, 5, 6, 64}, D ∈ {1, 16, 23, 32} and E ∈ {1, 63, 65, 257} once and the
corners (3, 1, 1) and (64, 32, 257).  A family is made for (T, D) with 257 rows; a test takes its first E.

Families.  Joint bounds: lower ∈ [−2, −1], upper ∈ [1, 2], and for D > 1 one joint without a lower and one without an upper
bound.  Rows alternate between "inside" (|q| ≤ 0.9: no limit hinge can be active, the hinge starts at |q| ≥ 0.98) and
"wide" (|q| ≤ 2.3, one interior entry of joint 0 beyond 2.05); ``family`` asserts on the inputs that the limit hinge is active somewhere in at least a quarter of
the rows and nowhere in at least a quarter.  g_c has entries of magnitude 200 – 300 with random signs: then every
column's ‖A_T⁻¹g‖∞ ≥ 10 (asserted), so step·‖A_T⁻¹g‖∞ ≥ 0.5 at STEP = 0.05.  The issue's bound on the stepped trajectory,
16·cond(A_T)·2⁻⁵²·step·‖A_T⁻¹g‖∞, then also covers the two roundings of the subtraction q − step·x (the kernel's and
numpy's, together at most 2⁻⁵²·(2.3 + step·‖x‖∞), which is below 16·2⁻⁵²·step·‖x‖∞ once step·‖x‖∞ ≥ 0.16).

Tolerances (the issue's): seed bit for bit; cost parts |Δ| ≤ 1e-12·Σ|term|; gradient |Δ| ≤ 1e-12·Σ|contribution|
(Σ over the products that enter an entry: the stencil's |coef·q| terms, |w_c·g_c|, and w_l·(|q| + |bound| + m_lim) for
an active hinge); stepped trajectory as above with cond(A_T) computed here; the one-step fixed point
‖A_T ξ + b‖∞ ≤ 16·cond(A_T)·2⁻⁵²·16·max|q|.
"""
import ctypes as C
import functools

import numpy as np
import torch

from compliancedex_amd import _native as N
from compliancedex_amd.trajectory import smoothness_matrix
from tests import _hand as H
from tests._sample import numpy_philox

SHAPES = ((3, 1, 1), (4, 16, 63), (5, 23, 65), (6, 32, 257), (64, 23, 65), (64, 32, 257))
IDS = [f"T{t}-D{d}-E{e}" for t, d, e in SHAPES]
assert {s[0] for s in SHAPES} == {3, 4, 5, 6, 64} and {s[1] for s in SHAPES} == {1, 16, 23, 32}
assert {s[2] for s in SHAPES} == {1, 63, 65, 257}
E_MAX = 257
GUARD = 4
STEP = 0.05
WEIGHTS = dict(w_smooth=1.3, w_col=0.7, w_lim=2.1, m_lim=0.02)
EPS = 2.0 ** -52
OUTS = ("traj", "cost", "best_cost", "best_iter", "best_traj")


def params(lower, upper, T, step=STEP, **over):
    v = dict(WEIGHTS, **over)
    p = N.CdxTrajParams()
    for d in range(len(lower)):
        p.lower[d], p.upper[d] = float(lower[d]), float(upper[d])
    p.w_smooth, p.w_col, p.w_lim, p.m_lim, p.step = v["w_smooth"], v["w_col"], v["w_lim"], v["m_lim"], float(step)
    p.T, p.n_dofs = T, len(lower)
    return p


def cond(T):
    return float(np.linalg.cond(smoothness_matrix(T)))


# ------------------------------------------------------------------ the numpy statement
def accelerations(q):
    """a [E, T, D] of q [E, T, D] with the rest-to-rest virtual points."""
    p = np.concatenate([q[:, :1], q, q[:, -1:]], 1)
    return (p[:, :-2] - 2.0 * p[:, 1:-1]) + p[:, 2:]


def hinge(q, lower, upper, m):
    return np.maximum(q - (upper - m), 0.0) - np.maximum((lower + m) - q, 0.0)


def statement(q, g_c, cost_t, lower, upper, step=STEP, **over):
    """One step in numpy float64 → dict(us, uc, ul [E], abs_us, abs_uc, abs_ul (Σ|term|), U, g [E, n, D] the gradient on
    the interior, abs_g (Σ|contribution|), x = A_T⁻¹g by a dense solve, new [E, T, D], active [E] rows with an active
    limit hinge)."""
    v = dict(WEIGHTS, **over)
    E, T, D = q.shape
    a = accelerations(q)
    us = 0.5 * (a * a).sum((1, 2))
    p = hinge(q[:, 1:-1], lower, upper, v["m_lim"])
    ul = 0.5 * (p * p).sum((1, 2))
    uc = cost_t.sum(1) if cost_t is not None else np.zeros(E)
    gs = (a[:, :-2] - 2.0 * a[:, 1:-1]) + a[:, 2:]
    gc = g_c[:, 1:-1] if g_c is not None else np.zeros((E, T - 2, D))
    g = (v["w_smooth"] * gs + v["w_col"] * gc) + v["w_lim"] * p
    pa = np.abs(np.concatenate([q[:, :1], q, q[:, -1:]], 1))
    abs_a = pa[:, :-2] + 2.0 * pa[:, 1:-1] + pa[:, 2:]
    bound = np.where(p > 0, np.abs(np.where(np.isfinite(upper), upper, 0.0)),
                     np.abs(np.where(np.isfinite(lower), lower, 0.0)))
    abs_p = np.where(p != 0, np.abs(q[:, 1:-1]) + bound + abs(v["m_lim"]), 0.0)
    abs_g = (abs(v["w_smooth"]) * (abs_a[:, :-2] + 2.0 * abs_a[:, 1:-1] + abs_a[:, 2:]) + np.abs(v["w_col"] * gc)
             + abs(v["w_lim"]) * abs_p)
    A = smoothness_matrix(T)
    x = np.linalg.solve(A, g.transpose(1, 0, 2).reshape(T - 2, E * D)).reshape(T - 2, E, D).transpose(1, 0, 2)
    new = np.array(q)
    new[:, 1:-1] = q[:, 1:-1] - step * x
    return dict(us=us, uc=uc, ul=ul, abs_us=us, abs_uc=np.abs(cost_t).sum(1) if cost_t is not None else np.zeros(E),
                abs_ul=ul, U=(v["w_smooth"] * us + v["w_col"] * uc) + v["w_lim"] * ul, g=g, abs_g=abs_g, x=x, new=new,
                active=(p != 0).any((1, 2)))


def autograd_gradient(q, g_c, lower, upper, **over):
    """∂U/∂(interior) by torch float64 autograd of U_s, the linear collision surrogate Σ g_c·q and U_l."""
    v = dict(WEIGHTS, **over)
    lo, hi = torch.tensor(np.asarray(lower)), torch.tensor(np.asarray(upper))
    xi = torch.tensor(q[:, 1:-1], requires_grad=True)
    full = torch.cat([torch.tensor(q[:, :1]), xi, torch.tensor(q[:, -1:])], 1)
    pad = torch.cat([full[:, :1], full, full[:, -1:]], 1)
    a = pad[:, :-2] - 2.0 * pad[:, 1:-1] + pad[:, 2:]
    U = v["w_smooth"] * 0.5 * (a * a).sum()
    p = torch.clamp(xi - (hi - v["m_lim"]), min=0.0) - torch.clamp((lo + v["m_lim"]) - xi, min=0.0)
    U = U + v["w_lim"] * 0.5 * (p * p).sum() + v["w_col"] * (torch.tensor(g_c[:, 1:-1]) * xi).sum()
    U.backward()
    return xi.grad.numpy()


def numpy_seed(G, seeds, T, D, qs, qg, amp, seed):
    """The seed rule → [G·seeds, T, D]."""
    rows = np.arange(G * seeds, dtype=np.uint64)
    i = rows[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None]
    r0 = numpy_philox((i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
    u01 = (r0.astype(np.float64) + 0.5) * 2.0 ** -32
    a = amp * (2.0 * u01 - 1.0)
    a[(np.arange(G * seeds) % seeds) == 0] = 0.0
    s, g = np.repeat(qs, seeds, 0)[:, None], np.repeat(qg, seeds, 0)[:, None]
    u = (np.arange(T, dtype=np.float64) / np.float64(T - 1))[None, :, None]
    w = u * (1.0 - u)
    out = (s + u * (g - s)) + a[:, None, :] * (16.0 * (w * w))
    out[:, 0], out[:, -1] = s[:, 0], g[:, 0]
    return out


# ------------------------------------------------------------------ families
@functools.lru_cache(None)
def family(T, D):
    """dict(lower, upper, q [257, T, D], g_c, cost_t, ref = statement(...)) — read-only, after the activity checks."""
    rng = np.random.default_rng(4000 + 64 * T + D)
    lower, upper = rng.uniform(-2.0, -1.0, D), rng.uniform(1.0, 2.0, D)
    if D > 1:
        lower[1], upper[D - 1] = -np.inf, np.inf
    q = rng.uniform(-1.0, 1.0, (E_MAX, T, D))
    q *= np.where(np.arange(E_MAX) % 2 == 0, 0.9, 2.3)[:, None, None]
    wide = np.arange(1, E_MAX, 2)  # (one interior entry of joint 0, bounded on both sides, is put past its hinge)
    q[wide, rng.integers(1, T - 1, len(wide)), 0] = rng.uniform(2.05, 2.3, len(wide)) * rng.choice([-1.0, 1.0], len(wide))
    g_c = rng.uniform(200.0, 300.0, (E_MAX, T, D)) * rng.choice([-1.0, 1.0], (E_MAX, T, D))
    cost_t = rng.uniform(0.0, 3.0, (E_MAX, T)) * (rng.random((E_MAX, T)) < 0.7)
    ref = statement(q, g_c, cost_t, lower, upper)
    act = ref["active"]
    assert act.mean() >= 0.25 and (~act).mean() >= 0.25, (T, D, act.mean())
    xmax = np.abs(ref["x"]).max(1)
    assert xmax.min() >= 10.0, (T, D, xmax.min())
    out = dict(lower=lower, upper=upper, q=q, g_c=g_c, cost_t=cost_t, ref=ref)
    for v in list(out.values()) + list(ref.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------ the host build
def f64(a):
    return None if a is None else np.ascontiguousarray(a, np.float64)


class HostBackend:
    @staticmethod
    def seed(G, seeds, T, D, qs, qg, amp, seed, out):
        return H.host_lib().cdxh_traj_seed(G, seeds, T, D, H.ptr(qs), H.ptr(qg), amp, seed, H.ptr(out))

    @staticmethod
    def step(par, E, traj, g_c, cost_t, iteration, cost, best_cost, best_iter, best_traj):
        return H.host_lib().cdxh_traj_step(par, E, H.ptr(traj), H.ptr(g_c), H.ptr(cost_t), iteration, H.ptr(cost),
                                           H.ptr(best_cost), H.ptr(best_iter), H.ptr(best_traj))


def host_gradient(par, q, g_c):
    g = np.zeros_like(q)
    rc = H.host_lib().cdxh_traj_gradient(C.byref(par), q.shape[0], H.ptr(f64(q)), H.ptr(f64(g_c)), H.ptr(g))
    assert rc == 0, rc
    return g[:, 1:-1]


def presets(E, T, D, best=None, seed=None):
    """The five outputs with GUARD rows after the E the call may write.  traj is filled by the caller; best_cost: +inf
    (or ``best`` [E])."""
    rng = np.random.default_rng(seed)
    n = E + GUARD
    out = dict(traj=np.full((n, T, D), 555.0), cost=np.full((n, 3), 777.0), best_cost=np.full(n, np.inf),
               best_iter=np.full(n, -7, np.int32), best_traj=np.full((n, T, D), 888.0))
    if best is not None:
        out["best_cost"][:E] = best
    if seed is not None:
        out["best_traj"] = rng.standard_normal((n, T, D))
    return out


def run_step(be, par, E, q, g_c, cost_t, iteration=0, best=None, nulls=(), over=None, seed=None):
    """One call on E rows → (rc, outputs with their guard rows, the presets)."""
    T, D = q.shape[1], q.shape[2]
    pre = presets(E, T, D, best, seed)
    pre["traj"][:E] = q[:E]
    outs = {k: (None if k in nulls else np.array(v)) for k, v in pre.items()}
    args = dict(par=C.byref(par), E=E, g_c=f64(g_c[:E]) if g_c is not None else None,
                cost_t=f64(cost_t[:E]) if cost_t is not None else None)
    args.update(over or {})
    rc = be.step(args["par"], args["E"], outs["traj"], args["g_c"], args["cost_t"], iteration, outs["cost"],
                 outs["best_cost"], outs["best_iter"], outs["best_traj"])
    return rc, outs, pre


def good_step(be, par, E, q, g_c, cost_t, **kw):
    """``run_step`` that must succeed → the first E rows of every output; guard rows and endpoint rows found untouched."""
    rc, outs, pre = run_step(be, par, E, q, g_c, cost_t, **kw)
    assert rc == 0, rc
    for k, v in outs.items():
        assert H.same_bits(v[E:], pre[k][E:]), ("guard rows written", k)
    assert H.same_bits(outs["traj"][:E, 0], q[:E, 0]) and H.same_bits(outs["traj"][:E, -1], q[:E, -1]), "endpoints"
    return {k: v[:E] for k, v in outs.items()}


def same(got, want, keys=OUTS, rows=None, tag=""):
    for k in keys:
        a, b = (got[k], want[k]) if rows is None else (got[k][rows[0]], want[k][rows[1]])
        assert H.same_bits(a, b), (tag, k, np.argwhere(np.asarray(a != b))[:4])


def run_seed(be, G, seeds, T, D, qs, qg, amp=0.3, seed=0, over=None):
    n = G * seeds
    pre = np.full((n + GUARD, T, D), 555.0)
    out = np.array(pre)
    args = dict(G=G, seeds=seeds, T=T, D=D, qs=f64(qs), qg=f64(qg), amp=amp, seed=seed, out=out)
    args.update(over or {})
    rc = be.seed(args["G"], args["seeds"], args["T"], args["D"], args["qs"], args["qg"], args["amp"], args["seed"],
                 args["out"])
    return rc, out, pre


# ------------------------------------------------------------------ the checks, shared by both files
SEED_KEY = 0x1234567887654321


def seed_inputs(T, D, E):
    rng = np.random.default_rng(50 + T + D)
    seeds = 1 if E == 1 else 5
    G = max(1, E // seeds)
    return G, seeds, rng.uniform(-2, 2, (G, D)), rng.uniform(-2, 2, (G, D))


def check_seed(be, T, D, E):
    """Bit for bit against numpy; seed 0 is the line; a row depends on (seed, g, s) alone; a non-finite start poisons its
    rows only; guard rows untouched."""
    G, seeds, qs, qg = seed_inputs(T, D, E)
    rc, out, pre = run_seed(be, G, seeds, T, D, qs, qg, 0.3, SEED_KEY)
    assert rc == 0 and H.same_bits(out[G * seeds:], pre[G * seeds:])
    got = out[:G * seeds]
    assert H.same_bits(got, numpy_seed(G, seeds, T, D, qs, qg, 0.3, SEED_KEY))
    assert H.same_bits(got[::seeds, 0], qs) and H.same_bits(got[::seeds, -1], qg)
    assert H.same_bits(got[::seeds], numpy_seed(G, 1, T, D, qs, qg, 0.0, 5))  # s = 0: no draw enters
    if seeds > 1 and T > 3:
        assert np.abs(got[1::seeds] - got[::seeds]).max() > 1e-3  # the other seeds are perturbed
        assert np.abs(got - np.repeat(got[::seeds], seeds, 0)).max() <= 0.3  # |a_d·bump| ≤ amp
    if G > 2:  # goals 1 … of the batch alone: the counter is the row's, so only equal (g, s) give equal rows
        rc, part, _ = run_seed(be, 2, seeds, T, D, qs[:2], qg[:2], 0.3, SEED_KEY)
        assert rc == 0 and H.same_bits(part[:2 * seeds], got[:2 * seeds])
        bad = np.array(qs)
        bad[1, D // 2] = np.nan
        badg = np.array(qg)
        badg[2, 0] = -np.inf
        rc, p, _ = run_seed(be, G, seeds, T, D, bad, badg, 0.3, SEED_KEY)
        rows = np.ones(G * seeds, bool)
        rows[seeds:3 * seeds] = False
        assert rc == 0 and H.same_bits(p[:G * seeds][rows], got[rows]) and np.isnan(p[:G * seeds][~rows]).all()


def check_seed_refusals(be):
    T, D = 5, 3
    qs, qg = np.zeros((2, D)), np.ones((2, D))

    def refused(**kw):
        rc, out, pre = run_seed(be, 2, 3, T, D, qs, qg, over=kw)
        assert rc == -1 and H.same_bits(out, pre), kw.keys()
    for kw in (dict(T=2), dict(T=65), dict(D=0), dict(D=33), dict(seeds=0), dict(G=-1), dict(amp=float("nan")),
               dict(amp=float("inf")), dict(qs=None), dict(qg=None), dict(out=None)):
        refused(**kw)
    rc, out, pre = run_seed(be, 2, 3, T, D, qs, qg, over=dict(G=0))
    assert rc == 0 and H.same_bits(out, pre)


def check_step_statement(be, T, D, E):
    """The step against the numpy statement at the issue's bounds; every output row and its guard rows."""
    f = family(T, D)
    par = params(f["lower"], f["upper"], T)
    got = good_step(be, par, E, f["q"], f["g_c"], f["cost_t"], iteration=3)
    ref = f["ref"]
    for k, name in enumerate(("us", "uc", "ul")):
        err = np.abs(got["cost"][:, k] - ref[name][:E])
        bound = 1e-12 * ref["abs_" + name][:E]
        print(name, "worst |Δ|/bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), name
    c = cond(T)
    xmax = np.abs(ref["x"][:E]).max(1, keepdims=True)
    bound = 16.0 * c * EPS * STEP * xmax
    err = np.abs(got["traj"][:, 1:-1] - ref["new"][:E, 1:-1])
    print("cond", c, "step worst |Δ|/bound", float((err / bound).max()))
    assert (err <= bound).all()
    # first call: every row wins, the best row is the input row, the best cost is U
    assert (got["best_iter"] == 3).all() and H.same_bits(got["best_traj"], f["q"][:E])
    U = ref["U"][:E]
    assert (np.abs(got["best_cost"] - U) <= 1e-12 * (WEIGHTS["w_smooth"] * ref["abs_us"][:E] + WEIGHTS["w_col"]
                                                      * ref["abs_uc"][:E] + WEIGHTS["w_lim"] * ref["abs_ul"][:E])).all()
    w = WEIGHTS
    assert H.same_bits(got["best_cost"], (w["w_smooth"] * got["cost"][:, 0] + w["w_col"] * got["cost"][:, 1])
                       + w["w_lim"] * got["cost"][:, 2])
    # no collision term: NULL g_c and cost_t are zeros
    bare = good_step(be, par, E, f["q"], None, None)
    zero = good_step(be, par, E, f["q"], np.zeros_like(f["q"]), np.zeros_like(f["cost_t"]))
    same(bare, zero, tag="NULL collision term")
    assert (bare["cost"][:, 1] == 0).all()


def check_gradient(T, D, E):
    """The host build's gradient against torch autograd of the statement."""
    f = family(T, D)
    par = params(f["lower"], f["upper"], T)
    g = host_gradient(par, f["q"][:E], f["g_c"][:E])
    ref = autograd_gradient(f["q"][:E], f["g_c"][:E], f["lower"], f["upper"])
    bound = 1e-12 * f["ref"]["abs_g"][:E]
    err = np.abs(g - ref)
    print("gradient worst |Δ|/bound", float((err / bound).max()))
    assert (err <= bound).all()
    assert (np.abs(f["ref"]["g"][:E] - ref) <= bound).all()  # (the numpy statement agrees with autograd too)


def check_fixed_point(be, T, D, E):
    """w_c = w_l = 0, step = 1/w_s: one step from any start lands on the minimum of U_s."""
    f = family(T, D)
    ws = WEIGHTS["w_smooth"]
    par = params(f["lower"], f["upper"], T, step=1.0 / ws, w_col=0.0, w_lim=0.0)
    got = good_step(be, par, E, f["q"], f["g_c"], f["cost_t"])
    a = accelerations(got["traj"])
    res = (a[:, :-2] - 2.0 * a[:, 1:-1]) + a[:, 2:]  # = A_T ξ + b
    bound = 16.0 * cond(T) * EPS * 16.0 * np.abs(f["q"][:E]).max()
    print("fixed point residual", float(np.abs(res).max()), "bound", bound)
    assert np.abs(res).max() <= bound


def check_best(be, T, D, E):
    """Strict improvement only: a preset best equal to U or just below U keeps its row, iteration and cost; a
    preset above U (or +inf) is replaced by U, the iteration passed in and the whole input row."""
    f = family(T, D)
    par = params(f["lower"], f["upper"], T)
    first = good_step(be, par, E, f["q"], f["g_c"], f["cost_t"])
    U = first["best_cost"]
    kind = np.arange(E) % 4  # 0: equal, 1: just below, 2: just above, 3: +inf
    best = np.where(kind == 0, U, np.where(kind == 1, np.nextafter(U, -np.inf), np.where(kind == 2, np.nextafter(U, np.inf),
                                                                                        np.inf)))
    rc, outs, pre = run_step(be, par, E, f["q"], f["g_c"], f["cost_t"], iteration=41, best=best, seed=8)
    assert rc == 0
    win = kind >= 2
    assert (outs["best_iter"][:E][win] == 41).all() and (outs["best_iter"][:E][~win] == -7).all()
    assert H.same_bits(outs["best_cost"][:E], np.where(win, U, best))
    assert H.same_bits(outs["best_traj"][:E][win], f["q"][:E][win])
    assert H.same_bits(outs["best_traj"][:E][~win], pre["best_traj"][:E][~win])
    assert H.same_bits(outs["traj"][:E], first["traj"]) and H.same_bits(outs["cost"][:E], first["cost"])


def poisoned(f, E=65):
    """The family's first E rows shuffled into 2E + 1 rows whose other rows hold a NaN, +inf or −inf (in turn) in traj,
    g_c or cost_t (in turn) → (index of each good row, its source row, q, g_c, cost_t, the input that was hit per row)."""
    rng = np.random.default_rng(11)
    n = 2 * E + 1
    at = np.sort(rng.permutation(n)[:E])
    src = rng.permutation(E)
    arrs = [np.array(a[rng.integers(0, E, n)]) for a in (f["q"], f["g_c"], f["cost_t"])]
    hit = np.full(n, -1)
    for r in range(n):
        hit[r] = r % 3 if r % 2 else (r // 2) % 3
        flat = arrs[hit[r]].reshape(n, -1)
        flat[r, rng.integers(flat.shape[1])] = (np.nan, np.inf, -np.inf)[(r // 3) % 3]
    for a, b in zip(arrs, (f["q"], f["g_c"], f["cost_t"])):
        a[at] = b[src]
    hit[at] = -1
    return (at, src, *arrs, hit)


def check_rows(be, T, D):
    """A row's bits depend neither on E, nor on its position, nor on non-finite neighbours, nor on the run; a
    poisoned row is NaN in its own float outputs and keeps its best entries."""
    f = family(T, D)
    par = params(f["lower"], f["upper"], T)
    E = 65
    clean = good_step(be, par, E, f["q"], f["g_c"], f["cost_t"])
    same(good_step(be, par, E, f["q"], f["g_c"], f["cost_t"]), clean, tag="second run")
    for n in (1, 63, 64):
        same(good_step(be, par, n, f["q"], f["g_c"], f["cost_t"]), {k: v[:n] for k, v in clean.items()}, tag=f"E={n}")
    last = good_step(be, par, 5, f["q"][60:65], f["g_c"][60:65], f["cost_t"][60:65])
    same(last, {k: v[60:65] for k, v in clean.items()}, tag="position")
    at, src, q, g_c, cost_t, hit = poisoned(f, E)
    n = len(q)
    assert {0, 1, 2} <= set(hit[hit >= 0])
    rc, outs, pre = run_step(be, par, n, q, g_c, cost_t, seed=9)
    assert rc == 0
    got = {k: v[:n] for k, v in outs.items()}
    same(got, clean, rows=(at, src), tag="neighbours")
    bad = np.setdiff1d(np.arange(n), at)
    assert np.isnan(got["cost"][bad]).all() and np.isnan(got["traj"][bad][:, 1:-1]).all()
    for k in ("best_cost", "best_iter", "best_traj"):
        assert H.same_bits(got[k][bad], pre[k][:n][bad]), k
    assert H.same_bits(got["traj"][:, 0], q[:, 0]) and H.same_bits(got["traj"][:, -1], q[:, -1])
    for k, v in outs.items():
        assert H.same_bits(v[n:], pre[k][n:]), k


def check_step_refusals(be):
    f = family(5, 23)
    E, T, D = 5, 5, 23

    def refused(p=None, nulls=(), **kw):
        p = p if p is not None else params(f["lower"], f["upper"], T)
        rc, outs, pre = run_step(be, p, E, f["q"], f["g_c"], f["cost_t"], nulls=nulls, over=kw)
        assert rc == -1, (kw.keys(), nulls, rc)
        for k, v in outs.items():
            assert v is None or H.same_bits(v, pre[k]), k

    def par(**kw):
        p = params(f["lower"], f["upper"], T)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    for bad in (dict(T=2), dict(T=65), dict(n_dofs=0), dict(n_dofs=33), dict(w_smooth=float("nan")),
                dict(w_col=float("inf")), dict(w_lim=float("-inf")), dict(m_lim=float("nan")), dict(step=float("inf")),
                dict(step=float("nan"))):
        refused(par(**bad))
    p = params(f["lower"], f["upper"], T)
    p.lower[3], p.upper[3] = 1.0, 0.5
    refused(p)
    p = params(f["lower"], f["upper"], T)
    p.upper[22] = float("nan")
    refused(p)
    p = params(f["lower"], f["upper"], T)
    p.lower[0] = float("nan")
    refused(p)
    refused(par=None)
    refused(E=-1)
    refused(g_c=None)
    refused(cost_t=None)
    for k in OUTS:
        refused(nulls=(k,))
    rc, outs, pre = run_step(be, params(f["lower"], f["upper"], T), E, f["q"], f["g_c"], f["cost_t"], over=dict(E=0))
    assert rc == 0
    for k, v in outs.items():
        assert H.same_bits(v, pre[k]), k


# ------------------------------------------------------------------ the loop, stated once over a backend
ROBOT = "iiwa7_allegro"
SCENE = dict(T=24, radius=0.03, obstacle=0.06, m_obj=0.01, w_obj=1.0, w_smooth=1.0, w_col=100.0, w_lim=100.0,
             m_lim=0.02, gain=1.0, iters=150)


@functools.lru_cache(None)
def scene():
    """The issue's scenario: dict(hs, lower, upper, q_start, q_goal, line [1, T, D], center, step)."""
    from compliancedex_amd.hand import HandSpheres
    from compliancedex_amd.trajectory import _limits_of, step_size
    from compliancedex_amd.urdf import load_robot
    desc = load_robot(ROBOT)
    hs = HandSpheres(desc, {b["name"]: [((0.0, 0.0, 0.0), SCENE["radius"])] for b in desc["bodies"]},
                     pairs=np.zeros((0, 2), np.int32))
    assert hs.n_spheres == 29 and hs.desc.n_dofs == 23
    lower, upper = (np.array(v) for v in _limits_of(hs))
    qs = np.zeros(23)
    qs[1], qs[3] = 0.6, -1.2
    qg = np.array(qs)
    qg[0], qg[5], qg[7:] = 1.2, 0.5, 0.3
    qs, qg = (np.clip(q, lower + 0.04, upper - 0.04) for q in (qs, qg))
    T = SCENE["T"]
    line = numpy_seed(1, 1, T, 23, qs[None], qg[None], 0.0, 0)
    _, centers = H.host_spheres(hs, line[0], None)
    center = centers[12, -1] + np.array([0.0, 0.0, 0.03])
    return dict(hs=hs, lower=lower, upper=upper, q_start=qs, q_goal=qg, line=line, center=center,
                step=step_size(T, SCENE["w_smooth"], SCENE["w_col"], SCENE["gain"]))


def obstacle(center, radius=None):
    """The analytic sphere at centres [..., 3] (numpy) → (d, ∇d)."""
    r = SCENE["obstacle"] if radius is None else radius

    def f(c):
        v = c - center
        n = np.linalg.norm(v, axis=-1)
        return n - r, v / n[..., None]
    return f


def hand_params(m_obj=None):
    return H.params_struct(floor=False, m_obj=SCENE["m_obj"] if m_obj is None else m_obj, m_self=0.0, m_floor=0.0,
                           w_obj=SCENE["w_obj"], w_self=1.0, w_floor=1.0, floor_z=0.0)


def loop(be, hs, par, hp, traj, obj, iters, record=None, replay=None, palm=None):
    """``iters`` iterations on traj [E, T, D]: spheres on the E·T waypoints, the object evaluated in numpy at the centres
    read back, the term at weight 1, the step.  ``record``: a list that receives every iteration's (poses, centres);
    ``replay``: such a list, used in place of this backend's own spheres launch.  → dict(traj, cost, best_cost,
    best_iter, best_traj, first_cost [E] = U of the input)."""
    E, T, D = traj.shape
    R = E * T
    st = dict(traj=np.array(traj), cost=np.zeros((E, 3)), best_cost=np.full(E, np.inf),
              best_iter=np.full(E, -1, np.int32), best_traj=np.array(traj))
    pal = None if palm is None else np.repeat(palm, T, 0)
    first = None
    for it in range(iters):
        if replay is not None:
            poses, centers = replay[it]
        else:
            poses, centers = be.spheres(hs, st["traj"].reshape(R, D), pal)
        if record is not None:
            record.append((np.array(poses), np.array(centers)))
        dist, gdist = obj(centers) if obj is not None else (None, None)
        outs = dict(loss=np.zeros(R), g_q=np.zeros((R, D)))
        rc = be.term(C.byref(hs.desc), C.byref(be.model(hs)), C.byref(hp), R, np.ascontiguousarray(poses, np.float32),
                     f64(centers), f64(dist), f64(gdist), None if pal is None else f64(pal[:, 3:]), 1.0, 0, outs)
        assert rc == 0, rc
        rc = be.step(C.byref(par), E, st["traj"], outs["g_q"].reshape(E, T, D), outs["loss"].reshape(E, T), it,
                     st["cost"], st["best_cost"], st["best_iter"], st["best_traj"])
        assert rc == 0, rc
        if it == 0:
            first = np.array(st["best_cost"])
    st["first_cost"] = first
    return st


def scene_params(sc, T=None):
    return params(sc["lower"], sc["upper"], SCENE["T"] if T is None else T, step=sc["step"], w_smooth=SCENE["w_smooth"],
                  w_col=SCENE["w_col"], w_lim=SCENE["w_lim"], m_lim=SCENE["m_lim"])


def host_depth(hs, traj, obj, refine=1):
    """The largest object penetration r − d over the path's samples (host spheres, numpy object), per row."""
    from compliancedex_amd.trajectory import path_samples
    x = path_samples(torch.from_numpy(np.ascontiguousarray(traj)), refine).numpy()
    E, Ns, D = x.shape
    _, centers = H.host_spheres(hs, x.reshape(E * Ns, D), None)
    d, _ = obj(centers)
    return (hs.radius[None] - d).reshape(E, Ns * hs.n_spheres).max(1)
