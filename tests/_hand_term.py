"""Shared checks of cdx_hand_term (the whole-hand cost and its pull-back in one weighted, optionally accumulating
launch; csrc/cdx_hand.h), run by the host file on libcdx_host.so and by the device file on the GPU.

A backend is an object with ``spheres(hs, q, palm)``, ``cost(hs, par, centers, dist, gdist)``, ``pullback(hs, poses, g,
po)`` (tests/_hand.py's host loaders or test_gpu_hand.py's device ones) and ``term(...)`` below.  Every comparison is
bit for bit: x, the term at weight 1 without accumulation, must be what cdx_hand_cost followed by cdx_hand_pullback
give, and any other call must be numpy's ``old + (weight * x)`` in float64 (two roundings, as the kernel's).

Families: tests/_hand.py's hand8, tree8 and allegro ones (S ∈ {1, 63, 65, 256}), E ∈ {1, 63, 65, 257}; before a family is
used ``fam`` asserts that at least a quarter of its rows have a positive cost.
"""
import ctypes as C

import numpy as np

from compliancedex_amd import _native as N
from tests import _hand as H

FAMILIES = tuple(f for f in H.FAMILIES if f[0] in ("hand8", "tree8", "allegro"))
IDS = [f"{c}-S{s}-{p}" for c, s, p in FAMILIES]
BATCHES = (1, 63, 65, 257)
GUARD = 4  # rows past every output, preset and found untouched
WEIGHT = 0.37
FLOATS = ("loss", "g_q", "g_pp", "g_po", "depth")
OUTS = FLOATS + ("worst",)
assert {f[1] for f in FAMILIES} == {1, 63, 65, 256}


def fam(case, S, pairs):
    f = H.family(case, S, pairs)
    assert (f["cost"]["cost"] > 0).mean() >= 0.25, (case, S, pairs)
    return f


def tails(hs):
    return dict(loss=(), g_q=(hs.desc.n_dofs,), g_pp=(3,), g_po=(3,), depth=(3,), worst=(3,))


def presets(hs, E, seed=None):
    """Outputs of E + GUARD rows: 777 / −777, or (seed) random values of mixed sign and magnitude."""
    rng = None if seed is None else np.random.default_rng(seed)
    out = {}
    for k, t in tails(hs).items():
        if k == "worst":
            out[k] = np.full((E + GUARD, *t), -777, np.int32)
        elif rng is None:
            out[k] = np.full((E + GUARD, *t), 777.0)
        else:
            out[k] = rng.standard_normal((E + GUARD, *t)) * 10.0 ** rng.integers(-6, 3, (E + GUARD, *t))
    return out


def host_term(chain, hand, par, E, poses, centers, dist, gdist, po, weight, accumulate, outs):
    """cdxh_hand_term on numpy arrays; ``outs``: dict of arrays written in place (a missing key: NULL) → rc."""
    lib = H.host_lib()
    return lib.cdxh_hand_term(chain, hand, par, E, H.ptr(poses), H.ptr(centers), H.ptr(dist), H.ptr(gdist), H.ptr(po),
                              weight, accumulate, *[H.ptr(outs.get(k)) for k in OUTS])


class HostBackend:
    spheres = staticmethod(H.host_spheres)
    cost = staticmethod(H.host_cost)
    pullback = staticmethod(H.host_pullback)
    model = staticmethod(H.host_model)
    term = staticmethod(host_term)


def run(be, hs, par, E, poses, centers, dist, gdist, po, weight=1.0, accumulate=0, preset=None, nulls=(), over=None):
    """One call on the first E rows → (rc, outputs with their guard rows, the presets).  ``over``: dict of chain / hand / par
    / E / a replaced input, for the refusals."""
    pre = presets(hs, E) if preset is None else preset
    outs = {k: np.array(v) for k, v in pre.items() if k not in nulls}
    f32 = lambda a: None if a is None else np.ascontiguousarray(a[:E], np.float32)  # noqa: E731
    f64 = lambda a: None if a is None else np.ascontiguousarray(a[:E], np.float64)  # noqa: E731
    args = dict(chain=C.byref(hs.desc), hand=C.byref(be.model(hs)), par=C.byref(par), E=E, poses=f32(poses),
                centers=f64(centers), dist=f64(dist), gdist=f64(gdist), po=f64(po))
    args.update(over or {})
    rc = be.term(args["chain"], args["hand"], args["par"], args["E"], args["poses"], args["centers"], args["dist"],
                 args["gdist"], args["po"], weight, accumulate, outs)
    return rc, outs, pre


def good(be, hs, par, E, *a, **kw):
    """``run`` that must succeed → the first E rows of every output, the guard rows found untouched."""
    rc, outs, pre = run(be, hs, par, E, *a, **kw)
    assert rc == 0, rc
    for k, v in outs.items():
        assert H.same_bits(v[E:], pre[k][E:]), ("guard rows written", k)
    return {k: v[:E] for k, v in outs.items()}


def pair(be, hs, par, poses, centers, dist, gdist, po):
    """x: cdx_hand_cost followed by cdx_hand_pullback."""
    cost, depth, worst, g = be.cost(hs, par, centers, dist, gdist)
    g_q, g_pp, g_po = be.pullback(hs, poses, g, po)
    return dict(loss=cost, g_q=g_q, g_pp=g_pp, g_po=g_po, depth=depth, worst=worst)


def expect(x, pre, E, weight, accumulate):
    """numpy's statement of the output rule."""
    out = {}
    for k in FLOATS[:4]:
        wx = np.float64(weight) * x[k]
        out[k] = pre[k][:E] + wx if accumulate else wx
    out["depth"], out["worst"] = x["depth"], x["worst"]
    return out


def same(got, want, keys=OUTS, rows=None, tag=""):
    for k in keys:
        a, b = (got[k], want[k]) if rows is None else (got[k][rows[0]], want[k][rows[1]])
        assert H.same_bits(a, b), (tag, k, np.argwhere(np.asarray(a != b))[:4])


def check_values(be, f):
    """weight 1 without accumulation is the pair; weight 0.37 accumulating is old + (0.37·x); NULL optional outputs
    and a NULL object change nothing else; every batch size, a second run and another position give the same bits."""
    hs, par, E = f["hs"], H.params_struct(), H.E_MAX
    poses = be.spheres(hs, f["q"], f["palm"])[0]
    po = f["palm"][:, 3:]
    inp = (poses, f["centers"], f["dist"], f["gdist"], po)
    x = pair(be, hs, par, *inp)
    assert (x["loss"] > 0).mean() >= 0.25
    one = good(be, hs, par, E, *inp)
    same(one, x, tag="weight 1")
    pre = presets(hs, E, seed=5)
    acc = good(be, hs, par, E, *inp, weight=WEIGHT, accumulate=1, preset=pre)
    same(acc, expect(x, pre, E, WEIGHT, 1), tag="accumulate")
    scaled = good(be, hs, par, E, *inp, weight=WEIGHT, accumulate=0, preset=pre)
    same(scaled, expect(x, pre, E, WEIGHT, 0), tag="weight")
    for n in BATCHES:
        same(good(be, hs, par, n, *inp), {k: v[:n] for k, v in one.items()}, tag=f"E={n}")
    same(good(be, hs, par, E, *inp), one, tag="second run")
    last = good(be, hs, par, 5, *[a[-5:] for a in inp])
    same(last, {k: v[-5:] for k, v in one.items()}, tag="position")
    part = good(be, hs, par, 65, *inp, nulls=("g_pp", "g_po", "depth", "worst"))
    same(part, {k: v[:65] for k, v in one.items()}, keys=("loss", "g_q"), tag="optional outputs")
    bare = good(be, hs, par, 65, poses, f["centers"], None, None, None)
    same(bare, pair(be, hs, par, poses[:65], f["centers"][:65], None, None, None), tag="no object, no palm angles")


def check_rows(be, f, E=65):
    """A row's bits do not depend on non-finite neighbours (NaN, +inf, −inf) nor on its position among them; a
    non-finite row is NaN in its own outputs, worst −1 — with and without accumulation."""
    hs, par = f["hs"], H.params_struct()
    poses0 = be.spheres(hs, f["q"][:E], f["palm"][:E])[0]
    clean = good(be, hs, par, E, poses0, f["centers"], f["dist"], f["gdist"], f["palm"][:, 3:])
    at, src, q, palm, cen, dist, gdist, _ = H.poisoned(f, E)
    n = len(q)
    poses1 = be.spheres(hs, q, palm)[0]
    assert H.same_bits(poses1[at], poses0[src])
    inp = (poses1, cen, dist, gdist, palm[:, 3:])
    bad = np.setdiff1d(np.arange(n), at)
    got = good(be, hs, par, n, *inp)
    same(got, clean, rows=(at, src), tag="neighbours")
    pre = presets(hs, n, seed=6)
    acc = good(be, hs, par, n, *inp, weight=WEIGHT, accumulate=1, preset=pre)
    for k in FLOATS[:4]:  # old + (0.37·x) with the row's own old value
        assert H.same_bits(acc[k][at], pre[k][at] + np.float64(WEIGHT) * clean[k][src]), k
    same(acc, clean, keys=("depth", "worst"), rows=(at, src), tag="neighbours, accumulating")
    for res in (got, acc):
        for k in FLOATS:
            assert np.isnan(res[k][bad]).all(), k
        assert (res["worst"][bad] == -1).all()


def check_refusals(be, f, other, deep):
    """Every refusal returns its code and leaves preset outputs untouched; E = 0 is a no-op.  ``other``: a model of
    another chain; ``deep``: a chain with a body below the depth limit."""
    hs, par, E = f["hs"], H.params_struct(), 5
    poses = be.spheres(hs, f["q"][:E], f["palm"][:E])[0]
    inp = (poses, f["centers"], f["dist"], f["gdist"], f["palm"][:, 3:])

    def refused(code, weight=1.0, accumulate=0, nulls=(), **kw):
        rc, outs, pre = run(be, hs, par, E, *inp, weight=weight, accumulate=accumulate, nulls=nulls, over=kw)
        assert rc == code, (kw.keys(), rc)
        for k, v in outs.items():
            assert H.same_bits(v, pre[k]), (kw.keys(), k)

    refused(-3, chain=None)
    refused(-3, chain=C.byref(deep))
    refused(-1, hand=None)
    refused(-1, par=None)
    refused(-1, hand=C.byref(be.model(other)))
    h = be.model(hs)
    for bad in (dict(n_spheres=257), dict(n_spheres=0), dict(n_pairs=-1), dict(n_bodies=33), dict(local=None),
                dict(radius=None), dict(body=None), dict(len=None)):
        hb = N.CdxHand()
        C.memmove(C.byref(hb), C.byref(h), C.sizeof(hb))
        for k, v in bad.items():
            setattr(hb, k, v)
        refused(-1, hand=C.byref(hb))
    refused(-1, par=C.byref(H.params_struct(w_obj=float("nan"))))
    refused(-1, E=-1)
    refused(-1, poses=None)
    refused(-1, centers=None)
    refused(-1, dist=None)
    refused(-1, gdist=None)
    refused(-1, nulls=("loss",))
    refused(-1, nulls=("g_q",))
    for w in (float("nan"), float("inf")):
        refused(-1, weight=w)
    refused(-1, accumulate=2)
    refused(-1, accumulate=-1)
    refused(0, E=0)
