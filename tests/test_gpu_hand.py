"""The whole-hand sphere kernels (cdx_hand_spheres / cdx_hand_cost / cdx_hand_pullback) on an MI355X through the C ABI,
with guard rows past every output found untouched: the device against the host build (bit for bit where no library sine
or cosine is involved) and against the float64 statement, the independence of rows and of the launch shape, the argument
checks, and the Python entry points of compliancedex_amd.hand on the packaged banana."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _chains, _hand as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 3  # output rows past the last, preset and found untouched
IDS = [f"{c}-S{s}-{p}" for c, s, p in H.FAMILIES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def _dev(a, dtype=np.float64):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _out(E, tail, dtype, fill):
    return torch.full((E + GUARD, *tail), fill, dtype=dtype, device=DEV)


def _take(outs, E):
    res = []
    for t in outs:
        a = t.cpu().numpy()
        guard = a[E:]
        assert (guard == guard.flat[0]).all() and guard.flat[0] in (777.0, -777), "guard rows written"
        res.append(a[:E])
    return res


def _lib():
    from compliancedex_amd import _native as N
    return N, N.load()


def dev_spheres(hs, q, palm=None):
    N, lib = _lib()
    q = _dev(q)
    E = q.shape[0]
    pp, po = (None, None) if palm is None else (_dev(palm[:, :3]), _dev(palm[:, 3:]))
    poses = _out(E, (hs.desc.n_bodies, 12), torch.float32, 777.0)
    centers = _out(E, (hs.n_spheres, 3), torch.float64, 777.0)
    N.check(lib.cdx_hand_spheres(C.byref(hs.desc), C.byref(hs.native()), E, N.ptr(q), N.ptr(pp), N.ptr(po), N.ptr(poses),
                                 N.ptr(centers), N.stream_ptr()), "cdx_hand_spheres")
    return _take((poses, centers), E)


def dev_cost(hs, params, centers, dist=None, gdist=None):
    N, lib = _lib()
    c, d, gd = _dev(centers), _dev(dist), _dev(gdist)
    E, S = c.shape[0], hs.n_spheres
    outs = (_out(E, (), torch.float64, 777.0), _out(E, (3,), torch.float64, 777.0), _out(E, (3,), torch.int32, -777),
            _out(E, (S, 3), torch.float64, 777.0))
    N.check(lib.cdx_hand_cost(C.byref(hs.native()), C.byref(params), E, N.ptr(c), N.ptr(d), N.ptr(gd),
                              *[N.ptr(t) for t in outs], N.stream_ptr()), "cdx_hand_cost")
    return _take(outs, E)


def dev_pullback(hs, poses, g, po=None):
    N, lib = _lib()
    p, g, po = _dev(poses, np.float32), _dev(g), _dev(po)
    E = p.shape[0]
    outs = (_out(E, (hs.desc.n_dofs,), torch.float64, 777.0), _out(E, (3,), torch.float64, 777.0),
            _out(E, (3,), torch.float64, 777.0))
    N.check(lib.cdx_hand_pullback(C.byref(hs.desc), C.byref(hs.native()), E, N.ptr(p), N.ptr(g), N.ptr(po),
                                  *[N.ptr(t) for t in outs], N.stream_ptr()), "cdx_hand_pullback")
    return _take(outs, E)


# ------------------------------------------------------------------ 7. device against the host build and the statement
@pytest.mark.parametrize("case,S,pairs", H.FAMILIES, ids=IDS)
def test_device_vs_host_and_statement(case, S, pairs):
    fam = H.family(case, S, pairs)
    hs, E, par = fam["hs"], H.E_MAX, H.params_struct()
    poses, centers = dev_spheres(hs, fam["q"], fam["palm"])
    hposes, hcenters = H.host_spheres(hs, fam["q"], fam["palm"])
    e = _chains.rel(centers, hcenters)
    print("centres device vs host", f"{e:.2e}")
    assert e < _chains.TOL["pos"]  # (the float32 sines and cosines of the two differ in the last place)
    H.check_centers(fam, centers, E)
    got = dev_cost(hs, par, fam["centers"], fam["dist"], fam["gdist"])
    for a, b in zip(got, H.host_cost(hs, par, fam["centers"], fam["dist"], fam["gdist"])):
        assert H.same_bits(a, b)
    H.check_cost(fam, got, E)
    g = fam["cost"]["g"]
    pull = dev_pullback(hs, poses, g, fam["palm"][:, 3:])
    for a, b in zip(pull, H.host_pullback(hs, poses, g, fam["palm"][:, 3:])):  # the device's own poses
        assert H.same_bits(a, b)
    H.check_pullback(fam, pull, E, poses)
    null = dev_pullback(hs, poses[:65], g[:65], None)
    for a, b in zip(null, dev_pullback(hs, poses[:65], g[:65], np.zeros((65, 3)))):
        assert H.same_bits(a, b)


# ------------------------------------------------------------------ 8. rows and launch shapes
@pytest.mark.parametrize("case,S,pairs", H.SMALL, ids=[f"{c}-S{s}-{p}" for c, s, p in H.SMALL])
def test_rows_and_launch_shapes(case, S, pairs):
    fam = H.family(case, S, pairs)
    hs, par = fam["hs"], H.params_struct()
    H.check_rows(fam, dev_spheres, dev_cost, dev_pullback)
    full = dev_spheres(hs, fam["q"], fam["palm"])
    cfull = dev_cost(hs, par, fam["centers"], fam["dist"], fam["gdist"])
    pfull = dev_pullback(hs, full[0], fam["cost"]["g"], fam["palm"][:, 3:])
    for E in H.BATCHES:
        for a, b in zip(dev_spheres(hs, fam["q"][:E], fam["palm"][:E]), full):
            assert H.same_bits(a, b[:E])
        for a, b in zip(dev_cost(hs, par, fam["centers"][:E], fam["dist"][:E], fam["gdist"][:E]), cfull):
            assert H.same_bits(a, b[:E])
        for a, b in zip(dev_pullback(hs, full[0][:E], fam["cost"]["g"][:E], fam["palm"][:E, 3:]), pfull):
            assert H.same_bits(a, b[:E])
    # a second run of the same launches: the same bits
    for a, b in zip(dev_spheres(hs, fam["q"], fam["palm"]), full):
        assert H.same_bits(a, b)
    for a, b in zip(dev_cost(hs, par, fam["centers"], fam["dist"], fam["gdist"]), cfull):
        assert H.same_bits(a, b)
    for a, b in zip(dev_pullback(hs, full[0], fam["cost"]["g"], fam["palm"][:, 3:]), pfull):
        assert H.same_bits(a, b)
    # the last rows of the batch: another position in another workgroup
    for a, b in zip(dev_spheres(hs, fam["q"][-5:], fam["palm"][-5:]), full):
        assert H.same_bits(a, b[-5:])


# ------------------------------------------------------------------ 9. argument checks
def test_argument_checks():
    N, lib = _lib()
    fam = H.family("hand8", 63, "full")
    hs, par = fam["hs"], H.params_struct()
    h, desc, E = hs.native(), hs.desc, 5
    q, palm = _dev(fam["q"][:E]), _dev(fam["palm"][:E])
    pp, po = palm[:, :3].contiguous(), palm[:, 3:].contiguous()
    poses = _out(E, (desc.n_bodies, 12), torch.float32, 777.0)
    cen = _out(E, (hs.n_spheres, 3), torch.float64, 777.0)
    cost, depth = _out(E, (), torch.float64, 777.0), _out(E, (3,), torch.float64, 777.0)
    worst, g = _out(E, (3,), torch.int32, -777), _out(E, (hs.n_spheres, 3), torch.float64, 777.0)
    gq, gpp, gpo = (_out(E, (k,), torch.float64, 777.0) for k in (desc.n_dofs, 3, 3))
    st = N.stream_ptr()
    P = N.ptr

    def spheres(c=C.byref(desc), hh=C.byref(h), e=E, q_=q, poses_=poses, cen_=cen):
        return lib.cdx_hand_spheres(c, hh, e, P(q_), P(pp), P(po), P(poses_), P(cen_), st)

    def cost_(hh=C.byref(h), p=C.byref(par), e=E, c=cen, d=None, gd=None, out=(cost, depth, worst, g)):
        return lib.cdx_hand_cost(hh, p, e, P(c), P(d), P(gd), *[P(t) for t in out], st)

    def pull(c=C.byref(desc), hh=C.byref(h), e=E, p=poses, g_=g, out=(gq, gpp, gpo)):
        return lib.cdx_hand_pullback(c, hh, e, P(p), P(g_), P(po), *[P(t) for t in out], st)

    assert spheres(c=None) == -3 and pull(c=None) == -3  # a null chain
    deep = _chains.raw_descriptor(_chains.line(17), ["b17"])
    assert spheres(c=C.byref(deep)) == -3 and pull(c=C.byref(deep)) == -3  # a body below the depth limit
    for bad in (dict(n_spheres=257), dict(n_spheres=0), dict(n_pairs=32769), dict(n_pairs=-1), dict(n_bodies=33),
                dict(local=None), dict(radius=None), dict(body=None), dict(len=None), dict(entry=None),
                dict(group_base=(C.c_int32 * 4)(0, -1, 0, 0)), dict(group_base=(C.c_int32 * 4)(1 << 24, 0, 0, 0))):
        hb = N.CdxHand()
        C.memmove(C.byref(hb), C.byref(h), C.sizeof(hb))
        for k, v in bad.items():
            setattr(hb, k, v)
        assert spheres(hh=C.byref(hb)) == -1 and cost_(hh=C.byref(hb)) == -1 and pull(hh=C.byref(hb)) == -1, bad
    assert spheres(hh=None) == -1 and cost_(hh=None) == -1 and pull(hh=None) == -1 and cost_(p=None) == -1
    other = H.family("tree8", 65, "one")["hs"]  # a model of another chain
    assert spheres(hh=C.byref(other.native())) == -1 and pull(hh=C.byref(other.native())) == -1
    assert spheres(q_=None) == -1 and spheres(poses_=None) == -1 and spheres(cen_=None) == -1
    assert cost_(c=None) == -1 and cost_(d=cost) == -1 and cost_(gd=g) == -1
    for k in range(4):
        assert cost_(out=tuple(None if i == k else t for i, t in enumerate((cost, depth, worst, g)))) == -1
    assert pull(p=None) == -1 and pull(g_=None) == -1
    for k in range(3):
        assert pull(out=tuple(None if i == k else t for i, t in enumerate((gq, gpp, gpo)))) == -1
    nan = H.params_struct(w_obj=float("nan"))
    assert cost_(p=C.byref(nan)) == -1
    assert spheres(e=-1) == -1 and cost_(e=-1) == -1 and pull(e=-1) == -1
    assert spheres(e=0) == 0 and cost_(e=0) == 0 and pull(e=0) == 0  # E = 0: OK, nothing touched
    # sizes over the limits at prepare
    assert lib.cdx_hand_bytes(257, 0) == 0 and lib.cdx_hand_bytes(1, 32769) == 0 and lib.cdx_hand_bytes(256, 32768) > 0
    tab = torch.zeros(lib.cdx_hand_bytes(3, 1), dtype=torch.uint8, device=DEV)
    loc, rad = np.zeros((3, 3), np.float32), np.full(3, 0.01)
    body, pr = np.array([0, 1, 1], np.int32), np.array([[0, 2]], np.int32)
    hb = N.CdxHand()

    def prep(nb=2, S=3, l=loc, r=rad, b=body, Pn=1, p=pr, t=tab, o=C.byref(hb)):
        return lib.cdx_hand_prepare(nb, S, H.ptr(l), H.ptr(r), H.ptr(b), Pn, H.ptr(p), P(t), o, st)
    assert prep() == 0 and hb.n_spheres == 3 and hb.n_pairs == 1
    assert prep(S=257) == -1 and prep(Pn=32769) == -1 and prep(nb=33) == -1 and prep(nb=1) == -1
    assert prep(l=None) == -1 and prep(r=None) == -1 and prep(b=None) == -1 and prep(p=None) == -1
    assert prep(t=None) == -1 and prep(o=None) == -1
    assert prep(r=np.array([0.01, -1.0, 0.01])) == -1 and prep(p=np.array([[2, 0]], np.int32)) == -1
    torch.cuda.synchronize()
    for t in (poses, cen, cost, depth, g, gq, gpp, gpo):
        assert (t == 777.0).all()
    assert (worst == -777).all()


# ------------------------------------------------------------------ 10. / 11. the Python entry points
def golden_hand():
    from compliancedex_amd.hand import HandSpheres
    with open(H.GOLDEN) as f:
        d = json.load(f)
    spheres = {}
    for link, c, r in zip(d["links"], d["centers"], d["radii"]):
        spheres.setdefault(link, []).append((c, r))
    hs = HandSpheres("allegro", spheres, device=DEV)
    assert hs.n_spheres == len(d["links"]) <= 256 and len(hs.pairs) <= 32768
    return hs


def banana(kind):
    """(object, its centre) of the packaged banana: "gpis", "mesh" (a PreparedMesh) or None."""
    from compliancedex_amd import PreparedMesh
    from compliancedex_amd.workloads import DATA, stored_gpis, surface_center
    if kind == "gpis":
        g = stored_gpis("banana", torch.device(DEV))
        return g, surface_center(g)
    if kind == "mesh":
        faces = torch.from_numpy(np.load(os.path.join(DATA, "meshes", "banana_faces.npy")).astype(np.float32)).to(DEV)
        return PreparedMesh(faces.reshape(-1, 3, 3)), np.load(os.path.join(DATA, "banana_center.npy"))
    return None, np.zeros(3)


def hand_rows(hs, center, E=65):
    """q around the rest pose and palm poses around the object's centre."""
    rng = np.random.default_rng(21)
    q = hs.rest_q[None] + 0.3 * rng.standard_normal((E, hs.desc.n_dofs))
    palm = np.concatenate([center[None] + rng.uniform(-0.1, 0.1, (E, 3)), rng.uniform(-H.PI, H.PI, (E, 3))], 1)
    return q, palm


@pytest.mark.parametrize("kind", ["gpis", "mesh", None])
def test_hand_collision_entry(kind):
    from compliancedex_amd import compute_sdf, hand_collision
    from compliancedex_amd.hand import cost_launch, pullback_launch, spheres_launch
    hs = golden_hand()
    obj, center = banana(kind)
    qn, pn = hand_rows(hs, center)
    q = _dev(qn).requires_grad_(True)
    palm = _dev(pn).requires_grad_(True)
    kw = dict(m_obj=0.005, m_self=0.002, m_floor=0.01, w_obj=2.0, w_self=3.0, w_floor=0.5)
    floor_z = float(center[2]) - 0.05
    cost, rep = hand_collision(hs, q, palm, obj, floor_z=floor_z, **kw)
    cost.sum().backward()
    # the ABI by hand: spheres, the object's distance, cost, pull-back of the ABI's own g_centers
    pp, po = palm.detach()[:, :3].contiguous(), palm.detach()[:, 3:].contiguous()
    poses, centers = spheres_launch(hs, q.detach(), pp, po)
    assert torch.equal(centers, rep["centers"])
    E, S = centers.shape[:2]
    X = centers.reshape(-1, 3)
    dist = gdist = None
    if kind == "gpis":
        dist = obj.pred_mean(X).reshape(E, S)
        assert torch.equal(rep["dist"], dist)
        gdist = _Grad.of(obj, X).reshape(E, S, 3)
    elif kind == "mesh":
        sq, sign, normal, _ = compute_sdf(X.float(), obj.faces)
        dist = (sign.double() * torch.sqrt(sq.double())).reshape(E, S)
        assert torch.equal(rep["dist"], dist)
        gdist = (sign.double()[:, None] * normal.double()).reshape(E, S, 3)
    par = H.params_struct(floor_z=floor_z, **kw)
    c2, depth, worst, g = cost_launch(hs, par, centers, dist, gdist)
    assert torch.equal(c2, cost.detach()) and torch.equal(depth, rep["depth"]) and torch.equal(worst, rep["worst"])
    g_q, g_pp, g_po = pullback_launch(hs, poses, g, po)
    assert torch.equal(q.grad, g_q) and torch.equal(palm.grad, torch.cat([g_pp, g_po], 1))
    assert torch.isfinite(cost).all() and (cost > 0).float().mean() > 0.25 and q.grad.abs().max() > 0
    assert (rep["depth"][:, 0] == -np.inf).all() == (kind is None)


class _Grad:
    @staticmethod
    def of(gpis, X):
        from compliancedex_amd.gpis import gpis_mean
        return gpis_mean(gpis.native_state(), X, want_grad=True)[1]


@pytest.mark.parametrize("kind", ["gpis", "mesh"])
def test_penetration_report(kind):
    from compliancedex_amd import penetration_report
    hs = golden_hand()
    obj, center = banana(kind)
    q = _dev(hs.rest_q[None])
    mid = [i for i, (l, c) in enumerate(zip(hs.links, hs.local)) if l == "base_link" and abs(c[1]) < 1e-6][1]
    ch = hs.centers(q)[0, mid].cpu().numpy()  # the palm's middle sphere in the hand frame
    inside = _dev(np.concatenate([center - ch, np.zeros(3)])[None])
    away = inside.clone()
    away[0, 2] += 1.0
    rep = penetration_report(hs, q, inside, obj)
    assert set(rep) == {"depth", "worst", "clear"}  # nothing resolved (or read back) until asked
    assert not bool(rep["clear"][0]) and float(rep["depth"][0, 0]) > 0
    assert rep["worst_links"][0][0] == "base_link"
    assert (rep["depth"][:, 2] == -np.inf).all() and rep["worst_links"][0][2] is None
    far = penetration_report(hs, q, away, obj)
    print(kind, "depth inside", rep["depth"].cpu().numpy(), "away", far["depth"].cpu().numpy())
    if kind == "mesh":
        assert bool(far["clear"][0])
        assert not bool(penetration_report(hs, q, away, obj, floor_z=float(away[0, 2]))["clear"][0])  # the floor class
    else:
        # The posterior mean is a distance only near the data it was fitted to: 1 m from the banana the thin-plate
        # extrapolation of the packaged state is −22 (measured), so with a GPIS the far hand is NOT reported clear.  The
        # far case is asserted on the mesh; here only that the answer is the mean's, whatever its sign.
        c = hs.centers(q, away)
        assert torch.equal(far["depth"][:, 0], (_dev(hs.radius)[None] - obj.pred_mean(c.reshape(-1, 3))[None]).max(1).values)
