"""The whole-hand sphere model without a GPU: the sphere and pair rules of compliancedex_amd.hand, and the host build of
csrc/cdx_hand.h (the code the kernels run) against the float64 statement of tests/_hand.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

from compliancedex_amd.hand import HandSpheres, box_spheres, cylinder_spheres, spheres_from_urdf
from tests import _chains, _hand as H, _host

IDS = [f"{c}-S{s}-{p}" for c, s, p in H.FAMILIES]

URDF = """<?xml version="1.0"?>
<robot name="prims">
  <link name="palm"><collision><origin xyz="0.01 0.02 0.03" rpy="0 0 1.5707963267948966"/>
    <geometry><box size="0.0408 0.1130 0.095"/></geometry></collision></link>
  <link name="finger"><collision><geometry><box size="0.0196 0.0275 0.054"/></geometry>
    <origin xyz="0 0 0.027" rpy="0 0 0"/></collision></link>
  <link name="rod"><collision><geometry><cylinder radius="0.01" length="0.05"/></geometry></collision></link>
  <link name="disc"><collision><origin xyz="0 0 0.1"/><geometry><cylinder radius="0.02" length="0.01"/></geometry>
    </collision></link>
  <link name="ball"><collision><origin xyz="0.1 0.2 0.3" rpy="0.3 0.2 0.1"/><geometry><sphere radius="0.015"/></geometry>
    </collision>
    <collision><geometry><mesh filename="ball.stl"/></geometry></collision></link>
  <joint name="j1" type="revolute"><parent link="palm"/><child link="finger"/><origin xyz="0 0 0.1"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1"/></joint>
  <joint name="j2" type="revolute"><parent link="finger"/><child link="rod"/><origin xyz="0 0 0.1"/><axis xyz="1 0 0"/>
    <limit lower="-1" upper="1"/></joint>
  <joint name="j3" type="fixed"><parent link="rod"/><child link="disc"/><origin xyz="0 0 0.1"/></joint>
  <joint name="j4" type="revolute"><parent link="disc"/><child link="ball"/><origin xyz="0 0 0.1"/><axis xyz="0 1 0"/>
    <limit lower="-1" upper="1"/></joint>
</robot>
"""


def _sorted(items):
    return sorted((tuple(round(v, 9) for v in c), round(r, 9)) for c, r in items)


# ------------------------------------------------------------------ 1. the box, cylinder and sphere rule
def test_primitive_rules(tmp_path):
    path = os.path.join(str(tmp_path), "prims.urdf")
    with open(path, "w") as f:
        f.write(URDF)
    spheres, skipped = spheres_from_urdf(path)
    # the Allegro palm: r = 0.0204, a 1 × 3 × 3 grid at y = 0, ±0.0361 and z = 0, ±0.0271; Rz(90°) takes (x, y, z) to
    # (−y, x, z), then the origin's translation
    want = [((-y + 0.01, 0.0 + 0.02, z + 0.03), 0.0204) for y in (-0.0361, 0.0, 0.0361) for z in (-0.0271, 0.0, 0.0271)]
    assert _sorted(spheres["palm"]) == _sorted(want)
    # an Allegro finger link: r = 0.0098, 1 × 2 × 3 at y = ±0.00395 and z = 0, ±0.0172 (moved up by 0.027)
    want = [((0.0, y, z + 0.027), 0.0098) for y in (-0.00395, 0.00395) for z in (-0.0172, 0.0, 0.0172)]
    assert _sorted(spheres["finger"]) == _sorted(want)
    # L ≥ 2ρ: r = ρ, n = ceil(0.05/0.02) = 3 centres from −L/2 + r to L/2 − r
    assert _sorted(spheres["rod"]) == _sorted([((0.0, 0.0, z), 0.01) for z in (-0.015, 0.0, 0.015)])
    # L < 2ρ: the box (0.04, 0.04, 0.01): r = 0.005, a 4 × 4 × 1 grid from −0.015 to 0.015
    g = (-0.015, -0.005, 0.005, 0.015)
    assert _sorted(spheres["disc"]) == _sorted([((x, y, 0.1), 0.005) for x in g for y in g])
    assert _sorted(spheres["ball"]) == _sorted([((0.1, 0.2, 0.3), 0.015)])
    assert skipped == [("ball", "ball.stl")]
    with pytest.raises(ValueError):
        spheres_from_urdf(path, strict=True)
    # neighbours at most 2r apart, every sphere inside its box
    for size in ((0.0408, 0.1130, 0.095), (0.0196, 0.0275, 0.054), (0.03, 0.03, 0.03), (0.02, 0.0401, 0.1)):
        items = box_spheres(size)
        c = np.array([x[0] for x in items])
        r = items[0][1]
        assert r == min(size) / 2
        assert (np.abs(c) + r <= np.array(size) / 2 + 1e-12).all()
        for ax in range(3):
            u = np.unique(np.round(c[:, ax], 12))
            assert len(u) == 1 or np.diff(u).max() <= 2 * r + 1e-12
    assert len(cylinder_spheres(0.01, 0.02)) == 1 and len(cylinder_spheres(0.01, 0.0201)) == 2
    hs = HandSpheres.from_urdf(path)
    assert hs.skipped == skipped and hs.n_spheres == 9 + 6 + 3 + 16 + 1
    assert (np.diff(hs.body) >= 0).all() and hs.links[0] == "palm" and hs.links[-1] == "ball"
    assert hs.local.dtype == np.float32 and (hs.radius == hs.radius.astype(np.float32)).all()
    with pytest.raises(ValueError):
        HandSpheres(path, {"nolink": [((0, 0, 0), 0.01)]})
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            HandSpheres(path, {"palm": [((0, 0, 0), bad)]})
    with pytest.raises(ValueError):
        HandSpheres(path, {})
    with pytest.raises(ValueError):
        HandSpheres(path, {"palm": [((0, 0, 0), 0.01)] * 257})


# ------------------------------------------------------------------ 2. the pair rule
def _pairs(hs):
    return {(int(a), int(b)) for a, b in hs.pairs}


def test_pair_rule_line():
    robot = _chains.line(6)
    one = {f"b{i}": [((0, 0, 0), 0.01)] for i in range(7)}
    for skip in (0, 1, 2):  # tree distance on a line is the index difference
        hs = HandSpheres(robot, one, skip=skip)
        assert _pairs(hs) == {(a, b) for a in range(7) for b in range(a + 1, 7) if b - a > skip}
    two = dict(one, b3=[((0, 0, 0), 0.01), ((0, 0.05, 0), 0.01)])  # spheres 3 and 4 share a body: never a pair
    hs = HandSpheres(robot, two, skip=0)
    assert (3, 4) not in _pairs(hs) and len(hs.pairs) == 8 * 7 // 2 - 1
    # bodies 0.1 apart: with r = 0.11 the pairs two bodies apart (0.22 > 0.2) overlap at rest and go, the rest stay
    hs = HandSpheres(robot, {k: [((0, 0, 0), 0.11)] for k in one}, skip=1)
    assert _pairs(hs) == {(a, b) for a in range(7) for b in range(a + 1, 7) if b - a > 2}
    # a curled rest pose: exactly the pairs that overlap there are removed
    rest = np.full(6, 1.0)
    hs = HandSpheres(robot, {k: [((0, 0, 0), 0.06)] for k in one}, skip=1, rest_q=rest)
    with torch.no_grad():
        c = H.centers_of(hs, torch.from_numpy(rest[None]), None)[0][0].numpy()
    over = {(a, b) for a in range(7) for b in range(a + 1, 7) if 0.12 - np.linalg.norm(c[a] - c[b]) > 0}
    far = {(a, b) for a in range(7) for b in range(a + 1, 7) if b - a > 1}
    assert over & far and far - over
    assert _pairs(hs) == far - over
    assert _pairs(HandSpheres(robot, {k: [((0, 0, 0), 0.06)] for k in one}, skip=1)) == far  # straight: none overlaps


def test_pair_rule_tree():
    robot = _chains.robot_dict("hand8")  # arm 0 … 4, fingers 5-8, 9-11, 12-15, 16-17 off body 4
    parent = [b["parent"] for b in robot["bodies"]]

    def dist(a, b):
        up = lambda x: [x] + (up(parent[x]) if parent[x] >= 0 else [])  # noqa: E731
        pa, pb = up(a), up(b)
        lca = next(x for x in pa if x in pb)
        return pa.index(lca) + pb.index(lca)
    hs = HandSpheres(robot, {b["name"]: [((0, 0, 0), 1e-4)] for b in robot["bodies"]}, skip=1)
    assert hs.tree_distance(8, 11) == 7 and hs.tree_distance(5, 9) == 2 and hs.tree_distance(4, 5) == 1
    assert hs.tree_distance(17, 0) == 6 and hs.tree_distance(3, 3) == 0
    n = len(parent)
    for skip in (0, 1, 2):
        hs = HandSpheres(robot, {b["name"]: [((0, 0, 0), 1e-4)] for b in robot["bodies"]}, skip=skip)
        assert _pairs(hs) == {(a, b) for a in range(n) for b in range(a + 1, n) if dist(a, b) > skip}
    hs1 = HandSpheres(robot, {"b5": [((0, 0, 0), 1e-4)], "b9": [((0, 0, 0), 1e-4)]}, skip=1)
    hs2 = HandSpheres(robot, {"b5": [((0, 0, 0), 1e-4)], "b9": [((0, 0, 0), 1e-4)]}, skip=2)
    assert _pairs(hs1) == {(0, 1)} and _pairs(hs2) == set()  # siblings across the common ancestor: 2 joints apart
    with pytest.raises(ValueError):
        HandSpheres(robot, {"b5": [((0, 0, 0), 0.01)]}, pairs=[[0, 0]])
    assert len(HandSpheres(robot, {"b5": [((0, 0, 0), 0.01)] * 3}, pairs=[[0, 2]]).pairs) == 1


def test_host_prepare_checks():
    local, radius = np.zeros((3, 3), np.float32), np.full(3, 0.01)
    body, pairs = np.array([0, 1, 1], np.int32), np.array([[0, 1], [0, 2]], np.int32)
    assert H.host_prepare_raw(2, local, radius, body, pairs)[0] == 0
    assert H.host_prepare_raw(2, local, radius, np.array([1, 0, 1], np.int32), pairs)[0] == -1  # not sorted by body
    assert H.host_prepare_raw(1, local, radius, body, pairs)[0] == -1  # a body the chain does not have
    assert H.host_prepare_raw(2, local, np.array([0.01, 0.0, 0.01]), body, pairs)[0] == -1
    assert H.host_prepare_raw(2, local, np.array([0.01, np.nan, 0.01]), body, pairs)[0] == -1
    assert H.host_prepare_raw(2, local, radius, body, np.array([[1, 1]], np.int32))[0] == -1
    assert H.host_prepare_raw(2, local, radius, body, np.array([[0, 3]], np.int32))[0] == -1
    rc, h, buf = H.host_prepare_raw(2, local, radius, body, pairs)
    # the partner table: entry k of sphere s at group_base[s / 64] + 64k + s % 64 = partner | pair << 8
    assert np.frombuffer(buf, np.int32, 3, h.len - buf.ctypes.data).tolist() == [2, 1, 1] and list(h.group_base) == [0, 128, 128, 128]
    en = np.frombuffer(buf, np.int32, 128, h.entry - buf.ctypes.data)
    assert [en[0] & 255, en[0] >> 8, en[64] & 255, en[64] >> 8] == [1, 0, 2, 1]
    assert [en[1] & 255, en[1] >> 8, en[2] & 255, en[2] >> 8] == [0, 0, 0, 1] and (en[3:64] == -1).all()
    # a sphere in more pairs than min(S − 1, P) can hold (a repeated pair) is refused
    assert H.host_prepare_raw(2, local, radius, body, np.array([[0, 1], [0, 1], [0, 1]], np.int32))[0] == -1


def test_sincos():
    """hand_sincos (what both builds run for the palm's angles) against libm: one unit in the last place."""
    x = np.concatenate([np.random.default_rng(0).uniform(-20, 20, 20000), np.linspace(-1e5, 1e5, 2001),
                        [0.0, math.pi / 2, math.pi, -math.pi / 4, 1e6]])
    s, c = np.zeros_like(x), np.zeros_like(x)
    H.host_lib().cdxh_hand_sincos(H.ptr(x), len(x), H.ptr(s), H.ptr(c))
    assert np.abs(s - np.sin(x)).max() <= 2.3e-16 and np.abs(c - np.cos(x)).max() <= 2.3e-16
    bad = np.array([np.nan, np.inf, -np.inf, 1.0000001e6])
    s, c = np.zeros_like(bad), np.zeros_like(bad)
    H.host_lib().cdxh_hand_sincos(H.ptr(bad), len(bad), H.ptr(s), H.ptr(c))
    assert np.isnan(s).all() and np.isnan(c).all()
    z = np.zeros(1)
    H.host_lib().cdxh_hand_sincos(H.ptr(z), 1, H.ptr(s), H.ptr(c))
    assert s[0] == 0.0 and c[0] == 1.0


# ------------------------------------------------------------------ 3. centres
@pytest.mark.parametrize("case,S,pairs", H.FAMILIES, ids=IDS)
def test_centers(case, S, pairs):
    fam = H.family(case, S, pairs)
    poses, centers = H.host_spheres(fam["hs"], fam["q"], fam["palm"])
    H.check_centers(fam, centers, H.E_MAX)
    for E in H.BATCHES[:-1]:
        p, c = H.host_spheres(fam["hs"], fam["q"][:E], fam["palm"][:E])
        assert H.same_bits(p, poses[:E]) and H.same_bits(c, centers[:E])


@pytest.mark.parametrize("case", ["hand8", "tree8", "line16", "allegro"])
def test_centers_at_link_origins_are_fk(case):
    """Spheres at the link origins: the centres are the host fk_forward positions of those links (requested at most 8
    tips at a time, without offsets) — the same recurrence, bit for bit."""
    robot = H.robot_of(case)
    hs = HandSpheres(robot, {b["name"]: [((0, 0, 0), 0.01)] for b in hs_bodies(robot)}, pairs=[])
    rng = np.random.default_rng(5)
    q = rng.uniform(-H.PI, H.PI, (65, hs.desc.n_dofs)).astype(np.float32)
    poses, centers = H.host_spheres(hs, q.astype(np.float64), None)
    names = [b["name"] for b in hs.chain.bodies]
    for lo in range(0, len(names), 8):
        pos, _ = _host.fk_forward(hs.chain.descriptor(names[lo:lo + 8], None), q)
        pos = pos.reshape(65, -1, 3)
        assert H.same_bits(pos, np.ascontiguousarray(poses[:, lo:lo + 8, 9:]))
        assert np.array_equal(pos.astype(np.float64), centers[:, lo:lo + 8])
    zero = np.zeros((65, 6))
    assert np.array_equal(H.host_spheres(hs, q.astype(np.float64), zero)[1], centers)  # null palm = identity palm


def hs_bodies(robot):
    from compliancedex_amd.urdf import load_robot
    return (robot if isinstance(robot, dict) else load_robot(robot))["bodies"]


# ------------------------------------------------------------------ 4. cost, depth, worst, g_centers
@pytest.mark.parametrize("case,S,pairs", H.FAMILIES, ids=IDS)
def test_cost(case, S, pairs):
    fam = H.family(case, S, pairs)
    got = H.host_cost(fam["hs"], H.params_struct(), fam["centers"], fam["dist"], fam["gdist"])
    H.check_cost(fam, got, H.E_MAX)
    if not len(fam["hs"].pairs):
        assert (got[1][:, 1] == -np.inf).all() and (got[2][:, 1] == -1).all()


def test_cost_classes_off_and_coincident_centres():
    fam = H.family("hand8", 63, "full")
    hs, c = fam["hs"], fam["centers"][:65]
    cost, depth, worst, g = H.host_cost(hs, H.params_struct(floor=False), c)
    ref = H.cost_of(hs, c, None, None, floor=False)
    assert (depth[:, [0, 2]] == -np.inf).all() and (worst[:, [0, 2]] == -1).all()
    assert np.array_equal(worst, ref["worst"]) and (np.abs(cost - ref["cost"]) <= 1e-12 * ref["abs_cost"]).all()
    assert (np.abs(g - ref["g"]) <= 1e-12 * ref["abs_g"]).all()
    # ρ = 0: the cost counts, the direction is zero
    two = HandSpheres(H.robot_of("hand8"), {"b3": [((0, 0, 0), 0.01)], "b7": [((0, 0, 0), 0.02)]}, pairs=[[0, 1]])
    same = np.tile(np.array([0.1, -0.2, 0.3]), (5, 2, 1))
    cost, depth, worst, g = H.host_cost(two, H.params_struct(floor=False, m_self=0.005, w_self=0.7), same)
    rr = float(np.float32(0.01)) + float(np.float32(0.02))  # (the model keeps float32 radii)
    np.testing.assert_allclose(cost, 0.7 * 0.5 * (rr + 0.005) ** 2, rtol=1e-14)
    assert (g == 0).all() and (depth[:, 1] == rr).all() and (worst[:, 1] == 0).all()


# ------------------------------------------------------------------ 5. pull-back
@pytest.mark.parametrize("case,S,pairs", H.FAMILIES, ids=IDS)
def test_pullback(case, S, pairs):
    fam = H.family(case, S, pairs)
    hs = fam["hs"]
    poses, _ = H.host_spheres(hs, fam["q"], fam["palm"])
    got = H.host_pullback(hs, poses, fam["cost"]["g"], fam["palm"][:, 3:])
    H.check_pullback(fam, got, H.E_MAX, poses)
    for j in range(1, hs.desc.n_bodies):
        b = hs.desc.bodies[j]
        if b.dof >= 0 and b.sign == 0:
            assert (got[0][:, b.dof] == 0).all()
    if case in _chains.CASES:
        assert any(hs.desc.bodies[j].dof >= 0 and hs.desc.bodies[j].sign == 0 for j in range(1, hs.desc.n_bodies))


def test_pullback_null_palm_is_identity_palm():
    fam = H.family("tree8", 65, "one")
    hs = fam["hs"]
    poses, _ = H.host_spheres(hs, fam["q"][:65], None)
    g = fam["cost"]["g"][:65]
    a, b = H.host_pullback(hs, poses, g, None), H.host_pullback(hs, poses, g, np.zeros((65, 3)))
    assert all(H.same_bits(x, y) for x, y in zip(a, b))
    ref = H.pullback_of(hs, fam["q"][:65], np.zeros((65, 6)), g)
    l1 = np.abs(g).sum((1, 2))
    assert (np.abs(a[0] - ref[0]).max(1) <= _chains.TOL_JAC * l1).all()
    assert (np.abs(a[1] - ref[1]).max(1) <= 1e-12 * l1).all()


# ------------------------------------------------------------------ 6. rows
@pytest.mark.parametrize("case,S,pairs", H.SMALL, ids=[f"{c}-S{s}-{p}" for c, s, p in H.SMALL])
def test_rows(case, S, pairs):
    H.check_rows(H.family(case, S, pairs), H.host_spheres, H.host_cost, H.host_pullback)


# ------------------------------------------------------------------ the fixture
def test_golden_allegro_spheres():
    with open(H.GOLDEN) as f:
        d = json.load(f)
    assert set(d) == {"links", "centers", "radii"} and len(d["links"]) == len(d["centers"]) == len(d["radii"])
    spheres = {}
    for link, c, r in zip(d["links"], d["centers"], d["radii"]):
        spheres.setdefault(link, []).append((c, r))
    hs = HandSpheres("allegro", spheres)
    assert hs.n_spheres == len(d["links"]) <= 256 and 0 < len(hs.pairs) <= 32768
    assert sum(link == "base_link" for link in hs.links) == 9  # the palm box: 1 × 3 × 3
    c = hs.rest_centers()
    a, b = hs.pairs[:, 0], hs.pairs[:, 1]
    assert (hs.radius[a] + hs.radius[b] - np.linalg.norm(c[a] - c[b], axis=1) <= 0).all()  # no cost at rest
