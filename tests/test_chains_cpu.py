"""FK, its gradients and the depth limit on synthetic chains (tests/_chains.py), on the CPU: the host build of the
per-candidate code (libcdx_host.so) against the float64 statement, the conditions that keep those comparisons from
passing on thin data, and the argument checks of every entry that walks a chain (the host twins, and libcdx.so's own
entries, which refuse before they touch a device).  No GPU.

Which form of the FK gradient each test reaches (csrc/cdx_fk.h):
  test_host_primitives_vs_statement   fk_tip, fk_tip_bwd<16> (the host's cdxh_fk_backward), fk_jacobian_tip
  test_closure_host_vs_oracle         fk_tip_bwd<16> inside closure_candidate (hand8, hand16)
  test_kingpis_host_vs_autograd       fk_tip_bwd<8> at its limit (hand8), fk_tip_bwd2<16> (hand9: first depth, hand16: last)
  test_collision_host_vs_oracle       fk_tip_bwd<16> inside collision_candidate (tree8: 8 anchors, 31 DOFs)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from compliancedex_amd import _native as N
from tests import _chains as ch
from tests import _host, _ik
from tests._helpers import oracle_gpis, oracle_gpis_at, rel_err
from tests._host import p

GUARD = 3  # output rows past the last, preset and found untouched
ECHAIN = -3


# ------------------------------------------------------------------ the family and its data
def test_family_reaches_the_descriptor_edges(tmp_path):
    seen = set()
    for case in ch.CASES:
        b, links = ch.bodies(case)
        d = ch.descriptor(case)
        assert d.n_dofs == sum(x["joint"] != "fixed" for x in b[1:])  # no shared DOFs: one per moving body
        assert sorted(d.bodies[i].dof for i in range(d.n_bodies) if d.bodies[i].dof >= 0) == list(range(d.n_dofs))
        signs = [(d.bodies[i].axis, d.bodies[i].sign) for i in range(1, d.n_bodies) if d.bodies[i].dof >= 0]
        seen |= set(signs)
        assert any(s == 0.0 for _, s in signs), case  # a joint with axis (0, 0, 0)
        on = _ik.on_path(d)
        zero = [d.bodies[i].dof for i in range(d.n_bodies) if d.bodies[i].dof >= 0 and d.bodies[i].sign == 0.0]
        assert on[:, zero].any(), case  # … on a tip's path
        # the same chain through the JSON file, as the optimisers load it
        from compliancedex_amd.chain import Chain
        from compliancedex_amd.urdf import load_robot
        dj = Chain(load_robot(ch.write_json(case, tmp_path))).descriptor(links, ch.tip_offsets(case))
        assert bytes(dj) == bytes(d)
    assert seen >= {(a, s) for a in (0, 1, 2) for s in (1.0, -1.0)}
    assert ch.depths("line8") == [8, 3] and ch.depths("line9") == [9, 0] and ch.depths("line16") == [16]
    t8 = ch.descriptor("tree8")
    assert (t8.n_bodies, t8.n_tips, t8.n_dofs) == (N.MAX_BODIES, N.MAX_TIPS, 31)
    assert min(ch.depths("tree8")) == 1 and max(ch.depths("tree8")) == 12
    parents = {t8.bodies[i].parent for i in range(t8.n_bodies)}
    assert any(t8.tip_body[k] in parents for k in range(8))  # a tip on an inner body
    for case, deepest in zip(ch.HANDS, (8, 9, 16)):
        assert ch.descriptor(case).n_tips == 4 and max(ch.depths(case)) == deepest
    for case in ("line9", "line16") + ch.HANDS:
        d = ch.descriptor(case)
        assert any(d.bodies[i].dof < 0 for i in range(1, d.n_bodies)), case  # a fixed joint


@pytest.mark.parametrize("offsets", [True, False])
@pytest.mark.parametrize("case", ch.CASES)
def test_reference_conditions(case, offsets):
    """Branch coverage and the exclusion cap are asserted inside _chains.reference; here also the reach."""
    ref = ch.reference(case, offsets)
    assert np.linalg.norm(ref["pos"], axis=2).max() <= ch.REACH
    assert ref["keep"].mean() >= 1.0 - ch.MAX_EXCLUDED
    if offsets:
        for br in (-1, 0, 1, 2):
            assert (ref["branch"] == br).sum() >= ch.MIN_PER_BRANCH


def test_statement_is_the_jacobian_transpose_away_from_the_scale():
    """Without offsets the detached scale plays no part: the statement's VJP is np_fk_jac's Jacobian transposed, up to
    the descriptor's F (float32 values, orthonormal to 6e-8 only): autograd differentiates the products as they are,
    the geometric Jacobian takes ω × (p − o) as if F were a rotation.  Two independent float64 statements that agree
    far below the tolerances; a wrong sign, axis or path in either shows at 1."""
    for case in ("line9", "tree8"):
        ref = ch.reference(case, False)
        _, lin, _ = _ik.np_fk_jac(ch.descriptor(case, False), ref["q"][:9])
        vjp = np.einsum("btid,bti->bd", lin, ref["gpos"][:9].astype(np.float64))
        assert ch.rel(vjp, ref["grad"][:9]) < 2e-7


def test_oracle_error_is_the_measured_one():
    """The tolerances are 4 × ORACLE_ERR: the float32 oracle against the float64 statement gives those figures (within
    a factor 2 either way: another libm or BLAS moves the last digit, a stale constant would be off by more)."""
    e = ch.measure_oracle()
    for k, v in ch.ORACLE_ERR.items():
        assert 0.5 * v <= e[k] <= 2.0 * v, (k, e[k], v)
        assert ch.TOL[k] == 4.0 * v


# ------------------------------------------------------------------ host build against the statement
def host_fk(desc, q, B, quat=True):
    T = desc.n_tips
    pos = np.full((B + GUARD, 3 * T), 7.0, np.float32)
    qt = np.full((B + GUARD, 4 * T), 7.0, np.float32)
    rc = _host.host().cdxh_fk_forward(C.byref(desc), p(np.ascontiguousarray(q[:B])), B, p(pos),
                                      p(qt) if quat else None)
    assert (pos[B:] == 7.0).all() and (qt[B:] == 7.0).all()
    return rc, pos[:B], qt[:B]


def host_bwd(desc, q, gpos, B):
    gq = np.full((B + GUARD, desc.n_dofs), 7.0, np.float32)
    rc = _host.host().cdxh_fk_backward(C.byref(desc), p(np.ascontiguousarray(q[:B])), B,
                                       p(np.ascontiguousarray(gpos[:B])), p(gq))
    assert (gq[B:] == 7.0).all()
    return rc, gq[:B]


def host_jac(desc, q, B, ang=True):
    T, D = desc.n_tips, desc.n_dofs
    lin = np.full((B + GUARD, T, 3, D), 7.0, np.float32)
    a = np.full((B + GUARD, T, 3, D), 7.0, np.float32)
    rc = _host.host().cdxh_fk_jacobian(C.byref(desc), p(np.ascontiguousarray(q[:B])), B, p(lin),
                                       p(a) if ang else None)
    assert (lin[B:] == 7.0).all() and (a[B:] == 7.0).all()
    return rc, lin[:B], a[:B] if ang else None


@pytest.mark.parametrize("offsets", [True, False])
@pytest.mark.parametrize("case", ch.CASES)
def test_host_primitives_vs_statement(case, offsets):
    def fk(desc, q, B):
        rc, pos, quat = host_fk(desc, q, B)
        assert rc == 0
        return pos, quat

    def bwd(desc, q, gpos, B):
        rc, g = host_bwd(desc, q, gpos, B)
        assert rc == 0
        return g

    def jac(desc, q, B, ang):
        rc, lin, a = host_jac(desc, q, B, ang)
        assert rc == 0
        return lin, a
    ch.check_primitives(case, offsets, fk, bwd, jac)


# ------------------------------------------------------------------ the depth limit
def deep_descriptor(depth, n_tips=1, offsets=False):
    robot = ch.line(depth)
    offs = [[0.01, -0.02, 0.03]] * n_tips if offsets else None
    return ch.raw_descriptor(robot, [f"b{depth}"] * n_tips, offs)


def test_depth_16_is_accepted_and_correct():
    for offsets in (False, True):
        desc = deep_descriptor(16, 1, offsets)
        assert bytes(desc) == bytes(ch.chain_of(ch.line(16)).descriptor(["b16"], [[0.01, -0.02, 0.03]] if offsets else None))
        q = np.full((3, 16), 0.1, np.float32)
        gpos = np.ones((3, 1, 3), np.float32)
        ref = ch.statement(desc, q, gpos)
        rc, pos, quat = host_fk(desc, q, 3)
        assert rc == 0 and ch.rel(pos.reshape(3, 1, 3), ref["pos"]) < ch.TOL["pos"]
        assert ch.rel(quat.reshape(3, 1, 4), ref["quat"]) < ch.TOL["quat"]
        rc, g = host_bwd(desc, q, gpos, 3)
        assert rc == 0 and ch.rel(g, ref["grad"]) < ch.TOL["grad"]
        assert (g[:, :15] != 0).all()  # every joint above the tip's own moves it, the root-side ones included
        rc, lin, _ = host_jac(desc, q, 3)
        assert rc == 0 and rel_err(lin, _ik.np_fk_jac(desc, q)[1]) < ch.TOL_JAC


@pytest.mark.parametrize("depth", [17, 19])
def test_chain_descriptor_refuses_an_over_deep_tip(depth):
    c = ch.chain_of(ch.line(depth))
    with pytest.raises(ValueError, match=rf"b{depth}.*{depth} bodies"):
        c.descriptor([f"b{depth}"])
    with pytest.raises(ValueError, match=rf"b{depth}"):
        c.descriptor(["b3", f"b{depth}"], [[0.0] * 3] * 2)
    assert c.descriptor(["b16", "b1"]).n_tips == 2  # the same robot's tips within the limit are fine
    assert N.MAX_DEPTH == 16


@pytest.mark.parametrize("depth", [17, 19])
def test_host_entries_refuse_an_over_deep_chain(depth):
    """Every cdxh_* twin returns CDX_ECHAIN and writes nothing.  (On the parent commit cdxh_fk_forward answered such a
    chain with the depth-16 position, (1.0502, 0.9784, 0) for (1.0473, 1.0783, 0) at depth 17.)"""
    from compliancedex_amd.problem import build_collision, build_problem
    h = _host.host()
    desc = deep_descriptor(depth, 1)
    q = np.full((2, depth), 0.1, np.float32)
    rc, pos, quat = host_fk(desc, q, 2)
    assert rc == ECHAIN and (pos == 7.0).all() and (quat == 7.0).all()
    rc, g = host_bwd(desc, q, np.ones((2, 1, 3), np.float32), 2)
    assert rc == ECHAIN and (g == 7.0).all()
    rc, lin, ang = host_jac(desc, q, 2)
    assert rc == ECHAIN and (lin == 7.0).all() and (ang == 7.0).all()
    # IK
    lower, upper = [-3.0] * depth, [3.0] * depth
    from compliancedex_amd.ik import ik_params
    par = ik_params(lower, upper, [0.0] * depth, 0.0, 5, 1e-5)
    outs = [np.full((2, depth), 7.0), np.full((2, 1), 7.0), np.full(2, -7, np.int32), np.full(2, -7, np.int32)]
    q0, target = np.zeros((2, depth)), np.zeros((2, 1, 3))
    rc = h.cdxh_ik_solve(C.byref(desc), C.byref(par), 2, p(q0), 1, p(target), None, None, None,
                         *[p(a) for a in outs])
    assert rc == ECHAIN and all((a == (7.0 if a.dtype == np.float64 else -7)).all() for a in outs)
    # closure: queries and cost
    d4 = deep_descriptor(depth, 4, offsets=True)
    prob = build_problem(d4, None, ref_q=[0.0] * depth)
    X = np.full((400, 3), 7.0)
    z = lambda *s: np.zeros(s)  # noqa: E731
    assert h.cdxh_closure_queries(C.byref(prob), 1, p(z(1, depth)), p(z(1, 4, 3)), p(z(1, 3)), p(z(1, 3)),
                                  p(X)) == ECHAIN and (X == 7.0).all()
    outs = [np.full(s, 7.0) for s in ((1,), (1, 4), (1, depth), (1, 4), (1, 4, 3), (1, 3), (1, 3))]
    flip = np.full(4, -7, np.int32)
    gp = [z(400), z(400, 3), z(400, 3), z(400), z(400, 3)]
    assert h.cdxh_closure_cost(C.byref(prob), 1, p(z(1, depth)), p(z(1, 4) + 10), p(z(1, 4, 3)), p(z(1, 3)),
                               p(z(1, 3)), p(z(3, 9)), *[p(a) for a in gp], *[p(a) for a in outs], p(flip)) == ECHAIN
    assert all((a == 7.0).all() for a in outs) and (flip == -7).all()
    # collision
    col = build_collision(d4, [[0, 1]])
    outs = [np.full(s, 7.0) for s in ((1,), (1, depth), (1, 3), (1, 3))]
    assert h.cdxh_collision(C.byref(col), 1, p(z(1, depth)), p(z(1, 3)), p(z(1, 3)),
                            *[p(a) for a in outs]) == ECHAIN and all((a == 7.0).all() for a in outs)
    # KinGPIS: the loop state of a valid chain, then the over-deep descriptor in its place
    from tests.test_gpis_mode_cpu import HostLoop, _inputs, _lib, _opt, _params
    hand = kingpis_hand("hand16")
    pose0, target0, comp0, noise = _inputs(1, hand, n=2)
    loop = HostLoop(1, hand, pose0, target0, comp0)
    for k in ("loss", "g_pose", "g_target", "g_comp", "pose", "v_pose"):
        loop.a[k][:] = 7.0
    prm, cfg = _params(1, hand), _opt((2e-3, 1e-3, 0.2))
    nz = np.ascontiguousarray(noise[0].reshape(2, 9))
    assert _lib().cdxh_gpis_mode_cost(d4, prm, loop.b, 2, 4, p(nz), 0, 0) == ECHAIN
    assert _lib().cdxh_gpis_mode_step(d4, prm, cfg, loop.b, 2, 4, 0, 0) == ECHAIN
    for k in ("loss", "g_pose", "g_target", "g_comp", "pose", "v_pose"):
        assert (loop.a[k] == 7.0).all(), k


def _device_entry_codes(desc4, desc1):
    """Return codes of libcdx.so's entries for a chain (4 tips where the entry wants the hand's four, else 1): every
    pointer NULL, E = 2 — a refused chain returns before any pointer is looked at and before any launch."""
    from compliancedex_amd.problem import build_collision, build_problem
    lib = N.load()
    D = desc4.n_dofs
    codes = {}
    codes["fk_forward"] = lib.cdx_fk_forward(desc1, None, 2, None, None, None)
    codes["fk_backward"] = lib.cdx_fk_backward(desc1, None, 2, None, None, None)
    codes["fk_jacobian"] = lib.cdx_fk_jacobian(desc1, None, 2, None, None, None)
    from compliancedex_amd.ik import ik_params
    par = ik_params([-3.0] * D, [3.0] * D, [0.0] * D, 0.0, 5, 1e-5)
    codes["ik_solve"] = lib.cdx_ik_solve(desc1, C.byref(par), 2, None, N.DTYPE_F64, *[None] * 9, None)
    prob = build_problem(desc4, None, ref_q=[0.0] * D)
    codes["closure"] = lib.cdx_closure(prob, 2, *([None] * 6), C.c_uint64(0), *([None] * 11))
    codes["closure_workspace"] = lib.cdx_closure_workspace(prob, 2)
    codes["collision_loss"] = lib.cdx_collision_loss(build_collision(desc4, [[0, 1]]), 2, *[None] * 7, 0, None)
    kp, cfg, buf = N.CdxKinParams(), N.CdxKinOpt(), N.CdxKinOptBuffers()
    kp.fe.n_tips = 4
    cfg.rule = 0
    codes["kin_cost"] = lib.cdx_kin_cost(desc4, kp, 2, *[None] * 14, 0, *[None] * 7, None)
    codes["kin_step"] = lib.cdx_kin_step(desc4, cfg, buf, 2, 4, 0, 0, None)
    buf.tips = 1  # (never read: the chain is looked at first)
    for clamp in (0, 1):  # the one-launch form and the two launches
        cfg.clamp_box = clamp
        codes[f"kin_iteration{clamp}"] = lib.cdx_kin_iteration(desc4, kp, cfg, buf, 2, 4, *[None] * 10, 0, 0, None)
    gp, go, gb = N.CdxGpisModeParams(), N.CdxGpisModeOpt(), N.CdxGpisModeBuffers()
    gp.mode, gp.fe.n_tips = 1, 4
    codes["gpis_mode_cost"] = lib.cdx_gpis_mode_cost(desc4, gp, gb, 2, 4, None, 0, 0, None)
    codes["gpis_mode_step"] = lib.cdx_gpis_mode_step(desc4, gp, go, gb, 2, 4, 0, 0, None)
    codes["gpis_mode_iteration"] = lib.cdx_gpis_mode_iteration(desc4, gp, go, gb, 2, 4, None, 0, 0, None)
    return codes


@pytest.mark.parametrize("depth", [17, 19])
def test_device_entries_refuse_an_over_deep_chain_before_any_launch(depth):
    codes = _device_entry_codes(deep_descriptor(depth, 4, True), deep_descriptor(depth, 1))
    assert codes.pop("closure_workspace") == 0  # (a byte count: 0 for a problem it refuses)
    assert all(v == ECHAIN for v in codes.values()), codes


def test_device_entries_take_depth_16_past_the_chain_check():
    """The same calls with the tip 16 levels deep fail later, on the NULL pointers (CDX_EINVAL; the Jacobian and IK
    entries name a null pointer CDX_ECHAIN, so they are left out), and the workspace has a size."""
    codes = _device_entry_codes(deep_descriptor(16, 4, True), deep_descriptor(16, 1))
    assert codes.pop("closure_workspace") > 0
    codes.pop("fk_jacobian"), codes.pop("ik_solve")
    assert all(v == -1 for v in codes.values()), codes


def test_kin_and_gpis_mode_entries_check_the_tree():
    """They checked sizes only: a tip_body past n_bodies was read past the struct.  Now CDX_ECHAIN, as for a parent
    that does not precede its child."""
    for edit in ("tip", "parent"):
        d4, d1 = deep_descriptor(16, 4, True), deep_descriptor(16, 1)
        for d in (d4, d1):
            if edit == "tip":
                d.tip_body[0] = d.n_bodies
            else:
                d.bodies[5].parent = 9
        codes = _device_entry_codes(d4, d1)
        assert codes.pop("closure_workspace") == 0
        assert all(v == ECHAIN for v in codes.values()), (edit, codes)


# ------------------------------------------------------------------ the gradient forms inside their pipelines (host)
@pytest.mark.parametrize("case", ["hand8", "hand16"])
def test_closure_host_vs_oracle(case):
    """test_closure_host_vs_reference's comparison on a synthetic hand, E = 5, against OracleProblem + autograd."""
    from compliancedex_amd.problem import build_problem
    q, comp, target, palm, noise = ch.closure_inputs(case)
    prob = build_problem(ch.descriptor(case), None, ref_q=[0.0] * q.shape[1])
    ref = ch.oracle_closure(case, q, comp, target, palm, noise)
    X = _host.closure_queries(prob, q, target, palm)
    E, T = q.shape[0], 4
    pre = X[(prob.n_query_levels + 1) * E * T:(prob.n_query_levels + 2) * E * T].reshape(E, T, 3)
    assert rel_err(pre, ref["pregrasp_tip"]) < 1e-6
    g = oracle_gpis("banana")
    Ms = prob.n_query_levels * E * T
    gp = oracle_gpis_at(g, X, with_std=False)
    gs = oracle_gpis_at(g, X[:Ms], with_std=True)
    gp["std"], gp["gstd"] = gs["std"], gs["gstd"]
    out = _host.closure_cost(prob, q, comp, target, palm, noise, gp)
    errs = {k: rel_err(out[k], ref[k]) for k in ("total_loss", "total_margin", "grad_q", "grad_comp", "grad_target",
                                                 "grad_palm_pos", "grad_palm_ori")}
    assert all(v < 1e-4 for v in errs.values()), errs
    assert np.array_equal(out["flip"].astype(bool), ref["flip"])


@pytest.fixture(scope="module")
def gpis():
    """test_gpis_mode_cpu's 60-point box GPIS."""
    from compliancedex_amd.workloads import box_arrays
    from oracle.cdx_oracle import OracleGPIS
    X1, y, noise = box_arrays(n_surface=26)
    return OracleGPIS.fit(X1[:60], y[:60], noise[:60], bias=1.0)


def kingpis_hand(case):
    """The `hand` dict of tests/test_gpis_mode_cpu.py for a synthetic hand, built as test_deep_chain_gradient_vs_autograd
    builds its own."""
    from oracle.cdx_oracle import OracleChain
    b, links = ch.bodies(case)
    desc = ch.descriptor(case)
    D = desc.n_dofs
    tips0 = _host.fk_forward(desc, np.zeros((1, D), np.float32))[0].reshape(4, 3).astype(np.float64)
    return dict(ochain=OracleChain(b), links=links, offsets=ch.tip_offsets(case), desc=desc, ref_q=np.zeros(D),
                palm=np.array([0.0, 0.0, 0.03]) - tips0.mean(0), D=D)


@pytest.mark.parametrize("case", ch.HANDS)
def test_kingpis_host_vs_autograd(case, gpis):
    """test_deep_chain_gradient_vs_autograd on the synthetic hands: one KinGPIS iteration's loss and gradients against
    autograd through the oracle FK, at that test's tolerance."""
    from tests.test_gpis_mode_cpu import TOL, _inputs, _one_row, _ref_loss
    hand = kingpis_hand(case)
    h = _one_row(1, hand, gpis, n=3)
    q0, target0, comp0, noise = _inputs(1, hand, seed=3, n=3)
    q, target, comp = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (q0, target0, comp0))
    l, _, _ = _ref_loss(1, gpis, hand, q, target, comp, torch.from_numpy(noise[0]))
    l.sum().backward()
    assert np.isfinite(h.a["loss"]).all() and rel_err(h.a["loss"], l.detach().numpy()) < TOL[1]
    for k, t in (("g_pose", q), ("g_target", target), ("g_comp", comp)):
        assert rel_err(h.a[k], t.grad.numpy()) < TOL[1], k


def test_collision_host_vs_oracle():
    r = ch.collision_rows()
    for E in (1, 65):
        cost, g_q, g_palm = _host.collision(ch.collision_descriptor(), r["q"][:E], r["palm"][:E])
        assert np.array_equal(cost != 0, r["cost"][:E] != 0)
        assert rel_err(cost, r["cost"][:E]) < 1e-4
        assert rel_err(g_q, r["grad_q"][:E]) < 1e-4
        assert rel_err(g_palm, r["grad_palm"][:E]) < 1e-4
