"""FK, its gradients and IK on synthetic chains (tests/_chains.py) on an MI355X: the three primitives against the
float64 statement on every case, IK at the workgroup size the largest chain forces, the four forms of the FK gradient
inside their pipelines on the synthetic hands, the FK-walk cache seen to hit, and the depth limit.

Which instantiation each test reaches (csrc/cdx_fk.h; <8> / <16>: the level bound, chosen at depth 8 | 9):
  test_primitives_vs_statement          fk_forward_kernel, fk_backward_kernel<8> (line8, hand8) and <16> (the others):
                                        fk_tip_bwd, the chain read in place from the kernel arguments; fk_jacobian_kernel
  test_ik_at_the_largest_launch_shape   ik_solve_kernel at 4 rows a workgroup (tree8: T = 8, D = 31) and at 64 (line16);
                                        fk_jacobian_tip
  test_closure_vs_oracle                closure_combine_kernel<4, 8> (hand8) and <4, 16> (hand16): fk_tip_walk3s + bwd3
  test_kingpis_fused_equals_eager       gpis_mode kernel<4, 16>: fk_tip_bwd2 at its first depth (hand9) and its last
                                        (hand16), against cdx_fk_backward<16> through autograd
  test_collision_vs_oracle              collision_kernel: fk_tip_bwd<16> on tree8's 8 anchors, 31 DOFs
  test_kin_loop_forms_agree             kin_cost4_kernel<16, true, true> (one launch: bwd3 through the FK-walk cache),
                                        kin_cost4_kernel<16, true> + kin_step_kernel (two launches), on hand9 and hand16
  test_kin_fused_equals_autograd        the same against cdx_fk_backward<16> through autograd
  test_fk_walk_cache_hits               the cache's tags and q-check slots after a one-launch loop (iiwa7_allegro, hand16)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _chains as ch
from tests import _ik
from tests._helpers import rel_err
from tests._ik import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4  # output rows past the last, preset and found untouched
ECHAIN = -3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from compliancedex_amd import _native
    _native.load()


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)


def _filled(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


# ------------------------------------------------------------------ the three primitives through the C ABI
def device_fk(desc, q, B):
    """→ (rc, pos [B, 3T], quat [B, 4T]); outputs preset to a sentinel, GUARD rows past the last found untouched."""
    from compliancedex_amd import _native as N
    T = desc.n_tips
    qd = _dev(q[:B], np.float32)
    pos, quat = _filled((B + GUARD, 3 * T), -7.0), _filled((B + GUARD, 4 * T), -9.0)
    rc = N.load().cdx_fk_forward(desc, N.ptr(qd), B, N.ptr(pos), N.ptr(quat), N.stream_ptr())
    pos, quat = pos.cpu().numpy(), quat.cpu().numpy()
    assert (pos[B:] == -7.0).all() and (quat[B:] == -9.0).all()
    return rc, pos[:B], quat[:B]


def device_bwd(desc, q, gpos, B):
    from compliancedex_amd import _native as N
    qd, gd = _dev(q[:B], np.float32), _dev(gpos[:B], np.float32)
    gq = _filled((B + GUARD, desc.n_dofs), -7.0)
    rc = N.load().cdx_fk_backward(desc, N.ptr(qd), B, N.ptr(gd), N.ptr(gq), N.stream_ptr())
    gq = gq.cpu().numpy()
    assert (gq[B:] == -7.0).all()
    return rc, gq[:B]


def device_jac(desc, q, B, ang=True):
    from compliancedex_amd import _native as N
    T, D = desc.n_tips, desc.n_dofs
    qd = _dev(q[:B], np.float32)
    lin = _filled((B + GUARD, T, 3, D), -7.0)
    a = _filled((B + GUARD, T, 3, D), -9.0)
    rc = N.load().cdx_fk_jacobian(desc, N.ptr(qd), B, N.ptr(lin), N.ptr(a) if ang else None, N.stream_ptr())
    lin, a = lin.cpu().numpy(), a.cpu().numpy()
    assert (lin[B:] == -7.0).all() and (a[B:] == -9.0).all() and (ang or (a == -9.0).all())
    return rc, lin[:B], a[:B] if ang else None


def _ok(out):
    assert out[0] == 0, out[0]
    return out[1] if len(out) == 2 else out[1:]


@pytest.mark.parametrize("offsets", [True, False])
@pytest.mark.parametrize("case", ch.CASES)
def test_primitives_vs_statement(case, offsets):
    """cdx_fk_forward, cdx_fk_backward and cdx_fk_jacobian at B = 1, 63, 65, 257 against the float64 statement, at
    4 × the oracle's own error (tests/_chains.py) and the project's 2e-5 for the Jacobian."""
    ch.check_primitives(case, offsets, lambda d, q, B: _ok(device_fk(d, q, B)),
                        lambda d, q, g, B: _ok(device_bwd(d, q, g, B)),
                        lambda d, q, B, ang: _ok(device_jac(d, q, B, ang)))


# ------------------------------------------------------------------ IK
@pytest.mark.parametrize("case", ["tree8", "line16"])
def test_ik_at_the_largest_launch_shape(case):
    """test_single_iteration_vs_host's assertions, and the same comparison after a full solve, with E one below and one
    above the workgroup's row count and at 67.  tree8 (T = 8, D = 31) needs 6 448 B a row: 4 rows a workgroup."""
    from compliancedex_amd import _native as N
    from tests.test_gpu_ik import solve
    desc = ch.descriptor(case)
    T, D = desc.n_tips, desc.n_dofs
    L = N.load().cdx_ik_rows_per_block(T, D)
    assert L == ch.ik_rows_per_block(T, D)
    if case == "tree8":
        assert ch.ik_mem_bytes(T, D) == 6448 and L == 4
    c = ch.ik_rows(case)
    assert (c["full"]["status"] == 0).all()  # (the host build converges on every row)
    for E in (L - 1, L + 1, 67):
        for name, iters in (("one", 1), ("full", _ik.MAX_ITERS)):
            dev = solve(desc, c["params"](iters), c["q0"][:E], c["target"][:E])
            ref = {k: v[:E] for k, v in c[name].items()}
            print(case, E, name, f"{rel_err(dev['q'], ref['q']):.2e}", "iters", np.bincount(dev["iters"]))
            assert rel_err(dev["q"], ref["q"]) < 2e-5
            assert same_bits(dev["iters"], ref["iters"]) and same_bits(dev["status"], ref["status"])
            if name == "one":
                assert (dev["iters"] == 1).all()


# ------------------------------------------------------------------ closure (bwd3 in closure_combine_kernel)
@pytest.mark.parametrize("case", ["hand8", "hand16"])
def test_closure_vs_oracle(case, tmp_path):
    """test_closure_single_candidate_vs_oracle at E = 5 on a chain loaded from a JSON path: the stored banana state,
    replayed Kabsch noise, OracleProblem + closure_with_grads at that test's 1e-4."""
    from compliancedex_amd import ProbabilisticGraspOptimizer
    from compliancedex_amd.workloads import stored_gpis
    _, links = ch.bodies(case)
    q, comp, target, palm, noise = ch.closure_inputs(case)
    E = len(q)
    opt = ProbabilisticGraspOptimizer(ch.write_json(case, tmp_path), links, ch.tip_offsets(case), palm_offset=palm,
                                      ref_q=[0.0] * q.shape[1], optimize_target=True, optimize_palm=True, device=DEV)
    t = [_dev(a).requires_grad_(True) for a in (q, comp, target, palm[:, :3], palm[:, 3:])]
    opt.closure(*t, 1, stored_gpis("banana", DEV), E, kabsch_noise=_dev(noise))
    ref = ch.oracle_closure(case, q, comp, target, palm, noise)
    assert rel_err(opt.total_loss.cpu(), ref["total_loss"]) < 1e-4
    for k, x in zip(("grad_q", "grad_comp", "grad_target", "grad_palm_pos", "grad_palm_ori"), t):
        assert rel_err(x.grad.cpu(), ref[k]) < 1e-4, (k, rel_err(x.grad.cpu(), ref[k]))
    assert np.array_equal(opt.kabsch_flip.cpu().numpy().astype(bool), ref["flip"])


# ------------------------------------------------------------------ KinGPIS (bwd2 in the deep gpis_mode kernel)
@pytest.mark.parametrize("E", [6, 67])
@pytest.mark.parametrize("case", ["hand9", "hand16"])
def test_kingpis_fused_equals_eager(case, E, tmp_path):
    """test_deep_chain_fused_equals_eager's comparison on the synthetic deep hands."""
    from compliancedex_amd import KinGPISGraspOptimizer
    from compliancedex_amd.optimizer import FINGERTIP_LB, FINGERTIP_UB
    from tests.test_gpu_gpis_mode import TOL, _banana, _noise
    links, offs, palm, q, target, comp = ch.hand_kin_inputs(case, E, q_scale=0.05)
    path = ch.write_json(case, tmp_path)
    res = []
    for fused in (True, False):
        o = KinGPISGraspOptimizer(path, links, offs, palm_offset=palm.astype(np.float64).tolist(), num_iters=4,
                                  optimize_target=True, ref_q=[0.0] * q.shape[1],
                                  tip_bounding_box=[FINGERTIP_LB, FINGERTIP_UB])
        args = [_dev(a).double() for a in (q, target, comp)]
        out = o.optimize(*args, 1, _banana(), verbose=False, kabsch_noise=_noise(E, 4), trace_rows=True, fused=fused)
        res.append((torch.stack(o.loss_rows).cpu().numpy(), [x.detach().cpu().numpy() for x in out[:3]]))
    (ra, oa), (rb, ob) = res
    print(case, E, f"{rel_err(ra, rb):.2e}", [f"{rel_err(x, y):.2e}" for x, y in zip(oa, ob)])
    assert np.isfinite(rb).all() and rel_err(ra, rb) < TOL["kingpis"], rel_err(ra, rb)
    for x, y in zip(oa, ob):
        assert rel_err(x, y) < TOL["kingpis"]


# ------------------------------------------------------------------ collision (bwd in collision_kernel)
@pytest.mark.parametrize("E", [1, 65])
def test_collision_vs_oracle(E):
    """cdx_collision_loss on tree8's eight tips as anchors against oracle.collision_loss and its autograd, at
    test_collision_vs_reference's 1e-4; outputs preset, rows past E untouched."""
    from compliancedex_amd import _native as N
    r = ch.collision_rows()
    q, palm = _dev(r["q"][:E]), r["palm"][:E]
    pp, po = _dev(palm[:, :3]), _dev(palm[:, 3:])
    D = q.shape[1]
    f64 = torch.float64
    cost, g_q = _filled((E + GUARD,), -7.0, f64), _filled((E + GUARD, D), -7.0, f64)
    g_pp, g_po = _filled((E + GUARD, 3), -7.0, f64), _filled((E + GUARD, 3), -7.0, f64)
    N.check(N.load().cdx_collision_loss(ch.collision_descriptor(), E, N.ptr(q), N.ptr(pp), N.ptr(po), N.ptr(cost),
                                        N.ptr(g_q), N.ptr(g_pp), N.ptr(g_po), 0, N.stream_ptr()), "cdx_collision_loss")
    cost, g_q, g_pp, g_po = (x.cpu().numpy() for x in (cost, g_q, g_pp, g_po))
    for x in (cost, g_q, g_pp, g_po):
        assert (x[E:] == -7.0).all()
    assert np.array_equal(cost[:E] != 0, r["cost"][:E] != 0)
    assert rel_err(cost[:E], r["cost"][:E]) < 1e-4
    assert rel_err(g_q[:E], r["grad_q"][:E]) < 1e-4
    assert rel_err(np.concatenate([g_pp[:E], g_po[:E]], 1), r["grad_palm"][:E]) < 1e-4


# ------------------------------------------------------------------ the Kin loop (bwd3 through the FK-walk cache)
KIN_E = 67


def _kin_run(case, path, iters=4, fused=True, noise=None, q_scale=0.3, seed=5, **loop_path):
    from compliancedex_amd import KinGraspOptimizer
    from compliancedex_amd.workloads import banana_mesh
    links, offs, palm, q, target, comp = ch.hand_kin_inputs(case, KIN_E, q_scale=q_scale)
    kin = KinGraspOptimizer(path, links, offs, palm_offset=palm.tolist(), num_iters=iters, optimize_target=True,
                            ref_q=[0.0] * q.shape[1], seed=seed)
    res = kin.optimize(*[_dev(a) for a in (q, target, comp)], 1.0, banana_mesh(), verbose=False, trace_rows=True,
                       kabsch_noise=noise, fused=fused, **loop_path)
    torch.cuda.synchronize()
    return kin, res


def _bits_equal(a, b):
    from tests.test_gpu_parity import _bitwise_equal_nan_aware
    if a.dtype == np.float64:
        return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint64)[~np.isnan(a)],
                                                                             b.view(np.uint64)[~np.isnan(b)])
    return _bitwise_equal_nan_aware(a, b)


@pytest.mark.parametrize("case", ["hand9", "hand16"])
def test_kin_loop_forms_agree(case, tmp_path):
    """test_kin_one_launch_iteration_equals_two_launches and _kin_fk_walk_cache ("alt", "nocache") on the synthetic deep
    hands, E = 67 (a partial last workgroup), 4 iterations: the cached one-launch loop, the loop whose cache is always
    one step stale, the one-launch loop without the cache and the two-launch loop give the same bits."""
    path = ch.write_json(case, tmp_path)
    outs = {}
    for name, loop_path in (("cached", dict(split_step=False, fk_cache=True)),
                            ("alt", dict(split_step="alt", fk_cache=True)),
                            ("nocache", dict(split_step=False, fk_cache=False)),
                            ("two", dict(split_step=True, fk_cache=True))):
        kin, res = _kin_run(case, path, **loop_path)
        outs[name] = ([t.cpu().numpy() for t in res[:3]] + [bool(res[3])] + [kin.best_loss.cpu().numpy()] +
                      [r.cpu().numpy() for r in kin.loss_rows] + [kin.last_tips.cpu().numpy()])
    assert np.isfinite(outs["two"][5]).sum() > KIN_E // 2  # the rows are live
    for other in ("alt", "nocache", "two"):
        assert len(outs[other]) == len(outs["cached"])
        for i, (a, b) in enumerate(zip(outs["cached"], outs[other])):
            assert (a == b) if isinstance(a, bool) else _bits_equal(a, b), (other, i)


@pytest.mark.parametrize("case", ["hand9", "hand16"])
def test_kin_fused_equals_autograd(case, tmp_path):
    """test_kin_optimiser_fused_equals_autograd_at_size's comparison (1e-4 of the largest loss per iteration, the same
    non-finite candidates, final parameters at 1e-4) on the synthetic deep hands with replayed Kabsch noise."""
    path = ch.write_json(case, tmp_path)
    g = torch.Generator(device=DEV).manual_seed(5)
    noise = [torch.rand(KIN_E, 3, 3, generator=g, device=DEV, dtype=torch.float64) for _ in range(4)]
    res = {}
    for fused in (True, False):
        o, out = _kin_run(case, path, fused=fused, noise=noise, q_scale=0.1)
        res[fused] = ([r.double().cpu().numpy() for r in o.loss_rows], [x.detach().double().cpu().numpy() for x in out[:3]])
    (ra, oa), (rb, ob) = res[True], res[False]
    for s, (a, b) in enumerate(zip(ra, rb)):
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), s
        print(case, s, f"{np.abs(a[fin] - b[fin]).max() / np.abs(b[fin]).max():.2e}")
        assert np.abs(a[fin] - b[fin]).max() <= 1e-4 * np.abs(b[fin]).max(), (s, np.abs(a[fin] - b[fin]).max())
    assert np.isfinite(rb[-1]).sum() > KIN_E // 2
    for x, y in zip(oa, ob):
        assert rel_err(x, y) < 1e-4


# ------------------------------------------------------------------ the FK-walk cache must be seen to hit
@pytest.mark.parametrize("robot", ["iiwa7_allegro", "hand16"])
def test_fk_walk_cache_hits(robot, tmp_path):
    """After a cached one-launch Kin loop (E = 67, 3 iterations) every lane's tag is the iteration count and every
    q-check slot holds the bits of the final joint row: the next iteration's check would pass.  (A tag or a slot that
    never matches passes every equality test of the cache — walking gives the same bits — and only loses the speed.)"""
    from compliancedex_amd import KinGraspOptimizer
    from compliancedex_amd.optimizers import kin_fk_cache_qcheck, kin_fk_cache_view
    from compliancedex_amd.workloads import banana_mesh, config4_kin_inputs
    E, iters = KIN_E, 3
    if robot == "iiwa7_allegro":
        links, offs, palm, q, target, comp = config4_kin_inputs(E, device=DEV, q_scale=0.05)
        path, depth = robot, 13
    else:
        links, offs, palm, q, target, comp = ch.hand_kin_inputs(robot, E, q_scale=0.05)
        path, depth = ch.write_json(robot, tmp_path), max(ch.depths(robot))
    kin = KinGraspOptimizer(path, links, offs, palm_offset=palm.tolist(), num_iters=iters, optimize_target=True,
                            ref_q=[0.0] * q.shape[1])
    kin.optimize(*[_dev(a) for a in (q, target, comp)], 1, banana_mesh(), verbose=False, trace_rows=True)
    torch.cuda.synchronize()
    st = kin.last_loop
    view = kin_fk_cache_view(st.fk_state, depth)
    assert len(view["tag"]) == (4 * E + 63) // 64 * 64
    assert (view["tag"][:4 * E] == iters).all(), np.unique(view["tag"][:4 * E])
    want = kin_fk_cache_qcheck(st.pose.view(E, -1))
    assert np.isfinite(want.view(np.float32)).all() and (want != 0).any()
    assert np.array_equal(view["qcheck"][:4 * E], want)
    assert same_bits(st.pose.view(E, -1).cpu().numpy(), kin.last_params[0].cpu().numpy())  # … the final joint rows


# ------------------------------------------------------------------ the depth limit
def _deep(depth, n_tips=1, offsets=False):
    offs = [[0.01, -0.02, 0.03]] * n_tips if offsets else None
    return ch.raw_descriptor(ch.line(depth), [f"b{depth}"] * n_tips, offs)


def test_depth_16_is_accepted_and_correct():
    for offsets in (False, True):
        desc = _deep(16, 1, offsets)
        q = np.full((3, 16), 0.1, np.float32)
        gpos = np.ones((3, 1, 3), np.float32)
        ref = ch.statement(desc, q, gpos)
        pos, quat = _ok(device_fk(desc, q, 3))
        assert ch.rel(pos.reshape(3, 1, 3), ref["pos"]) < ch.TOL["pos"]
        assert ch.rel(quat.reshape(3, 1, 4), ref["quat"]) < ch.TOL["quat"]
        g = _ok(device_bwd(desc, q, gpos, 3))
        assert ch.rel(g, ref["grad"]) < ch.TOL["grad"] and (g[:, :15] != 0).all()
        lin, _ = _ok(device_jac(desc, q, 3))
        assert rel_err(lin, _ik.np_fk_jac(desc, q)[1]) < ch.TOL_JAC


@pytest.mark.parametrize("depth", [17, 19])
def test_over_deep_chain_is_refused_and_nothing_written(depth):
    """CDX_ECHAIN with device outputs in place and their sentinel untouched: the FK entries, IK and the collision loss.
    (The closure, Kin and GPIS-mode entries refuse the same chains before they look at any pointer:
    tests/test_chains_cpu.py calls them without a device.)"""
    from compliancedex_amd import _native as N
    from compliancedex_amd.ik import ik_params
    from compliancedex_amd.problem import build_collision
    lib = N.load()
    desc = _deep(depth)
    q = np.full((2, depth), 0.1, np.float32)
    rc, pos, quat = device_fk(desc, q, 2)
    assert rc == ECHAIN and (pos == -7.0).all() and (quat == -9.0).all()
    rc, g = device_bwd(desc, q, np.ones((2, 1, 3), np.float32), 2)
    assert rc == ECHAIN and (g == -7.0).all()
    rc, lin, ang = device_jac(desc, q, 2)
    assert rc == ECHAIN and (lin == -7.0).all() and (ang == -9.0).all()
    par = ik_params([-3.0] * depth, [3.0] * depth, [0.0] * depth, 0.0, 5, 1e-5)
    f64 = torch.float64
    q0, target = _filled((2, depth), 0.1, f64), _filled((2, 1, 3), 0.5, f64)
    outs = [_filled((2, depth), -7.0, f64), _filled((2, 1), -7.0, f64), _filled((2,), -7, torch.int32),
            _filled((2,), -7, torch.int32)]
    rc = lib.cdx_ik_solve(desc, C.byref(par), 2, N.ptr(q0), N.DTYPE_F64, N.ptr(target), None, None, None, None,
                          *[N.ptr(x) for x in outs], N.stream_ptr())
    assert rc == ECHAIN and all(bool((x == -7).all()) for x in outs)
    col = build_collision(_deep(depth, 4, True), [[0, 1]])
    ins = [_filled((2, depth), 0.1, f64), _filled((2, 3), 0.1, f64), _filled((2, 3), 0.1, f64)]
    outs = [_filled(s, -7.0, f64) for s in ((2,), (2, depth), (2, 3), (2, 3))]
    rc = lib.cdx_collision_loss(col, 2, *[N.ptr(x) for x in ins], *[N.ptr(x) for x in outs], 0, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == ECHAIN and all(bool((x == -7.0).all()) for x in outs)
