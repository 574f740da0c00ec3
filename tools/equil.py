"""The disturbance-load test (cdx_grasp_equilibrium + cdx_equil_reduce through ``disturbance_report``) timed on the
GPU: E = 4096, 16 384 and 65 536 grasps of T = 4 contacts under W = 26 loads each — the weight of 0.4 kg in the 26
cube-lattice directions, acting at each grasp's stiffness centre.  The grasps are random contacts on a 10 × 6 × 6 cm
ellipsoid, pressed in 4 … 12 mm with 3 mm of noise, stiffness 80 … 400 N/m (the "shallow" family of tests/_equil.py).

Per size: the kernels (one solve launch and one reduction launch; ``disturbance_report`` allocates its outputs); a torch
statement of the same rule on the device — all E·W items advanced together with batched torch operators,
``torch.linalg.cholesky_ex`` for the 6 × 6 factorisations, a masked accept, and one host read per iteration to learn
whether any item still runs —; and the host build of the rule on one core (cdxh_grasp_equilibrium, wall clock) up to
--host-rows.  Besides the times the record keeps the iteration counts, the statuses, how far the torch statement's
poses are from the kernel's and the verdicts.

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.

Without --child the tool is the driver: every size runs in a child process of its own under ``timeout``, one after the
other, and the first that fails, faults or runs out of time ends the run.  One JSON line per size is printed and
appended to the record (default profiles/equil.jsonl).  Needs a GPU: there is no fallback.

  python tools/equil.py [--reps 7] [--rows 4096,16384,65536] [--out PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.fps import event_ms, stats  # noqa: E402

MU, MASS, W_DIRS, T = 1.0, 0.4, 26, 4


def grasps(E, seed=0):
    import numpy as np
    g = np.random.default_rng(seed)
    axes = np.array([0.05, 0.03, 0.03])
    u = g.normal(size=(E, T, 3))
    pts = u / np.linalg.norm(u, axis=-1, keepdims=True) * axes
    nh = pts / axes ** 2
    nh /= np.linalg.norm(nh, axis=-1, keepdims=True)
    tgt = pts - nh * g.uniform(0.004, 0.012, (E, T, 1)) + g.normal(scale=0.003, size=(E, T, 3))
    return pts, tgt, g.uniform(80.0, 400.0, (E, T)), nh


def torch_equil(pts, tgt, k, nrm, f, mu, tol=1e-8, max_iters=60, mu0=1e-3, mu_min=1e-9, mu_max=1e6, nu=10.0):
    """The rule of csrc/cdx_equil.h with torch operators (float64, finite inputs, loads [W, 3] at the stiffness centre)
    → (rot [N, 3, 3], t [N, 3], margin [N, T], iters [N], status [N]) over the N = E·W items."""
    import torch
    E, W = pts.shape[0], f.shape[0]
    rep = lambda x: x.repeat_interleave(W, 0)  # noqa: E731
    pts, tgt, k, nrm = rep(pts), rep(tgt), rep(k), rep(nrm)
    f = f.repeat(E, 1)
    M = pts.shape[0]
    K = k.sum(1)
    o = (k.unsqueeze(2) * pts).sum(1) / K.unsqueeze(1)
    P, G = pts - o.unsqueeze(1), tgt - o.unsqueeze(1)
    ell = P.norm(dim=2).amax(1)
    Fs = (k * (P - G).norm(dim=2)).sum(1) + f.norm(dim=1)
    eye3 = torch.eye(3, dtype=torch.float64, device=pts.device)
    eye6 = torch.eye(6, dtype=torch.float64, device=pts.device)

    def skew(s):
        z = torch.zeros_like(s[:, 0])
        return torch.stack([torch.stack([z, -s[:, 2], s[:, 1]], 1), torch.stack([s[:, 2], z, -s[:, 0]], 1),
                            torch.stack([-s[:, 1], s[:, 0], z], 1)], 1)

    def energy_change(R, t, D, dv):
        a = torch.einsum("mij,mtj->mti", R, P)
        d = torch.einsum("mij,mtj->mti", D, a) + dv.unsqueeze(1)
        return (k * (d * (a + t.unsqueeze(1) - G + 0.5 * d)).sum(2)).sum(1) - (f * dv).sum(1)

    R, t = eye3.repeat(M, 1, 1), torch.zeros(M, 3, dtype=torch.float64, device=pts.device)
    damp = torch.full_like(K, mu0)
    iters = torch.zeros(M, dtype=torch.int32, device=pts.device)
    status = torch.full_like(iters, -1)
    active = torch.ones(M, dtype=torch.bool, device=pts.device)
    scale = torch.cat([(1.0 / ell).unsqueeze(1).expand(M, 3), torch.ones_like(t)], 1)
    while True:
        a = torch.einsum("mij,mtj->mti", R, P)
        r = a + t.unsqueeze(1) - G
        gv = (k.unsqueeze(2) * r).sum(1) - f
        gw = (k.unsqueeze(2) * torch.cross(a, r, dim=2)).sum(1)  # (the load acts at the centre: b = 0)
        ar = torch.einsum("mti,mtj->mtij", a, r)
        ww = (((a * a).sum(2) - (a * r).sum(2))[..., None, None] * eye3 - torch.einsum("mti,mtj->mtij", a, a) +
              0.5 * (ar + ar.transpose(2, 3)))
        S = skew((k.unsqueeze(2) * a).sum(1))
        H = torch.zeros(M, 6, 6, dtype=torch.float64, device=pts.device)
        H[:, :3, :3], H[:, :3, 3:], H[:, 3:, :3] = (k[..., None, None] * ww).sum(1), S, -S
        H[:, 3:, 3:] = K[:, None, None] * eye3
        H = H * scale.unsqueeze(2) * scale.unsqueeze(1)
        conv = (gv.norm(dim=1) <= tol * Fs) & (gw.norm(dim=1) <= tol * Fs * ell)
        stop = active & (conv | (iters >= max_iters))
        status = torch.where(stop, torch.where(conv, 0, 1).to(torch.int32), status)
        active = active & ~stop
        if not bool(active.any()):
            break
        iters = iters + active.to(torch.int32)
        L, info = torch.linalg.cholesky_ex(H + (damp * K)[:, None, None] * eye6)
        h = -torch.cat([gw / ell.unsqueeze(1), gv], 1)
        d = torch.cholesky_solve(h.unsqueeze(2), torch.where((info == 0)[:, None, None], L, eye6)).squeeze(2)
        av = 0.5 * d[:, :3] / ell.unsqueeze(1)
        s = (av * av).sum(1)[:, None, None]
        aa = 2.0 * torch.einsum("mi,mj->mij", av, av) + 2.0 * skew(av)
        cay, D = ((1.0 - s) * eye3 + aa) / (1.0 + s), (aa - 2.0 * s * eye3) / (1.0 + s)
        acc = active & (info == 0) & (energy_change(R, t, D, d[:, 3:]) < 0)
        R, t = torch.where(acc[:, None, None], cay @ R, R), torch.where(acc[:, None], t + d[:, 3:], t)
        damp = torch.where(active, torch.where(acc, (damp / nu).clamp(min=mu_min), (damp * nu).clamp(max=mu_max)), damp)
    force = k.unsqueeze(2) * (G - (torch.einsum("mij,mtj->mti", R, P) + t.unsqueeze(1)))
    m = torch.einsum("mij,mtj->mti", R, nrm / nrm.norm(dim=2, keepdim=True))
    margin = -(force * m).sum(2) / force.norm(dim=2) - 1.0 / (1.0 + mu * mu) ** 0.5
    return R, t, margin, iters, status


def host_ms(pts, tgt, k, nrm, f):
    """cdxh_grasp_equilibrium on one core, wall clock."""
    import ctypes as C
    import numpy as np
    from compliancedex_amd import _host
    from compliancedex_amd.stability import equil_params
    lib, p = _host.load(), _host.ptr
    E, W = len(pts), len(f)
    n = E * W
    c = np.ascontiguousarray(np.repeat(((k[..., None] * pts).sum(1) / k.sum(1)[:, None])[:, None], W, 1))
    fe = np.ascontiguousarray(np.tile(f, (E, 1, 1)))
    out = [np.empty((n, T)), np.empty((n, T)), np.empty(n), np.empty(n), np.empty(n, np.uint8), np.empty(n, np.int32),
           np.empty(n, np.int32)]
    par = equil_params(T, MU)
    t0 = time.perf_counter()
    rc = lib.cdxh_grasp_equilibrium(C.byref(par), E, W, p(pts), p(tgt), p(k), p(nrm), p(fe), p(c), 0, None, None, None,
                                    *[p(x) for x in out])
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0
    return ms


def run_size(E, args):
    import numpy as np
    import torch
    from compliancedex_amd import disturbance_report, gravity_loads
    pts, tgt, k, nrm = grasps(E)
    f, _ = gravity_loads(MASS, directions=W_DIRS)
    d = [torch.from_numpy(x).cuda() for x in (pts, tgt, k, nrm)]
    fd = torch.from_numpy(f).cuda()
    paths = {"kernel": lambda: disturbance_report(*d, MU, fd), "torch": lambda: torch_equil(*d, fd, MU)}
    for fn in paths.values():  # warm-up: code objects, allocator blocks
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(args.reps):
        for n, fn in paths.items():
            ms[n].append(event_ms(fn)[0])
    rep = paths["kernel"]()
    R, t, margin, iters, status = paths["torch"]()
    res = rep.result
    it = res.iters.reshape(-1).cpu().numpy()
    both = ((res.status.reshape(-1) == 0) & (status == 0)).cpu().numpy()
    rec = {"E": E, "W": W_DIRS, "T": T, "items": E * W_DIRS, **{n: stats(v) for n, v in ms.items()},
           "torch_over_kernel": round(float(np.median(ms["torch"]) / np.median(ms["kernel"])), 1),
           "iters_median": float(np.median(it)), "iters_max": int(it.max()),
           "status_counts": np.bincount(res.status.reshape(-1).cpu().numpy(), minlength=3).tolist(),
           "torch_status_counts": np.bincount(status.cpu().numpy(), minlength=3).tolist(),
           "torch_iters_max": int(iters.max()),
           "torch_rot_diff": float((res.rot.reshape(-1, 3, 3) - R).abs().amax((1, 2)).cpu().numpy()[both].max()),
           "torch_margin_diff": float((res.margin.reshape(-1, T) - margin).abs().amax(1).cpu().numpy()[both].max()),
           "grasps_that_hold": int(rep.holds.sum()), "loads_that_fail": int(rep.n_failed.sum())}
    if E <= args.host_rows:
        rec["host_one_core_ms"] = round(host_ms(pts, tgt, k, nrm, f), 1)
        rec["host_over_kernel"] = round(rec["host_one_core_ms"] / rec["kernel"]["median_ms"], 1)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--child", action="store_true", help="one size (--rows) in this process")
    ap.add_argument("--host-rows", type=int, default=65536)
    ap.add_argument("--step-seconds", type=int, default=150, help="time limit of each size's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "equil.jsonl"))
    args = ap.parse_args()
    rows = [int(v) for v in args.rows.split(",")]
    if not args.child:
        for E in rows:
            cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--child",
                   "--rows", str(E), "--reps", str(args.reps), "--host-rows", str(args.host_rows), "--out", args.out]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit(f"E={E} ended with status {rc}: nothing more is started")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/equil.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = run_size(rows[0], args)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
