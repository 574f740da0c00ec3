"""The batched minimum-wrench solve (cdx_min_wrench) timed on the GPU: E = 4096, 16 384 and 65 536 candidates of four
contacts, on two input families — A: contacts on a 2–8 cm blob with outward normals tilted by 0.1 of noise (grasps that
close), D: the same contacts with random normals (adversarial: many rows need hundreds of iterations, a few thousands).

Per shape: the one-launch solve (the time of ``min_wrench``, which allocates its eight outputs); a torch statement of
the same iteration on the device — batched tensors for the ADMM updates, one batched ``torch.linalg.solve_ex`` for the
inverses of the 6 × 6 systems and a ``bmm`` with them per iteration, the certificate every ``check_every`` iterations
with one ``all()`` read back per check to end the loop —; and the host build of the rule on one core (cdxh_min_wrench, wall clock) up to --host-rows.  Besides the
times the record keeps the status counts and the iteration histogram of the kernel, the share of rows the torch
statement certified, and how far its forces are from the kernel's.

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.

Without --family the tool is the driver: every shape runs in a child process of its own under ``timeout``, one after
the other, and the first that fails, faults or runs out of time ends the run.  One JSON line per shape is printed and
appended to the record (default profiles/wrench.jsonl).  Needs a GPU: there is no fallback.

  python tools/wrench.py [--reps 7] [--rows 4096,16384,65536] [--families A,D] [--out PATH]
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

MU, FMIN, REG, RHO, TOL, MAX_ITERS, CHECK_EVERY = 1.0, 5.0, 1e-2, 0.05, 1e-9, 2000, 10
ITER_BINS = [0, 50, 100, 200, 300, 500, 1000, 2000]


def inputs(family, E, T=4, seed=0):
    """(tips, normals) [E, T, 3] as numpy arrays: the recipe of the test families A (noise 0.1) and D (random
    normals)."""
    import numpy as np
    g = np.random.default_rng(seed)
    p = g.normal(size=(E, T, 3))
    p /= np.linalg.norm(p, axis=-1, keepdims=True)
    p = p * g.uniform(0.02, 0.08, (E, T, 1)) + g.normal(scale=0.05, size=(E, 1, 3))
    if family == "D":
        n = g.normal(size=(E, T, 3))
    else:
        n = p - p.mean(axis=1, keepdims=True)
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        n = n + 0.1 * g.normal(size=(E, T, 3))
    return p, n / np.linalg.norm(n, axis=-1, keepdims=True)


def torch_min_wrench(tips, normals, mu=MU, fmin=FMIN, reg=REG, rho=RHO, tol=TOL, max_iters=MAX_ITERS,
                     check_every=CHECK_EVERY):
    """The rule of csrc/cdx_wrench.h with torch operators on the device → (forces, dual, gap, iters, certified)."""
    import torch
    E, T = tips.shape[:2]
    kappa = reg + rho

    def project(v):
        a = -(v * nh).sum(-1)
        t = -v - a.unsqueeze(-1) * nh
        tn = t.norm(dim=-1)
        safe = torch.where(tn > 0, tn, torch.ones_like(tn))
        inside = tn <= mu * a
        apex = ~inside & (mu * tn <= -a)
        ab = (mu * tn + a) / (1.0 + mu * mu)
        a2 = torch.where(inside, a, torch.where(apex, torch.zeros_like(a), ab))
        sc = torch.where(inside, torch.ones_like(a), torch.where(apex, torch.zeros_like(a), mu * ab / safe))
        low = ~(a2 >= fmin)
        a2 = torch.where(low, torch.full_like(a2, fmin), a2)
        sc = torch.where(low, torch.where(tn > mu * fmin, mu * fmin / safe, torch.ones_like(tn)), sc)
        return -(a2.unsqueeze(-1) * nh + sc.unsqueeze(-1) * t)

    def certificate(F, y):
        P = (0.5 * F.sum(1).norm(dim=-1) + 0.5 * torch.cross(r, F, dim=-1).sum(1).norm(dim=-1) +
             0.5 * reg * (F * F).sum((1, 2)))
        g = y[:, None, :3] + torch.cross(y[:, None, 3:].expand(E, T, 3), r, dim=-1)
        x = project(-g / reg)
        return P, (0.5 * reg * (x * x).sum(-1) + (g * x).sum(-1)).sum(1)

    def shrink(v, thr):
        vn = v.norm(dim=-1, keepdim=True)
        return torch.where(vn <= thr, torch.zeros_like(v), v * (1.0 - thr / torch.where(vn > 0, vn, torch.ones_like(vn))))

    def clip(v):
        vn = v.norm(dim=-1, keepdim=True)
        return torch.where(vn > 0.5, v * (0.5 / vn), v)

    nh = normals / normals.norm(dim=-1, keepdim=True)
    r = tips - tips.mean(dim=1, keepdim=True)
    l2 = (r * r).sum((1, 2)) / T
    ell = torch.where(l2 > 0, l2.sqrt(), torch.ones_like(l2)).view(E, 1)
    rs = r / ell.unsqueeze(2)
    zero = torch.zeros_like(rs[..., 0])
    skew = torch.stack([zero, -rs[..., 2], rs[..., 1], rs[..., 2], zero, -rs[..., 0], -rs[..., 1], rs[..., 0], zero],
                       dim=-1).view(E, T, 3, 3)
    A = torch.cat([torch.eye(3, dtype=tips.dtype, device=tips.device).expand(E, T, 3, 3), skew], dim=2)  # [E, T, 6, 3]
    S = (kappa / rho) * torch.eye(6, dtype=tips.dtype, device=tips.device) + (A @ A.transpose(2, 3)).sum(1)
    # S⁻¹ once, by LU with pivoting (solve_ex, as tools/ik.py: at E = 65 536 the batched Cholesky pair of this stack
    # certified no row at all, while it agrees with the kernel to 1e-13 on the smaller batches)
    Sinv = torch.linalg.solve_ex(S, torch.eye(6, dtype=tips.dtype, device=tips.device).expand(E, 6, 6))[0]
    z, u = -fmin * nh, torch.zeros_like(nh)
    zw, uw = torch.zeros(E, 6, dtype=tips.dtype, device=tips.device), torch.zeros(E, 6, dtype=tips.dtype, device=tips.device)
    y = torch.zeros_like(zw)
    best = torch.full((E,), float("inf"), dtype=tips.dtype, device=tips.device)
    bestP = torch.zeros_like(best)
    F, dual = z.clone(), y.clone()
    iters = torch.zeros(E, dtype=torch.int32, device=tips.device)
    done = torch.zeros(E, dtype=torch.bool, device=tips.device)
    it = 0
    while True:
        P, D = certificate(z, y)
        better = ~done & (P - D < best)
        best = torch.where(better, P - D, best)
        bestP = torch.where(better, P, bestP)
        F = torch.where(better.view(E, 1, 1), z, F)
        dual = torch.where(better.view(E, 1), y, dual)
        done = done | (best <= tol * bestP.abs().clamp(min=1.0))
        if it >= max_iters or bool(done.all()):
            break
        while True:
            it += 1
            iters += ~done
            df, dt = (zw - uw)[:, None, :3], ((zw - uw)[:, 3:] / ell)[:, None, :]
            b = rho * ((df + torch.cross(dt.expand(E, T, 3), r, dim=-1)) + (z - u))
            h = torch.cat([b.sum(1), torch.cross(r, b, dim=-1).sum(1) / ell], dim=1)
            w = torch.bmm(Sinv, h.unsqueeze(2)).squeeze(2)
            x = (b - (w[:, None, :3] + torch.cross((w[:, 3:] / ell)[:, None, :].expand(E, T, 3), r, dim=-1))) / kappa
            vf = x.sum(1) + uw[:, :3]
            vt = torch.cross(r, x, dim=-1).sum(1) / ell + uw[:, 3:]
            zf, zt = shrink(vf, 0.5 / rho), shrink(vt, 0.5 * ell / rho)
            zw, uw = torch.cat([zf, zt], 1), torch.cat([vf - zf, vt - zt], 1)
            v = x + u
            z = project(v)
            u = v - z
            if it >= max_iters or it % check_every == 0:
                break
        y = torch.cat([clip(rho * uw[:, :3]), clip(rho * uw[:, 3:] / ell)], 1)
    return F, dual, best, iters, done


def host_seconds(tips, normals):
    """Seconds of cdxh_min_wrench on one core, and its status / iteration arrays."""
    import numpy as np
    from compliancedex_amd import _host
    from compliancedex_amd.wrench import wrench_params
    lib, p = _host.load(), _host.ptr
    E, T = tips.shape[:2]
    par = wrench_params(T, MU, FMIN, REG, MAX_ITERS, TOL, RHO, CHECK_EVERY)
    out = [np.empty((E, T, 3)), np.empty(E), np.empty((E, T)), np.empty((E, 6)), np.empty(E), np.empty(E, np.int32),
           np.empty(E, np.int32), np.empty((E, T, 3))]
    t = time.perf_counter()
    rc = lib.cdxh_min_wrench(par, E, p(tips), p(normals), *[p(a) for a in out])
    dt = time.perf_counter() - t
    assert rc == 0
    return dt, out[6], out[5]


def run_shape(family, E, args):
    import numpy as np
    import torch
    from compliancedex_amd import _native as N, min_wrench
    tips_h, normals_h = inputs(family, E)
    tips, normals = torch.from_numpy(tips_h).cuda(), torch.from_numpy(normals_h).cuda()
    paths = {"kernel": lambda: min_wrench(tips, normals, MU, FMIN, REG, MAX_ITERS, TOL, RHO),
             "torch": lambda: torch_min_wrench(tips, normals)}
    for f in paths.values():  # warm-up: code objects, allocator blocks
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(args.reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    rec = {"family": family, "E": E, "T": 4, "rows_per_block": int(N.load().cdx_wrench_rows_per_block(4)),
           **{n: stats(v) for n, v in ms.items()}}
    res = paths["kernel"]()
    tF, _, _, titers, tdone = paths["torch"]()
    status, iters = res.status.cpu().numpy(), res.iters.cpu().numpy()
    rec["kernel_status_counts"] = [int((status == s).sum()) for s in (0, 1, 2)]
    rec["kernel_iters_median_max"] = [int(np.median(iters)), int(iters.max())]
    rec["kernel_iters_bins"] = ITER_BINS
    rec["kernel_iters_hist"] = np.histogram(iters, bins=ITER_BINS + [MAX_ITERS + 1])[0].tolist()
    # the launch ends with its slowest wave, a wave with its slowest row: the mean over waves of the per-wave maximum
    lanes = rec["rows_per_block"]
    pad = np.pad(iters, (0, -len(iters) % lanes))
    rec["kernel_iters_mean"] = round(float(iters.mean()), 1)
    rec["kernel_iters_mean_of_wave_max"] = round(float(pad.reshape(-1, lanes).max(1).mean()), 1)
    rec["torch_certified"] = round(float(tdone.double().mean()), 5)
    rec["torch_iters_median_max"] = [int(titers.median()), int(titers.max())]
    both = (res.status == 0) & tdone
    rec["torch_forces_max_dist"] = float((tF - res.forces)[both].reshape(-1, 12).norm(dim=1).max()) if bool(both.any()) else None
    rec["torch_over_kernel"] = round(rec["torch"]["median_ms"] / rec["kernel"]["median_ms"], 1)
    if E <= args.host_rows:
        sec, hstatus, hiters = host_seconds(tips_h, normals_h)
        rec["host_one_core_ms"] = round(sec * 1e3, 2)
        rec["host_status_counts"] = [int((hstatus == s).sum()) for s in (0, 1, 2)]
        rec["host_over_kernel"] = round(sec * 1e3 / rec["kernel"]["median_ms"], 1)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--families", default="A,D")
    ap.add_argument("--family", default=None, help="child mode: one shape in this process (with --rows one size)")
    ap.add_argument("--host-rows", type=int, default=65536)
    ap.add_argument("--step-seconds", type=int, default=150, help="time limit of each shape's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wrench.jsonl"))
    args = ap.parse_args()
    rows = [int(v) for v in args.rows.split(",")]
    if args.family is None:
        for family in args.families.split(","):
            for E in rows:
                cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--family",
                       family, "--rows", str(E), "--reps", str(args.reps), "--host-rows", str(args.host_rows), "--out",
                       args.out]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    raise SystemExit(f"family {family} E={E} ended with status {rc}: nothing more is started")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/wrench.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = run_shape(args.family, rows[0], args)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
