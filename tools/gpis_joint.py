"""The GPIS joint posterior of value and gradient (cdx_gpis_joint through ``gpis_joint_cov``) timed on the GPU:
M = 4·4096, 4·16 384 and 4·65 536 queries — four fingertips of that many candidates — on the stored banana state
(N = 361) and on the N = 2000 synthetic banana, the queries 1 cm around the inducing points.

Per state and size: the kernel (one MFMA launch and one finalize launch); ``cdx_gpis_std`` without its gradient at the
same state and queries — the new pass does four times its MFMA work —; a float64 torch statement on the device, the
columns [k, ∇k] built with torch operators and whitened by ``Linv @ B``, 16 384 queries at a time; and, at the smallest
size of a state of at most --host-n inducing points, the host build of the rule on one core (cdxh_gpis_joint, wall
clock).  Besides the times the record keeps how far the torch statement's Σ is from the kernel's, in the scaled error
of tests/_joint.py, and the medians of the angular and offset standard deviations there.

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.

Without --child the tool is the driver: every (state, size) runs in a child process of its own under ``timeout``, one
after the other, and the first that fails, faults or runs out of time ends the run.  One JSON line per case is printed
and appended to the record (default profiles/gpis_joint.jsonl).  Needs a GPU: there is no fallback.

  python tools/gpis_joint.py [--reps 7] [--rows 16384,65536,262144] [--states banana,banana2000] [--out PATH]
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

CHUNK = 16384


def torch_joint(Linv, X1, X, R, prior):
    """Σ [M, 10] of a TPS state with torch operators: B = [k, ∇k], W = Linv @ B, P0 − WᵀW."""
    import torch
    N = X1.shape[0]
    iu = torch.triu_indices(4, 4, device=X.device)
    out = []
    for c0 in range(0, X.shape[0], CHUNK):
        d = X[c0:c0 + CHUNK, None, :] - X1[None]
        r2 = (d * d).sum(-1)
        r = r2.sqrt()
        B = torch.cat([(2.0 * r2 * r - 3.0 * R * r2 + R ** 3).unsqueeze(-1), (6.0 * r - 6.0 * R).unsqueeze(-1) * d], -1)
        m = B.shape[0]
        W = (Linv @ B.permute(1, 0, 2).reshape(N, m * 4)).view(N, m, 4)
        S = torch.diag(prior) - torch.einsum("nma,nmb->mab", W, W)
        out.append(S[:, iu[0], iu[1]])
    return torch.cat(out)


def host_ms(st, X1, Linv_t, X, R, sigma):
    import ctypes as C
    import numpy as np
    from compliancedex_amd import _host
    from compliancedex_amd._native import CdxGpis
    lib, p = _host.load(), _host.ptr
    g = CdxGpis(X1=X1.ctypes.data, Linv_t=Linv_t.ctypes.data, N=len(X1), N_pad=Linv_t.shape[0], kernel=0, R=R, sigma=sigma)
    cov = np.empty((len(X), 10))
    t0 = time.perf_counter()
    rc = lib.cdxh_gpis_joint(C.byref(g), p(X), len(X), p(cov))
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0
    return ms, cov


def run_case(name, M, args):
    import numpy as np
    import torch
    from compliancedex_amd import gpis_joint_cov
    from compliancedex_amd.gpis import gpis_std, joint_cov_matrix, joint_prior, normal_covariance, gpis_mean
    from compliancedex_amd.workloads import stored_gpis, synthetic_banana_gpis
    g = stored_gpis("banana") if name == "banana" else synthetic_banana_gpis(2000)
    st = g.native_state()
    N = st.desc.N
    R = float(g.R)
    X1 = g.X1.double()
    rng = np.random.default_rng(0)
    X = X1[torch.from_numpy(rng.integers(0, N, M)).cuda()] + 0.01 * torch.from_numpy(rng.standard_normal((M, 3))).cuda()
    X = X.contiguous()
    prior = torch.tensor(joint_prior("tps", R, g.sigma), dtype=torch.float64, device="cuda")
    Linv = st.Linv[:N, :N].contiguous()
    paths = {"kernel": lambda: gpis_joint_cov(st, X), "std": lambda: gpis_std(st, X, want_grad=False)[0],
             "torch": lambda: torch_joint(Linv, X1, X, R, prior)}
    for fn in paths.values():  # warm-up: code objects, allocator blocks, workspaces
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(args.reps):
        for n, fn in paths.items():
            ms[n].append(event_ms(fn)[0])
    cov, ref = paths["kernel"](), paths["torch"]()
    iu = torch.triu_indices(4, 4, device="cuda")
    scale = (prior[iu[0]] * prior[iu[1]]).sqrt()
    unc = normal_covariance(gpis_mean(st, X, want_grad=True)[1], joint_cov_matrix(cov))
    eig = torch.linalg.eigvalsh(joint_cov_matrix(cov))[:, 0]
    med = float(np.median(ms["kernel"]))
    rec = {"state": name, "N": N, "M": M, **{n: stats(v) for n, v in ms.items()},
           "kernel_over_std": round(med / float(np.median(ms["std"])), 2),
           "torch_over_kernel": round(float(np.median(ms["torch"])) / med, 1),
           "mfma_tflops": round(4.0 * M * N * (N + 1) / (med * 1e-3) / 1e12, 2),  # 2 flops × 4 columns × N(N+1)/2
           "torch_scaled_diff": float(((cov - ref).abs() / scale).max()),
           "min_eig_over_k0": float(eig.min() / prior[0]), "indefinite": int((eig <= 0).sum()),
           "angle_std_median_rad": float(unc.angle_std.median()), "offset_std_median_m": float(unc.offset_std.median())}
    if N <= args.host_n and M == min(args.rows_list):
        hm, hc = host_ms(st, X1.cpu().numpy(), st.Linv_t.cpu().numpy(), X.cpu().numpy(), R, float(g.sigma))
        rec["host_one_core_ms"] = round(hm, 1)
        rec["host_over_kernel"] = round(hm / med, 1)
        rec["host_scaled_diff"] = float(((cov.cpu() - torch.from_numpy(hc)).abs() / scale.cpu()).max())
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="16384,65536,262144")
    ap.add_argument("--states", default="banana,banana2000")
    ap.add_argument("--child", action="store_true", help="one case (--states, first of --rows … --case-rows) in this process")
    ap.add_argument("--case-rows", type=int, default=0)
    ap.add_argument("--host-n", type=int, default=512, help="largest N the one-core host build is timed at")
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of each case's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gpis_joint.jsonl"))
    args = ap.parse_args()
    args.rows_list = [int(v) for v in args.rows.split(",")]
    if not args.child:
        for name in args.states.split(","):
            for M in args.rows_list:
                cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__),
                       "--child", "--states", name, "--rows", args.rows, "--case-rows", str(M), "--reps", str(args.reps),
                       "--host-n", str(args.host_n), "--out", args.out]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    raise SystemExit(f"{name} M={M} ended with status {rc}: nothing more is started")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpis_joint.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = run_case(args.states, args.case_rows or args.rows_list[0], args)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
