"""The trajectory optimiser timed on the GPU, one iteration split into its four launches, and the step gain measured.

  launches  T = 32, G·seeds·T = 4096, 16 384 and 65 536 waypoint rows, on two set-ups: ``allegro`` (the recorded 87
            spheres of tests/golden/spheres_allegro.json, the packaged banana GPIS: the cdx_gpis_mean launch) and
            ``iiwa7`` (iiwa7_allegro with HandSpheres.along_links at radius 0.03, the packaged banana mesh through
            PreparedMesh.query).  Timed separately: cdx_hand_spheres, the object's distance, cdx_hand_term, cdx_traj_step;
            next to cdx_traj_step the same rule in torch operators on the device (a Cholesky solve with the factor of A_T
            computed once) and cdxh_traj_step of the host build on one core (host clock).  ``step_share`` is
            cdx_traj_step's share of the four launches' sum.
  gain      iterations until the scenario of tests/_traj.py (iiwa7_allegro, 29 spheres, T = 24, a sphere of radius 0.06
            on the straight line) is clear at refine = 4, per gain; ``None``: not within --iters.  A count, not a time.

Device times are HIP events around one call after a warm-up call of every path; the median of --reps and the spread
(max − min)/median are kept.  Without --shape the tool is the driver: every shape runs in a child process of its own
under ``timeout``, one after the other, and the first that fails, faults or runs out of time ends the run.  One JSON
line per shape is printed and appended to the record (default profiles/traj.jsonl).  Needs a GPU: there is no fallback.

  python tools/traj.py [--reps 7] [--rows 4096,16384,65536] [--gains 0.25,0.5,1,2,4,8] [--iters 150] [--out PATH]
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
from tools.hand_collision import KW, model, the_object  # noqa: E402

T = 32


def setup(kind, dev):
    """(robot name, sphere model, object, palm pose [6], floor_z) of a set-up."""
    import numpy as np
    from compliancedex_amd.hand import HandSpheres
    if kind == "allegro":
        hs = model(None, dev)
        obj, center = the_object("gpis", dev)
        return "allegro", hs, obj, np.concatenate([center + [0.0, 0.0, 0.08], [np.pi, 0.0, 0.0]]), float(center[2]) - 0.05
    hs = HandSpheres.along_links("iiwa7_allegro", 0.03, device=dev)
    obj, center = the_object("mesh", dev)
    return "iiwa7_allegro", hs, obj, np.concatenate([center - [0.5, 0.0, 0.3], np.zeros(3)]), float(center[2]) - 0.05


def torch_step(A_chol, lower, upper, w, q, g_c, cost_t, best_cost, best_iter, best_traj, it):
    """cdx_traj.h's rule with torch operators: several launches and temporaries."""
    import torch
    ws, wc, wl, m, step = w
    p = torch.cat([q[:, :1], q, q[:, -1:]], 1)
    a = (p[:, :-2] - 2.0 * p[:, 1:-1]) + p[:, 2:]
    xi = q[:, 1:-1]
    h = torch.clamp(xi - (upper - m), min=0.0) - torch.clamp((lower + m) - xi, min=0.0)
    U = (ws * 0.5 * (a * a).sum((1, 2)) + wc * cost_t.sum(1)) + wl * 0.5 * (h * h).sum((1, 2))
    g = (ws * ((a[:, :-2] - 2.0 * a[:, 1:-1]) + a[:, 2:]) + wc * g_c[:, 1:-1]) + wl * h
    E, n, D = g.shape
    x = torch.cholesky_solve(g.permute(1, 0, 2).reshape(n, E * D), A_chol).reshape(n, E, D).permute(1, 0, 2)
    win = U < best_cost
    best_cost.copy_(torch.where(win, U, best_cost))
    best_iter.copy_(torch.where(win, torch.full_like(best_iter, it), best_iter))
    best_traj.copy_(torch.where(win[:, None, None], q, best_traj))
    q[:, 1:-1] -= step * x


def run_launches(kind, rows, args):
    import ctypes as C
    import numpy as np
    import torch
    from compliancedex_amd import DifferentiableRobotModel, TrajectoryOptimizer, _host, _native as N, seed_trajectories
    from compliancedex_amd.hand import object_distance
    from compliancedex_amd.trajectory import smoothness_matrix
    dev = torch.device("cuda")
    robot, hs, obj, palm6, floor_z = setup(kind, dev)
    E = rows // T
    opt = TrajectoryOptimizer(DifferentiableRobotModel(robot, device=dev), hs, T=T, **KW)
    D, S = opt.D, hs.n_spheres
    lo = np.where(np.isfinite(opt.lower), np.array(opt.lower) + 0.04, -1.0)
    hi = np.where(np.isfinite(opt.upper), np.array(opt.upper) - 0.04, 1.0)
    rng = np.random.default_rng(0)
    G = max(1, E // 8)
    qs = np.clip(hs.rest_q[None] + 0.2 * rng.standard_normal((G, D)), lo, hi)
    qg = np.clip(hs.rest_q[None] + 0.4 * rng.standard_normal((G, D)), lo, hi)
    traj = seed_trajectories(torch.from_numpy(qs).to(dev), torch.from_numpy(qg).to(dev), T, E // G, amp=0.3, seed=1)
    E = traj.shape[0]
    b = opt.buffers(E, dev)
    opt.optimize(traj, obj, torch.from_numpy(palm6).to(dev), floor_z, iters=3)  # fills every buffer, warms every launch
    palm = torch.from_numpy(palm6).to(dev).expand(E * T, 6)
    pp, po = palm[:, :3].contiguous(), palm[:, 3:].contiguous()
    hp = opt.hand_params
    lib, st = N.load(), N.stream_ptr(dev)
    chain, mdl, R = C.byref(hs.desc), C.byref(hs.native()), E * T
    q = b.traj.view(R, D)
    from compliancedex_amd.gpis import GPIS
    state = obj.native_state() if isinstance(obj, GPIS) else None
    keep = {}

    def spheres():
        N.check(lib.cdx_hand_spheres(chain, mdl, R, N.ptr(q), N.ptr(pp), N.ptr(po), N.ptr(b.poses), N.ptr(b.centers), st),
                "cdx_hand_spheres")

    def distance():
        if state is not None:
            N.check(lib.cdx_gpis_mean(state.desc, N.ptr(b.centers), R * S, N.ptr(b.dist), N.ptr(b.gdist), None, st),
                    "cdx_gpis_mean")
            keep["d"] = (b.dist, b.gdist)
        else:
            d, gd = object_distance(obj, b.centers)
            keep["d"] = (d.contiguous(), gd.contiguous())

    def term():
        d, gd = keep["d"]
        N.check(lib.cdx_hand_term(chain, mdl, C.byref(hp), R, N.ptr(b.poses), N.ptr(b.centers), N.ptr(d), N.ptr(gd),
                                  N.ptr(po), 1.0, 0, N.ptr(b.cost_t), N.ptr(b.g_c), None, None, None, None, st),
                "cdx_hand_term")

    start = traj.clone()

    def step():
        b.traj.copy_(start)  # (every repeat steps the same iterate; the copy is timed with it in all three paths)
        N.check(lib.cdx_traj_step(C.byref(opt.params), E, N.ptr(b.traj), N.ptr(b.g_c), N.ptr(b.cost_t), 0, N.ptr(b.cost),
                                  N.ptr(b.best_cost), N.ptr(b.best_iter), N.ptr(b.best_traj), st), "cdx_traj_step")

    A_chol = torch.linalg.cholesky(torch.from_numpy(smoothness_matrix(T)).to(dev))
    lower, upper = (torch.tensor(v, dtype=torch.float64, device=dev) for v in (opt.lower, opt.upper))
    w = (opt.params.w_smooth, opt.params.w_col, opt.params.w_lim, opt.params.m_lim, opt.params.step)
    tq, tbc, tbi, tbt = start.clone(), b.best_cost.clone(), b.best_iter.clone(), b.best_traj.clone()

    def torch_ops():
        tq.copy_(start)
        torch_step(A_chol, lower, upper, w, tq, b.g_c.view(E, T, D), b.cost_t.view(E, T), tbc, tbi, tbt, 0)

    paths = {"spheres": spheres, "distance": distance, "term": term, "step": step, "step_torch": torch_ops}
    for f in paths.values():
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(args.reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    # the host build on one core (host clock around the same rule on the same inputs)
    hl = _host.load()
    arr = {k: getattr(b, k).cpu().numpy().copy() for k in ("g_c", "cost_t", "cost", "best_cost", "best_iter", "best_traj")}
    h0 = start.cpu().numpy()
    host_ms = []
    for _ in range(3):
        ht = h0.copy()
        t0 = time.perf_counter()
        rc = hl.cdxh_traj_step(C.byref(opt.params), E, _host.ptr(ht), _host.ptr(arr["g_c"]), _host.ptr(arr["cost_t"]), 0,
                               _host.ptr(arr["cost"]), _host.ptr(arr["best_cost"]), _host.ptr(arr["best_iter"]),
                               _host.ptr(arr["best_traj"]))
        host_ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
    step()
    torch.cuda.synchronize()
    same = bool((b.traj.cpu().numpy() == ht).all())
    rec = {"shape": "launches", "setup": kind, "rows": R, "E": E, "T": T, "D": D, "S": S, "pairs": len(hs.pairs),
           **{n: stats(v) for n, v in ms.items()}, "step_host_1core": stats(host_ms), "device_equals_host_bits": same}
    four = sum(rec[n]["median_ms"] for n in ("spheres", "distance", "term", "step"))
    rec["iteration_ms"] = round(four, 4)
    rec["step_share"] = round(rec["step"]["median_ms"] / four, 4)
    rec["torch_over_step"] = round(rec["step_torch"]["median_ms"] / rec["step"]["median_ms"], 2)
    return rec


def run_gain(gain, args):
    import numpy as np
    import torch
    from compliancedex_amd import DifferentiableRobotModel, TrajectoryOptimizer, trajectory_report
    from tests import _traj as J
    dev = torch.device("cuda")
    sc, S = J.scene(), J.SCENE
    opt = TrajectoryOptimizer(DifferentiableRobotModel("iiwa7_allegro", device=dev), sc["hs"], T=S["T"],
                              w_smooth=S["w_smooth"], w_col=S["w_col"], w_lim=S["w_lim"], m_lim=S["m_lim"], gain=gain,
                              m_obj=S["m_obj"], w_obj=S["w_obj"])
    c = torch.tensor(sc["center"], device=dev)

    def obj(X):
        v = X - c
        n = v.norm(dim=-1)
        return n - S["obstacle"], v / n[:, None]
    q = torch.from_numpy(sc["line"]).to(dev)
    first, best = None, np.inf
    for it in range(args.iters):
        q = opt.optimize(q, obj, iters=1).last
        rep = trajectory_report(sc["hs"], q, obj, refine=4)
        ok = bool(rep["clear"][0]) and bool(rep["within_limits"][0]) and bool(torch.isfinite(q).all())
        if ok and first is None:
            first = it + 1
        if not bool(torch.isfinite(q).all()):
            break
        best = min(best, float(rep["depth"][0, 0]))
    rep = trajectory_report(sc["hs"], q, obj, refine=4)
    return {"shape": "gain", "gain": gain, "step": opt.step, "iters": args.iters, "iterations_to_clear": first,
            "clear_at_end": bool(rep["clear"][0]), "depth_at_end": float(rep["depth"][0, 0]), "least_depth": best,
            "smoothness_at_end": float(rep["smoothness"][0]), "finite": bool(torch.isfinite(q).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--setups", default="allegro,iiwa7")
    ap.add_argument("--gains", default="0.25,0.5,1,2,4,8")
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--shape", default=None, help="child mode: launches:<setup>:<rows> or gain:<gain>,<gain>,…")
    ap.add_argument("--step-seconds", type=int, default=150, help="time limit of each shape's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "traj.jsonl"))
    args = ap.parse_args()
    if args.shape is None:
        shapes = [f"launches:{k}:{int(r)}" for k in args.setups.split(",") if k for r in args.rows.split(",") if r]
        shapes += [f"gain:{args.gains}"] if args.gains else []
        for shape in shapes:
            cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--shape",
                   shape, "--reps", str(args.reps), "--iters", str(args.iters), "--out", args.out]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit(f"{shape} ended with status {rc}: nothing more is started")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/traj.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    parts = args.shape.split(":")
    recs = [run_launches(parts[1], int(parts[2]), args)] if parts[0] == "launches" else \
        [run_gain(float(g), args) for g in parts[1].split(",")]
    for rec in recs:
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
