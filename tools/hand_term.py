"""The whole-hand collision term of the optimisers timed on the GPU (Allegro, the recorded 87 spheres of
tests/golden/spheres_allegro.json, the packaged banana GPIS).

  kernel  cdx_hand_term (one accumulating launch) against cdx_hand_cost followed by cdx_hand_pullback on the same
          poses, centres and distances, E = 4096, 16 384 and 65 536.
  loops   per-iteration time of the fused ProbabilisticGraspOptimizer and KinGPISGraspOptimizer loops with and without
          ``hand_term`` at E = 4096 on the stored banana state (KinGPIS also in its two-launch form without the term,
          which is the form the term uses): the whole optimize() call over --iters iterations, divided by --iters.

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.

Without --shape the tool is the driver: every shape runs in a child process of its own under ``timeout``, one after the
other, and the first that fails, faults or runs out of time ends the run.  One JSON line per shape is printed and
appended to the record (default profiles/hand_term.jsonl).  Needs a GPU: there is no fallback.

  python tools/hand_term.py [--reps 7] [--rows 4096,16384,65536] [--loop-rows 4096] [--iters 20] [--out PATH]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.fps import event_ms, stats  # noqa: E402
from tools.hand_collision import KW, inputs, model  # noqa: E402


def timed(paths, reps):
    import torch
    for f in paths.values():  # warm-up: code objects, allocator blocks
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    return ms


def run_kernel(E, args):
    import ctypes as C
    import torch
    from compliancedex_amd import HandTerm, _native as N
    from compliancedex_amd.hand import cost_launch, object_distance, pullback_launch, spheres_launch
    from compliancedex_amd.workloads import stored_gpis, surface_center
    dev = torch.device("cuda")
    hs = model(None, dev)
    obj = stored_gpis("banana", dev)
    center = surface_center(obj)
    term = HandTerm(hs, weight=0.37, floor_z=float(center[2]) - 0.05, **KW)
    par = term.params()
    qh, ph = inputs(hs, center, E)
    q, palm = torch.from_numpy(qh).to(dev), torch.from_numpy(ph).to(dev)
    pp, po = palm[:, :3].contiguous(), palm[:, 3:].contiguous()
    S = hs.n_spheres
    poses, centers = spheres_launch(hs, q, pp, po)
    dist, gdist = object_distance(obj, centers.reshape(-1, 3))
    dist, gdist = dist.reshape(E, S).contiguous(), gdist.reshape(E, S, 3).contiguous()
    f64 = dict(dtype=torch.float64, device=dev)
    loss, g_q, g_pp, g_po = torch.zeros(E, **f64), torch.zeros(E, hs.desc.n_dofs, **f64), torch.zeros(E, 3, **f64), \
        torch.zeros(E, 3, **f64)
    depth, worst = torch.empty(E, 3, **f64), torch.empty(E, 3, dtype=torch.int32, device=dev)
    lib, stream = N.load(), N.stream_ptr(dev)

    def one():
        N.check(lib.cdx_hand_term(C.byref(hs.desc), C.byref(hs.native()), C.byref(par), E, N.ptr(poses), N.ptr(centers),
                                  N.ptr(dist), N.ptr(gdist), N.ptr(po), term.weight, 1, N.ptr(loss), N.ptr(g_q),
                                  N.ptr(g_pp), N.ptr(g_po), N.ptr(depth), N.ptr(worst), stream), "cdx_hand_term")

    def two():
        g = cost_launch(hs, par, centers, dist, gdist)[3]
        return pullback_launch(hs, poses, g, po)

    ms = timed({"term": one, "pair": two}, args.reps)
    rec = {"shape": "kernel", "E": E, "S": S, "pairs": len(hs.pairs), **{n: stats(v) for n, v in ms.items()}}
    rec["pair_over_term"] = round(rec["pair"]["median_ms"] / rec["term"]["median_ms"], 3)
    return rec


def run_loops(E, args):
    import numpy as np
    import torch
    from compliancedex_amd import HandTerm, KinGPISGraspOptimizer, ProbabilisticGraspOptimizer
    from compliancedex_amd.optimizer import FINGERTIP_LB, FINGERTIP_UB
    from compliancedex_amd.urdf import load_robot
    from compliancedex_amd.workloads import prob_inputs, stored_gpis, surface_center
    dev = torch.device("cuda")
    hs = model(None, dev)
    gpis = stored_gpis("banana", dev)
    center = surface_center(gpis)
    term = HandTerm(hs, weight=2.0e4, floor_z=float(center[2]) - 0.05, **KW)
    cfg = load_robot("allegro")["config"]
    q, comp, target, palm = prob_inputs(cfg["ref_q"], E, seed=0, spread=True)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (q, target, comp)]
    prob = ProbabilisticGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"], ref_q=cfg["ref_q"],
                                       optimize_target=True, optimize_palm=True, num_iters=args.iters, device=dev,
                                       palm_offset=palm)
    kin = KinGPISGraspOptimizer("allegro", cfg["ee_link_name"], cfg["ee_link_offset"], palm_offset=palm[0, :3].tolist(),
                                num_iters=args.iters, optimize_target=True, ref_q=cfg["ref_q"],
                                tip_bounding_box=[FINGERTIP_LB, FINGERTIP_UB])
    paths = {
        "prob": lambda: prob.optimize(*t, 1, gpis, verbose=False),
        "prob_term": lambda: prob.optimize(*t, 1, gpis, verbose=False, hand_term=term),
        "kingpis": lambda: kin.optimize(*t, 1, gpis, verbose=False, fused=True),
        "kingpis_split": lambda: kin.optimize(*t, 1, gpis, verbose=False, fused=True, split_step=True),
        "kingpis_term": lambda: kin.optimize(*t, 1, gpis, verbose=False, fused=True, hand_term=term),
    }
    ms = timed(paths, args.reps)
    rec = {"shape": "loops", "E": E, "S": hs.n_spheres, "iters": args.iters,
           **{n: stats([v / args.iters for v in vs]) for n, vs in ms.items()}}
    rec["prob_term_adds_ms"] = round(rec["prob_term"]["median_ms"] - rec["prob"]["median_ms"], 4)
    rec["kingpis_term_adds_ms"] = round(rec["kingpis_term"]["median_ms"] - rec["kingpis"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--loop-rows", default="4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", default=None, help="child mode: kernel or loops, one size (--rows) in this process")
    ap.add_argument("--step-seconds", type=int, default=150, help="time limit of each shape's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hand_term.jsonl"))
    args = ap.parse_args()
    if args.shape is None:
        shapes = [("kernel", int(v)) for v in args.rows.split(",") if v] + \
                 [("loops", int(v)) for v in args.loop_rows.split(",") if v]
        for shape, E in shapes:
            cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--shape",
                   shape, "--rows", str(E), "--reps", str(args.reps), "--iters", str(args.iters), "--out", args.out]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit(f"{shape} E={E} ended with status {rc}: nothing more is started")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/hand_term.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    E = int(args.rows.split(",")[0])
    rec = (run_kernel if args.shape == "kernel" else run_loops)(E, args)
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
