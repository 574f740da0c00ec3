"""The "see and export the fitted object" half of the GPIS workflow, timed on the GPU at steps = 100 (10⁶ cells) on the
stored banana state (N = 361) and on synthetic_banana_gpis(2000):

  (a) get_visualization_data(fused=False)   the per-slice path: 100 slices × (mean, std, mean again for the normal)
                                            and three copies with a sync per slice
  (b) get_visualization_data(fused=True)    one cdx_gpis_field call and one copy back
  (c) topcd on the device                   numpy float32 inputs: upload, count, one host read, place, copy back
  (d) cdxh_surface_extract on the host      the same cell rule as a plain C++ loop (the CPU yardstick)
  (e) surface()                             mean-only field, count, place, normals of the surface cells alone
  (f) the mean-only kernel                  cdx_gpis_field asking for the mean alone (the TPS mean kernel without its
                                            gradient sums) against cdx_gpis_field with the normal and against
                                            cdx_gpis_mean with null gradient outputs (both the full kernel): HIP
                                            events around native calls on preallocated buffers, alternating

Wall-clock ms around calls that end in a device synchronise (the copies back), after a warm-up call of each; (a) and
(b) alternate within every repeat.  Besides the times the record keeps what must not change: max |a − b| of the two
paths' outputs, and whether (c), (d) and (e) give the same cloud.

Every GPU step runs in a child process of its own under a time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the GPU after it).  One JSON line per step is printed and appended to the
record (default profiles/gpis_field.jsonl).

  python tools/gpis_field.py [--steps 100] [--reps 5] [--states banana,synthetic2000] [--out PATH] [--timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BOXES = {  # (lb, ub): the object with a margin, unequal along x, y, z
    "banana": ([-0.10, -0.06, -0.08], [0.12, 0.07, 0.05]),
    "synthetic2000": ([-0.05, -0.12, -0.04], [0.09, 0.12, 0.05]),
}


def stats(ms):
    import numpy as np
    med = float(np.median(ms))
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 3)}


def load_gpis(state):
    from compliancedex_amd.workloads import stored_gpis, synthetic_banana_gpis
    return synthetic_banana_gpis(2000, "cuda") if state == "synthetic2000" else stored_gpis(state, "cuda")


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def step_visualization(g, state, steps, reps):
    """(a) against (b), alternating."""
    import numpy as np
    lb, ub = BOXES[state]
    paths = {"eager": lambda: g.get_visualization_data(lb, ub, steps=steps),
             "fused": lambda: g.get_visualization_data(lb, ub, steps=steps, fused=True)}
    out = {k: timed(f)[1] for k, f in paths.items()}  # warm-up: code objects, allocator blocks, the state
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            ms[k].append(timed(f)[0])
    e, f = out["eager"], out["fused"]
    rec = {"a_eager": stats(ms["eager"]), "b_fused": stats(ms["fused"])}
    rec["ratio_a_over_b"] = round(rec["a_eager"]["median_ms"] / rec["b_fused"]["median_ms"], 2)
    rec["max_abs_diff"] = {"mean": float(np.abs(e[0] - f[0]).max()), "std": float(np.abs(e[1] - f[1]).max()),
                           "normal": float(np.abs(e[2] - f[2]).max())}
    return rec


def step_surface(g, state, steps, reps):
    """(c), (d), (e) on one field."""
    import numpy as np
    import torch
    from compliancedex_amd import _host, _native as N
    lb, ub = BOXES[state]
    mean, _, normal, _, _ = g.get_visualization_data(lb, ub, steps=steps, fused=True)
    host, p = _host.load(), _host.ptr
    axes = [np.linspace(lb[d], ub[d], steps) for d in range(3)]
    cap = (steps - 2) ** 3
    hp, hn = np.zeros((cap, 3)), np.zeros((cap, 3), np.float32)

    def host_extract():
        return host.cdxh_surface_extract(p(mean), p(normal), N.DTYPE_F32, steps, 0, p(axes[0]), p(axes[1]), p(axes[2]),
                                         cap, None, p(hp), p(hn))

    paths = {"c_topcd_device": lambda: g.topcd(mean, normal, lb, ub, steps=steps), "d_extract_host": host_extract,
             "e_surface": lambda: g.surface(lb, ub, steps=steps)}
    out = {k: timed(f)[1] for k, f in paths.items()}
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            ms[k].append(timed(f)[0])
    n = int(out["d_extract_host"])
    cp, cn = out["c_topcd_device"]
    ep, en = (t.cpu().numpy() for t in out["e_surface"])
    rec = {k: stats(v) for k, v in ms.items()}
    rec["surface_points"] = n
    rec["c_equals_d"] = bool(len(cp) == n and np.array_equal(cp, hp[:n]) and np.array_equal(cn, hn[:n]))
    rec["e_points_equal_c"] = bool(np.array_equal(ep, cp))
    rec["e_normals_max_abs_diff_c"] = float(np.abs(en.astype(np.float32) - cn).max()) if len(ep) == len(cp) and n else None
    torch.cuda.synchronize()
    return rec


def step_mean_only(g, state, steps, reps):
    """(f): the three native calls, 10 enqueued back to back per timing, alternating."""
    import torch
    from compliancedex_amd import _native as N
    lib = N.load()
    st = g.native_state()
    dev = g.X1.device
    lb, ub = BOXES[state]
    ax = g._query_axes(lb, ub, steps)
    n = steps ** 3
    X = torch.empty(n, 3, dtype=torch.float64, device=dev)
    N.check(lib.cdx_gpis_field_points(N.ptr(ax[0]), N.ptr(ax[1]), N.ptr(ax[2]), steps, None, n, N.ptr(X),
                                      N.stream_ptr(dev)), "cdx_gpis_field_points")
    mean = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3)]
    normal = torch.empty(n, 3, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.cdx_gpis_field_workspace(st.desc, steps, 0), dtype=torch.uint8, device=dev)
    s = N.stream_ptr(dev)

    def field(m, nrm):
        N.check(lib.cdx_gpis_field(st.desc, N.ptr(ax[0]), N.ptr(ax[1]), N.ptr(ax[2]), steps, 0, N.ptr(m), None, N.ptr(nrm),
                                   N.ptr(ws), s), "cdx_gpis_field")

    paths = {"field_mean_only": lambda: field(mean[0], None), "field_mean_normal": lambda: field(mean[1], normal),
             "mean_call_full_kernel": lambda: N.check(lib.cdx_gpis_mean(st.desc, N.ptr(X), n, N.ptr(mean[2]), None, None, s),
                                                      "cdx_gpis_mean")}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    inner = 10

    def timed_events(f):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(inner):
            f()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / inner

    for f in paths.values():
        timed_events(f)
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            ms[k].append(timed_events(f))
    rec = {k: stats(v) for k, v in ms.items()}
    rec["calls_per_timing"] = inner
    rec["mean_bits_equal"] = bool(torch.equal(mean[0], mean[1]) and torch.equal(mean[0], mean[2]))
    return rec


STEPS = {"visualization": step_visualization, "surface": step_surface, "mean_only": step_mean_only}


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpis_field.py measures on the GPU: no device found")
    g = load_gpis(args.state)
    rec = {"case": "gpis_field", "step": args.child, "state": args.state, "N": int(g.X1.shape[0]), "steps": args.steps,
           "repeats": args.reps}
    rec.update(STEPS[args.child](g, args.state, args.steps, args.reps))
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--states", default="banana,synthetic2000")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gpis_field.jsonl"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per GPU step")
    ap.add_argument("--child", choices=sorted(STEPS))
    ap.add_argument("--state")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for state in args.states.split(","):
        if state not in BOXES:
            raise SystemExit(f"unknown state {state!r}")
    for state in args.states.split(","):
        for step in ("visualization", "surface", "mean_only"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--state", state, "--steps", str(args.steps),
                   "--reps", str(args.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{step} on {state} ran past {args.timeout} s: stopping here")
            lines = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
            if r.returncode != 0 or not lines:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{step} on {state} failed (exit {r.returncode}): stopping here")
            print(lines[-1], flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(lines[-1] + "\n")


if __name__ == "__main__":
    main()
