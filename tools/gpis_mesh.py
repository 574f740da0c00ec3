"""The "mesh of the completed shape" step of the GPIS workflow, timed on the GPU at steps = 100 (10⁶ nodes) on the stored
banana state (N = 361) and on synthetic_banana_gpis(2000):

  (a) tomesh on the device        a numpy float64 lattice: upload, count, one host read, place, copy back
  (b) the two native calls        cdx_gpis_mesh_count and cdx_gpis_mesh_place on preallocated device buffers, HIP events
                                  around 10 calls enqueued back to back
  (c) cdxh_mesh_extract           the same rule as plain C++ loops on the host (the CPU yardstick)
  (d) a vectorised torch statement of the rule on the device (boolean masks, sorts and searchsorted)
  (e) surface_mesh(refine=0)      mean-only field, count, read, place, normals at the vertices
  (f) surface_mesh(refine=3)      the same plus three refinement steps
  (g) one refinement step split   the GPIS mean call at the vertices against the torch statement's ops around it
                                  (mesh.EdgeRefiner) and against the kernels surface_mesh uses
                                  (cdx_gpis_mesh_refine_init / _step), HIP events: the kernel exists because the torch
                                  ops of a step cost more than the mean call

Wall-clock ms around calls that end in a device synchronise, after a warm-up call of each, the paths of a step
alternating within every repeat; median and (max − min)/median are kept.  Besides the times the record keeps what must
not change: whether (a), (c) and (d) give the same mesh, whether (e) equals (a) on its own lattice, and max |mean| at
the vertices with and without refinement.

Every GPU step runs in a child process of its own under a time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the GPU after it).  One JSON line per step is printed and appended to the
record (default profiles/gpis_mesh.jsonl).

  python tools/gpis_mesh.py [--steps 100] [--reps 5] [--states banana,synthetic2000] [--out PATH] [--timeout 300]
"""
import argparse
import itertools
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BOXES = {  # (lb, ub): the object with a margin, unequal along x, y, z (tools/gpis_field.py's)
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


def measure(paths, reps):
    out = {k: timed(f)[1] for k, f in paths.items()}  # warm-up: code objects, allocator blocks, the state
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            ms[k].append(timed(f)[0])
    return out, {k: stats(v) for k, v in ms.items()}


def torch_mesh(mean, axes):
    """The rule of csrc/cdx_mesh.h as whole-lattice torch ops: (vertices, keys, faces int32) on mean's device."""
    import torch
    from compliancedex_amd.mesh import EDGE_OFFSETS, EdgeRefiner
    s, dev = mean.shape[0], mean.device
    inside = mean < 0
    idx = torch.arange(s ** 3, device=dev).view(s, s, s)
    keys = []
    for d, (di, dj, dk) in enumerate(EDGE_OFFSETS):
        crossing = inside[:s - di, :s - dj, :s - dk] != inside[di:, dj:, dk:]
        keys.append(7 * idx[:s - di, :s - dj, :s - dk][crossing] + d)
    keys = torch.sort(torch.cat(keys)).values
    vertices = EdgeRefiner(keys, mean, axes).vertices()  # (its first vertex is the rule's)
    ends = (axes[:, -1] - axes[:, 0]).cpu()
    gsign = -int(torch.sign(ends).prod())
    cube = idx[:s - 1, :s - 1, :s - 1].reshape(-1)
    edge_type = {o: n for n, o in enumerate(EDGE_OFFSETS)}
    rows, order = [], []
    for tet, perm in enumerate(itertools.permutations(range(3))):
        corner = [(0, 0, 0)]
        for ax in perm:
            corner.append(tuple(c + (a == ax) for a, c in enumerate(corner[-1])))
        node = [cube + (q[0] * s + q[1]) * s + q[2] for q in corner]
        ins = [inside.view(-1)[n] for n in node]
        code = ins[0].int() + 2 * ins[1].int() + 4 * ins[2].int() + 8 * ins[3].int()
        psign = 1 if perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1

        def key(x, y, sel):
            lo, hi = min(x, y), max(x, y)
            return 7 * node[lo][sel] + edge_type[tuple(h - l for h, l in zip(corner[hi], corner[lo]))]

        for bits in range(1, 15):
            sel = code == bits
            inn = [q for q in range(4) if (bits >> q) & 1]
            out = [q for q in range(4) if not (bits >> q) & 1]
            if len(inn) == 2:
                (a, b), (c, d) = inn, out
                det = gsign * psign * (-1) ** sum(x > y for x in inn for y in out)
                tris = [((a, c), (a, d), (b, d)), ((a, c), (b, d), (b, c))]
                swap = det < 0
            else:
                lone, rest = (inn[0], out) if len(inn) == 1 else (out[0], inn)
                det = gsign * psign * (-1) ** lone
                tris = [tuple((lone, r) for r in rest)]
                swap = det < 0 if len(inn) == 1 else det > 0
            for t, (e0, e1, e2) in enumerate(tris):
                if swap:
                    e1, e2 = e2, e1
                rows.append(torch.stack([key(*e0, sel), key(*e1, sel), key(*e2, sel)], dim=1))
                order.append((cube[sel] * 6 + tet) * 2 + t)
    rows = torch.cat(rows)[torch.sort(torch.cat(order)).indices]
    return vertices, keys, torch.searchsorted(keys, rows).to(torch.int32)


def step_tomesh(g, state, steps, reps):
    """(a) – (d) on one lattice: the state's mean on the float64 point axes."""
    import numpy as np
    import torch
    from compliancedex_amd import _host, _native as N
    lb, ub = BOXES[state]
    dev = g.X1.device
    pax = g._point_axes(lb, ub, steps)
    grid = torch.stack(torch.meshgrid(pax[0], pax[1], pax[2], indexing="xy"), dim=3)
    mean_d = g.pred_mean(grid).contiguous()
    mean = mean_d.cpu().numpy()
    axes = [np.ascontiguousarray(a) for a in pax.cpu().numpy()]
    host, p = _host.load(), _host.ptr
    counts = np.zeros(2, np.int64)
    args = [p(mean), N.DTYPE_F64, steps, p(axes[0]), p(axes[1]), p(axes[2])]
    assert host.cdxh_mesh_extract(*args, 0, 0, None, None, None, p(counts)) == 0
    V, F = int(counts[0]), int(counts[1])
    hv, hk, hf = np.zeros((V, 3)), np.zeros(V, np.int64), np.zeros((F, 3), np.int32)

    def host_extract():
        return host.cdxh_mesh_extract(*args, V, F, p(hv), p(hk), p(hf), p(counts))

    paths = {"a_tomesh_device": lambda: g.tomesh(mean, lb, ub, steps=steps), "c_extract_host": host_extract,
             "d_torch_statement": lambda: torch_mesh(mean_d, pax)}
    out, rec = measure(paths, reps)
    av, af = out["a_tomesh_device"]
    tv, tk, tf = (t.cpu().numpy() for t in out["d_torch_statement"])
    rec.update(vertices=V, faces=F)
    rec["a_equals_c"] = bool(av.tobytes() == hv.tobytes() and af.tobytes() == hf.tobytes())
    rec["d_equals_c"] = bool(tv.tobytes() == hv.tobytes() and tk.tobytes() == hk.tobytes() and tf.tobytes() == hf.tobytes())

    # (b) the native calls alone
    lib = N.load()
    ws = torch.empty(lib.cdx_gpis_mesh_workspace(steps), dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    v = torch.empty(V, 3, dtype=torch.float64, device=dev)
    e = torch.empty(V, dtype=torch.int64, device=dev)
    f = torch.empty(F, 3, dtype=torch.int32, device=dev)
    s = N.stream_ptr(dev)
    calls = {"b_count": lambda: N.check(lib.cdx_gpis_mesh_count(N.ptr(mean_d), N.DTYPE_F64, steps, N.ptr(ws), N.ptr(totals),
                                                                s), "count"),
             "b_place": lambda: N.check(lib.cdx_gpis_mesh_place(N.ptr(mean_d), N.DTYPE_F64, steps, N.ptr(pax[0]),
                                                                N.ptr(pax[1]), N.ptr(pax[2]), N.ptr(ws), V, F, N.ptr(v),
                                                                N.ptr(e), N.ptr(f), s), "place")}
    rec.update(event_timings(calls, reps, 10))
    rec["calls_per_timing"] = 10
    rec["b_equals_c"] = bool(v.cpu().numpy().tobytes() == hv.tobytes() and f.cpu().numpy().tobytes() == hf.tobytes())
    return rec


def event_timings(calls, reps, inner):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(fn):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(inner):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / inner

    for fn in calls.values():
        run(fn)
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(run(fn))
    return {k: stats(v) for k, v in ms.items()}


def step_surface_mesh(g, state, steps, reps):
    """(e), (f), (g)."""
    import torch
    from compliancedex_amd.gpis import gpis_mean
    from compliancedex_amd.mesh import EdgeRefiner, refine_vertices
    lb, ub = BOXES[state]
    paths = {"e_surface_mesh_refine0": lambda: g.surface_mesh(lb, ub, steps=steps),
             "f_surface_mesh_refine3": lambda: g.surface_mesh(lb, ub, steps=steps, refine=3)}
    out, rec = measure(paths, reps)
    v0, f0, _ = out["e_surface_mesh_refine0"]
    v3, f3, _ = out["f_surface_mesh_refine3"]
    pax = g._point_axes(lb, ub, steps)
    grid = torch.stack(torch.meshgrid(pax[0], pax[1], pax[2], indexing="xy"), dim=3)
    lattice = g.pred_mean(grid).contiguous()
    tv, tf = g.tomesh(lattice, lb, ub, steps=steps)
    rec.update(vertices=int(v0.shape[0]), faces=int(f0.shape[0]))
    rec["e_equals_tomesh_of_its_lattice"] = bool(v0.cpu().numpy().tobytes() == tv.tobytes() and
                                                 f0.cpu().numpy().tobytes() == tf.tobytes())
    rec["faces_unchanged_by_refine"] = bool(torch.equal(f0, f3))
    e0, e3 = float(g.pred_mean(v0).abs().max()), float(g.pred_mean(v3).abs().max())
    rec["max_abs_mean_refine0"], rec["max_abs_mean_refine3"] = e0, e3
    rec["refine3_over_refine0"] = e3 / e0 if e0 > 0 else None

    # (g) one refinement step: the mean call against everything else in the step
    st = g.native_state()
    from compliancedex_amd import _native as N
    _, edges, _ = g._mesh_extract(lattice, N.DTYPE_F64, steps, pax)
    X = v0.contiguous()

    def mean_fn(Y):
        return gpis_mean(st, Y, want_grad=False)[0]

    def whole_step():
        EdgeRefiner(edges, lattice, pax).step(mean_fn)

    def setup_only():
        EdgeRefiner(edges, lattice, pax)

    lib = N.load()
    nv = X.shape[0]
    state = torch.empty(5, nv, dtype=torch.float64, device=X.device)
    fv = mean_fn(X)
    out = torch.empty_like(X)
    s = N.stream_ptr(X.device)

    def kernel_init():
        N.check(lib.cdx_gpis_mesh_refine_init(N.ptr(lattice), N.DTYPE_F64, steps, N.ptr(pax[0]), N.ptr(pax[1]),
                                              N.ptr(pax[2]), N.ptr(edges), nv, N.ptr(state), N.ptr(out), s), "init")

    def kernel_step():
        N.check(lib.cdx_gpis_mesh_refine_step(N.ptr(fv), steps, N.ptr(pax[0]), N.ptr(pax[1]), N.ptr(pax[2]), N.ptr(edges),
                                              nv, N.ptr(state), N.ptr(out), s), "step")

    rec.update(event_timings({"g_mean_call": lambda: mean_fn(X), "g_refiner_setup": setup_only,
                              "g_setup_and_one_step": whole_step, "g_kernel_init": kernel_init,
                              "g_kernel_step": kernel_step}, reps, 5))
    rec["refine3_equals_torch_statement"] = bool(torch.equal(v3, refine_vertices(g.pred_mean, edges, lattice, pax, 3)))
    m, su, ws = (rec[k]["median_ms"] for k in ("g_mean_call", "g_refiner_setup", "g_setup_and_one_step"))
    rec["g_torch_ops_per_step_ms"] = round(ws - su - m, 3)
    return rec


STEPS = {"tomesh": step_tomesh, "surface_mesh": step_surface_mesh}


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpis_mesh.py measures on the GPU: no device found")
    g = load_gpis(args.state)
    rec = {"case": "gpis_mesh", "step": args.child, "state": args.state, "N": int(g.X1.shape[0]), "steps": args.steps,
           "repeats": args.reps}
    rec.update(STEPS[args.child](g, args.state, args.steps, args.reps))
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--states", default="banana,synthetic2000")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gpis_mesh.jsonl"))
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
        for step in ("tomesh", "surface_mesh"):
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
