"""Farthest-point sampling (cdx_fps) timed on the GPU at the reference's sizes:

  200 from 2048     the cropped cloud in front of gpis.fit (optimize_pregrasp.py:904)
  2048 from 8192    the one-workgroup path at its capacity, where automatic mode changes paths
  2048 from 10⁵
  2048 from 10⁶     the depth image of get_observable_pcd.py:40

Each shape in mode "block" (one workgroup per cloud, one launch) where the capacity admits it and in mode "rounds" (one
launch per round), against two baselines: the host build of the same rule on one core (cdxh_fps, wall clock) and a
plain torch loop of the rule on the device with an argmax per round — what a user could do on the device without
cdx_fps.  Then GPIS.fit_pointcloud end to end (sample, recipe, fit) at 200 from 10⁵.

Device times are HIP events around one call on preallocated inputs after a warm-up call of every path, the paths
alternating within each repeat; the median of --reps and the spread (max − min)/median are kept.  Besides the times the
record keeps what must not change: whether every path returned the host build's indices.  "rounds" at 200 from 2048
is launch-bound, so its time per round is the per-round launch cost.

One JSON line per shape is printed and appended to the record (default profiles/fps.jsonl).  Needs a GPU: there is no
fallback.

  python tools/fps.py [--reps 7] [--out PATH] [--shapes 2048:200,8192:2048,100000:2048,1000000:2048] [--no-host]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stats(ms):
    import numpy as np
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "spread": round((max(ms) - min(ms)) / med, 3),
            "n": len(ms)}


def cloud(P, seed=0):
    """The reference's partial banana cloud resampled to P rows with 2 mm of jitter (seeded)."""
    import numpy as np
    base = np.load(os.path.join(REPO, "compliancedex_amd", "data", "partial_pcd_banana.npy"))
    rng = np.random.default_rng(seed)
    return base[rng.integers(0, len(base), P)] + 0.002 * rng.standard_normal((P, 3))


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_loop(x, k, start=0):
    """The rule with plain torch operators: several launches and temporaries per round."""
    import torch
    finite = torch.isfinite(x).all(dim=1)
    dist = torch.where(finite, float("inf"), -1.0).to(torch.float64)
    sel = torch.empty(k, dtype=torch.int64, device=x.device)
    s = torch.tensor(start, device=x.device)
    for i in range(k):
        sel[i] = s
        d = x - x[s]
        q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        dist = torch.where(finite & (q < dist), q, dist)
        s = torch.argmax(dist)
    return sel


def host_fps(X, k):
    """(seconds on one core, sel) of cdxh_fps."""
    import numpy as np
    from compliancedex_amd import _host, _native as N
    lib = _host.load()
    sel = np.empty(k, np.int64)
    t = time.perf_counter()
    rc = lib.cdxh_fps(_host.ptr(X), N.DTYPE_F64, len(X), 1, k, 0, _host.ptr(sel), None, None)
    dt = time.perf_counter() - t
    assert rc == 0
    return dt, sel


def run_shape(P, k, reps, with_host):
    import numpy as np
    import torch
    from compliancedex_amd import farthest_point_sample
    from compliancedex_amd.pointcloud import capacity
    X = cloud(P)
    x = torch.from_numpy(X).cuda()
    paths = {"rounds": lambda: farthest_point_sample(x, k, mode="rounds"), "torch_loop": lambda: torch_loop(x, k)}
    if P <= capacity():
        paths["block"] = lambda: farthest_point_sample(x, k, mode="block")
    out = {n: f() for n, f in paths.items()}  # warm-up: code objects, allocator blocks
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    rec = {"P": P, "K": k, "capacity": capacity(), **{n: stats(v) for n, v in ms.items()}}
    rec["rounds_us_per_round"] = round(1e3 * rec["rounds"]["median_ms"] / max(k - 1, 1), 3)
    ref = out["rounds"].cpu().numpy()
    if with_host:
        sec, hsel = host_fps(X, k)
        rec["host_one_core_ms"] = round(sec * 1e3, 2)
        ref = hsel
    rec["same_indices"] = {n: bool(np.array_equal(o.cpu().numpy(), ref)) for n, o in out.items()}
    for n in paths:
        if n != "torch_loop":
            rec[f"torch_loop_over_{n}"] = round(rec["torch_loop"]["median_ms"] / rec[n]["median_ms"], 2)
            if with_host:
                rec[f"host_over_{n}"] = round(rec["host_one_core_ms"] / rec[n]["median_ms"], 1)
    return rec


def run_fit(P, k, reps):
    """GPIS.fit_pointcloud end to end (sample, bounding box, recipe, cdx_gpis_fit), and its sampling call alone."""
    import torch
    from compliancedex_amd import GPIS, farthest_point_sample
    x = torch.from_numpy(cloud(P, seed=1)).cuda()
    weights = torch.rand(50, k, generator=torch.Generator().manual_seed(0)).cuda()
    g = GPIS(0.08, 1.0)
    paths = {"fit_pointcloud": lambda: g.fit_pointcloud(x, num_points=k, weights=weights),
             "sample_only": lambda: farthest_point_sample(x, k)}
    for f in paths.values():
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    return {"fit_pointcloud": {"P": P, "K": k, **{n: stats(v) for n, v in ms.items()}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fps.jsonl"))
    ap.add_argument("--shapes", default="2048:200,8192:2048,100000:2048,1000000:2048")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/fps.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def keep(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for spec in args.shapes.split(","):
        P, k = (int(v) for v in spec.split(":"))
        keep(run_shape(P, k, args.reps, not args.no_host))
    keep(run_fit(100000, 200, args.reps))


if __name__ == "__main__":
    main()
