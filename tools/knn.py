"""k-nearest-neighbour search (cdx_knn) timed on the GPU: the reference's partial banana cloud resampled with jitter
(as tools/fps.py does) to 2048, 10⁴, 10⁵ and 10⁶ rows and to 256, 512, 1024, 4096 and 2·10⁴ around the automatic
thresholds, every row a query, K = 1, 20, 30 and 64.

Per shape: the scan and the grid walk, each query timed alone as one call of ``knn`` (which allocates its three
outputs, so below 10⁴ rows a time is mostly Python, allocator and launch overhead), and cdx_knn_prepare timed
separately; a torch statement of the query on the device (cdist + topk, float64) where the P × P matrix fits, and the
host build of the rule on one core (cdxh_knn, wall clock) up to --host-rows.  The scan costs P² pairs, so at 10⁶ rows it
is timed for K = 30 only, with --big-reps repeats.  Hybrid search (K = 30 within a radius of 3 mm, which cuts a
share of the lists short, recorded as short_lists) is timed in both paths from 10⁴ rows on, the scan up to 10⁵.  Then end to end: estimate_normals(knn=30) per size, and
GPIS.fit_pointcloud with and without outlier=(20, 2.0) at 10⁵ rows.

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.  Besides the times the record keeps what must
not change: whether the walk returned the scan's bits.  The automatic threshold of cdx_knn is read off
these records.

One JSON line per shape is printed and appended to the record (default profiles/knn.jsonl).  Needs a GPU: there is no
fallback.

  python tools/knn.py [--reps 7] [--big-reps 3] [--sizes 256,…,1000000] [--ks 1,20,30,64] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.fps import cloud, event_ms, stats  # noqa: E402


def host_knn_seconds(X, k):
    """Seconds of cdxh_knn (brute force) on one core."""
    import numpy as np
    from compliancedex_amd import _host, _native as N
    lib = _host.load()
    idx = np.empty((len(X), k), np.int64)
    t = time.perf_counter()
    rc = lib.cdxh_knn(_host.ptr(X), N.DTYPE_F64, len(X), None, len(X), k, float("inf"), 1, _host.ptr(idx), None, None)
    dt = time.perf_counter() - t
    assert rc == 0
    return dt, idx


def torch_knn(x, k):
    """The query stated in torch: the whole P × P matrix, then topk."""
    import torch
    d = torch.cdist(x, x)
    return torch.topk(d, k, dim=1, largest=False, sorted=True)


def timed(paths, reps):
    import torch
    for f in paths.values():  # warm-up: code objects, allocator blocks
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    return {n: stats(v) for n, v in ms.items()}


def run_shape(P, k, args):
    import numpy as np
    import torch
    from compliancedex_amd import KnnGrid, knn
    X = cloud(P)
    x = torch.from_numpy(X).cuda()
    grid = KnnGrid(x)
    big = P >= 500000
    reps = args.big_reps if big else args.reps
    paths = {"grid": lambda: knn(x, k, mode="grid", grid=grid), "prepare": lambda: grid.prepare(x)}
    if not big or k == 30:
        paths["scan"] = lambda: knn(x, k, mode="scan")
    if P * P * 8 <= args.torch_bytes:
        paths["torch_cdist_topk"] = lambda: torch_knn(x, k)
    rec = {"P": P, "K": k, **timed(paths, reps)}
    walk = knn(x, k, mode="grid", grid=grid)
    if "scan" in paths:
        scan = knn(x, k, mode="scan")
        rec["grid_equals_scan"] = bool(all(torch.equal(a, b) for a, b in zip(scan, walk)))
        rec["scan_over_grid"] = round(rec["scan"]["median_ms"] / rec["grid"]["median_ms"], 2)
        rec["scan_over_grid_with_prepare"] = round(
            rec["scan"]["median_ms"] / (rec["grid"]["median_ms"] + rec["prepare"]["median_ms"]), 2)
    if "torch_cdist_topk" in paths:
        rec["torch_over_grid"] = round(rec["torch_cdist_topk"]["median_ms"] / rec["grid"]["median_ms"], 2)
    if P <= args.host_rows:
        sec, hidx = host_knn_seconds(X, k)
        rec["host_one_core_ms"] = round(sec * 1e3, 2)
        rec["grid_equals_host"] = bool(np.array_equal(walk[0].cpu().numpy(), hidx))
    return rec


def run_radius(P, args, radius=0.003, k=30):
    """Hybrid search: lists cut short by the radius, so the walk ends on max_d2."""
    import torch
    from compliancedex_amd import KnnGrid, knn
    x = torch.from_numpy(cloud(P)).cuda()
    grid = KnnGrid(x)
    big = P >= 500000
    paths = {"grid": lambda: knn(x, k, max_distance=radius, mode="grid", grid=grid)}
    if not big:
        paths["scan"] = lambda: knn(x, k, max_distance=radius, mode="scan")
    rec = {"radius": {"P": P, "K": k, "radius": radius, **timed(paths, args.big_reps if big else args.reps)}}
    walk = knn(x, k, max_distance=radius, mode="grid", grid=grid)
    rec["radius"]["short_lists"] = round(float((walk[2] < k).double().mean()), 3)
    if not big:
        scan = knn(x, k, max_distance=radius, mode="scan")
        rec["radius"]["grid_equals_scan"] = bool(all(torch.equal(a, b) for a, b in zip(scan, walk)))
    return rec


def run_normals(P, reps):
    import torch
    from compliancedex_amd import estimate_normals
    x = torch.from_numpy(cloud(P, seed=2)).cuda()
    return {"estimate_normals": {"P": P, "knn": 30, **timed({"estimate_normals": lambda: estimate_normals(x)}, reps)}}


def run_fit(P, k, reps):
    """GPIS.fit_pointcloud end to end with and without the outlier mask in front of the sampling."""
    import torch
    from compliancedex_amd import GPIS, statistical_outlier_mask
    x = torch.from_numpy(cloud(P, seed=1)).cuda()
    weights = torch.rand(50, k, generator=torch.Generator().manual_seed(0)).cuda()
    g = GPIS(0.08, 1.0)
    paths = {"fit_pointcloud": lambda: g.fit_pointcloud(x, num_points=k, weights=weights),
             "fit_pointcloud_outlier": lambda: g.fit_pointcloud(x, num_points=k, weights=weights, outlier=(20, 2.0)),
             "mask_only": lambda: statistical_outlier_mask(x, 20, 2.0)}
    return {"fit_pointcloud": {"P": P, "K": k, **timed(paths, reps)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--big-reps", type=int, default=3)
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,10000,20000,100000,1000000")
    ap.add_argument("--ks", default="1,20,30,64")
    ap.add_argument("--host-rows", type=int, default=10000)
    ap.add_argument("--torch-bytes", type=float, default=4e9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "knn.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/knn.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    from compliancedex_amd.pointcloud import auto_grid_rows
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def keep(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        rec["auto_grid_rows"] = auto_grid_rows()
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    sizes = [int(v) for v in args.sizes.split(",")]
    for P in sizes:
        for k in (int(v) for v in args.ks.split(",")):
            keep(run_shape(P, k, args))
    for P in sizes:
        if P >= 10000:
            keep(run_radius(P, args))
    for P in sizes:
        keep(run_normals(P, args.big_reps if P >= 500000 else args.reps))
    keep(run_fit(100000, 200, args.reps))


if __name__ == "__main__":
    main()
