"""Ray casting (cdx_ray_cast, cdx_depth_render) timed on the GPU on the packaged banana mesh (16 384 faces):

  cast      10⁴, 10⁵ and 10⁶ random rays — origins on a shell around the mesh, aimed at points near its surface —
            scan against walk, with the (ray, face) pairs the walk evaluated per ray (cdx_ray_stats)
  render    a 1000 × 1000 depth image, the reference's size (get_observable_pcd.py:9), scan against walk
  cloud     observable_pointcloud end to end at 1000 × 1000, 2048 points

against two baselines: a vectorised torch statement of the same rule on the device (rays in blocks of 2048 against all
faces; up to --torch-max rays) and the host build on one core (cdxh_ray_cast, wall clock; up to --host-max rays).
What is not run is recorded as null, never estimated.

Device times are HIP events around one call on preallocated inputs after a warm-up call of every path, the paths
alternating within each repeat; the median of --reps and the spread (max − min)/median are kept.  Besides the times the
record keeps what must not change: whether walk, scan and the baselines returned the same hits.

One JSON line per measurement is printed and appended to the record (default profiles/raycast.jsonl).  Needs a GPU: there
is no fallback.

  python tools/raycast.py [--reps 5] [--out PATH] [--rays 10000,100000,1000000] [--torch-max 100000] [--host-max 10000]
"""
import argparse
import ctypes as C
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


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def banana_faces():
    import numpy as np
    d = np.load(os.path.join(REPO, "compliancedex_amd", "data", "meshes", "banana_mesh.npz"))
    v, tri = np.asarray(d["vertices"], np.float64), np.asarray(d["triangles"], np.int64)
    return v[tri.flatten()].reshape(len(tri), 3, 3).astype(np.float32)


def random_rays(faces, R, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    v = faces.astype(np.float64).reshape(-1, 3)
    c, ext = v.mean(axis=0), np.linalg.norm(v.max(axis=0) - v.min(axis=0))
    u = rng.standard_normal((R, 3))
    o = c + 2.0 * ext * u / np.linalg.norm(u, axis=1, keepdims=True)
    target = v[rng.integers(0, len(v), R)] + 0.02 * ext * rng.standard_normal((R, 3))
    return o, target - o


def torch_cast(faces, o, d, tmin=0.0, tmax=float("inf"), block=2048):
    """The rule of csrc/cdx_ray.h with plain torch operators: every ray of a block against every face."""
    import torch
    f = faces.double()
    v0 = f[:, 0]
    e1, e2 = f[:, 1] - v0, f[:, 2] - v0

    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    def cross(a, b):
        return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                            a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)
    n12 = dot(e1, e1) * dot(e2, e2)
    R = o.shape[0]
    t_out = torch.full((R,), float("inf"), dtype=torch.float64, device=o.device)
    f_out = torch.full((R,), -1, dtype=torch.int32, device=o.device)
    idx = torch.arange(f.shape[0], device=o.device)
    for r0 in range(0, R, block):
        ob, db = o[r0:r0 + block, None, :], d[r0:r0 + block, None, :]
        p = cross(db, e2[None])
        det = dot(e1[None], p)
        ok = torch.isfinite(det) & (det * det > (n12[None] * dot(db, db)) * 2.0 ** -40)
        T = ob - v0[None]
        u = dot(T, p) / det
        q = cross(T, e1[None])
        v = dot(db, q) / det
        t = dot(e2[None], q) / det
        hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tmin) & (t <= tmax)
        valid = (torch.isfinite(ob).all(-1) & torch.isfinite(db).all(-1) & (db != 0).any(-1))
        t = torch.where(hit & valid, t, float("inf"))
        tm = t.min(dim=1).values
        first = torch.where(t == tm[:, None], idx[None], f.shape[0]).min(dim=1).values
        any_hit = torch.isfinite(tm)
        t_out[r0:r0 + block] = tm
        f_out[r0:r0 + block] = torch.where(any_hit, first, -1).to(torch.int32)
    return t_out, f_out


def host_cast(faces, o, d):
    """(seconds on one core, t, face) of cdxh_ray_cast."""
    import numpy as np
    from compliancedex_amd import _host
    lib, p = _host.load(), _host.ptr
    R = len(o)
    t, face = np.empty(R), np.empty(R, np.int32)
    t0 = time.perf_counter()
    rc = lib.cdxh_ray_cast(p(faces), len(faces), p(o), p(d), R, 0.0, float("inf"), p(t), p(face), None)
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt, t, face


def walk_pairs(fn):
    """(pairs, rays) the walk counted during fn()."""
    import torch
    from compliancedex_amd import _native as N
    lib = N.load()
    out = (C.c_uint64 * 2)()
    N.check(lib.cdx_ray_stats(1, None, N.stream_ptr()), "cdx_ray_stats")
    fn()
    torch.cuda.synchronize()
    N.check(lib.cdx_ray_stats(0, out, N.stream_ptr()), "cdx_ray_stats")
    return int(out[0]), int(out[1])


def timed(paths, reps):
    import torch
    out = {n: f() for n, f in paths.items()}  # warm-up: code objects, allocator blocks
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    return {n: stats(v) for n, v in ms.items()}, out


def run_cast(pm, faces_np, R, reps, torch_max, host_max):
    import numpy as np
    import torch
    from compliancedex_amd import cast_rays
    on, dn = random_rays(faces_np, R)
    o, d = torch.from_numpy(on).cuda(), torch.from_numpy(dn).cuda()
    paths = {"scan": lambda: cast_rays(pm, o, d, mode="scan"), "walk": lambda: cast_rays(pm, o, d, mode="walk")}
    if R <= torch_max:
        paths["torch"] = lambda: torch_cast(pm.faces, o, d)
    st, out = timed(paths, reps)
    rec = {"what": "cast", "R": R, "F": int(pm.num_faces), **st, "torch": st.get("torch"), "host_one_core_ms": None}
    pairs, rays = walk_pairs(paths["walk"])
    rec["walk_pairs_per_ray"] = round(pairs / max(rays, 1), 2)
    rec["scan_over_walk"] = round(st["scan"]["median_ms"] / st["walk"]["median_ms"], 2)
    ref_t, ref_f = (x.cpu().numpy() for x in out["scan"])
    rec["hit_share"] = round(float((ref_f >= 0).mean()), 4)
    same = {n: bool(np.array_equal(out[n][1].cpu().numpy(), ref_f) and
                    out[n][0].cpu().numpy().tobytes() == ref_t.tobytes()) for n in paths}
    if R <= host_max:
        sec, ht, hf = host_cast(faces_np, on, dn)
        rec["host_one_core_ms"] = round(sec * 1e3, 1)
        same["host"] = bool(np.array_equal(hf, ref_f) and ht.tobytes() == ref_t.tobytes())
    rec["same_bits_as_scan"] = same
    if "torch" in st:
        rec["torch_over_walk"] = round(st["torch"]["median_ms"] / st["walk"]["median_ms"], 1)
    return rec


def run_render(pm, faces_np, size, reps):
    import numpy as np
    import torch
    from compliancedex_amd import Camera, observable_pointcloud, render_depth
    v = faces_np.astype(np.float64).reshape(-1, 3)
    c = 0.5 * (v.min(axis=0) + v.max(axis=0))
    cam = Camera.look_at(c + np.array([-0.3, 0.0, 0.0]), c, (0.0, 0.0, 1.0), 70.0, size, size)  # the reference's pose
    paths = {"scan": lambda: render_depth(pm, cam, mode="scan"), "walk": lambda: render_depth(pm, cam, mode="walk")}
    st, out = timed(paths, reps)
    pairs, rays = walk_pairs(paths["walk"])
    rec = {"what": "render", "W": size, "H": size, "F": int(pm.num_faces), **st,
           "walk_pairs_per_ray": round(pairs / max(rays, 1), 2),
           "scan_over_walk": round(st["scan"]["median_ms"] / st["walk"]["median_ms"], 2),
           "hit_share": round(float((out["walk"] > 0).double().mean()), 4),
           "same_bits_as_scan": bool(torch.equal(out["walk"], out["scan"]))}
    cloud = {"observable_pointcloud": lambda: observable_pointcloud(pm, cam, num_points=2048)}
    st2, out2 = timed(cloud, reps)
    rec2 = {"what": "cloud", "W": size, "H": size, "num_points": 2048, **st2,
            "finite": bool(torch.isfinite(out2["observable_pointcloud"]).all())}
    return rec, rec2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "raycast.jsonl"))
    ap.add_argument("--rays", default="10000,100000,1000000")
    ap.add_argument("--torch-max", type=int, default=100000)
    ap.add_argument("--host-max", type=int, default=10000)
    ap.add_argument("--size", type=int, default=1000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/raycast.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import PreparedMesh, _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def keep(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    faces_np = banana_faces()
    pm = PreparedMesh(torch.from_numpy(faces_np).cuda())
    pm.ray_records()
    for R in (int(v) for v in args.rays.split(",")):
        keep(run_cast(pm, faces_np, R, args.reps, args.torch_max, args.host_max))
    for rec in run_render(pm, faces_np, args.size, args.reps):
        keep(rec)


if __name__ == "__main__":
    main()
