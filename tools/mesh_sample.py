"""Area-weighted surface sampling (cdx_sample_prepare / cdx_sample_draw) timed on the GPU:

  the banana mesh           16 384 faces, exactly the "table" path's capacity: both draw paths
  a synthetic mesh          10⁶ faces: the "splitters" path (runs of 512 faces finished in global memory)

at 10⁴, 10⁶ and 10⁷ samples, points only and with every output, and the prepare call of each mesh.  Two baselines: a
torch statement of the same rule on the device (Philox and the 64-bit multiply in int64 tensor ops, torch.searchsorted
for the face, gathers for the point) — what a user could do on the device without cdx_sample — and the host build of the
rule on one core (cdxh_sample_draw, wall clock).

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.  The draw's output rate (bytes written over
time) is stated against the 6.29 TB/s a copy kernel reaches on this part's HBM (8.0 TB/s by specification).  Besides
the times the record keeps what must not change: whether every path returned the host build's faces and points.

First of all the reference's opening on the banana end to end, on a sampler built once: the Poisson-disk cloud (4096 of
20 480 uniform samples, and 128 of 640) and GPIS.fit_mesh; --samples "" stops after it.

One JSON line for that and one per (mesh, samples) is printed and appended to the record (default profiles/mesh_sample.jsonl).  Needs a
GPU: there is no fallback.

  python tools/mesh_sample.py [--reps 7] [--out PATH] [--samples 10000,1000000,10000000] [--no-host] [--no-torch]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_COPY_TBS = 6.29  # measured float4 copy on MI355X; 8.0 TB/s is the specification
M32 = 0xFFFFFFFF


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


def synthetic_mesh(F, seed=0):
    """F float32 triangles of log-uniform size (two decades) around random centres."""
    import numpy as np
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((F, 1, 3))
    size = 10.0 ** rng.uniform(-3, -1, (F, 1, 1))
    return (centre + size * rng.standard_normal((F, 3, 3))).astype(np.float32)


def mul32(a, b):
    """(high, low) 32-bit words of a·b for int64 tensors (or ints) holding 32-bit words: no product passes 2⁶³."""
    a0, a1, b0, b1 = a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16
    p00 = a0 * b0
    mid = a0 * b1 + a1 * b0 + (p00 >> 16)
    return a1 * b1 + (mid >> 16), ((mid & 0xFFFF) << 16) | (p00 & 0xFFFF)


def torch_draw(faces64, cdf, total, seed, first, K):
    """The rule with plain torch operators on the device: (points, face)."""
    import torch
    i = first + torch.arange(K, dtype=torch.int64, device=cdf.device)
    c0, c1 = i & M32, (i >> 32) & M32
    c2, c3 = torch.zeros_like(i), torch.zeros_like(i)
    k0, k1 = seed & M32, seed >> 32
    for _ in range(10):
        h0, l0 = mul32(c0, 0xD2511F53)
        h1, l1 = mul32(c2, 0xCD9E8D57)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    bl, bh = total & M32, total >> 32
    ll, hl, lh, hh = mul32(c0, bl), mul32(c1, bl), mul32(c0, bh), mul32(c1, bh)
    w1 = ll[0] + hl[1] + lh[1]
    w2 = hl[0] + lh[0] + hh[1] + (w1 >> 32)
    t = ((hh[0] + (w2 >> 32)) << 32) | (w2 & M32)  # below total < 2⁶⁰
    face = torch.searchsorted(cdf, t, right=True)
    u, v = (c2.double() + 0.5) * 2.0 ** -32, (c3.double() + 0.5) * 2.0 ** -32
    flip = u + v > 1.0
    u, v = torch.where(flip, 1.0 - u, u), torch.where(flip, 1.0 - v, v)
    f = faces64[face]
    return (f[:, 0] + u[:, None] * (f[:, 1] - f[:, 0])) + v[:, None] * (f[:, 2] - f[:, 0]), face


def host_run(faces, K, seed):
    """(prepare seconds, draw seconds, points, face) of the host build on one core."""
    import numpy as np
    from compliancedex_amd import _host, _native as N
    lib, p = _host.load(), _host.ptr
    cdf, info = np.zeros(len(faces), np.uint64), np.zeros(1, np.int32)
    t0 = time.perf_counter()
    assert lib.cdxh_sample_prepare(p(faces), N.DTYPE_F32, len(faces), p(cdf), p(info)) == 0
    t1 = time.perf_counter()
    points, face = np.empty((K, 3)), np.empty(K, np.int64)
    assert lib.cdxh_sample_draw(p(faces), N.DTYPE_F32, len(faces), p(cdf), seed, 0, K, p(points), p(face), None,
                                None) == 0
    return t1 - t0, time.perf_counter() - t1, points, face


def run_mesh(name, faces, samples, reps, with_host, with_torch, keep):
    import numpy as np
    import torch
    from compliancedex_amd import SurfaceSampler
    from compliancedex_amd.sampling import table_capacity
    f = torch.from_numpy(faces).cuda()
    F = len(faces)
    sampler = SurfaceSampler(f)  # warm-up of prepare
    torch.cuda.synchronize()
    prep = stats([event_ms(lambda: SurfaceSampler(f))[0] for _ in range(reps)])  # with the one-word read-back
    modes = ["splitters"] + (["table"] if F <= table_capacity() else [])
    faces64, total = f.double(), int(sampler.cdf[-1].item())
    seed = 0
    for K in samples:
        paths = {}
        for m in modes:
            paths[m] = lambda m=m: sampler.draw(K, seed, want_face=True, mode=m)
            paths[m + "_points_only"] = lambda m=m: (sampler.draw(K, seed, mode=m),)
            paths[m + "_all"] = lambda m=m: sampler.draw(K, seed, want_face=True, want_normal=True, want_bary=True,
                                                         mode=m)
        paths["auto"] = lambda: sampler.draw(K, seed, want_face=True)
        if with_torch:
            paths["torch"] = lambda: torch_draw(faces64, sampler.cdf, total, seed, 0, K)
        out = {n: fn() for n, fn in paths.items()}  # warm-up: code objects, allocator blocks
        torch.cuda.synchronize()
        ms = {n: [] for n in paths}
        for _ in range(reps):
            for n, fn in paths.items():
                ms[n].append(event_ms(fn)[0])
        rec = {"mesh": name, "F": F, "K": K, "table_capacity": table_capacity(), "prepare": prep,
               **{n: stats(v) for n, v in ms.items()}}
        out_bytes = {"": 32, "_points_only": 24, "_all": 72}
        for m in modes:
            for suffix, b in out_bytes.items():
                tbs = b * K / (rec[m + suffix]["median_ms"] * 1e-3) / 1e12
                rec[m + suffix]["output_TBs"] = round(tbs, 4)
                rec[m + suffix]["share_of_hbm_copy"] = round(tbs / HBM_COPY_TBS, 4)
        ref_points, ref_face = out[modes[0]][0].cpu().numpy(), out[modes[0]][1].cpu().numpy()
        if with_host and K <= 10 ** 7:
            psec, dsec, ref_points, ref_face = host_run(faces, K, seed)
            rec["host_one_core_prepare_ms"], rec["host_one_core_draw_ms"] = round(psec * 1e3, 2), round(dsec * 1e3, 2)
            for m in modes:
                rec[f"host_over_{m}"] = round(rec["host_one_core_draw_ms"] / rec[m]["median_ms"], 1)
        same = {}
        for n, o in out.items():
            if n == "torch":  # faces exactly; torch may contract the point's arithmetic
                same[n] = bool(np.array_equal(o[1].cpu().numpy(), ref_face) and
                               np.allclose(o[0].cpu().numpy(), ref_points, rtol=0, atol=1e-12))
            else:
                same[n] = bool(o[0].cpu().numpy().tobytes() == ref_points.tobytes() and
                               (len(o) < 2 or np.array_equal(o[1].cpu().numpy(), ref_face)))
        rec["same_as_host"] = same
        if with_torch:
            for m in modes:
                rec[f"torch_over_{m}"] = round(rec["torch"]["median_ms"] / rec[m]["median_ms"], 2)
        keep(rec)


def run_fit(faces, reps):
    """The reference's opening on a mesh object end to end: the Poisson-disk cloud (4096 of 20 480 uniform samples) and
    GPIS.fit_mesh on top of it, on a sampler built once."""
    import torch
    from compliancedex_amd import GPIS, SurfaceSampler, sample_points_poisson_disk
    sampler = SurfaceSampler(torch.from_numpy(faces).cuda())
    weights = torch.rand(50, 200, generator=torch.Generator().manual_seed(0)).cuda()
    g = GPIS(0.08, 1.0)
    paths = {"poisson_disk_4096": lambda: sample_points_poisson_disk(sampler, 4096),
             "poisson_disk_128": lambda: sample_points_poisson_disk(sampler, 128),
             "fit_mesh": lambda: g.fit_mesh(sampler, weights=weights)}
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(reps):
        for n, fn in paths.items():
            ms[n].append(event_ms(fn)[0])
    return {"mesh": "banana", "F": len(faces), **{n: stats(v) for n, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_sample.jsonl"))
    ap.add_argument("--samples", default="10000,1000000,10000000")
    ap.add_argument("--synthetic-faces", type=int, default=10 ** 6)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_sample.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def keep(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    samples = [int(v) for v in args.samples.split(",") if v]
    banana = np.load(os.path.join(REPO, "compliancedex_amd", "data", "meshes", "banana_faces.npy"))
    keep(run_fit(banana, args.reps))
    if not samples:
        return
    run_mesh("banana", banana, samples, args.reps, not args.no_host, not args.no_torch, keep)
    run_mesh(f"synthetic_{args.synthetic_faces}", synthetic_mesh(args.synthetic_faces), samples, args.reps,
             not args.no_host, not args.no_torch, keep)


if __name__ == "__main__":
    main()
