"""The whole-hand sphere collision term timed on the GPU: E = 4096, 16 384 and 65 536 candidates of the Allegro hand
(the spheres of a URDF's collision primitives; without --urdf the recorded ones of tests/golden/spheres_allegro.json)
against the packaged banana as a GPIS and as a prepared mesh.

Per shape and object kind: the three kernels on their own (cdx_hand_spheres, cdx_hand_cost, cdx_hand_pullback), the
object's distance query, and ``hand_collision`` end to end with its backward (cost.sum().backward() into q and the palm
pose); a torch-operator statement of the same rule on the device — every body's pose by batched 3 × 3 products, the
three hinges over gathered pairs, autograd for the gradient, given the same distance query —; and the host build of
the three kernels' rule on one core (wall clock) up to --host-rows.  The record keeps how far the torch statement's
cost and gradients are from the kernels'.

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.

Without --kind the tool is the driver: every shape runs in a child process of its own under ``timeout``, one after the
other, and the first that fails, faults or runs out of time ends the run.  One JSON line per shape is printed and
appended to the record (default profiles/hand_collision.jsonl).  Needs a GPU: there is no fallback.

  python tools/hand_collision.py [--reps 7] [--rows 4096,16384,65536] [--kinds gpis,mesh] [--urdf PATH] [--out PATH]
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

KW = dict(m_obj=0.005, m_self=0.002, m_floor=0.01, w_obj=2.0, w_self=3.0, w_floor=0.5)


def model(urdf, device):
    from compliancedex_amd.hand import HandSpheres
    if urdf:
        return HandSpheres.from_urdf(urdf, robot="allegro", device=device)
    with open(os.path.join(REPO, "tests", "golden", "spheres_allegro.json")) as f:
        d = json.load(f)
    spheres = {}
    for link, c, r in zip(d["links"], d["centers"], d["radii"]):
        spheres.setdefault(link, []).append((c, r))
    return HandSpheres("allegro", spheres, device=device)


def the_object(kind, device):
    import numpy as np
    import torch
    from compliancedex_amd import PreparedMesh
    from compliancedex_amd.workloads import DATA, stored_gpis, surface_center
    if kind == "gpis":
        g = stored_gpis("banana", device)
        return g, surface_center(g)
    faces = torch.from_numpy(np.load(os.path.join(DATA, "meshes", "banana_faces.npy")).astype(np.float32)).to(device)
    return PreparedMesh(faces.reshape(-1, 3, 3)), np.load(os.path.join(DATA, "banana_center.npy"))


def inputs(hs, center, E, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    q = hs.rest_q[None] + 0.3 * rng.standard_normal((E, hs.desc.n_dofs))
    palm = np.concatenate([center[None] + rng.uniform(-0.1, 0.1, (E, 3)), rng.uniform(-np.pi, np.pi, (E, 3))], 1)
    return q, palm


def _axis_rot(axis, th):
    import torch
    c, s = torch.cos(th), torch.sin(th)
    A = torch.zeros(th.shape[0], 3, 3, dtype=th.dtype, device=th.device)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    A[:, axis, axis] = 1.0
    A[:, i, i] = c
    A[:, j, j] = c
    A[:, i, j] = -s
    A[:, j, i] = s
    return A


def torch_centers(hs, tables, q, palm):
    """The rule of cdx_hand_spheres with torch operators in float64 → centres [E, S, 3]."""
    import torch
    F, tb, body, local = tables
    E = q.shape[0]
    R = [torch.eye(3, dtype=q.dtype, device=q.device).expand(E, 3, 3)]
    t = [torch.zeros(E, 3, dtype=q.dtype, device=q.device)]
    for i in range(1, hs.desc.n_bodies):
        b = hs.desc.bodies[i]
        t.append(t[b.parent] + R[b.parent] @ tb[i])
        Rn = R[b.parent] @ F[i]
        if b.dof >= 0:
            Rn = Rn @ _axis_rot(b.axis, float(b.sign) * q[:, b.dof])
        R.append(Rn)
    R, t = torch.stack(R, 1), torch.stack(t, 1)
    ch = (R[:, body] @ local[None, :, :, None]).squeeze(-1) + t[:, body]
    Rp = (_axis_rot(0, palm[:, 3]) @ _axis_rot(1, palm[:, 4])) @ _axis_rot(2, palm[:, 5])
    return (Rp[:, None] @ ch[..., None]).squeeze(-1) + palm[:, None, :3]


def torch_cost(tables, centers, dist, gdist, floor_z):
    """The rule of cdx_hand_cost with torch operators (the distance enters as d + ∇d·(c − c₀)) → cost [E]."""
    import torch
    r, pa, pb = tables
    d = dist + (gdist * (centers - centers.detach())).sum(-1)
    cost = KW["w_obj"] * 0.5 * (torch.clamp(r + KW["m_obj"] - d, min=0.0) ** 2).sum(1)
    rho = (centers[:, pa] - centers[:, pb]).norm(dim=-1)
    cost = cost + KW["w_self"] * 0.5 * (torch.clamp(r[pa] + r[pb] + KW["m_self"] - rho, min=0.0) ** 2).sum(1)
    h = centers[:, :, 2] - floor_z
    return cost + KW["w_floor"] * 0.5 * (torch.clamp(r + KW["m_floor"] - h, min=0.0) ** 2).sum(1)


def host_seconds(hs, q, palm, dist, gdist, floor_z):
    """Seconds of the host build's spheres + cost + pull-back on one core."""
    import numpy as np
    from compliancedex_amd import _host, _native as N
    lib, p = _host.load(), _host.ptr
    S, Pn, E = hs.n_spheres, len(hs.pairs), q.shape[0]
    buf = np.zeros(lib.cdxh_hand_bytes(S, Pn), np.uint8)
    h = N.CdxHand()
    assert lib.cdxh_hand_prepare(hs.desc.n_bodies, S, p(hs.local), p(hs.radius), p(hs.body), Pn, p(hs.pairs), p(buf),
                                 h) == 0
    par = N.CdxHandParams()
    for k, v in KW.items():
        setattr(par, k, v)
    par.floor_z, par.floor_on = floor_z, 1
    pp, po = np.ascontiguousarray(palm[:, :3]), np.ascontiguousarray(palm[:, 3:])
    poses, cen = np.empty((E, hs.desc.n_bodies, 12), np.float32), np.empty((E, S, 3))
    cost, depth, worst, g = np.empty(E), np.empty((E, 3)), np.empty((E, 3), np.int32), np.empty((E, S, 3))
    g_q, g_pp, g_po = np.empty((E, hs.desc.n_dofs)), np.empty((E, 3)), np.empty((E, 3))
    t = time.perf_counter()
    rc = lib.cdxh_hand_spheres(hs.desc, h, E, p(q), p(pp), p(po), p(poses), p(cen))
    rc |= lib.cdxh_hand_cost(h, par, E, p(cen), p(dist), p(gdist), p(cost), p(depth), p(worst), p(g))
    rc |= lib.cdxh_hand_pullback(hs.desc, h, E, p(poses), p(g), p(po), p(g_q), p(g_pp), p(g_po))
    dt = time.perf_counter() - t
    assert rc == 0
    return dt


def run_shape(kind, E, args):
    import numpy as np
    import torch
    from compliancedex_amd import hand_collision
    from compliancedex_amd.hand import cost_launch, object_distance, pullback_launch, spheres_launch
    from compliancedex_amd import _native as N
    dev = torch.device("cuda")
    hs = model(args.urdf, dev)
    obj, center = the_object(kind, dev)
    floor_z = float(center[2]) - 0.05
    qh, ph = inputs(hs, center, E)
    q, palm = torch.from_numpy(qh).to(dev), torch.from_numpy(ph).to(dev)
    pp, po = palm[:, :3].contiguous(), palm[:, 3:].contiguous()
    S = hs.n_spheres
    par = N.CdxHandParams()
    for k, v in KW.items():
        setattr(par, k, v)
    par.floor_z, par.floor_on = floor_z, 1
    f64 = dict(dtype=torch.float64, device=dev)
    chain = (torch.tensor([list(hs.desc.bodies[i].F) for i in range(hs.desc.n_bodies)], **f64).view(-1, 3, 3),
             torch.tensor([list(hs.desc.bodies[i].t) for i in range(hs.desc.n_bodies)], **f64),
             torch.from_numpy(hs.body.astype(np.int64)).to(dev), torch.from_numpy(hs.local.astype(np.float64)).to(dev))
    pairs = torch.from_numpy(hs.pairs.astype(np.int64)).to(dev)
    ctab = (torch.from_numpy(hs.radius).to(dev), pairs[:, 0].contiguous(), pairs[:, 1].contiguous())
    poses, centers = spheres_launch(hs, q, pp, po)
    dist, gdist = object_distance(obj, centers.reshape(-1, 3))
    dist, gdist = dist.reshape(E, S).contiguous(), gdist.reshape(E, S, 3).contiguous()
    g = cost_launch(hs, par, centers, dist, gdist)[3]

    def end_to_end():
        qq, pl = q.clone().requires_grad_(True), palm.clone().requires_grad_(True)
        cost, _ = hand_collision(hs, qq, pl, obj, floor_z=floor_z, **KW)
        cost.sum().backward()
        return cost.detach(), qq.grad, pl.grad

    def torch_end_to_end():
        qq, pl = q.clone().requires_grad_(True), palm.clone().requires_grad_(True)
        c = torch_centers(hs, chain, qq, pl)
        d, gd = object_distance(obj, c.detach().reshape(-1, 3))
        cost = torch_cost(ctab, c, d.reshape(E, S), gd.reshape(E, S, 3), floor_z)
        cost.sum().backward()
        return cost.detach(), qq.grad, pl.grad

    paths = {"spheres": lambda: spheres_launch(hs, q, pp, po),
             "cost": lambda: cost_launch(hs, par, centers, dist, gdist),
             "pullback": lambda: pullback_launch(hs, poses, g, po),
             "query": lambda: object_distance(obj, centers.reshape(-1, 3)),
             "hand_collision": end_to_end, "torch": torch_end_to_end}
    for f in paths.values():  # warm-up: code objects, allocator blocks
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(args.reps):
        for n, f in paths.items():
            ms[n].append(event_ms(f)[0])
    rec = {"kind": kind, "E": E, "S": S, "pairs": len(hs.pairs), "bodies": hs.desc.n_bodies,
           **{n: stats(v) for n, v in ms.items()}}
    a, b = end_to_end(), torch_end_to_end()
    rec["torch_rel_diff"] = [float((x - y).abs().max() / y.abs().max().clamp(min=1e-300)) for x, y in zip(a, b)]
    rec["active_rows"] = round(float((a[0] > 0).double().mean()), 4)
    rec["torch_over_kernels"] = round(rec["torch"]["median_ms"] / rec["hand_collision"]["median_ms"], 2)
    if E <= args.host_rows:
        sec = host_seconds(hs, qh, ph, dist.cpu().numpy(), gdist.cpu().numpy(), floor_z)
        rec["host_one_core_ms"] = round(sec * 1e3, 2)
        three = sum(rec[k]["median_ms"] for k in ("spheres", "cost", "pullback"))
        rec["host_over_three_kernels"] = round(sec * 1e3 / three, 1)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--kinds", default="gpis,mesh")
    ap.add_argument("--kind", default=None, help="child mode: one shape in this process (with --rows one size)")
    ap.add_argument("--urdf", default=None, help="an Allegro URDF whose collision primitives give the spheres")
    ap.add_argument("--host-rows", type=int, default=16384)
    ap.add_argument("--step-seconds", type=int, default=150, help="time limit of each shape's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hand_collision.jsonl"))
    args = ap.parse_args()
    rows = [int(v) for v in args.rows.split(",")]
    if args.kind is None:
        for kind in args.kinds.split(","):
            for E in rows:
                cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--kind",
                       kind, "--rows", str(E), "--reps", str(args.reps), "--host-rows", str(args.host_rows), "--out",
                       args.out] + (["--urdf", args.urdf] if args.urdf else [])
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    raise SystemExit(f"kind {kind} E={E} ended with status {rc}: nothing more is started")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/hand_collision.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = run_shape(args.kind, rows[0], args)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
