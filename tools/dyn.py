"""Rigid-body dynamics (cdx_dyn_inverse, cdx_dyn_inertia, cdx_dyn_forward) timed on the GPU: E = 4096, 16 384 and
65 536 rows of the Allegro hand (22 bodies, D = 16) and of iiwa7_allegro (29 bodies, D = 23), q uniform in the joint
box, q̇, q̈, f ~ N(0, 1), float64 I/O.

Per shape and entry: the one-launch kernel through ``DifferentiableRobotModel`` (which allocates its output); a torch
statement of the same rule on the device — the recursive Newton–Euler sweeps of csrc/cdx_dyn.h written with batched torch
operators, one small launch per body and operation, H by D such passes, the forward dynamics by ``torch.linalg.solve``
—; and the host build of the rule on one core (cdxh_dyn_*, wall clock) up to --host-rows.  Besides the times the record
keeps how far the torch statement is from the kernel (max|a − b| / max|b|) and each kernel's rows per workgroup.

Device times are HIP events around one call after a warm-up call of every path, the paths alternating within each
repeat; the median of --reps and the spread (max − min)/median are kept.

Without --robot the tool is the driver: every shape runs in a child process of its own under ``timeout``, one after the
other, and the first that fails, faults or runs out of time ends the run.  One JSON line per shape is printed and
appended to the record (default profiles/dyn.jsonl).  Needs a GPU: there is no fallback.

  python tools/dyn.py [--reps 7] [--rows 4096,16384,65536] [--robots allegro,iiwa7_allegro] [--out PATH]
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


class TorchDynamics:
    """The rule of csrc/cdx_dyn.h with torch operators on the device (float64; float32 sines and cosines)."""

    def __init__(self, rm, device):
        import torch
        self.torch = torch
        d, dy = rm._dyn_descriptor(None, None), rm.chain.dynamics_descriptor()
        self.n, self.D = d.n_bodies, d.n_dofs
        t = lambda v: torch.tensor(v, dtype=torch.float64, device=device)  # noqa: E731
        self.bodies = []
        for i in range(self.n):
            b = d.bodies[i]
            x = list(dy.inertia[i])
            S = [0.0, 0.0, 0.0]
            if b.dof >= 0:
                S[b.axis] = float(b.sign)
            self.bodies.append(dict(parent=int(b.parent), dof=int(b.dof), axis=int(b.axis), sign=float(b.sign),
                                    F=t(list(b.F)).view(3, 3), p=t(list(b.t)), S=t(S), m=float(dy.mass[i]),
                                    mc=t(list(dy.mcom[i])),
                                    I=t([[x[0], x[1], x[2]], [x[1], x[3], x[4]], [x[2], x[4], x[5]]])))
        self.damping = t(list(dy.damping)[:self.D])

    def poses(self, q):
        torch = self.torch
        B = q.shape[0]
        out = [None]
        for b in self.bodies[1:]:
            if b["dof"] < 0:
                out.append(b["F"].expand(B, 3, 3))
                continue
            th = (b["sign"] * q[:, b["dof"]]).float()
            c, s = torch.cos(th).double(), torch.sin(th).double()
            A = torch.zeros(B, 3, 3, dtype=torch.float64, device=q.device)
            u, v = [(1, 2), (2, 0), (0, 1)][b["axis"]]
            A[:, b["axis"], b["axis"]] = 1.0
            A[:, u, u], A[:, v, v], A[:, u, v], A[:, v, u] = c, c, -s, s
            out.append(b["F"] @ A)
        return out

    def inverse(self, E, qd, qdd, g):
        """tau [B, D] without damping from the joint poses E, q̇, q̈ (None: zero) and the gravity g [3]."""
        torch = self.torch
        B = E[1].shape[0]
        dev = E[1].device
        zero = torch.zeros(B, 3, dtype=torch.float64, device=dev)
        cross = lambda a, b: torch.cross(a, b.expand_as(a) if b.ndim == 1 else b, dim=-1)  # noqa: E731
        tv = lambda M, v: torch.einsum("bji,bj->bi", M, v)  # noqa: E731
        st = [(zero, zero, zero, (-g).expand(B, 3))]
        for i in range(1, self.n):
            b = self.bodies[i]
            w0, v0, al0, a0 = st[b["parent"]]
            wj = b["S"] * qd[:, b["dof"], None] if (b["dof"] >= 0 and qd is not None) else zero
            zj = b["S"] * qdd[:, b["dof"], None] if (b["dof"] >= 0 and qdd is not None) else zero
            w = tv(E[i], w0) + wj
            v = tv(E[i], v0 + torch.cross(w0, b["p"].expand(B, 3), dim=-1))
            al = tv(E[i], al0) + zj + torch.cross(w, wj, dim=-1)
            a = tv(E[i], a0 + torch.cross(al0, b["p"].expand(B, 3), dim=-1)) + torch.cross(v, wj, dim=-1)
            st.append((w, v, al, a))
        nn, ff = [None] * self.n, [None] * self.n
        for i in range(1, self.n):
            b = self.bodies[i]
            w, v, al, a = st[i]
            mc = b["mc"].expand(B, 3)
            hn = w @ b["I"].T + cross(mc, v)
            hf = b["m"] * v - cross(mc, w)
            nn[i] = al @ b["I"].T + cross(mc, a) + cross(w, hn) + cross(v, hf)
            ff[i] = b["m"] * a - cross(mc, al) + cross(w, hf)
        tau = torch.zeros(B, self.D, dtype=torch.float64, device=dev)
        for i in range(self.n - 1, 0, -1):
            b = self.bodies[i]
            if b["dof"] >= 0:
                tau[:, b["dof"]] = b["sign"] * nn[i][:, b["axis"]]
            if b["parent"] > 0:
                Ef = torch.einsum("bij,bj->bi", E[i], ff[i])
                nn[b["parent"]] = nn[b["parent"]] + torch.einsum("bij,bj->bi", E[i], nn[i]) + cross(b["p"].expand(B, 3), Ef)
                ff[b["parent"]] = ff[b["parent"]] + Ef
        return tau

    def inverse_dynamics(self, q, qd, qdd):
        g = self.torch.tensor([0.0, 0.0, -9.81], dtype=self.torch.float64, device=q.device)
        return self.inverse(self.poses(q), qd, qdd, g) + self.damping * qd

    def inertia(self, q, E=None):
        torch = self.torch
        E = self.poses(q) if E is None else E
        g = torch.zeros(3, dtype=torch.float64, device=q.device)
        eye = torch.eye(self.D, dtype=torch.float64, device=q.device)
        return torch.stack([self.inverse(E, None, eye[j].expand(q.shape[0], self.D), g) for j in range(self.D)], dim=2)

    def forward_dynamics(self, q, qd, f):
        torch = self.torch
        E = self.poses(q)
        g = torch.tensor([0.0, 0.0, -9.81], dtype=torch.float64, device=q.device)
        nle = self.inverse(E, qd, None, g)
        return torch.linalg.solve(self.inertia(q, E), (f - nle).unsqueeze(2)).squeeze(2)


def host_ms(rm, q, qd, qdd, f):
    """Milliseconds of the three host entries on one core."""
    import ctypes
    import numpy as np
    from compliancedex_amd import _host, _native as N
    lib, p = _host.load(), _host.ptr
    desc, dy = rm._dyn_descriptor(None, None), ctypes.byref(rm.chain.dynamics_descriptor())
    q, qd, qdd, f = (np.ascontiguousarray(t.cpu().numpy()) for t in (q, qd, qdd, f))
    B, D = q.shape
    out, H = np.empty_like(q), np.empty((B, D, D))
    res = {}
    t = time.perf_counter()
    rc = lib.cdxh_dyn_inverse(desc, dy, B, p(q), p(qd), p(qdd), N.DTYPE_F64, 1, 1, None, 0, None, p(out))
    res["inverse"] = (time.perf_counter() - t) * 1e3
    assert rc == 0
    t = time.perf_counter()
    rc = lib.cdxh_dyn_inertia(desc, dy, B, p(q), N.DTYPE_F64, p(H))
    res["inertia"] = (time.perf_counter() - t) * 1e3
    assert rc == 0
    t = time.perf_counter()
    rc = lib.cdxh_dyn_forward(desc, dy, B, p(q), p(qd), p(f), N.DTYPE_F64, 1, 0, None, 0, p(out))
    res["forward"] = (time.perf_counter() - t) * 1e3
    assert rc == 0
    return res


def run_shape(robot, E, args):
    import torch
    from compliancedex_amd import DifferentiableRobotModel, _native as N
    from compliancedex_amd.ik import joint_box
    rm = DifferentiableRobotModel(robot, device="cuda")
    lower, upper = joint_box(rm.get_joint_limits())
    lo, hi = torch.tensor(lower, dtype=torch.float64), torch.tensor(upper, dtype=torch.float64)
    g = torch.Generator().manual_seed(0)
    D = rm._n_dofs
    q = (lo + (hi - lo) * torch.rand(E, D, generator=g, dtype=torch.float64)).cuda()
    qd, qdd, f = (torch.randn(E, D, generator=g, dtype=torch.float64).cuda() for _ in range(3))
    td = TorchDynamics(rm, "cuda")
    paths = {"inverse": lambda: rm.compute_inverse_dynamics(q, qd, qdd),
             "inverse_torch": lambda: td.inverse_dynamics(q, qd, qdd),
             "inertia": lambda: rm.compute_lagrangian_inertia_matrix(q),
             "inertia_torch": lambda: td.inertia(q),
             "forward": lambda: rm.compute_forward_dynamics(q, qd, f),
             "forward_torch": lambda: td.forward_dynamics(q, qd, f)}
    for fn in paths.values():  # warm-up: code objects, allocator blocks
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in paths}
    for _ in range(args.reps):
        for n, fn in paths.items():
            ms[n].append(event_ms(fn)[0])
    n_bodies = len(rm.chain.bodies)
    rec = {"robot": robot, "E": E, "D": D, "bodies": n_bodies, **{n: stats(v) for n, v in ms.items()}}
    lib = N.load()
    for k, name in enumerate(("inverse", "inertia", "forward")):
        a, b = paths[name](), paths[name + "_torch"]()
        rec[name + "_torch_rel_diff"] = float((a - b).abs().max() / b.abs().max())
        rec[name + "_torch_over_kernel"] = round(rec[name + "_torch"]["median_ms"] / rec[name]["median_ms"], 1)
        rec[name + "_rows_per_block"] = int(lib.cdx_dyn_rows_per_block(n_bodies, D, k))
    if E <= args.host_rows:
        for name, v in host_ms(rm, q, qd, qdd, f).items():
            rec[name + "_host_one_core_ms"] = round(v, 2)
            rec[name + "_host_over_kernel"] = round(v / rec[name]["median_ms"], 1)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--robots", default="allegro,iiwa7_allegro")
    ap.add_argument("--robot", default=None, help="child mode: one shape in this process (with --rows one size)")
    ap.add_argument("--host-rows", type=int, default=65536)
    ap.add_argument("--step-seconds", type=int, default=150, help="time limit of each shape's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dyn.jsonl"))
    args = ap.parse_args()
    rows = [int(v) for v in args.rows.split(",")]
    if args.robot is None:
        for robot in args.robots.split(","):
            for E in rows:
                cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--robot",
                       robot, "--rows", str(E), "--reps", str(args.reps), "--host-rows", str(args.host_rows), "--out",
                       args.out]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    raise SystemExit(f"{robot} E={E} ended with status {rc}: nothing more is started")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/dyn.py needs a GPU: a CPU run gives no time")
    from compliancedex_amd import _native
    _native.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = run_shape(args.robot, rows[0], args)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
