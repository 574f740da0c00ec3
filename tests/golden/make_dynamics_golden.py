"""Generates the dynamics fixtures by running the REFERENCE's robot model on the CPU.

Container-only (needs the reference checkout ``_refload.REF``): ``python tests/golden/make_dynamics_golden.py``.
Writes ``tests/golden/dyn_{allegro,leap,iiwa7_allegro}.npz``: seeded inputs at B = 16 and the reference's
``compute_inverse_dynamics`` (the four (include_gravity, use_damping) combinations), ``compute_lagrangian_inertia_matrix``
and ``compute_forward_dynamics`` (with and without damping; a clone of ``f`` goes in, the reference writes into it) on
them — results only.  Nothing from the reference is copied; it is imported and executed via ``_refload.py``.

``_refload``'s URDF stand-in reports every link's inertial as absent (FK does not use it), which would make the
reference fall back to mass 1 everywhere.  This script leaves ``_refload.py`` as it is and replaces
``differentiable_robot_model.urdf_utils.URDF`` with a reader that also returns each link's ``<inertial>`` (mass, origin
xyz, the six inertia entries) — the fields ``urdf_utils.py:85-113`` reads.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

B = 16


def _urdf_with_inertials(path):
    robot = _refload._urdf_from_xml_file(path)
    els = {el.get("name"): el for el in ET.parse(path).getroot() if el.tag == "link"}
    for link in robot.links:
        ine = els[link.name].find("inertial")
        if ine is None:
            continue
        org, mass, mat = ine.find("origin"), ine.find("mass"), ine.find("inertia")
        link.inertial = _refload._Obj(
            mass=float(mass.get("value")),
            origin=_refload._Obj(position=_refload._floats(org.get("xyz") if org is not None else None, 3, (0, 0, 0))),
            inertia=_refload._Obj(**{k: float(mat.get(k, 0)) for k in ("ixx", "ixy", "ixz", "iyy", "iyz", "izz")}))
    return robot


def main():
    ref = _refload.load()
    torch = ref.torch
    from differentiable_robot_model import urdf_utils
    urdf_utils.URDF = _refload._Obj(from_xml_file=_urdf_with_inertials)
    for k, (robot, rel) in enumerate(_refload.URDFS.items()):
        with contextlib.redirect_stdout(io.StringIO()) as out:
            model = ref.rm.DifferentiableRobotModel(os.path.join(ref.ref, rel))
        assert "No dynamics information" not in out.getvalue(), robot
        lim = model.get_joint_limits()
        lo = np.array([j["lower"] for j in lim])
        hi = np.array([j["upper"] for j in lim])
        rng = np.random.default_rng(500 + k)
        D = len(lo)
        q = (lo + (hi - lo) * rng.random((B, D))).astype(np.float32)
        qd, qdd, f = (rng.standard_normal((B, D)).astype(np.float32) for _ in range(3))
        t = lambda a: torch.from_numpy(a.copy())  # noqa: E731
        res = dict(q=q, qd=qd, qdd=qdd, f=f)
        with torch.no_grad():
            for g in (0, 1):
                for d in (0, 1):
                    res[f"tau_g{g}_d{d}"] = model.compute_inverse_dynamics(t(q), t(qd), t(qdd), include_gravity=bool(g),
                                                                           use_damping=bool(d)).numpy()
            res["H"] = model.compute_lagrangian_inertia_matrix(t(q)).numpy()
            for d in (0, 1):
                res[f"fd_d{d}"] = model.compute_forward_dynamics(t(q), t(qd), t(f), include_gravity=True,
                                                                 use_damping=bool(d)).numpy()
        path = os.path.join(HERE, f"dyn_{robot}.npz")
        np.savez_compressed(path, **res)
        print(robot, {k: v.shape for k, v in res.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
