"""Generates the lattice-field fixtures by running the REFERENCE itself on CPU.

Container-only (needs the reference checkout ``_refload.py`` points at): ``python tests/golden/make_field_golden.py``.
Nothing from the reference is copied; it is imported and executed via ``_refload.py``, as ``make_golden.py`` does.

  field_<state>_s<steps>.npz
      mean, std, normal   GPIS.get_visualization_data(lb, ub, steps) (gpis.py:113-125), float32
      lb, ub, steps       its arguments (the boxes are unequal along x, y, z so that a swapped axis shows)
      pts_np, nrm_np      GPIS.topcd (gpis.py:127-150) on those numpy arrays
      pts_t, nrm_t        GPIS.topcd on the same arrays as tensors: the reference then reads mean and normal
                          flipped along k (:130-133) while the points stay unflipped
      n_internal          cells with mean < 0
      min_abs_mean        min |mean| over the lattice: asserted ≥ 1e-6 here, so a 1e-8 parity error of a mean
                          cannot flip a sign (the surface tests compare cell sets exactly)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

CASES = [
    ("banana", [-0.10, -0.06, -0.08], [0.12, 0.07, 0.05], 13),
    ("mug", [-0.07, -0.09, -0.06], [0.08, 0.06, 0.09], 9),
]


def load_state(ns, name):
    g = ns.gpis.GPIS(0.08, 1.0)
    cwd = os.getcwd()
    os.chdir(ns.ref)
    try:
        g.load_state_data(f"{name}_state")
    finally:
        os.chdir(cwd)
    return g


def gen_field(ns, state, lb, ub, steps):
    torch = ns.torch
    g = load_state(ns, state)
    with torch.no_grad():
        mean, std, normal, _, _ = g.get_visualization_data(lb, ub, steps=steps)
    assert mean.dtype == np.float32 and normal.dtype == np.float32
    assert np.isfinite(mean).all() and np.isfinite(std).all() and np.isfinite(normal).all()
    min_abs = float(np.abs(mean).min())
    assert min_abs >= 1e-6, (state, min_abs)
    pts_np, nrm_np = g.topcd(mean, normal, lb, ub, steps=steps)
    pts_t, nrm_t = g.topcd(torch.from_numpy(mean), torch.from_numpy(normal), lb, ub, steps=steps)
    assert pts_np.dtype == np.float64 and pts_np.shape[1] == 3 and len(pts_np) > 0 and len(pts_t) > 0
    # steps = 2 has no interior cell: (0, 3) outputs
    p2, n2 = g.topcd(mean[:2, :2, :2], normal[:2, :2, :2], lb, ub, steps=2)
    assert p2.shape == (0, 3) and n2.shape == (0, 3)
    name = f"field_{state}_s{steps}.npz"
    np.savez_compressed(os.path.join(HERE, name), mean=mean, std=std, normal=normal, lb=np.asarray(lb, np.float64),
                        ub=np.asarray(ub, np.float64), steps=np.int64(steps), pts_np=pts_np,
                        nrm_np=np.ascontiguousarray(nrm_np), pts_t=pts_t, nrm_t=np.ascontiguousarray(nrm_t),
                        n_internal=np.int64((mean < 0).sum()), min_abs_mean=np.float64(min_abs))
    print(f"{name}: {len(pts_np)} surface points ({len(pts_t)} flipped) from {int((mean < 0).sum())} internal cells, "
          f"min |mean| {min_abs:.2e}, {os.path.getsize(os.path.join(HERE, name))} bytes")


def main():
    ns = _refload.load()
    for case in CASES:
        gen_field(ns, *case)


if __name__ == "__main__":
    main()
