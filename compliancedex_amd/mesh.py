"""What goes with ``GPIS.tomesh`` / ``GPIS.surface_mesh``: the lattice edges behind the mesh's vertices, their
refinement along those edges, and the ways from the mesh into the triangle-mesh half of the package.

A vertex of the marching-tetrahedra mesh (csrc/cdx_mesh.h) sits on one lattice edge, named by its key 7c + d: the
lower node c = (i·s + j)·s + k and one of seven offsets d.  ``EdgeRefiner`` moves every vertex along its own edge
towards the zero of a field by bracketed regula falsi — plain torch ops over the keys, with the field as a callable, so
it runs on any device; the faces never change.  ``GPIS.surface_mesh`` runs the same rule as a kernel
(cdx_gpis_mesh_refine_init / _step): the torch ops of a step cost more than the GPIS mean call they surround.
"""
from __future__ import annotations

import numpy as np
import torch

EDGE_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))  # (i, j, k) of type d


def edge_ends(edges, steps):
    """Lattice indices of both ends of the edges with keys ``edges`` [V]: (a [V, 3], b [V, 3]) int64 (i, j, k)."""
    c = torch.div(edges, 7, rounding_mode="floor")
    d = edges - 7 * c
    k = c % steps
    r = torch.div(c, steps, rounding_mode="floor")
    a = torch.stack([torch.div(r, steps, rounding_mode="floor"), r % steps, k], dim=1)
    off = torch.tensor(EDGE_OFFSETS, dtype=torch.int64, device=edges.device)
    return a, a + off[d]


def edge_points(edges, axes, steps):
    """Positions of both ends: (Pa [V, 3], Pb [V, 3]); ``axes`` [3, steps] are the point axes (x, y, z) and node
    (i, j, k) sits at (x[j], y[i], z[k])."""
    a, b = edge_ends(edges, steps)
    pa = torch.stack([axes[0][a[:, 1]], axes[1][a[:, 0]], axes[2][a[:, 2]]], dim=1)
    pb = torch.stack([axes[0][b[:, 1]], axes[1][b[:, 0]], axes[2][b[:, 2]]], dim=1)
    return pa, pb


class EdgeRefiner:
    """Bracketed regula falsi of every vertex along its lattice edge.  The state per vertex is (ta, fa, tb, fb), the
    bracket's ends as parameters of the edge and the field there, beginning at the edge's ends with the lattice's
    values; ``t`` is the vertex, Pa + t·(Pb − Pa).  ``step(mean_fn)`` evaluates ``mean_fn`` ([V, 3] → [V]) at the
    vertices, replaces the bracket end whose ``inside`` (value < 0) is the vertex's, and sets
    t = ta + (tb − ta)·fa/(fa − fb), the midpoint when that is non-finite or outside [ta, tb]; a vertex whose value is
    non-finite is left alone.  Vertices never leave their edge."""

    def __init__(self, edges, lattice_mean, axes):
        steps = lattice_mean.shape[0]
        axes = torch.as_tensor(axes, dtype=torch.float64, device=edges.device)
        f = lattice_mean.reshape(-1).to(torch.float64)
        a, b = edge_ends(edges, steps)
        self.pa, self.pb = edge_points(edges, axes, steps)
        self.fa = f[(a[:, 0] * steps + a[:, 1]) * steps + a[:, 2]]
        self.fb = f[(b[:, 0] * steps + b[:, 1]) * steps + b[:, 2]]
        self.ta = torch.zeros_like(self.fa)
        self.tb = torch.ones_like(self.fa)
        self.t = self._secant()

    def _secant(self):
        t = self.ta + (self.tb - self.ta) * (self.fa / (self.fa - self.fb))
        ok = torch.isfinite(t) & (t >= self.ta) & (t <= self.tb)
        return torch.where(ok, t, 0.5 * (self.ta + self.tb))

    def vertices(self):
        return self.pa + self.t.unsqueeze(1) * (self.pb - self.pa)

    def step(self, mean_fn):
        fv = mean_fn(self.vertices()).reshape(-1).to(torch.float64)
        live = torch.isfinite(fv)
        low = live & ((fv < 0) == (self.fa < 0))  # the vertex is on a's side: it becomes the lower end
        high = live & ~low
        self.ta = torch.where(low, self.t, self.ta)
        self.fa = torch.where(low, fv, self.fa)
        self.tb = torch.where(high, self.t, self.tb)
        self.fb = torch.where(high, fv, self.fb)
        self.t = torch.where(live, self._secant(), self.t)
        return fv


def refine_vertices(mean_fn, edges, lattice_mean, axes, steps):
    """The vertices after ``steps`` refinement steps (``EdgeRefiner``)."""
    r = EdgeRefiner(edges, lattice_mean, axes)
    for _ in range(int(steps)):
        r.step(mean_fn)
    return r.vertices()


def mesh_face_vertices(vertices, faces):
    """float32 [F, 3, 3] ``face_vertices`` of a mesh (``index_vertices_by_faces``): what ``compute_sdf``,
    ``PreparedMesh``, ``cast_rays`` and ``render_depth`` take.  numpy arrays or tensors; tensors stay on their device."""
    from .torchsdf import index_vertices_by_faces
    v = torch.as_tensor(vertices)
    f = torch.as_tensor(faces).to(v.device, torch.int64)
    return index_vertices_by_faces(v.to(torch.float32), f).contiguous()


def to_triangle_mesh(vertices, faces):
    """The optimisers' ``TriangleMesh`` (``SDFGraspOptimizer`` / ``KinGraspOptimizer``'s ``object_mesh``) of a mesh."""
    from .optimizers import TriangleMesh

    def host(x):
        return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return TriangleMesh(host(vertices), host(faces))
