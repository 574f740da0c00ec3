"""From a mesh to a cloud of its whole surface, on MI355X.

Every run of the reference on a mesh object opens with open3d's ``mesh.sample_points_poisson_disk(4096)``
(optimize_pregrasp.py:887); the script behind its stored GPIS states does the same with 64 and 128 points
(gpis.py:199-263).  Here the uniform sample is cdx_sample_prepare / cdx_sample_draw (csrc/cdx_sample.hip, the rule in
csrc/cdx_sample.h: integer area weights, Philox4x32-10 keyed by ``seed`` and counted by the sample's index) and the
Poisson-disk cloud is a farthest-point sample (cdx_fps) of ``init_factor`` times as many uniform samples.

Parity with open3d is unpinned and not attempted (open3d is not a dependency): its uniform sampler draws from its own
generator and its Poisson-disk sampler is weighted sample elimination; both clouds here are reproducible from ``seed``
alone, on any launch shape.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N


def _require_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what} must be a CUDA (ROCm) tensor: compliancedex_amd has no CPU path")


def table_capacity():
    """Largest mesh (faces) whose table the draw's "table" mode keeps whole in LDS."""
    return int(N.load().cdx_sample_table_capacity())


class SurfaceSampler:
    """The sampling table of a mesh (cdx_sample_prepare): ``face_vertices`` [F, 3, 3] float32 or float64 on the
    device.  The handle owns a private copy of the faces.  Building it reads one word back (a wait on the current
    stream, once per mesh) and raises ValueError for a mesh none of whose faces has area.  Faces with a non-finite
    coordinate, no area, or less than 2⁻³² of the largest face's area are never drawn."""

    def __init__(self, face_vertices):
        _require_cuda(face_vertices, "face vertices")
        if face_vertices.dim() != 3 or tuple(face_vertices.shape[1:]) != (3, 3) or face_vertices.shape[0] == 0:
            raise ValueError(f"face vertices must be a non-empty [F, 3, 3] tensor, got {tuple(face_vertices.shape)}")
        if face_vertices.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"face vertices must be float32 or float64, got {face_vertices.dtype}")
        lib = N.load()
        self.faces = face_vertices.detach().contiguous().clone()
        F, dev = self.faces.shape[0], self.faces.device
        need = lib.cdx_sample_prepare_workspace(F)
        if need == 0:
            raise ValueError(f"cdx_sample_prepare takes no mesh of {F} faces")
        self._dtype = N.DTYPE_F32 if self.faces.dtype == torch.float32 else N.DTYPE_F64
        self.cdf = torch.empty(F, dtype=torch.int64, device=dev)  # the bits are uint64
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        N.check(lib.cdx_sample_prepare(N.ptr(self.faces), self._dtype, F, N.ptr(workspace), N.ptr(self.cdf),
                                       N.ptr(info), N.stream_ptr(dev)), "cdx_sample_prepare")
        if int(info.item()) != 0:
            raise ValueError("mesh has no face with a finite, non-zero area: nothing to sample")

    @property
    def num_faces(self):
        return self.faces.shape[0]

    def draw(self, K, seed=0, first=0, want_face=False, want_normal=False, want_bary=False, mode="auto"):
        """Samples ``first`` … ``first + K − 1`` of the stream ``seed`` (both in 0 … 2⁶⁴ − 1): points [K, 3] float64
        on the device, uniform over the surface; with any ``want_*`` a tuple of the points and, in this order, the
        requested ones of face [K] int64, normal [K, 3] (the face's unit normal, by its winding) and bary [K, 2]
        ((u, v): point = v0 + u·(v1 − v0) + v·(v2 − v0)).  A sample depends on (seed, its index) only: the first k of a
        K-sample are the k-sample, and ranks share a stream through ``first``.  ``mode``: "table" (the whole table in
        LDS, up to ``table_capacity()`` faces), "splitters" or "auto"; all give the same bits.  No host
        synchronisation."""
        K, seed, first = int(K), int(seed), int(first)
        if K < 0:
            raise ValueError(f"K must be ≥ 0, got {K}")
        if not (0 <= seed < 2 ** 64 and 0 <= first < 2 ** 64):
            raise ValueError("seed and first must be in 0 … 2⁶⁴ − 1")
        if mode not in N.SAMPLE_MODES:
            raise ValueError(f"mode must be one of {sorted(N.SAMPLE_MODES)}, got {mode!r}")
        if mode == "table" and self.num_faces > table_capacity():
            raise ValueError(f"mode 'table' takes up to {table_capacity()} faces, the mesh has {self.num_faces}")
        dev = self.faces.device
        points = torch.empty(K, 3, dtype=torch.float64, device=dev)
        face = torch.empty(K, dtype=torch.int64, device=dev) if want_face else None
        normal = torch.empty(K, 3, dtype=torch.float64, device=dev) if want_normal else None
        bary = torch.empty(K, 2, dtype=torch.float64, device=dev) if want_bary else None
        N.check(N.load().cdx_sample_draw(N.ptr(self.faces), self._dtype, self.num_faces, N.ptr(self.cdf), seed, first,
                                         K, N.SAMPLE_MODES[mode], N.ptr(points), N.ptr(face), N.ptr(bary),
                                         N.ptr(normal), N.stream_ptr(dev)), "cdx_sample_draw")
        extra = tuple(x for x in (face, normal, bary) if x is not None)
        return (points,) + extra if extra else points


def surface_sampler(mesh, device="cuda"):
    """The ``SurfaceSampler`` of ``mesh``: a SurfaceSampler itself, a ``PreparedMesh`` (its sampler is built on first
    use and kept, like its ray records), a ``TriangleMesh`` (its float64 vertices, uploaded to ``device``; nothing is
    kept, ``scale`` changes the mesh in place) or an [F, 3, 3] device tensor."""
    from .torchsdf import PreparedMesh
    if isinstance(mesh, SurfaceSampler):
        return mesh
    if isinstance(mesh, PreparedMesh):
        if mesh._sampler is None:
            mesh._sampler = SurfaceSampler(mesh.faces)
        return mesh._sampler
    if hasattr(mesh, "vertices") and hasattr(mesh, "triangles"):
        v, tri = np.asarray(mesh.vertices, dtype=np.float64), np.asarray(mesh.triangles, dtype=np.int64)
        if tri.ndim != 2 or tri.shape[1] != 3 or len(tri) == 0:
            raise ValueError("mesh has no triangles")
        return SurfaceSampler(torch.from_numpy(v[tri.reshape(-1)].reshape(len(tri), 3, 3)).to(device))
    return SurfaceSampler(mesh)


def sample_points_uniformly(mesh, number_of_points, seed=0, first=0, want_face=False, want_normal=False,
                            want_bary=False, device="cuda"):
    """open3d's ``TriangleMesh.sample_points_uniformly`` on the device: ``number_of_points`` points [K, 3] float64,
    uniform over the surface of ``mesh`` (see ``surface_sampler`` for what a mesh may be), and what
    ``SurfaceSampler.draw`` returns with ``want_*``.  Reproducible from ``seed``; parity with open3d's generator is
    unpinned and not attempted."""
    return surface_sampler(mesh, device).draw(number_of_points, seed, first, want_face, want_normal, want_bary)


def sample_points_poisson_disk(mesh, number_of_points, init_factor=5, seed=0, want_face=False, want_normal=False,
                               device="cuda"):
    """The cloud the reference takes with open3d's ``sample_points_poisson_disk(number_of_points, init_factor)``:
    ``init_factor·number_of_points`` uniform samples, then a farthest-point sample of them beginning at row 0 (cdx_fps).
    Points [K, 3] float64 in selection order (every prefix is itself such a cloud), and with ``want_face`` /
    ``want_normal`` a tuple with the face index [K] / unit normal [K, 3] of each chosen point.  open3d eliminates
    samples by a weighted priority instead; parity with it is unpinned and not attempted.  No host synchronisation
    beyond the sampler's."""
    from . import pointcloud as PC
    K, init_factor = int(number_of_points), int(init_factor)
    if K < 1 or init_factor < 1:
        raise ValueError("number_of_points and init_factor must be ≥ 1")
    drawn = surface_sampler(mesh, device).draw(init_factor * K, seed, 0, want_face, want_normal)
    uniform = drawn[0] if isinstance(drawn, tuple) else drawn
    sel, _, points = PC.fps(uniform, K, 0, gather=True)
    extra = tuple(x[sel] for x in drawn[1:]) if isinstance(drawn, tuple) else ()
    return (points,) + extra if extra else points
