"""Helpers shared by test_field_cpu.py and test_gpu_field.py: the host surface extract and the rule in numpy."""
import numpy as np

from tests._host import host, p

F32, F64 = 0, 1  # CDX_DTYPE_*


def point_axes(lb, ub, steps):
    """topcd's float64 point axes (gpis.py:144-146)."""
    return [np.linspace(lb[d], ub[d], steps) for d in range(3)]


def host_extract(mean, normal, steps, flip, axes, capacity=None, dtype=None):
    """cdxh_surface_extract on host arrays: (count, cells, points, normals) with `capacity` rows (default: all)."""
    lib = host()
    mean = np.ascontiguousarray(mean)
    normal = np.ascontiguousarray(normal, dtype=mean.dtype)
    if dtype is None:
        dtype = {np.dtype(np.float32): F32, np.dtype(np.float64): F64}[mean.dtype]
    cap = max(steps - 2, 0) ** 3 if capacity is None else capacity
    cells = np.full(cap, -1, np.int64)
    pts = np.full((cap, 3), -7.0)
    nrm = np.full((cap, 3), -7.0, mean.dtype)
    ax = [np.ascontiguousarray(a, np.float64) for a in axes]
    n = lib.cdxh_surface_extract(p(mean), p(normal), dtype, steps, flip, p(ax[0]), p(ax[1]), p(ax[2]), cap, p(cells),
                                 p(pts), p(nrm))
    return n, cells, pts, nrm


def numpy_rule(mean, flip):
    """The cell rule of csrc/cdx_field.h, vectorised: the boolean mask of surface cells."""
    m = mean[:, :, ::-1] if flip else mean
    internal = m < 0
    mask = np.zeros_like(internal)
    if mean.shape[0] < 3:
        return mask
    c = internal[1:-1, 1:-1, 1:-1]
    open_nb = (~internal[:-2, 1:-1, 1:-1] | ~internal[2:, 1:-1, 1:-1] | ~internal[1:-1, :-2, 1:-1] |
               ~internal[1:-1, 2:, 1:-1] | ~internal[1:-1, 1:-1, :-2] | ~internal[1:-1, 1:-1, 2:])
    mask[1:-1, 1:-1, 1:-1] = c & open_nb
    return mask


def numpy_extract(mean, normal, flip, axes):
    """(cells, points, normals) of the rule, as topcd builds them (gpis.py:143-150)."""
    mask = numpy_rule(mean, flip)
    allp = np.stack(np.meshgrid(*axes, indexing="xy"), axis=3)
    nsrc = normal[:, :, ::-1] if flip else normal
    return np.flatnonzero(mask.reshape(-1)), allp[mask], nsrc[mask]


def salted_mean(rng, steps, dtype):
    """A random mean with NaN, +0.0 and −0.0 cells (none of them internal)."""
    mean = rng.standard_normal((steps, steps, steps)).astype(dtype)
    salt = rng.integers(0, 12, mean.shape)
    mean[salt == 0] = np.nan
    mean[salt == 1] = 0.0
    mean[salt == 2] = -0.0
    return mean
