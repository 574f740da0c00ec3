"""Helpers shared by test_fps_cpu.py and test_gpu_fps.py: the farthest-point sampling rule of csrc/cdx_fps.h stated in
numpy, the host build (cdxh_fps) and the clouds both files sample."""
import os

import numpy as np

from tests._host import host, p
from tests.conftest import GOLDEN

F32, F64 = 0, 1  # CDX_DTYPE_*


def numpy_fps(X, K, start=0):
    """(sel int64 [K], radius f64 [K], points f64 [K, 3]) of the rule, vectorised over rows.  A float32 cloud is
    widened first; np.argmax returns the smallest index among the maxima."""
    X = np.asarray(X).astype(np.float64)
    finite = np.isfinite(X).all(axis=1)
    dist = np.where(finite, np.inf, -1.0)
    sel = np.empty(K, np.int64)
    radius = np.empty(K, np.float64)
    s = int(start)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(K):
            sel[i] = s
            radius[i] = dist[s]
            d = X - X[s]
            q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            dist = np.where(finite & (q < dist), q, dist)
            s = int(np.argmax(dist))
    return sel, radius, X[sel]


def host_fps(X, K, start=0, dtype=None):
    """cdxh_fps on a [P, 3] or [B, P, 3] host array in its own dtype: (rc, sel, radius, points)."""
    lib = host()
    X = np.ascontiguousarray(X)
    B, P = (X.shape[0], X.shape[1]) if X.ndim == 3 else (1, X.shape[0])
    if dtype is None:
        dtype = {np.dtype(np.float32): F32, np.dtype(np.float64): F64}[X.dtype]
    rows = max(K, 0)
    shape = (B, rows) if X.ndim == 3 else (rows,)
    sel = np.full(shape, -1, np.int64)
    radius = np.full(shape, -7.0)
    points = np.full(shape + (3,), -7.0)
    rc = lib.cdxh_fps(p(X), dtype, P, B, K, start, p(sel), p(radius), p(points))
    return rc, sel, radius, points


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def banana():
    """The reference's partial_pcd/banana.npy: 2048 × 3 float64."""
    return np.load(os.path.join(GOLDEN, "partial_pcd_banana.npy"))


def normal_cloud(P, seed=None):
    return np.random.default_rng(P if seed is None else seed).standard_normal((P, 3))


def lattice(nx, ny, nz):
    """The integer lattice in C order of (i, j, k): equal distances everywhere, so equal maxima really occur."""
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=3).reshape(-1, 3) \
        .astype(np.float64)


def duplicates():
    """15 rows that are 5 distinct points, each three times in a row."""
    x = np.array([0.0, 5.0, 2.0, 10.0, 7.5])
    return np.repeat(np.stack([x, np.ones(5), -2.0 * np.ones(5)], axis=1), 3, axis=0)


DUPLICATES_SEL = [0, 9, 3, 12, 6, 0, 0, 0, 0]
DUPLICATES_RADIUS = [np.inf, 100.0, 25.0, 6.25, 4.0, 0.0, 0.0, 0.0, 0.0]

NONFINITE_ROWS = {3: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 130: (0, -np.inf), 299: (2, np.nan)}


def salted_cloud(P=300):
    """A normal cloud with NaN and ±inf in single coordinates of the rows NONFINITE_ROWS."""
    X = normal_cloud(P, seed=7)
    for row, (col, v) in NONFINITE_ROWS.items():
        X[row, col] = v
    return X


def all_nonfinite(P=70):
    X = normal_cloud(P, seed=11)
    X[np.arange(P), np.arange(P) % 3] = np.array([np.nan, np.inf, -np.inf])[np.arange(P) % 3]
    return X


def edge_sizes(capacity):
    """P one below, at and one above every tiling constant of the two device paths: the wave (64), the per-round
    workgroup (256), the one-workgroup path's workgroup (1024, also the per-round path's rows per workgroup), its
    steps of rows per lane (2048, 4096) and its capacity."""
    out = []
    for c in (64, 256, 1024, 2048, 4096, capacity):
        out += [c - 1, c, c + 1]
    return sorted(set(out))


def shared_cases(capacity):
    """name → (cloud, K, start): the cases both the host build and the device are checked on."""
    cases = {f"edge_P{P}": (normal_cloud(P), 5, 0) for P in edge_sizes(capacity)}
    cases["K_equals_P_65"] = (normal_cloud(65, seed=165), 65, 0)
    cases["banana_f64"] = (banana(), 200, 0)
    cases["banana_f32"] = (banana().astype(np.float32), 200, 0)
    cases["start_last"] = (normal_cloud(1500, seed=3), 12, 1499)
    cases["duplicates"] = (duplicates(), 9, 0)
    cases["nonfinite"] = (salted_cloud(), 40, 0)
    cases["nonfinite_start"] = (salted_cloud(), 40, 64)
    cases["all_nonfinite"] = (all_nonfinite(), 5, 2)
    cases["lattice_small"] = (lattice(13, 13, 11), 32, 0)
    return cases


def large_cases():
    """Beyond every one-workgroup capacity: the tie lattice and the ragged normal cloud."""
    return {"lattice": (lattice(35, 35, 33), 32, 0),
            "ragged_70001": (np.random.default_rng(70001).standard_normal((70001, 3)), 64, 0)}
