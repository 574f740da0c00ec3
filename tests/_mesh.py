"""Helpers shared by test_mesh_cpu.py and test_gpu_mesh.py: the marching-tetrahedra rule of csrc/cdx_mesh.h stated in
numpy (written from the rule's prose, not from the header), the host build's binding, and topology checks."""
import itertools

import numpy as np

from tests._field import F32, F64, salted_mean
from tests._host import host, p

OFFSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]  # edge types, in (i, j, k)
PERMS = list(itertools.permutations(range(3)))  # lexicographic: the six Kuhn tetrahedra


def numpy_mesh(mean, axes):
    """(vertices f64 [V, 3], keys int64 [V], faces int32 [F, 3]) of the rule on lattice ``mean`` [s, s, s] with point
    axes (px, py, pz): node (i, j, k) at (px[j], py[i], pz[k])."""
    s = mean.shape[0]
    px, py, pz = (np.asarray(a, np.float64) for a in axes)
    empty = np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros((0, 3), np.int32)
    if s < 2:
        return empty
    with np.errstate(invalid="ignore"):
        inside = mean < 0
    f = mean.astype(np.float64)
    idx = np.arange(s ** 3, dtype=np.int64).reshape(s, s, s)

    def pos(i, j, k):
        return np.stack([px[j], py[i], pz[k]], axis=-1)

    # vertices: the crossing edges in ascending key order
    keys = []
    for d, (di, dj, dk) in enumerate(OFFSETS):
        a = idx[:s - di, :s - dj, :s - dk]
        crossing = inside[:s - di, :s - dj, :s - dk] != inside[di:, dj:, dk:]
        keys.append(7 * a[crossing] + d)
    keys = np.sort(np.concatenate(keys))
    c, d = keys // 7, keys % 7
    i, j, k = np.unravel_index(c, (s, s, s))
    off = np.array(OFFSETS)[d]
    ib, jb, kb = i + off[:, 0], j + off[:, 1], k + off[:, 2]
    fa, fb = f[i, j, k], f[ib, jb, kb]
    with np.errstate(all="ignore"):
        t = fa / (fa - fb)
        t = np.where((t >= 0) & (t <= 1), t, 0.5)
    pa, pb = pos(i, j, k), pos(ib, jb, kb)
    vertices = pa + t[:, None] * (pb - pa)

    # faces: per cube, tetrahedron, triangle
    ci, cj, ck = (g.reshape(-1) for g in np.meshgrid(*[np.arange(s - 1)] * 3, indexing="ij"))
    ncubes = len(ci)
    edge_type = {o: n for n, o in enumerate(OFFSETS)}
    rows = []  # (cube, tet, tri, key0, key1, key2)
    for tet, perm in enumerate(PERMS):
        corner = [np.zeros(3, int)]
        for ax in perm:
            e = np.zeros(3, int)
            e[ax] = 1
            corner.append(corner[-1] + e)
        ijk = [(ci + q[0], cj + q[1], ck + q[2]) for q in corner]
        ins = np.stack([inside[x] for x in ijk], axis=1)  # [ncubes, 4]
        P = [pos(*x) for x in ijk]

        def key(x, y, sel):
            lo, hi = min(x, y), max(x, y)  # corners are ordered along the path: the earlier one is the lower node
            d = edge_type[tuple(corner[hi] - corner[lo])]
            return 7 * idx[ijk[lo][0][sel], ijk[lo][1][sel], ijk[lo][2][sel]] + d

        def det(x0, x1, x2, x3, sel):
            m = np.stack([P[x1][sel] - P[x0][sel], P[x2][sel] - P[x0][sel], P[x3][sel] - P[x0][sel]], axis=1)
            return np.linalg.det(m) if len(m) else np.zeros(0)

        def emit(sel, tri, e0, e1, e2, swap):
            k0, k1, k2 = key(*e0, sel), key(*e1, sel), key(*e2, sel)
            k1, k2 = np.where(swap, k2, k1), np.where(swap, k1, k2)
            cube = np.flatnonzero(sel)
            rows.append(np.stack([cube, np.full_like(cube, tet), np.full_like(cube, tri), k0, k1, k2], axis=1))

        for bits in range(1, 15):
            pat = np.array([(bits >> q) & 1 for q in range(4)], bool)
            sel = np.all(ins == pat, axis=1)
            if not sel.any():
                continue
            inn = [q for q in range(4) if pat[q]]
            out = [q for q in range(4) if not pat[q]]
            if len(inn) == 1:
                a, (o1, o2, o3) = inn[0], out
                emit(sel, 0, (a, o1), (a, o2), (a, o3), det(a, o1, o2, o3, sel) < 0)
            elif len(inn) == 3:
                (a1, a2, a3), o = inn, out[0]
                emit(sel, 0, (a1, o), (a2, o), (a3, o), det(o, a1, a2, a3, sel) > 0)
            else:
                (a, b), (c_, d_) = inn, out
                swap = det(a, b, c_, d_, sel) < 0
                emit(sel, 0, (a, c_), (a, d_), (b, d_), swap)
                emit(sel, 1, (a, c_), (b, d_), (b, c_), swap)
    if not rows:
        return vertices, keys, empty[2]
    rows = np.concatenate(rows)
    assert ncubes * 12 >= len(rows)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    faces = np.searchsorted(keys, rows[:, 3:]).astype(np.int32)
    assert np.array_equal(keys[faces], rows[:, 3:])
    return vertices, keys, faces


def host_mesh(mean, axes, vcap=None, fcap=None, dtype=None):
    """cdxh_mesh_extract on host arrays: ((V, F), vertices, keys, faces) with vcap / fcap rows (default: all), rows
    past the capacity left at guard values."""
    lib = host()
    mean = np.ascontiguousarray(mean)
    s = mean.shape[0]
    if dtype is None:
        dtype = {np.dtype(np.float32): F32, np.dtype(np.float64): F64}[mean.dtype]
    ax = [np.ascontiguousarray(a, np.float64) for a in axes]
    counts = np.full(2, -5, np.int64)
    if vcap is None or fcap is None:
        rc = lib.cdxh_mesh_extract(p(mean), dtype, s, p(ax[0]), p(ax[1]), p(ax[2]), 0, 0, None, None, None, p(counts))
        assert rc == 0
        vcap = int(counts[0]) if vcap is None else vcap
        fcap = int(counts[1]) if fcap is None else fcap
    v = np.full((vcap, 3), -7.0)
    keys = np.full(vcap, -1, np.int64)
    faces = np.full((fcap, 3), -1, np.int32)
    rc = lib.cdxh_mesh_extract(p(mean), dtype, s, p(ax[0]), p(ax[1]), p(ax[2]), vcap, fcap, p(v), p(keys), p(faces),
                               p(counts))
    assert rc == 0
    return (int(counts[0]), int(counts[1])), v, keys, faces


def host_refine(mean, fv, axes, keys, state=None):
    """cdxh_mesh_refine: fv None starts the state from the lattice, else one step: (state [5, V], vertices [V, 3])."""
    lib = host()
    mean = np.ascontiguousarray(mean)
    dtype = {np.dtype(np.float32): F32, np.dtype(np.float64): F64}[mean.dtype]
    ax = [np.ascontiguousarray(a, np.float64) for a in axes]
    keys = np.ascontiguousarray(keys, np.int64)
    V = len(keys)
    state = np.full((5, V), -7.0) if state is None else np.ascontiguousarray(state).copy()
    v = np.full((V, 3), -7.0)
    fvp = None if fv is None else p(np.ascontiguousarray(fv, np.float64))
    rc = lib.cdxh_mesh_refine(p(mean), dtype, fvp, mean.shape[0], p(ax[0]), p(ax[1]), p(ax[2]), p(keys), V, p(state),
                              p(v))
    assert rc == 0
    return state, v


def salted_inf_mean(rng, steps, dtype):
    """tests/_field.salted_mean (NaN, +0, −0 cells) plus ±inf cells."""
    mean = salted_mean(rng, steps, dtype)
    salt = rng.integers(0, 14, mean.shape)
    mean[salt == 0] = np.inf
    mean[salt == 1] = -np.inf
    return mean


def sphere_field(axes, radius=0.7):
    """|P| − radius on the lattice of ``axes``: [s, s, s] with node (i, j, k) at (px[j], py[i], pz[k])."""
    X, Y, Z = np.meshgrid(*axes, indexing="xy")
    return np.sqrt(X * X + Y * Y + Z * Z) - radius


SPHERE_AXES = (np.linspace(-1, 1, 12), np.linspace(-1.1, 1.2, 12), np.linspace(-0.9, 1, 12))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def edge_counts(faces):
    """(directed [E', 2] and their counts, undirected [E, 2] and their counts) of a face list."""
    f = np.asarray(faces, np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    d, dc = np.unique(de, axis=0, return_counts=True)
    u, uc = np.unique(np.sort(de, axis=1), axis=0, return_counts=True)
    return d, dc, u, uc


def euler(n_vertices, faces):
    _, _, u, _ = edge_counts(faces)
    return n_vertices - len(u) + len(faces)


def signed_volume(vertices, faces):
    v = vertices[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def key_ends(keys, steps):
    """Lattice (i, j, k) of both ends of the edges with these keys: ([n, 3], [n, 3])."""
    c, d = np.asarray(keys) // 7, np.asarray(keys) % 7
    a = np.stack(np.unravel_index(c, (steps,) * 3), axis=1)
    return a, a + np.array(OFFSETS)[d]
