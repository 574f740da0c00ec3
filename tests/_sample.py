"""Helpers shared by test_sample_cpu.py and test_gpu_sample.py: the surface-sampling rule of csrc/cdx_sample.h stated in
numpy (Philox4x32-10, prepare, draw), the host build (cdxh_sample_prepare / cdxh_sample_draw / cdxh_philox4x32_10) and
the meshes both files sample."""
import os

import numpy as np

from tests._fps import numpy_fps, same_bits  # noqa: F401  (same_bits is re-exported)
from tests._host import host, p
from tests.conftest import REPO

F32, F64 = 0, 1  # CDX_DTYPE_*
MESHES = os.path.join(REPO, "compliancedex_amd", "data", "meshes")
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# counter words, key words → output words (the vectors of the Random123 distribution's kat_vectors)
PHILOX_VECTORS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def numpy_philox(counter, key):
    """Philox4x32-10 over arrays: counter = 4 and key = 2 broadcastable arrays of 32-bit words → 4 uint64 arrays of
    32-bit words."""
    c0, c1, c2, c3 = [np.asarray(c, np.uint64) & M32 for c in counter]
    k0, k1 = [np.asarray(k, np.uint64) & M32 for k in key]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def mulhi64(a, b):
    """High 64 bits of a·b, a a uint64 array and b a Python int below 2⁶⁴."""
    a = np.asarray(a, np.uint64)
    al, ah = a & M32, a >> S32
    bl, bh = np.uint64(b & 0xFFFFFFFF), np.uint64(b >> 32)
    ll, hl, lh, hh = al * bl, ah * bl, al * bh, ah * bh
    cross = (ll >> S32) + (hl & M32) + (lh & M32)
    return hh + (hl >> S32) + (lh >> S32) + (cross >> S32)


def numpy_geometry(faces):
    """(v0, e1, e2, c [F, 3], n2 [F], area [F]) of the rule; numpy rounds every product and difference on its own."""
    f = np.asarray(faces).astype(np.float64)
    with np.errstate(all="ignore"):
        v0, e1, e2 = f[:, 0], f[:, 1] - f[:, 0], f[:, 2] - f[:, 0]
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        n2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        ok = np.isfinite(f).all(axis=(1, 2)) & np.isfinite(n2) & (n2 != 0)
        area = np.where(ok, 0.5 * np.sqrt(np.where(ok, n2, 1.0)), 0.0)
    return v0, e1, e2, c, n2, area


def numpy_prepare(faces):
    """(C uint64 [F], info) of the rule."""
    area = numpy_geometry(faces)[5]
    A = area.max()
    w = np.floor(area / A * 4294967296.0).astype(np.uint64) if A > 0 else np.zeros(len(area), np.uint64)
    return np.cumsum(w, dtype=np.uint64), int(not A > 0)


def numpy_draw(faces, cdf, seed, first, K):
    """(points [K, 3], face int64 [K], bary [K, 2], normal [K, 3]) of the rule."""
    v0, e1, e2, c, n2, _ = numpy_geometry(faces)
    T = int(cdf[-1])
    i = np.uint64(first) + np.arange(K, dtype=np.uint64)  # wraps at 2⁶⁴
    zero = np.zeros(K, np.uint64)
    r0, r1, r2, r3 = numpy_philox((i & M32, i >> S32, zero, zero), (seed & 0xFFFFFFFF, seed >> 32))
    t = mulhi64((r1 << S32) | r0, T)
    u, v = (r2.astype(np.float64) + 0.5) * 2.0 ** -32, (r3.astype(np.float64) + 0.5) * 2.0 ** -32
    flip = u + v > 1.0
    u, v = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - v, v)
    if T == 0:
        nan3 = np.full((K, 3), np.nan)
        return nan3, np.full(K, -1, np.int64), np.full((K, 2), np.nan), nan3.copy()
    f = np.searchsorted(cdf, t, side="right").astype(np.int64)  # the smallest f with C_f > t
    points = (v0[f] + u[:, None] * e1[f]) + v[:, None] * e2[f]
    normal = c[f] / np.sqrt(n2[f])[:, None]
    return points, f, np.stack([u, v], axis=1), normal


def _dtype(faces):
    return {np.dtype(np.float32): F32, np.dtype(np.float64): F64}[faces.dtype]


def host_philox(counter, key):
    lib = host()
    c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    lib.cdxh_philox4x32_10(p(c), p(k), p(out))
    return tuple(int(x) for x in out)


def host_prepare(faces, dtype=None, F=None):
    """cdxh_sample_prepare on a host array in its own dtype: (rc, C uint64 [F], info)."""
    lib = host()
    faces = np.ascontiguousarray(faces)
    cdf = np.zeros(len(faces), np.uint64)
    info = np.full(1, -1, np.int32)
    rc = lib.cdxh_sample_prepare(p(faces), _dtype(faces) if dtype is None else dtype, len(faces) if F is None else F,
                                 p(cdf), p(info))
    return rc, cdf, int(info[0])


def host_draw(faces, cdf, seed, first, K):
    """cdxh_sample_draw: (rc, points, face, bary, normal)."""
    lib = host()
    faces = np.ascontiguousarray(faces)
    rows = max(K, 0)
    points, face = np.full((rows, 3), -7.0), np.full(rows, -9, np.int64)
    bary, normal = np.full((rows, 2), -7.0), np.full((rows, 3), -7.0)
    rc = lib.cdxh_sample_draw(p(faces), _dtype(faces), len(faces), p(cdf), seed, first, K, p(points), p(face), p(bary),
                              p(normal))
    return rc, points, face, bary, normal


def same_draw(a, b):
    """Two (points, face, bary, normal) results are the same bits (NaN included)."""
    return all(same_bits(x, y) for x, y in zip(a, b))


def mesh(name):
    """A packaged mesh's [F, 3, 3] face vertices: "banana", "cube" or "sphere42"."""
    return np.load(os.path.join(MESHES, f"{name}_faces.npy"))


def random_faces(F, seed=None, dtype=np.float64):
    """F triangles around random centres whose sizes spread over four decades."""
    rng = np.random.default_rng(F if seed is None else seed)
    centre = rng.standard_normal((F, 1, 3))
    size = 10.0 ** rng.uniform(-3, 1, (F, 1, 1))
    return (centre + size * rng.standard_normal((F, 3, 3))).astype(dtype)


def salted_faces(F=300):
    """Random faces with the kinds the rule never draws at the rows DEAD_ROWS."""
    f = random_faces(F, seed=17)
    f[3, 1, 0] = np.nan
    f[64, 0, 2] = np.inf
    f[65, 2, 1] = -np.inf
    f[100, 1] = f[100, 0]                        # two equal vertices
    f[101] = np.array([[0., 0., 0.], [1., 1., 1.], [2., 2., 2.]])  # collinear
    f[102] = 0.0
    f[299] = np.array([[0., 0., 0.], [1e200, 0., 0.], [0., 1e200, 0.]])  # n2 overflows
    return f


DEAD_ROWS = (3, 64, 65, 100, 101, 102, 299)


def tiny_beside_unit():
    """A right triangle of area 1 (legs 2 and 1) between two of area 2⁻⁴⁰ (legs 2⁻¹⁹ and 2⁻²⁰), all exact."""
    unit = [[0., 0., 0.], [2., 0., 0.], [0., 1., 0.]]
    tiny = [[5., 0., 0.], [5. + 2.0 ** -19, 0., 0.], [5., 2.0 ** -20, 0.]]
    return np.array([tiny, unit, tiny])


def all_degenerate(F=70):
    f = random_faces(F, seed=23)
    f[::3, 2] = f[::3, 1]
    f[1::3, 0, 0] = np.nan
    f[2::3] = 1.5
    return f


def shared_cases():
    """name → faces: the meshes both the host build and the device are checked on."""
    cases = {f"random_F{F}": random_faces(F) for F in (1, 2, 63, 64, 65, 255, 256, 257, 5000)}
    cases["random_f32_F257"] = random_faces(257, seed=1257, dtype=np.float32)
    cases["cube"] = mesh("cube")
    cases["sphere42"] = mesh("sphere42")
    cases["banana"] = mesh("banana")
    cases["banana_f64"] = mesh("banana").astype(np.float64) * 1.0000001
    cases["salted"] = salted_faces()
    cases["tiny_beside_unit"] = tiny_beside_unit()
    cases["all_degenerate"] = all_degenerate()
    return cases


def binomial_z(counts, weights, K):
    """|z| of each count against Binomial(K, w/Σw)."""
    prob = weights.astype(np.float64) / float(weights.sum())
    return np.abs(counts - K * prob) / np.sqrt(K * prob * (1.0 - prob))


def weights_of(cdf):
    return np.diff(np.concatenate([np.zeros(1, np.uint64), cdf])).astype(np.uint64)


def min_pairwise(X):
    d = X[:, None, :] - X[None, :, :]
    q = (d * d).sum(axis=2)
    q[np.arange(len(X)), np.arange(len(X))] = np.inf
    return float(np.sqrt(q.min()))


def numpy_poisson(faces, K, init_factor=5, seed=0):
    """The Poisson composition in numpy: init_factor·K uniform draws, then farthest-point sampling from row 0.
    (points [K, 3], face [K], normal [K, 3], sel [K], radius [K], the uniform points)."""
    cdf, _ = numpy_prepare(faces)
    pts, face, _, normal = numpy_draw(faces, cdf, seed, 0, init_factor * K)
    sel, radius, chosen = numpy_fps(pts, K, 0)
    return chosen, face[sel], normal[sel], sel, radius, pts
