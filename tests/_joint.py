"""Test helpers of the GPIS joint posterior of value and gradient (csrc/cdx_gpis_joint.h): a float64 numpy statement of
Σ(x) = P0 − WᵀW built from the formulas alone with a numpy Cholesky of the state's own E11 (the reference has no such
function, so nothing is read from it), the state and query recipes, the scaled error every check uses and a wrapper of
the host build.  Shared by tests/test_joint_cpu.py (host build) and tests/test_gpu_joint.py (device)."""
import ctypes as C

import numpy as np

from compliancedex_amd._native import KERNELS, CdxGpis
from tests._host import host, p

SIGMA = 0.08
TRIU = [(a, b) for a in range(4) for b in range(a, 4)]  # ff, fx, fy, fz, xx, xy, xz, yy, yz, zz


# ------------------------------------------------------------------ the kernels, from gpis.py:16-29
def np_k(kernel, r2, R, sigma=SIGMA):
    """(k, kd) at squared distances r2: the covariance and the factor of ∂k/∂x = kd·(x − x_j)."""
    r = np.sqrt(r2)
    tps, tps_d = 2.0 * r2 * r - 3.0 * R * r2 + R ** 3, 6.0 * r - 6.0 * R
    rbf = np.exp(-0.5 * r2 / sigma ** 2)
    rbf_d = -rbf / sigma ** 2
    return {"tps": (tps, tps_d), "rbf": (rbf, rbf_d), "joint": (0.3 * rbf + 0.7 * tps, 0.3 * rbf_d + 0.7 * tps_d)}[kernel]


def np_prior(kernel, R, sigma=SIGMA):
    """diag P0 = (k0, κ, κ, κ), κ = −k″(0) along an axis: 6R (TPS), 1/σ² (RBF), 0.3/σ² + 0.7·6R (joint)."""
    k0 = {"tps": R ** 3, "rbf": 1.0, "joint": 0.3 + 0.7 * R ** 3}[kernel]
    kappa = {"tps": 6.0 * R, "rbf": 1.0 / sigma ** 2, "joint": 0.3 / sigma ** 2 + 0.7 * 6.0 * R}[kernel]
    return np.array([k0, kappa, kappa, kappa])


def forward_substitute(L, B):
    """L⁻¹·B for a lower-triangular L [N, N] and B [N, K], 64 rows at a time."""
    N = len(L)
    W = np.zeros_like(B)
    for i0 in range(0, N, 64):
        i1 = min(i0 + 64, N)
        rhs = B[i0:i1] - L[i0:i1, :i0] @ W[:i0]
        for i in range(i0, i1):
            W[i] = (rhs[i - i0] - L[i, i0:i] @ W[i0:i]) / L[i, i]
    return W


def np_b(kernel, X1, R, X, sigma=SIGMA):
    """[M, N, 4]: (k, ∂ₓk, ∂ᵧk, ∂_z k) of every query against every inducing point."""
    d = X[:, None, :] - X1[None, :, :]
    with np.errstate(all="ignore"):
        k, kd = np_k(kernel, (d * d).sum(-1), R, sigma)
        return np.concatenate([k[..., None], kd[..., None] * d], -1)


def np_joint(kernel, X1, E11, R, X, sigma=SIGMA):
    """The statement: [M, 10], the upper triangle of P0 − WᵀW with W = L⁻¹·[k, ∇k], E11 = L·Lᵀ."""
    X1, E11, X = (np.asarray(a, np.float64) for a in (X1, E11, X))
    M, N = len(X), len(X1)
    B = np_b(kernel, X1, float(R), X.reshape(-1, 3), sigma)
    L = np.linalg.cholesky(E11)
    W = forward_substitute(L, B.transpose(1, 0, 2).reshape(N, M * 4)).reshape(N, M, 4)
    G = np.einsum("nma,nmb->mab", W, W)
    S = np.diag(np_prior(kernel, float(R), sigma))[None] - G
    return np.stack([S[:, a, b] for a, b in TRIU], 1)


def np_joint_solve(kernel, X1, E11, R, X, sigma=SIGMA):
    """The same Σ without the factor: P0 − Bᵀ·E11⁻¹·B by numpy's general solve."""
    B = np_b(kernel, np.asarray(X1, np.float64), float(R), np.asarray(X, np.float64).reshape(-1, 3), sigma)
    Z = np.linalg.solve(np.asarray(E11, np.float64), B.transpose(1, 0, 2).reshape(len(X1), -1)).reshape(B.transpose(1, 0, 2).shape)
    S = np.diag(np_prior(kernel, float(R), sigma))[None] - np.einsum("mna,nmb->mab", B, Z)
    return np.stack([S[:, a, b] for a, b in TRIU], 1)


def scaled_error(a, b, kernel, R, sigma=SIGMA):
    """max over entries of |ΔΣ_ab| / sqrt(P0_aa·P0_bb) between two [M, 10] arrays."""
    p0 = np_prior(kernel, float(R), sigma)
    scale = np.array([np.sqrt(p0[i] * p0[j]) for i, j in TRIU])
    a, b = np.asarray(a, np.float64).reshape(-1, 10), np.asarray(b, np.float64).reshape(-1, 10)
    return float((np.abs(a - b) / scale).max()) if len(a) else 0.0


def full(cov10):
    """[M, 10] → the symmetric [M, 4, 4]."""
    cov10 = np.asarray(cov10)
    S = np.zeros(cov10.shape[:-1] + (4, 4))
    for e, (a, b) in enumerate(TRIU):
        S[..., a, b] = S[..., b, a] = cov10[..., e]
    return S


# ------------------------------------------------------------------ states and queries
def sphere_points(n, seed):
    """The arrays of tests/test_gpu_edges._random_gpis: points on a 5 cm sphere, the first four pushed out as exterior
    anchors → (X1 [n, 3], y [n, 1], noise [n])."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    X1 = 0.05 * d
    y = np.zeros((n, 1))
    noise = np.full(n, 0.005)
    k = min(4, n)
    X1[:k] *= 3.0
    y[:k] = 0.1
    noise[:k] = 0.2
    return X1, y, noise


def np_state(kernel, n, seed=None, sigma=SIGMA):
    """GPIS.fit (gpis.py:33-40) in numpy on sphere_points → (X1, E11, R)."""
    X1, _, noise = sphere_points(n, n if seed is None else seed)
    d = np.linalg.norm(X1[:, None] - X1[None], axis=-1)
    R = float(d.max()) if kernel != "rbf" else 0.0
    E11 = np_k(kernel, d * d, R, sigma)[0] + np.diag(noise ** 2)
    return X1, E11, R


def queries(X1, M, seed, jitter=0.01):
    """M queries around the inducing points (1 cm jitter by default)."""
    rng = np.random.default_rng(seed)
    X1 = np.asarray(X1, np.float64)
    return X1[rng.integers(0, len(X1), M)] + jitter * rng.standard_normal((M, 3))


# ------------------------------------------------------------------ the host build
def descriptor(kernel, X1, Linv_t, R, sigma=SIGMA):
    """A cdx_gpis over host arrays (kept alive by the returned tuple): Linv_t [N_pad, N_pad] zero-padded."""
    X1 = np.ascontiguousarray(X1, np.float64)
    Linv_t = np.ascontiguousarray(Linv_t, np.float64)
    g = CdxGpis(X1=X1.ctypes.data, Linv_t=Linv_t.ctypes.data, N=len(X1), N_pad=Linv_t.shape[0], kernel=KERNELS[kernel],
                R=float(R), sigma=float(sigma))
    return g, (X1, Linv_t)


def np_linv_t(E11, pad=0):
    """(L⁻¹)ᵀ of E11 = L·Lᵀ from numpy, zero-padded by ``pad`` rows and columns."""
    N = len(E11)
    Linv = forward_substitute(np.linalg.cholesky(E11), np.eye(N))
    out = np.zeros((N + pad, N + pad))
    out[:N, :N] = Linv.T
    return out


def host_joint(kernel, X1, Linv_t, R, X, sigma=SIGMA, preset=None):
    """cdxh_gpis_joint → [M, 10]."""
    g, keep = descriptor(kernel, X1, Linv_t, R, sigma)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    cov = np.full((len(X), 10), -7.0 if preset is None else preset)
    rc = host().cdxh_gpis_joint(C.byref(g), p(X), len(X), p(cov))
    assert rc == 0, rc
    del keep
    return cov


def host_kernel_values(kernel, r2, R, sigma=SIGMA):
    """(k, kd, k0, κ) of csrc/cdx_gpis.h at squared distance r2."""
    out = np.zeros(4)
    rc = host().cdxh_gpis_kernel_values(KERNELS[kernel], float(r2), float(R), float(sigma), p(out))
    assert rc == 0, rc
    return out


# ------------------------------------------------------------------ grasps on the 5 cm sphere
def closing_grasps(E):
    """tests/_equil.py's family of grasps that close ("firm": four contacts near a tetrahedron's directions, pressed
    in 8 … 12 mm) moved from its ellipsoid onto the 5 cm sphere of sphere_points → (contact, target, stiffness)."""
    from tests import _equil
    pts, tgt, k, _ = _equil.family("firm", E, 4)
    u = _equil.unit(pts / _equil.AXES)
    return 0.05 * u, 0.05 * u + (tgt - pts), k
