"""Drop-in for the reference GPIS class (gpis.py:4-168) on MI355X.

Same constructor, attributes (``R, X1, y1, E11, bias, sigma, noise``), state files and
methods (``fit``, ``pred``, ``compute_normal``, ``compute_multinormals``,
``save_state_data``, ``load_state_data``, ``get_visualization_data``, ``topcd``).  Queries run on the
gfx950 kernels (cdx_gpis_mean / cdx_gpis_std); there is no CPU path.

Beyond the reference: ``field`` evaluates mean / std / normal on a whole lattice in one native call
(``get_visualization_data(fused=True)`` is that plus one copy back), ``topcd`` compacts the surface cells on
the device (cdx_gpis_surface_count / _place, the reference's triple Python loop), and ``surface`` chains the
two without the lattice leaving the device; ``fit_pointcloud`` goes from a raw sensed cloud to the fitted state
(farthest-point sampling by cdx_fps, then the reference's recipe: pointcloud.py); ``tomesh`` turns a lattice field into
a watertight triangle mesh by marching tetrahedra on the device (cdx_gpis_mesh_count / _place, the rule of
csrc/cdx_mesh.h; the reference's Poisson reconstruction is not reproduced) and ``surface_mesh`` goes from the state to
that mesh, optionally refined along the lattice edges, without the lattice leaving the device.  ``pred_joint`` is the
posterior of the value and its gradient together, a 4-vector Gaussian per query (cdx_gpis_joint: Σ = P0 − WᵀW, three
more whitened columns a query than the std pass); ``normal_uncertainty`` turns it into the covariance of the unit
normal, an angular standard deviation and the standard deviation of the surface's position, and ``sample_joint`` /
``sample_normals`` draw from it — the probabilistic counterpart of ``compute_multinormals``, whose nested subsets of
the inducing points (gpis.py:89-111) are a heuristic with no such meaning.

Differences in *how*, not *what*: ``fit`` builds R and E11 with cdx_gpis_fit, and L⁻¹ (E11 = LLᵀ),
E11⁻¹ and α = L⁻ᵀL⁻¹y1 are factored once per state on the device by cdx_gpis_factor (blocked
Cholesky; the reference re-solves E11 on every ``pred`` and inverts it on every
``compute_normal``); only the diagonal of the posterior covariance is formed, in the whitened
form k0 − ‖L⁻¹k‖² (the reference builds the M×M matrix, gpis.py:57-58).
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple

import numpy as np
import torch

from . import _native as N

_PKG_STATES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gpis_states")
# Closure screening margin Δ = SCREEN_MARGIN × the calibrated max error of the split-precision estimate of std²
# (cdx_gpis.screen_delta).  A constant: no environment variable can shrink the margin of the shipped path.
SCREEN_MARGIN = 32.0
CALIB_QUERIES = 8192      # near the object (displaced inducing points, bounding box ± 5 cm)
CALIB_FAR_QUERIES = 4096  # 5 cm … 3.5R from the inducing points (the screen's whole finite range)


NormalUncertainty = namedtuple("NormalUncertainty", ["normal", "cov_normal", "angle_std", "offset_std"])
NormalUncertainty.__doc__ = """At queries […, 3]: normal […, 3] = ∇mean/‖∇mean‖; cov_normal […, 3, 3], the first-order
covariance of the unit normal (I − n̂n̂ᵀ)·Σ_g·(I − n̂n̂ᵀ)/‖∇mean‖² with Σ_g the posterior covariance of the gradient;
angle_std […] = sqrt(trace cov_normal), the angular standard deviation in rad (first order: a value near or above 1 says
that the normal is hardly determined, not that it is known to that angle); offset_std […] = sqrt(max(Σ00, 0))/‖∇mean‖,
the standard deviation of the surface's position along the normal, in metres."""

# Upper-triangle order of cdx_gpis_joint's 10 entries → the 4 × 4 matrix.
_TRIU = [(a, b) for a in range(4) for b in range(a, 4)]
_FILL = [[_TRIU.index((min(a, b), max(a, b))) for b in range(4)] for a in range(4)]
PIVOT_REL = 1e-12  # a Cholesky pivot ≤ this × its prior entry gets no noise


def _require_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what} must be a CUDA (ROCm) tensor: compliancedex_amd has no CPU path")


class _State:
    """Device-resident padded state + the cdx_gpis descriptor pointing at it."""

    def __init__(self, X1, y1, E11, R, bias, kernel, sigma):
        dev = X1.device
        n = X1.shape[0]
        Np = (n + N.NPAD_ALIGN - 1) // N.NPAD_ALIGN * N.NPAD_ALIGN
        lib = N.load()
        E11 = E11.to(dev, torch.float64).contiguous()
        y1 = y1.to(dev, torch.float64).reshape(-1).contiguous()
        self.Ainv = torch.empty(Np, Np, dtype=torch.float64, device=dev)
        self.Linv_t = torch.empty(Np, Np, dtype=torch.float64, device=dev)
        self.Linv = torch.empty(Np, Np, dtype=torch.float64, device=dev)
        self.alpha = torch.empty(Np, dtype=torch.float64, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.cdx_gpis_factor_workspace(Np), dtype=torch.uint8, device=dev)
        N.check(lib.cdx_gpis_factor(N.ptr(E11), N.ptr(y1), n, Np, N.ptr(ws), N.ptr(self.Ainv), N.ptr(self.Linv_t), N.ptr(self.Linv), N.ptr(self.alpha),
                                    N.ptr(info), N.stream_ptr(dev)), "cdx_gpis_factor")
        bad = int(info.item())  # one host sync per state build
        del ws
        if bad:
            raise RuntimeError(f"GPIS E11 is not positive definite (pivot {bad} of {n})")
        self.X1 = X1[:1].to(torch.float64).repeat(Np, 1).contiguous()
        self.X1[:n] = X1.to(torch.float64)
        self.desc = N.CdxGpis(X1=self.X1.data_ptr(), alpha=self.alpha.data_ptr(), Ainv=self.Ainv.data_ptr(),
                              Linv_t=self.Linv_t.data_ptr(), Linv=self.Linv.data_ptr(), N=n,
                              N_pad=Np, kernel=N.KERNELS[kernel], R=float(R), sigma=float(sigma), bias=float(bias))
        # split-precision variance screen (fp16 slices of scaled L⁻ᵀ): built once per state
        self.screen = torch.empty(lib.cdx_gpis_screen_bytes(Np), dtype=torch.uint8, device=dev)
        N.check(lib.cdx_gpis_screen_prepare(self.desc, N.ptr(self.screen), N.stream_ptr(dev)), "cdx_gpis_screen_prepare")
        self.desc.screen = self.screen.data_ptr()
        self.desc.screen_delta = 0.0
        self.ws = None
        self.screen_ws = None
        self.joint_ws = None
        self.screen_err, bands = self._calibrate_screen(X1[:n].to(torch.float64), R, kernel)
        # the closure keeps every fingertip whose estimate is within 2Δ_f of its group's leader
        k0 = {"tps": float(R) ** 3, "rbf": 1.0, "joint": 0.3 + 0.7 * float(R) ** 3}[kernel]
        ok = SCREEN_MARGIN > 0 and np.isfinite(self.screen_err)
        self.desc.screen_delta = max(SCREEN_MARGIN * self.screen_err, 2.0 ** -40 * k0) if ok else 0.0
        if ok:
            self.screen_bands = bands
            w = (ctypes.c_double * N.SCREEN_BANDS)(*bands)
            N.check(lib.cdx_gpis_screen_set_bands(self.desc, w, N.stream_ptr(dev)), "cdx_gpis_screen_set_bands")

    def _calibrate_screen(self, X1, R, kernel):
        """(max |estimate − exact| of k0 − ‖L⁻¹k‖², per-band weights) over calibration queries around
        this state, in units of the row scale max(1, ‖Ṽ‖²/k0) the closure's margin uses: the inducing points
        displaced by 0–3 cm and uniform points in their bounding box ± 5 cm (the near set: mostly
        finite estimates, else the state is not screened), plus the far set — inducing points pushed
        5 cm … 3.5R along random directions, log-uniform, i.e. the screen's whole finite range,
        where the margin grows with ‖Ṽ‖² (one host sync).  The closure's margin is SCREEN_MARGIN ×
        this."""
        dev = X1.device
        gen = torch.Generator(device="cpu").manual_seed(0)
        n = X1.shape[0]
        pts = [X1 + sc * torch.randn(n, 3, generator=gen, dtype=torch.float64).to(dev)
               for sc in (0.0, 0.002, 0.005, 0.01, 0.03)]
        lo, hi = X1.min(0).values - 0.05, X1.max(0).values + 0.05
        pts.append(lo + (hi - lo) * torch.rand(2 * n, 3, generator=gen, dtype=torch.float64).to(dev))
        Xn = torch.cat(pts)
        if Xn.shape[0] > CALIB_QUERIES:
            Xn = Xn[torch.randperm(Xn.shape[0], generator=gen)[:CALIB_QUERIES].to(dev)]
        r_far = max(3.5 * float(R), 0.05) if kernel != "rbf" else 1.0
        d = torch.exp(torch.empty(CALIB_FAR_QUERIES, dtype=torch.float64).uniform_(
            float(np.log(0.05)), float(np.log(max(r_far, 0.0501))), generator=gen))
        u = torch.randn(CALIB_FAR_QUERIES, 3, generator=gen, dtype=torch.float64)
        u = u / u.norm(dim=1, keepdim=True)
        base = torch.randint(0, n, (CALIB_FAR_QUERIES,), generator=gen)
        Xf = X1[base.to(dev)] + (d.unsqueeze(1) * u).to(dev)
        Xc = torch.cat([Xn, Xf]).contiguous()
        est = self.screen_var(Xc)
        exact = exact_var(self, Xc)
        # a query beyond the screen's safe radius estimates NaN (the closure then runs its whole
        # group exactly), so the bound is over finite estimates; mostly NaN near the object: no screening
        ok = torch.isfinite(est)
        if int(ok[:Xn.shape[0]].sum()) < Xn.shape[0] // 2:
            return float("nan"), None
        k0 = {"tps": float(R) ** 3, "rbf": 1.0, "joint": 0.3 + 0.7 * float(R) ** 3}[kernel]
        scale = ((k0 - est[ok]) / k0).clamp(min=1.0) if k0 > 0 else torch.ones_like(est[ok])
        err = (est[ok] - exact[ok]).abs() / scale
        self.calib_far_finite = int(ok[Xn.shape[0]:].sum())
        gmax = float(err.max())
        # per-band envelope (cdx_screen.h screen_margin): band b = ⌊4·|x − c|/ρ⌋ with the device's own
        # centre c and 4/ρ; a band's weight is the largest error of its own and every lower band,
        # relative to the global maximum — bands above the highest calibrated one keep weight 1
        info = (ctypes.c_double * 8)()
        N.check(N.load().cdx_gpis_screen_info(self.desc, info, N.stream_ptr(dev)), "cdx_gpis_screen_info")
        ctr = torch.tensor([info[0], info[1], info[2]], dtype=torch.float64, device=dev)
        t = (Xc[ok] - ctr).norm(dim=1) * info[5]
        band = torch.clamp(torch.floor(t), 0, N.SCREEN_BANDS - 1).to(torch.int64)
        per = torch.zeros(N.SCREEN_BANDS, dtype=torch.float64, device=dev).scatter_reduce(0, band, err, "amax")
        per = per.cpu().numpy()
        top = int(band.max())
        env = np.maximum.accumulate(per)
        w = np.ones(N.SCREEN_BANDS)
        if gmax > 0:
            w[:top + 1] = np.maximum(env[:top + 1] / gmax, 2.0 ** -20)
        self.calib_band_err = per
        return gmax, [float(x) for x in w]

    def screen_var(self, X):
        """Split-precision estimate of k0 − ‖L⁻¹k‖² at X [M, 3] (cdx_gpis_screen_var)."""
        lib = N.load()
        X = X.contiguous()
        M = X.shape[0]
        out = torch.empty(M, dtype=torch.float64, device=X.device)
        if M:
            need = lib.cdx_gpis_screen_workspace(self.desc, M)
            if self.screen_ws is None or self.screen_ws.numel() < need:
                self.screen_ws = torch.empty(need, dtype=torch.uint8, device=X.device)
            N.check(lib.cdx_gpis_screen_var(self.desc, N.ptr(X), M, N.ptr(out), N.ptr(self.screen_ws),
                                            N.stream_ptr(X.device)), "cdx_gpis_screen_var")
        return out

    def workspace(self, M):
        need = N.load().cdx_gpis_std_workspace(self.desc, M)
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.X1.device)
        return self.ws


def gpis_mean(state, X, want_grad=True, want_normal=False):
    lib = N.load()
    X = X.contiguous()
    M = X.shape[0]
    mean = torch.empty(M, dtype=torch.float64, device=X.device)
    gmean = torch.empty(M, 3, dtype=torch.float64, device=X.device) if want_grad else None
    normal = torch.empty(M, 3, dtype=torch.float64, device=X.device) if want_normal else None
    N.check(lib.cdx_gpis_mean(state.desc, N.ptr(X), M, N.ptr(mean), N.ptr(gmean), N.ptr(normal),
                              N.stream_ptr(X.device)), "cdx_gpis_mean")
    return mean, gmean, normal


def exact_var(state, X):
    """The signed fp64 k0 − ‖L⁻¹k‖² at X (cdx_gpis_std keeps it at the head of its workspace)."""
    M = X.shape[0]
    gpis_std(state, X, want_grad=False)
    return state.ws[:M * 8].view(torch.float64).clone()


def gpis_std(state, X, want_grad=True):
    lib = N.load()
    X = X.contiguous()
    M = X.shape[0]
    std = torch.empty(M, dtype=torch.float64, device=X.device)
    gstd = torch.empty(M, 3, dtype=torch.float64, device=X.device) if want_grad else None
    if M:
        ws = state.workspace(M)
        N.check(lib.cdx_gpis_std(state.desc, N.ptr(X), M, N.ptr(std), N.ptr(gstd), N.ptr(ws),
                                 N.stream_ptr(X.device)), "cdx_gpis_std")
    return std, gstd


def gpis_joint_cov(state, X):
    """The posterior covariance of (f, ∂f/∂x, ∂f/∂y, ∂f/∂z) at X [M, 3] → [M, 10], the upper triangle row-major
    (ff, fx, fy, fz, xx, xy, xz, yy, yz, zz), signed (cdx_gpis_joint)."""
    lib = N.load()
    X = X.contiguous()
    M = X.shape[0]
    cov = torch.empty(M, 10, dtype=torch.float64, device=X.device)
    if M:
        need = lib.cdx_gpis_joint_workspace(state.desc, M)
        if getattr(state, "joint_ws", None) is None or state.joint_ws.numel() < need:
            state.joint_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=X.device)
        N.check(lib.cdx_gpis_joint(state.desc, N.ptr(X), M, N.ptr(cov), N.ptr(state.joint_ws), N.stream_ptr(X.device)),
                "cdx_gpis_joint")
    return cov


def joint_prior(kernel, R, sigma):
    """(k0, κ, κ, κ): the prior variances of the value and of the gradient's components (csrc/cdx_gpis.h)."""
    R, inv_s2 = float(R), 1.0 / (float(sigma) * float(sigma))
    k0, kappa = {"tps": (R ** 3, 6.0 * R), "rbf": (1.0, inv_s2),
                 "joint": (0.3 + 0.7 * R ** 3, 0.3 * inv_s2 + 0.7 * 6.0 * R)}[kernel]
    return (k0, kappa, kappa, kappa)


def joint_cov_matrix(cov10):
    """[…, 10] upper triangle → the symmetric […, 4, 4]."""
    idx = torch.tensor(_FILL, dtype=torch.long, device=cov10.device)
    return cov10[..., idx]


def normal_covariance(grad, cov):
    """The delta method for n̂ = g/‖g‖ at the mean gradient ``grad`` […, 3] with the joint covariance ``cov``
    […, 4, 4] → NormalUncertainty.  Pure torch ops."""
    norm = grad.norm(dim=-1, keepdim=True)
    n = grad / norm
    P = torch.eye(3, dtype=grad.dtype, device=grad.device) - n.unsqueeze(-1) * n.unsqueeze(-2)
    cn = P @ cov[..., 1:, 1:] @ P / (norm * norm).unsqueeze(-1)
    tr = cn.diagonal(dim1=-2, dim2=-1).sum(-1)
    return NormalUncertainty(n, cn, tr.clamp(min=0.0).sqrt(), cov[..., 0, 0].clamp(min=0.0).sqrt() / norm.squeeze(-1))


def joint_cholesky(cov, prior):
    """The lower factor L […, 4, 4] of cov […, 4, 4], L·Lᵀ = cov, written out element by element (no batched LAPACK
    call, nothing raises).  A pivot ≤ PIVOT_REL × its prior entry — a component the data determine, or an indefinite Σ
    far from the data — zeroes its column: that component gets no noise of its own."""
    L = [[None] * 4 for _ in range(4)]
    zero = torch.zeros_like(cov[..., 0, 0])
    for j in range(4):
        d = cov[..., j, j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        ok = d > PIVOT_REL * prior[j]
        root = torch.where(ok, d, torch.ones_like(d)).sqrt()
        L[j][j] = torch.where(ok, root, zero)
        for i in range(j + 1, 4):
            v = cov[..., i, j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = torch.where(ok, v / root, zero)
        for i in range(j):
            L[i][j] = zero
    return torch.stack([torch.stack(row, -1) for row in L], -2)


def _standard_normal(shape, device, generator):
    """The sampler's noise: float64 standard normals on ``device`` (``generator``: a generator of that device)."""
    return torch.randn(shape, dtype=torch.float64, device=device, generator=generator)


def normals_from_samples(samples):
    """Joint draws […, 4] → (unit normals […, 3], surface offsets […] = −f/‖g‖: where, along the drawn normal and to
    first order, the drawn surface lies from the query)."""
    g = samples[..., 1:]
    norm = g.norm(dim=-1)
    return g / norm.unsqueeze(-1), -samples[..., 0] / norm


class _Pred(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, state):
        need = ctx.needs_input_grad[0]
        mean, gmean, _ = gpis_mean(state, X, want_grad=need)
        std, gstd = gpis_std(state, X, want_grad=need)
        ctx.save_for_backward(gmean if need else None, gstd if need else None)
        return mean, std

    @staticmethod
    def backward(ctx, g_mean, g_std):
        gmean, gstd = ctx.saved_tensors
        gX = None
        if ctx.needs_input_grad[0]:
            gX = torch.zeros_like(gmean)
            if g_mean is not None:
                gX = gX + g_mean.unsqueeze(1) * gmean
            if g_std is not None:
                gX = gX + g_std.unsqueeze(1) * gstd
        return gX, None


class GPIS:
    """GP implicit surface (gpis.py:4-168)."""

    def __init__(self, sigma=0.6, bias=2, kernel="tps"):
        if kernel not in N.KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}")
        self.sigma = sigma
        self.bias = bias
        self.fraction = None
        self.kernel = kernel
        self._state = None
        self._state_key = None
        self._gen = 0  # bumped by fit / load_state_data

    # ----------------------------------------------------------------- fit / io
    def fit(self, X1, y1, noise=0.0):
        """R = max cdist, E11 = K(X1, X1) + diag(noise²) (gpis.py:33-40), built on the device
        by cdx_gpis_fit; ``noise`` is a scalar or a per-point vector, as in the reference."""
        _require_cuda(X1, "GPIS fit points")
        dev = X1.device
        X1d = X1.to(torch.float64).contiguous()
        n = X1d.shape[0]
        if torch.is_tensor(noise):
            nz = noise.to(dev, torch.float64).reshape(-1)
            nz = (nz.expand(n) if nz.numel() == 1 else nz).contiguous()
        else:
            nz = torch.full((n,), float(noise), dtype=torch.float64, device=dev)
        E11 = torch.empty(n, n, dtype=torch.float64, device=dev)
        R = torch.zeros((), dtype=torch.float64, device=dev)
        lib = N.load()
        N.check(lib.cdx_gpis_fit(N.ptr(X1d), n, N.ptr(nz), N.KERNELS[self.kernel], float(self.sigma), N.ptr(E11),
                                 N.ptr(R), N.stream_ptr(dev)), "cdx_gpis_fit")
        if self.kernel in ("tps", "joint"):
            self.R = R
        self.X1 = X1
        self.y1 = y1 - self.bias
        self.noise = noise
        self.E11 = E11
        self._state = None
        self._gen += 1

    def fit_pointcloud(self, points, num_points=200, bound=0.15, n_internal=50, sharpness=30.0,
                       noise=(0.2, 0.005, 0.1), center="bbox", weights=None, generator=None, start=0,
                       outlier=None):
        """From a raw cloud [P, 3] on the device to the fitted state (optimize_pregrasp.py:904-922): a
        farthest-point sample of ``num_points`` rows (cdx_fps, beginning at row ``start``), the recipe of
        ``pointcloud.completion_arrays`` around it, then ``fit``.  ``center="bbox"`` shifts the exterior points by
        the centre of the bounding box of the whole finite cloud (:894), computed on the device; None leaves them at
        the origin, anything else is the centre itself.  ``bound=0.1, n_internal=5, sharpness=10,
        noise=(0.3, σ_obs, 0.02), center=None`` is train_gpis_completion.py.  The chosen rows stay in
        ``self.sample_index`` (selection order).  ``outlier=(nb_neighbors, std_ratio)`` first sets the rows that
        ``pointcloud.statistical_outlier_mask`` rejects to NaN: they are then never sampled and are left out of the
        bounding-box centre (``start`` itself is taken as given).  No host synchronisation from the cloud to
        ``E11``; returns self."""
        from . import pointcloud as PC
        _require_cuda(points, "point cloud")
        if points.dim() != 2:
            raise ValueError(f"point cloud must be [P, 3], got {tuple(points.shape)}")
        if outlier is not None:
            nb_neighbors, std_ratio = outlier
            keep = PC.statistical_outlier_mask(points, int(nb_neighbors), float(std_ratio))
            points = torch.where(keep.unsqueeze(1), points.detach(), torch.full_like(points, float("nan")))
        sel, _, surface = PC.fps(points, num_points, start, gather=True)
        if isinstance(center, str):
            if center != "bbox":
                raise ValueError(f"center must be 'bbox', None or a point, got {center!r}")
            center = PC.bbox_center(points)
        X1, y, nz = PC.completion_arrays(surface, bound, n_internal, sharpness, noise, center=center, weights=weights,
                                         generator=generator)
        self.fit(X1, y, noise=nz)
        self.sample_index = sel
        return self

    def fit_mesh(self, mesh, num_points=200, cloud_points=4096, init_factor=5, seed=0, **recipe):
        """From a ground-truth mesh to the fitted state: the Poisson-disk cloud the reference opens with
        (``sampling.sample_points_poisson_disk(mesh, cloud_points, init_factor, seed)``, optimize_pregrasp.py:887),
        then ``fit_pointcloud`` on it with ``num_points`` and the ``recipe`` arguments — the exterior points sit
        around the bounding-box centre of that cloud (:888).  ``mesh``: a ``TriangleMesh``, a ``PreparedMesh``, a
        ``SurfaceSampler`` or an [F, 3, 3] device tensor.  The cloud stays in ``self.sample_cloud``.  No host
        synchronisation beyond the sampler's one word per mesh; returns self."""
        from .sampling import sample_points_poisson_disk
        cloud = sample_points_poisson_disk(mesh, cloud_points, init_factor=init_factor, seed=seed)
        self.fit_pointcloud(cloud, num_points=num_points, **recipe)
        self.sample_cloud = cloud
        return self

    def save_state_data(self, name="gpis_state"):
        """npz {R, X1, y1, E11, bias} under gpis_states/ (gpis.py:155-160)."""
        os.makedirs("gpis_states", exist_ok=True)
        bias = self.bias.cpu().numpy() if torch.is_tensor(self.bias) else self.bias
        np.savez(f"gpis_states/{name}.npz", R=self.R.cpu().numpy(), X1=self.X1.cpu().numpy(),
                 y1=self.y1.cpu().numpy(), E11=self.E11.cpu().numpy(), bias=bias)

    def load_state_data(self, name="gpis_state", device="cuda"):
        """Reads gpis_states/{name}.npz (cwd first, then the packaged states) (gpis.py:162-168)."""
        path = f"gpis_states/{name}.npz"
        if not os.path.exists(path):
            path = os.path.join(_PKG_STATES, f"{name}.npz")
        data = np.load(path)
        self.R = torch.from_numpy(data["R"]).to(device)
        self.X1 = torch.from_numpy(data["X1"]).to(device)
        self.y1 = torch.from_numpy(data["y1"]).to(device)
        self.E11 = torch.from_numpy(data["E11"]).to(device)
        self.bias = torch.from_numpy(data["bias"]).double().to(device)
        self._state = None
        self._gen += 1

    # ------------------------------------------------------------ native state
    def _state_inputs(self):
        return (self.X1, self.y1, self.E11, getattr(self, "R", None), self.bias)

    def _state_current(self):
        """The cached state is current while every input is the same object (the cache holds them,
        so an id cannot be recycled) at the same torch version counter (an in-place edit bumps it),
        with the same kernel / sigma and no fit / load since."""
        if self._state is None or self._state_key is None:
            return False
        refs, vers, kernel, sigma, gen = self._state_key
        cur = self._state_inputs()
        for a, b, v in zip(refs, cur, vers):
            if torch.is_tensor(a) or torch.is_tensor(b):
                if a is not b or a._version != v:
                    return False
            elif a != b:
                return False
        return kernel == self.kernel and sigma == self.sigma and gen == self._gen

    def native_state(self):
        # no device->host sync per query (the key is host-side object identity + version counters);
        # the reference re-solves E11 on every call (gpis.py:53), this rebuilds only when it changed
        if not self._state_current():
            _require_cuda(self.X1, "GPIS state")
            R = float(self.R) if hasattr(self, "R") else 0.0
            self._state = _State(self.X1, self.y1, self.E11, R, float(self.bias), self.kernel, self.sigma)
            ins = self._state_inputs()
            self._state_key = (ins, tuple(t._version if torch.is_tensor(t) else None for t in ins), self.kernel,
                               self.sigma, self._gen)
        return self._state

    # ---------------------------------------------------------------- queries
    def pred(self, X2):
        """(mean, sqrt|diag Σ|) with the reference's shape rule (gpis.py:43-59)."""
        _require_cuda(X2, "GPIS query")
        shape = list(X2.shape)
        shape[-1] = 1
        Xf = X2.reshape(-1, 3).to(torch.float64)
        mean, std = _Pred.apply(Xf, self.native_state())
        return mean.view(shape[:-1]), std.view(shape[:-1])

    def pred_mean(self, X2):
        """Mean only (no posterior-variance GEMM); same shape rule as ``pred``."""
        _require_cuda(X2, "GPIS query")
        shape = list(X2.shape[:-1])
        mean, _, _ = gpis_mean(self.native_state(), X2.reshape(-1, 3).to(torch.float64).detach(), want_grad=False)
        return mean.view(shape)

    def compute_normal(self, X2, index=None):
        """∇mean/(‖∇mean‖+1e-8), detached (gpis.py:63-87).  ``index`` restricts the
        inducing points whose weights contribute, as the reference does."""
        _require_cuda(X2, "GPIS query")
        input_shape = X2.shape
        X = X2.detach().reshape(-1, 3).to(torch.float64).contiguous()
        st = self.native_state()
        if index is None:
            _, _, normal = gpis_mean(st, X, want_grad=False, want_normal=True)
            return normal.view(input_shape)
        idx = torch.as_tensor(index, device=X.device, dtype=torch.long)
        mask = torch.zeros_like(st.alpha)
        mask[idx] = 1.0
        sub = _State.__new__(_State)
        sub.__dict__.update(st.__dict__)
        sub.alpha = st.alpha * mask
        sub.desc = N.CdxGpis(X1=st.desc.X1, alpha=sub.alpha.data_ptr(), Ainv=st.desc.Ainv, Linv_t=st.desc.Linv_t, Linv=st.desc.Linv, N=st.desc.N,
                             N_pad=st.desc.N_pad, kernel=st.desc.kernel, R=st.desc.R, sigma=st.desc.sigma,
                             bias=st.desc.bias)
        _, _, normal = gpis_mean(sub, X, want_grad=False, want_normal=True)
        return normal.view(input_shape), st.alpha[idx].sum()

    def compute_multinormals(self, X2, num_normal_samples):
        """Normals from nested subsets of the inducing points (gpis.py:89-111)."""
        if self.fraction is None:
            self.fraction = torch.linspace(0.8, 1, num_normal_samples // 2)
            self.indices = []
            n = len(self.X1)
            for i in range(num_normal_samples // 2):
                self.indices.append(list(range(int(self.fraction[i] * n))))
            self.indices.append(list(range(n)))
            for i in range(num_normal_samples // 2):
                self.indices.append(list(range(int(1 - self.fraction[-i - 1]), n)))
        normals, weights = [], []
        for i in range(num_normal_samples):
            nrm, w = self.compute_normal(X2, self.indices[i])
            normals.append(nrm)
            weights.append(w.reshape(1))
        weights = torch.hstack(weights)
        return torch.stack(normals, dim=1), weights / weights.sum()

    # ------------------------------------------------- joint posterior of (f, ∇f)
    def pred_joint(self, X2):
        """(mean4 […, 4], cov […, 4, 4]): the posterior of (f, ∂f/∂x, ∂f/∂y, ∂f/∂z) at X2 […, 3], a Gaussian per
        query (queries are not correlated with each other here).  mean4 is (mean, ∇mean) of cdx_gpis_mean, cov the
        symmetric fill of cdx_gpis_joint's 10 entries; cov[…, 0, 0] is the signed variance whose sqrt|·| ``pred``
        returns.  Positive definite near the data; a TPS or joint state is indefinite farther than R from an inducing
        point, and the matrix is returned as it is.  Detached: no autograd."""
        _require_cuda(X2, "GPIS query")
        lead = list(X2.shape[:-1])
        X = X2.detach().reshape(-1, 3).to(torch.float64).contiguous()
        st = self.native_state()
        mean, gmean, _ = gpis_mean(st, X, want_grad=True)
        cov = joint_cov_matrix(gpis_joint_cov(st, X))
        return torch.cat([mean.unsqueeze(1), gmean], 1).view(lead + [4]), cov.view(lead + [4, 4])

    def _joint_prior(self):
        return joint_prior(self.kernel, float(self.R) if hasattr(self, "R") else 0.0, self.sigma)

    def normal_uncertainty(self, X2):
        """How well the surface normal and the surface's position are known at X2 […, 3] → NormalUncertainty (first
        order in the gradient's posterior covariance; torch ops on ``pred_joint``)."""
        mean4, cov = self.pred_joint(X2)
        return normal_covariance(mean4[..., 1:], cov)

    def sample_joint(self, X2, num_samples, generator=None):
        """``num_samples`` draws of (f, ∇f) at every query of X2 […, 3] → […, S, 4]: mean4 + L·z with L the 4 × 4 factor
        of ``joint_cholesky`` and z standard normal from ``generator`` (a generator of the queries' device).  Every query
        is drawn on its own: the correlation between queries is not modelled."""
        return self._draw_joint(*self.pred_joint(X2), num_samples, generator)

    def _draw_joint(self, mean4, cov, num_samples, generator):
        L = joint_cholesky(cov, self._joint_prior())
        z = _standard_normal(list(mean4.shape[:-1]) + [int(num_samples), 4], mean4.device, generator)
        return mean4.unsqueeze(-2) + (L.unsqueeze(-3) @ z.unsqueeze(-1)).squeeze(-1)

    def sample_normals(self, X2, num_samples, generator=None):
        """(unit normals […, S, 3], surface offsets […, S]) of ``sample_joint``'s draws (``normals_from_samples``);
        with no noise a draw is the mean normal ∇mean/‖∇mean‖."""
        return normals_from_samples(self.sample_joint(X2, num_samples, generator))

    def get_visualization_data(self, lb, ub, steps=100, fused=False):
        """Mean / std / normal on a steps³ grid (gpis.py:113-125).  ``fused=True`` evaluates the whole grid with
        one ``field`` call and one copy back instead of three kernel chains and three copies per slice."""
        if fused:
            with torch.no_grad():
                m, v, nrm = self.field(lb, ub, steps)
                out = torch.cat([m.reshape(-1), v.reshape(-1), nrm.reshape(-1)]).float().cpu().numpy()
            n = steps ** 3
            return (out[:n].reshape(steps, steps, steps), out[n:2 * n].reshape(steps, steps, steps),
                    out[2 * n:].reshape(steps, steps, steps, 3), np.asarray(lb), np.asarray(ub))
        dev = self.X1.device
        grid = torch.stack(torch.meshgrid(torch.linspace(lb[0], ub[0], steps), torch.linspace(lb[1], ub[1], steps),
                                          torch.linspace(lb[2], ub[2], steps), indexing="xy"), dim=3).double().to(dev)
        m = torch.zeros(steps, steps, steps)
        v = torch.zeros(steps, steps, steps)
        nrm = torch.zeros(steps, steps, steps, 3)
        with torch.no_grad():
            for i in range(steps):
                mean, var = self.pred(grid[i].reshape(-1, 3))
                nrm[i] = self.compute_normal(grid[i].reshape(-1, 3)).view(steps, steps, 3).cpu()
                m[i] = mean.view(steps, steps).cpu()
                v[i] = var.view(steps, steps).cpu()
        return m.numpy(), v.numpy(), nrm.numpy(), np.asarray(lb), np.asarray(ub)

    # ------------------------------------------------- lattice field / surface
    @staticmethod
    def _check_steps(steps):
        steps = int(steps)
        if not 1 <= steps <= N.FIELD_MAX_STEPS:
            raise ValueError(f"steps must be in 1..{N.FIELD_MAX_STEPS}, got {steps}")
        return steps

    def _query_axes(self, lb, ub, steps):
        """The reference's query axes (gpis.py:114-116): float32 linspace, then double; [3, steps] on the device."""
        ax = torch.stack([torch.linspace(float(lb[d]), float(ub[d]), steps) for d in range(3)]).double()
        return ax.to(self.X1.device).contiguous()

    def _point_axes(self, lb, ub, steps):
        """topcd's point axes (gpis.py:144-146): float64 numpy linspace; [3, steps] on the device."""
        lb, ub = np.asarray(lb), np.asarray(ub)
        ax = np.stack([np.linspace(lb[d], ub[d], steps) for d in range(3)]).astype(np.float64)
        return torch.from_numpy(ax).to(self.X1.device).contiguous()

    def field(self, lb, ub, steps=100, std=True, normal=True, chunk=0):
        """(mean [s, s, s], std [s, s, s] or None, normal [s, s, s, 3] or None), f64 on the device, on the lattice
        of ``get_visualization_data``: cell (i, j, k) at (x[j], y[i], z[k]).  One cdx_gpis_field call: the cells go
        through the mean kernel (mean and normal in one pass) and the whitened std pass ``chunk`` at a time
        (0: a default that keeps the workspace under 1 GiB), with no host sync."""
        steps = self._check_steps(steps)
        if chunk < 0:
            raise ValueError("chunk must be >= 0")
        st = self.native_state()
        dev = self.X1.device
        lib = N.load()
        ax = self._query_axes(lb, ub, steps)
        mean = torch.empty(steps, steps, steps, dtype=torch.float64, device=dev)
        sd = torch.empty(steps, steps, steps, dtype=torch.float64, device=dev) if std else None
        nrm = torch.empty(steps, steps, steps, 3, dtype=torch.float64, device=dev) if normal else None
        ws = torch.empty(max(lib.cdx_gpis_field_workspace(st.desc, steps, chunk), 1), dtype=torch.uint8, device=dev)
        N.check(lib.cdx_gpis_field(st.desc, N.ptr(ax[0]), N.ptr(ax[1]), N.ptr(ax[2]), steps, chunk, N.ptr(mean),
                                   N.ptr(sd), N.ptr(nrm), N.ptr(ws), N.stream_ptr(dev)), "cdx_gpis_field")
        return mean, sd, nrm

    def _surface_count(self, mean, dtype, steps, flip):
        """count + scan on the stream; (workspace, the total: ONE host read)."""
        lib = N.load()
        dev = mean.device
        ws = torch.empty(max(lib.cdx_gpis_surface_workspace(steps), 1), dtype=torch.uint8, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        N.check(lib.cdx_gpis_surface_count(N.ptr(mean), dtype, steps, flip, N.ptr(ws), N.ptr(total),
                                           N.stream_ptr(dev)), "cdx_gpis_surface_count")
        return ws, int(total.item())

    def topcd(self, test_mean, test_normal, lb, ub, steps=100):
        """Surface point cloud of a lattice field (gpis.py:127-150): (points float64 [n, 3], normals [n, 3]) as
        numpy — the interior cells with mean < 0 that have a face neighbour with mean ≥ 0, in C order.  Tensor
        inputs are read flipped along k as the reference does (:130-133, the points are not); numpy inputs are
        not.  Count and ordered placement run on the device (cdx_gpis_surface_count / _place)."""
        steps = self._check_steps(steps)
        _require_cuda(self.X1, "GPIS state")
        dev = self.X1.device
        flip = 1 if torch.is_tensor(test_mean) else 0
        if torch.is_tensor(test_normal) != bool(flip):
            raise TypeError("topcd takes test_mean and test_normal both as tensors or both as numpy arrays")
        mean = (test_mean.detach() if flip else torch.from_numpy(np.ascontiguousarray(test_mean))).to(dev)
        nrm = (test_normal.detach() if flip else torch.from_numpy(np.ascontiguousarray(test_normal))).to(dev)
        if mean.dtype not in (torch.float32, torch.float64):
            mean = mean.double()
        nrm = nrm.to(mean.dtype).contiguous()
        mean = mean.contiguous()
        if tuple(mean.shape) != (steps,) * 3 or tuple(nrm.shape) != (steps,) * 3 + (3,):
            raise ValueError(f"topcd expects mean [{steps}]*3 and normal [{steps}]*3 + [3], got "
                             f"{tuple(mean.shape)} and {tuple(nrm.shape)}")
        dtype = N.DTYPE_F32 if mean.dtype == torch.float32 else N.DTYPE_F64
        ws, n = self._surface_count(mean, dtype, steps, flip)
        points = torch.empty(n, 3, dtype=torch.float64, device=dev)
        normals = torch.empty(n, 3, dtype=mean.dtype, device=dev)
        if n:
            pax = self._point_axes(lb, ub, steps)
            N.check(N.load().cdx_gpis_surface_place(N.ptr(mean), N.ptr(nrm), dtype, steps, flip, N.ptr(pax[0]),
                                                    N.ptr(pax[1]), N.ptr(pax[2]), N.ptr(ws), n, None, N.ptr(points),
                                                    N.ptr(normals), N.stream_ptr(dev)), "cdx_gpis_surface_place")
        return points.cpu().numpy(), normals.cpu().numpy()

    def surface(self, lb, ub, steps=100):
        """The surface cloud straight from the state: (points [n, 3], normals [n, 3]) f64 device tensors, the
        cloud ``topcd`` gives for the numpy outputs of ``get_visualization_data`` without the lattice leaving the
        device.  Mean only on the lattice (no std pass), count and placement of the surface cells, then normals
        from one mean-kernel call on the surviving cells alone.  One host sync, for the count."""
        steps = self._check_steps(steps)
        st = self.native_state()
        dev = self.X1.device
        lib = N.load()
        with torch.no_grad():
            mean, _, _ = self.field(lb, ub, steps, std=False, normal=False)
            ws, n = self._surface_count(mean, N.DTYPE_F64, steps, 0)
            points = torch.empty(n, 3, dtype=torch.float64, device=dev)
            normals = torch.empty(n, 3, dtype=torch.float64, device=dev)
            if n:
                pax = self._point_axes(lb, ub, steps)
                qax = self._query_axes(lb, ub, steps)
                cells = torch.empty(n, dtype=torch.int64, device=dev)
                N.check(lib.cdx_gpis_surface_place(N.ptr(mean), None, N.DTYPE_F64, steps, 0, N.ptr(pax[0]),
                                                   N.ptr(pax[1]), N.ptr(pax[2]), N.ptr(ws), n, N.ptr(cells),
                                                   N.ptr(points), None, N.stream_ptr(dev)), "cdx_gpis_surface_place")
                X = torch.empty(n, 3, dtype=torch.float64, device=dev)
                N.check(lib.cdx_gpis_field_points(N.ptr(qax[0]), N.ptr(qax[1]), N.ptr(qax[2]), steps, N.ptr(cells), n,
                                                  N.ptr(X), N.stream_ptr(dev)), "cdx_gpis_field_points")
                m2 = torch.empty(n, dtype=torch.float64, device=dev)
                N.check(lib.cdx_gpis_mean(st.desc, N.ptr(X), n, N.ptr(m2), None, N.ptr(normals), N.stream_ptr(dev)),
                        "cdx_gpis_mean")
        return points, normals

    # ------------------------------------------------------- iso-surface mesh
    def _mesh_extract(self, mean, dtype, steps, pax):
        """count → ONE host read (both totals) → place: (vertices [V, 3] f64, edges [V] int64, faces [F, 3] int32)."""
        lib = N.load()
        dev = mean.device
        ws = torch.empty(max(lib.cdx_gpis_mesh_workspace(steps), 1), dtype=torch.uint8, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        N.check(lib.cdx_gpis_mesh_count(N.ptr(mean), dtype, steps, N.ptr(ws), N.ptr(totals), N.stream_ptr(dev)),
                "cdx_gpis_mesh_count")
        nv, nf = (int(x) for x in totals.cpu())
        vertices = torch.empty(nv, 3, dtype=torch.float64, device=dev)
        edges = torch.empty(nv, dtype=torch.int64, device=dev)
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        if nv:
            N.check(lib.cdx_gpis_mesh_place(N.ptr(mean), dtype, steps, N.ptr(pax[0]), N.ptr(pax[1]), N.ptr(pax[2]),
                                            N.ptr(ws), nv, nf, N.ptr(vertices), N.ptr(edges), N.ptr(faces),
                                            N.stream_ptr(dev)), "cdx_gpis_mesh_place")
        return vertices, edges, faces

    def tomesh(self, test_mean, lb, ub, steps=100):
        """Triangle mesh of the zero level of a lattice field: (vertices float64 [V, 3], triangles int32 [F, 3]) as
        numpy.  ``test_mean`` [steps]*3 is a numpy array or a tensor, float32 or float64, read as it stands (no flip:
        that is ``topcd``'s reference quirk) on ``topcd``'s float64 point lattice.  Marching tetrahedra on the lattice
        (csrc/cdx_mesh.h): a vertex on every lattice edge whose ends differ in mean < 0, triangles wound outwards,
        closed and manifold wherever the surface stays off the lattice's border.  The reference meshes its completed
        shape with open3d's Poisson reconstruction (train_gpis_completion.py:67-76); parity with it is not attempted.
        Count and ordered placement run on the device (cdx_gpis_mesh_count / _place); one host read for the totals."""
        steps = self._check_steps(steps)
        _require_cuda(self.X1, "GPIS state")
        dev = self.X1.device
        mean = (test_mean.detach() if torch.is_tensor(test_mean) else
                torch.from_numpy(np.ascontiguousarray(test_mean))).to(dev)
        if mean.dtype not in (torch.float32, torch.float64):
            mean = mean.double()
        mean = mean.contiguous()
        if tuple(mean.shape) != (steps,) * 3:
            raise ValueError(f"tomesh expects mean [{steps}]*3, got {tuple(mean.shape)}")
        dtype = N.DTYPE_F32 if mean.dtype == torch.float32 else N.DTYPE_F64
        vertices, _, faces = self._mesh_extract(mean, dtype, steps, self._point_axes(lb, ub, steps))
        return vertices.cpu().numpy(), faces.cpu().numpy()

    def surface_mesh(self, lb, ub, steps=100, refine=0, normals=True):
        """The mesh straight from the state: (vertices [V, 3] f64, faces [F, 3] int32, normals [V, 3] f64 or None) as
        device tensors.  The mean alone is evaluated on the lattice of the float64 point axes (one set of axes for
        evaluation and placement: a vertex's end values are the field at its end positions), then count, one host
        read, place — ``tomesh`` of that lattice without it leaving the device.  ``refine`` steps of bracketed regula
        falsi move every vertex along its own lattice edge towards the zero of the GPIS mean (cdx_gpis_mesh_refine_init /
        _step with one cdx_gpis_mean call per step; ``mesh.EdgeRefiner`` is the same rule in torch ops, with the same
        bits); the faces do not change.  The normals are the GPIS normals at the vertices (one
        cdx_gpis_mean call, as ``surface`` does)."""
        steps = self._check_steps(steps)
        st = self.native_state()
        dev = self.X1.device
        lib = N.load()
        with torch.no_grad():
            pax = self._point_axes(lb, ub, steps)
            mean = torch.empty(steps, steps, steps, dtype=torch.float64, device=dev)
            ws = torch.empty(max(lib.cdx_gpis_field_workspace(st.desc, steps, 0), 1), dtype=torch.uint8, device=dev)
            N.check(lib.cdx_gpis_field(st.desc, N.ptr(pax[0]), N.ptr(pax[1]), N.ptr(pax[2]), steps, 0, N.ptr(mean), None,
                                       None, N.ptr(ws), N.stream_ptr(dev)), "cdx_gpis_field")
            vertices, edges, faces = self._mesh_extract(mean, N.DTYPE_F64, steps, pax)
            nv = vertices.shape[0]
            if refine and nv:
                # bracketed regula falsi along each vertex's own edge (csrc/cdx_mesh.h; mesh.EdgeRefiner states it
                # in torch ops): cdx_gpis_mesh_refine_init, then per step one cdx_gpis_mean and one _refine_step
                state = torch.empty(5, nv, dtype=torch.float64, device=dev)
                fv = torch.empty(nv, dtype=torch.float64, device=dev)
                s = N.stream_ptr(dev)
                N.check(lib.cdx_gpis_mesh_refine_init(N.ptr(mean), N.DTYPE_F64, steps, N.ptr(pax[0]), N.ptr(pax[1]),
                                                      N.ptr(pax[2]), N.ptr(edges), nv, N.ptr(state), N.ptr(vertices), s),
                        "cdx_gpis_mesh_refine_init")
                for _ in range(int(refine)):
                    N.check(lib.cdx_gpis_mean(st.desc, N.ptr(vertices), nv, N.ptr(fv), None, None, s), "cdx_gpis_mean")
                    N.check(lib.cdx_gpis_mesh_refine_step(N.ptr(fv), steps, N.ptr(pax[0]), N.ptr(pax[1]), N.ptr(pax[2]),
                                                          N.ptr(edges), nv, N.ptr(state), N.ptr(vertices), s),
                            "cdx_gpis_mesh_refine_step")
            nrm = None
            if normals:
                nrm = torch.empty(nv, 3, dtype=torch.float64, device=dev)
                if nv:
                    m2 = torch.empty(nv, dtype=torch.float64, device=dev)
                    N.check(lib.cdx_gpis_mean(st.desc, N.ptr(vertices), nv, N.ptr(m2), None, N.ptr(nrm),
                                              N.stream_ptr(dev)), "cdx_gpis_mean")
        return vertices, faces, nrm
