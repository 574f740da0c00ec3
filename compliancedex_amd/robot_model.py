"""Drop-in for ``DifferentiableRobotModel`` FK (thirdparty/differentiable-robot-model/
differentiable_robot_model/robot_model.py) on MI355X: ``compute_forward_kinematics``
(:224-264) with the reference's float32 arithmetic and gradient (cdx_fk_forward /
cdx_fk_backward), ``compute_endeffector_jacobian`` (:643-683, cdx_fk_jacobian) and, beyond the
reference, batched inverse kinematics (cdx_ik_solve, ik.py).  Dynamics (ID/FD/ABA, :266-806) are
not on the path.
"""
from __future__ import annotations

import torch

from . import _native as N
from .chain import Chain
from .urdf import load_robot


class _FK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, chain_desc):
        lib = N.load()
        qf = q.detach().to(torch.float32).contiguous()
        B, T = qf.shape[0], chain_desc.n_tips
        pos = torch.empty(B, 3 * T, dtype=torch.float32, device=q.device)
        quat = torch.empty(B, 4 * T, dtype=torch.float32, device=q.device)
        N.check(lib.cdx_fk_forward(chain_desc, N.ptr(qf), B, N.ptr(pos), N.ptr(quat), N.stream_ptr(q.device)),
                "cdx_fk_forward")
        ctx.save_for_backward(qf)
        ctx.chain_desc = chain_desc
        ctx.q_dtype = q.dtype
        ctx.mark_non_differentiable(quat)
        return pos, quat

    @staticmethod
    def backward(ctx, g_pos, g_quat):
        (qf,) = ctx.saved_tensors
        gq = None
        if ctx.needs_input_grad[0] and g_pos is not None:
            lib = N.load()
            gq = torch.empty_like(qf)
            N.check(lib.cdx_fk_backward(ctx.chain_desc, N.ptr(qf), qf.shape[0],
                                        N.ptr(g_pos.to(torch.float32).contiguous()), N.ptr(gq),
                                        N.stream_ptr(qf.device)), "cdx_fk_backward")
            gq = gq.to(ctx.q_dtype)
        return gq, None


class DifferentiableRobotModel(torch.nn.Module):
    """``urdf_path``: a URDF file, or a packaged robot name (allegro, leap, iiwa7_allegro)."""

    def __init__(self, urdf_path: str, name="", device=None):
        super().__init__()
        self.name = name
        self._device = torch.device(device) if device is not None else torch.device("cuda")
        self.chain = Chain(load_robot(urdf_path))
        self._n_dofs = self.chain.n_dofs
        self._name_to_idx_map = dict(self.chain.index)
        self._desc_cache = {}

    def _descriptor(self, link_names, offsets):
        key = (tuple(link_names), None if offsets is None else tuple(tuple(float(v) for v in o) for o in offsets))
        d = self._desc_cache.get(key)
        if d is None:
            d = self._desc_cache[key] = self.chain.descriptor(list(link_names), offsets)
        return d

    def get_joint_limits(self):
        return [dict(lower=b["lower"], upper=b["upper"]) for i, b in enumerate(self.chain.bodies) if self.chain.dof[i] >= 0]

    def compute_forward_kinematics(self, q: torch.Tensor, link_names: list, recursive: bool = False, offsets=None):
        """→ (pos [B, 3L], quat [B, 4L] xyzw), float32 (robot_model.py:224-264).

        ``recursive=True`` returns the same fresh-state result: the reference's recursive
        branch composes with each body's pose left over from the previous call
        (rigid_body.py:111-118) and is used only by the out-of-scope Kin/WC optimizers."""
        self._check_q(q)
        squeeze = q.ndim == 1
        q2 = q.unsqueeze(0) if squeeze else q
        pos, quat = _FK.apply(q2, self._descriptor(link_names, offsets))
        if squeeze:
            return pos[0], quat[0]
        return pos, quat

    def _check_q(self, q):
        if q.device.type != self._device.type:
            raise AssertionError(f"Input argument of different device as module: {q.device}")
        if q.ndim not in (1, 2):
            raise AssertionError("Input tensors must have ndim of 1 or 2.")
        if q.shape[-1] != self._n_dofs:
            raise AssertionError(f"q must have {self._n_dofs} joints")
        if not q.is_cuda:
            raise RuntimeError("compliancedex_amd FK runs on the GPU only")

    def compute_fingertip_jacobians(self, q: torch.Tensor, link_names: list, offsets=None):
        """→ (lin [B, T, 3, D], ang [B, T, 3, D]) float32: the geometric Jacobians of the links' positions (with
        ``offsets``: of the offset points) and the joint axes, columns of joints off a link's path 0.  ``q`` is
        rounded to float32 like the FK's.  The true derivative of ``compute_forward_kinematics``'s positions — its
        autograd gradient differs where an offset is set (the reference's detached quaternion scale).  No autograd
        through it."""
        self._check_q(q)
        lib = N.load()
        qf = q.detach().to(torch.float32)
        qf = (qf.unsqueeze(0) if qf.ndim == 1 else qf).contiguous()
        B, T, D = qf.shape[0], len(link_names), self._n_dofs
        lin = torch.empty(B, T, 3, D, dtype=torch.float32, device=q.device)
        ang = torch.empty(B, T, 3, D, dtype=torch.float32, device=q.device)
        N.check(lib.cdx_fk_jacobian(self._descriptor(link_names, offsets), N.ptr(qf), B, N.ptr(lin), N.ptr(ang),
                                    N.stream_ptr(q.device)), "cdx_fk_jacobian")
        return lin, ang

    def compute_endeffector_jacobian(self, q: torch.Tensor, link_name: str, offset=None):
        """→ (lin_jac [B, 3, n_dofs], ang_jac [B, 3, n_dofs]) float32 (robot_model.py:643-683; ``offset``, a point in
        the link's frame, is the one addition)."""
        lin, ang = self.compute_fingertip_jacobians(q, [link_name], None if offset is None else [offset])
        return lin[:, 0], ang[:, 0]

    def inverse_kinematics(self, target, link_names, offsets=None, q0=None, palm_pose=None, palm_offset=None,
                           weights=None, ref_q=None, rho=0.0, max_iters=None, tol=1e-5, solve_palm=False, **lm):
        """Joint angles whose fingertips reach ``target`` [E, T, 3] → IKResult(q, err, iters, status); see
        ik.solve_ik.  ``solve_palm=True`` solves the palm's pose with the joints → IKPoseResult (ik.solve_ik_pose);
        ``palm_pose`` is then only the start (None: the Kabsch start).  ``max_iters`` None: 50, or 100 with the palm."""
        from .ik import solve_ik, solve_ik_pose
        if solve_palm:
            return solve_ik_pose(self, target, link_names, offsets, q0, palm_pose, palm_offset, weights, ref_q, rho,
                                 100 if max_iters is None else max_iters, tol, **lm)
        return solve_ik(self, target, link_names, offsets, q0, palm_pose, palm_offset, weights, ref_q, rho,
                        50 if max_iters is None else max_iters, tol, **lm)
