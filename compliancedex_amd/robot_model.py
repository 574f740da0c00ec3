"""Drop-in for ``DifferentiableRobotModel`` FK (thirdparty/differentiable-robot-model/
differentiable_robot_model/robot_model.py) on MI355X: ``compute_forward_kinematics``
(:224-264) with the reference's float32 arithmetic and gradient (cdx_fk_forward /
cdx_fk_backward), ``compute_endeffector_jacobian`` (:643-683, cdx_fk_jacobian), beyond the
reference batched inverse kinematics (cdx_ik_solve, ik.py), and the dynamics block (:266-640):
``compute_inverse_dynamics``, ``compute_non_linear_effects``, ``compute_lagrangian_inertia_matrix``,
``compute_forward_dynamics`` on the device (cdx_dyn_inverse / cdx_dyn_inertia / cdx_dyn_forward, csrc/cdx_dyn.h), with
``gravity_compensation`` and ``get_joint_effort_limits`` beside them.  The dynamics carry no autograd (the
reference's learnable-parameter variants, :686-806, are not provided).
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
        self._dyn_cache = {}

    def _descriptor(self, link_names, offsets):
        key = (tuple(link_names), None if offsets is None else tuple(tuple(float(v) for v in o) for o in offsets))
        d = self._desc_cache.get(key)
        if d is None:
            d = self._desc_cache[key] = self.chain.descriptor(list(link_names), offsets)
        return d

    def get_joint_limits(self):
        return [dict(lower=b["lower"], upper=b["upper"]) for i, b in enumerate(self.chain.bodies) if self.chain.dof[i] >= 0]

    def get_joint_effort_limits(self):
        """The URDF's ``limit effort`` per joint (N·m), in DOF order."""
        return self.chain.effort_limits()

    # ---------------------------------------------------------------- dynamics (no autograd through any of them)
    def _dyn(self, device):
        """(host cdx_dyn, its device copy): the kernels read the constants from device memory (include/cdx.h)."""
        key = str(device)
        hit = self._dyn_cache.get(key)
        if hit is None:
            host = self.chain.dynamics_descriptor()
            dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device)
            hit = self._dyn_cache[key] = (host, dev)
        return hit

    def _dyn_descriptor(self, link_names, offsets):
        if not link_names:
            link_names, offsets = [], None
        key = ("dyn", tuple(link_names), None if offsets is None else tuple(tuple(float(v) for v in o) for o in offsets))
        d = self._desc_cache.get(key)
        if d is None:
            d = self._desc_cache[key] = self.chain.descriptor(list(link_names), offsets, check_depth=False)
        return d

    def _dyn_rows(self, q, *others):
        """q and its companions as detached contiguous [B, D] tensors of q's dtype (float32 or float64)."""
        self._check_q(q)
        dtype = q.dtype if q.dtype in (torch.float32, torch.float64) else torch.float64
        out = []
        for t in (q,) + others:
            if t is None:
                out.append(None)
                continue
            t = torch.as_tensor(t, device=q.device).detach().to(dtype)
            t = t.unsqueeze(0) if t.ndim == 1 else t
            if t.ndim != 2 or t.shape[1] != self._n_dofs or t.shape[0] != (out[0].shape[0] if out else t.shape[0]):
                raise AssertionError(f"expected [batch_size, {self._n_dofs}] like q, got {tuple(t.shape)}")
            out.append(t.contiguous())
        return out, (N.DTYPE_F64 if dtype == torch.float64 else N.DTYPE_F32), q.ndim == 1

    @staticmethod
    def _gravity_arg(gravity, B, device):
        """(tensor | None, per_row) of a gravity [3] or [B, 3] in the base frame."""
        if gravity is None:
            return None, 0
        g = torch.as_tensor(gravity, dtype=torch.float64, device=device).detach()
        if g.shape not in ((3,), (B, 3)):
            raise ValueError(f"gravity must have shape (3,) or ({B}, 3), got {tuple(g.shape)}")
        return g.contiguous(), int(g.ndim == 2)

    def compute_inverse_dynamics(self, q, qd, qdd_des, include_gravity=True, use_damping=True, *, gravity=None,
                                 tip_forces=None, link_names=None, offsets=None):
        """→ tau [B, D] of q's dtype: the joint torques that give ``qdd_des`` at (q, qd) (robot_model.py:322-391;
        recursive Newton–Euler in one launch, cdx_dyn_inverse).  ``use_damping`` adds damping·qd.  Beyond the
        reference: ``gravity`` [3] or [B, 3], the gravity vector in the base frame (None: (0, 0, −9.81)), and
        ``tip_forces`` [B, T, 3], external forces in the base frame acting at ``link_names`` (+ ``offsets``, points in
        the links' frames) — tau is then what the joints must supply, τ − Σ JᵀF.  ``qd`` / ``qdd_des`` None: zero.
        No autograd: inputs are detached."""
        (q2, qd2, qdd2), dtype, squeeze = self._dyn_rows(q, qd, qdd_des)
        lib = N.load()
        B = q2.shape[0]
        tf = None
        if tip_forces is not None:
            if not link_names:
                raise ValueError("tip_forces needs link_names")
            tf = torch.as_tensor(tip_forces, dtype=torch.float64, device=q.device).detach()
            if tf.shape != (B, len(link_names), 3):
                raise ValueError(f"tip_forces must have shape {(B, len(link_names), 3)}, got {tuple(tf.shape)}")
            tf = tf.contiguous()
        g, per_row = self._gravity_arg(gravity, B, q.device)
        tau = torch.empty_like(q2)
        N.check(lib.cdx_dyn_inverse(self._dyn_descriptor(link_names if tf is not None else None, offsets),
                                    N.ptr(self._dyn(q.device)[1]), B, N.ptr(q2), N.ptr(qd2), N.ptr(qdd2), dtype,
                                    int(bool(include_gravity)), int(bool(use_damping)), N.ptr(g), per_row, N.ptr(tf),
                                    N.ptr(tau), N.stream_ptr(q.device)), "cdx_dyn_inverse")
        return tau[0] if squeeze else tau

    def compute_non_linear_effects(self, q, qd, include_gravity=True, use_damping=True):
        """→ [B, D]: Coriolis, centrifugal, gravity and damping torques — the inverse dynamics at zero acceleration
        (robot_model.py:394-416).  No autograd."""
        return self.compute_inverse_dynamics(q, qd, None, include_gravity, use_damping)

    def gravity_compensation(self, q, gravity=None):
        """→ [B, D]: the torques that hold the chain still at q against ``gravity`` (base frame; None: (0, 0, −9.81)).
        No autograd."""
        return self.compute_inverse_dynamics(q, None, None, True, False, gravity=gravity)

    def compute_lagrangian_inertia_matrix(self, q, include_gravity=True, use_damping=True):
        """→ H [B, D, D] of q's dtype, symmetric bit for bit (robot_model.py:419-466; cdx_dyn_inertia).  The two flags
        cancel in the reference (H is a difference of two passes that share them) and are accepted.  No autograd."""
        (q2,), dtype, squeeze = self._dyn_rows(q)
        lib = N.load()
        B, D = q2.shape
        H = torch.empty(B, D, D, dtype=q2.dtype, device=q.device)
        N.check(lib.cdx_dyn_inertia(self._dyn_descriptor(None, None), N.ptr(self._dyn(q.device)[1]), B, N.ptr(q2), dtype,
                                    N.ptr(H), N.stream_ptr(q.device)), "cdx_dyn_inertia")
        return H[0] if squeeze else H

    def compute_forward_dynamics(self, q, qd, f, include_gravity=True, use_damping=False, *, gravity=None):
        """→ qdd [B, D] of q's dtype: the accelerations the torques ``f`` cause at (q, qd) (robot_model.py:504-640;
        cdx_dyn_forward solves H·qdd = f − damping·qd − nle, what the reference's articulated-body sweep solves).
        ``use_damping`` takes damping·qd from a copy: the caller's ``f`` is not written (the reference edits it in
        place, :537).  No autograd."""
        (q2, qd2, f2), dtype, squeeze = self._dyn_rows(q, qd, f)
        if f2 is None:
            raise ValueError("f is required")
        lib = N.load()
        B = q2.shape[0]
        g, per_row = self._gravity_arg(gravity, B, q.device)
        qdd = torch.empty_like(q2)
        N.check(lib.cdx_dyn_forward(self._dyn_descriptor(None, None), N.ptr(self._dyn(q.device)[1]), B, N.ptr(q2),
                                    N.ptr(qd2), N.ptr(f2), dtype, int(bool(include_gravity)), int(bool(use_damping)),
                                    N.ptr(g), per_row, N.ptr(qdd), N.stream_ptr(q.device)), "cdx_dyn_forward")
        return qdd[0] if squeeze else qdd

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
                           weights=None, ref_q=None, rho=0.0, max_iters=None, tol=1e-5, solve_palm=False,
                           target_rot=None, oriented=None, joints=None, rot_weights=0.1, **lm):
        """Joint angles whose fingertips reach ``target`` [E, T, 3] → IKResult(q, err, iters, status); see
        ik.solve_ik.  ``solve_palm=True`` solves the palm's pose with the joints → IKPoseResult (ik.solve_ik_pose);
        ``palm_pose`` is then only the start (None: the Kabsch start).  ``target_rot`` [E, T, 3, 3] or [E, T, 4] (xyzw)
        also asks for the links' orientations → IKFrameResult (ik.solve_ik_frames, which explains ``oriented``,
        ``joints`` and ``rot_weights``); ``palm_pose`` is then the pose of the chain's root.  ``max_iters`` None: 50, or
        100 with the palm or with orientations."""
        from .ik import solve_ik, solve_ik_frames, solve_ik_pose
        if target_rot is not None:
            if solve_palm:
                raise ValueError("target_rot and solve_palm=True exclude each other: the free-wrist solve takes "
                                 "positions only")
            return solve_ik_frames(self, target, target_rot, link_names, offsets, q0, palm_pose, palm_offset, weights,
                                   rot_weights, oriented, joints, ref_q, rho, 100 if max_iters is None else max_iters,
                                   tol, **lm)
        if oriented is not None or joints is not None:
            raise ValueError("oriented / joints need target_rot")
        if solve_palm:
            return solve_ik_pose(self, target, link_names, offsets, q0, palm_pose, palm_offset, weights, ref_q, rho,
                                 100 if max_iters is None else max_iters, tol, **lm)
        return solve_ik(self, target, link_names, offsets, q0, palm_pose, palm_offset, weights, ref_q, rho,
                        50 if max_iters is None else max_iters, tol, **lm)
