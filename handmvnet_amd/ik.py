"""Hand pose parameters on the device: everything the reference's JointsToVertices (models/joints_to_vertices.py:9-50) does around its
MANO layer -- the three-point rigid alignment onto the template (utils/misc.py:10-47), the analytic inverse kinematics adaptive_IK
(utils/analytical_ik.py:50-138) and the un-alignment of the vertices -- as two device launches (csrc/hand_ik.hip, include/handmv.h
"hand IK") instead of a per-sample host loop (handmvnet.py:395-398: readback, numpy, upload, per sample).

    hand_ik(joints_mm, template)     -> (pose_R [B, 16, 3, 3], align [B, 12] float64, status [B]): the 16 rotation matrices a MANO layer
                                        takes -- the hand's joint angles, a product output in their own right
    rigid_unapply(points, align)     -> R^T (points - t)
    JointsToVertices(mano_layer)     the batched drop-in for the reference class; the MANO layer is the caller's

The MANO layer is plugged in as a callable: mano.ManoSkin (this package's skinning kernel over the caller's MANO arrays) or the
caller's own, e.g. a manopth ManoLayer."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .mano import ManoSkin

STATUS_OK, STATUS_NONFINITE = 0, 1   # include/handmv.h: hmv_op_hand_ik


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ordinal(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _check_template(template) -> torch.Tensor:
    if not isinstance(template, torch.Tensor) or tuple(template.shape) != (21, 3):
        raise ValueError("template must be a [21, 3] tensor (the flat-hand joints of the MANO layer)")
    return template


def hand_ik(joints_mm: torch.Tensor, template: torch.Tensor, return_aligned: bool = False):
    """joints_mm fp32 [B, 21, 3] (the prediction in millimetres, joints_cam * 1000) and the flat-hand template [21, 3] of the MANO
    layer in its units -> (pose_R fp32 [B, 16, 3, 3], align float64 [B, 12] = ret_R row-major then ret_t, status int32 [B]; with
    return_aligned also joints_to_mano fp32 [B, 21, 3]).  pose_R[:, 0] is the global rotation -- a reflection for a mirrored hand with
    a non-planar palm, as in the reference -- and slot ID2ROT[k] the rotation of joint k against its parent.  status 1: some value of
    the row is non-finite (a non-finite input, a bone collinear with its template bone, coincident points); the values are what the
    reference computes there, NaN included.  Device tensors in and out on the current stream; nothing synchronises."""
    if not isinstance(joints_mm, torch.Tensor) or joints_mm.dim() != 3 or tuple(joints_mm.shape[1:]) != (21, 3):
        raise ValueError("joints_mm must be a [B, 21, 3] tensor")
    _check_template(template)
    if not joints_mm.is_cuda or not template.is_cuda:
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: joints_mm and template must be CUDA(HIP) tensors (no CPU fallback)")
    dev = joints_mm.device
    b = int(joints_mm.shape[0])
    j = joints_mm.detach().contiguous().float()
    t = template.detach().to(dev).contiguous().float()
    pose = torch.empty(b, 16, 3, 3, device=dev, dtype=torch.float32)
    align = torch.empty(b, 12, device=dev, dtype=torch.float64)
    status = torch.empty(b, device=dev, dtype=torch.int32)
    aligned = torch.empty(b, 21, 3, device=dev, dtype=torch.float32) if return_aligned else None
    if b > 0:
        with torch.cuda.device(dev):
            rc = _lib.load().hmv_op_hand_ik(_ordinal(dev), j.data_ptr(), t.data_ptr(), b, pose.data_ptr(), align.data_ptr(),
                                            aligned.data_ptr() if aligned is not None else None, status.data_ptr(), _stream(dev))
        _lib.check(rc)
    return (pose, align, status, aligned) if return_aligned else (pose, align, status)


def rigid_unapply(points: torch.Tensor, align: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """points fp32 [B, N, 3] and align float64 [B, 12] as hand_ik returned it -> R^T (points - t) fp32 [B, N, 3], computed in fp64
    and rounded once (joints_to_vertices.py:48).  out may be `points` itself (contiguous fp32): the op works in place."""
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError("points must be a [B, N, 3] tensor")
    if not isinstance(align, torch.Tensor) or tuple(align.shape) != (points.shape[0], 12) or align.dtype != torch.float64:
        raise ValueError(f"align must be a float64 [{points.shape[0]}, 12] tensor, as hand_ik returns it")
    if not points.is_cuda or not align.is_cuda:
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: points and align must be CUDA(HIP) tensors (no CPU fallback)")
    dev = points.device
    b, n_pts = int(points.shape[0]), int(points.shape[1])
    p = points.detach().contiguous().float()
    a = align.to(dev).contiguous()
    if out is None:
        out = torch.empty_like(p)
    elif tuple(out.shape) != tuple(p.shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous fp32 tensor of points' shape on points' device")
    if b > 0 and n_pts > 0:
        with torch.cuda.device(dev):
            rc = _lib.load().hmv_op_rigid_unapply(_ordinal(dev), p.data_ptr(), a.data_ptr(), b, n_pts, out.data_ptr(), _stream(dev))
        _lib.check(rc)
    return out


class JointsToVertices:
    """The reference's JointsToVertices (joints_to_vertices.py:9-50), batched and on the device.

        j2v = JointsToVertices(mano_layer)            # e.g. manopth.ManoLayer(root_rot_mode="rotmat", joint_rot_mode="rotmat", ...).to(dev)
        vertices = j2v(joints_cam * 1000)             # [B, 21, 3] mm -> [B, Nv, 3]
        model.joints_to_vertices = j2v                # and test_step reports the vertex metrics (get_vertices: true)

    mano_layer: any callable that maps rotation matrices [B, 16, 3, 3] to (vertices [B, Nv, 3], joints [B, 21, 3]) on the device of
    its input.  template: its flat-hand joints [21, 3]; by default mano_layer(identity)[1], as joints_to_vertices.py:23.  The
    constructor reads the template back once to refuse one with a zero-length bone (every result would be NaN).  __call__ runs the
    IK launch, the layer and the un-alignment launch with no copy to the host, and leaves last_pose_R [B, 16, 3, 3] and last_status
    [B] (hand_ik's) on the object.  With a mano.ManoSkin as mano_layer (this package's own MANO layer) the alignment goes into the skin
    launch and there is no un-alignment launch; the skin's own status is mano_layer.last_status."""

    PARENTS = (0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19)   # SNAP_PARENT, analytical_ik.py:8-30

    def __init__(self, mano_layer, template=None, device=None):
        if not callable(mano_layer):
            raise TypeError("mano_layer must be callable: rotation matrices [B, 16, 3, 3] -> (vertices [B, Nv, 3], joints [B, 21, 3])")
        self.mano_layer = mano_layer
        if template is None:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            template = mano_layer(torch.eye(3, device=dev).repeat(1, 16, 1, 1))[1]
            template = template.reshape(-1, 3) if isinstance(template, torch.Tensor) and template.numel() == 63 else template
        template = torch.as_tensor(template)
        _check_template(template)
        if device is not None:
            template = template.to(device)
        host = template.detach().double().cpu()
        if not bool(torch.isfinite(host).all()):
            raise ValueError("template holds a non-finite joint")
        bones = host[1:] - host[list(self.PARENTS[1:])]
        if bool((bones.norm(dim=-1) == 0).any()):
            k = int((bones.norm(dim=-1) == 0).nonzero()[0]) + 1
            raise ValueError(f"template has a zero-length bone (joint {k} coincides with its parent {self.PARENTS[k]})")
        self.joints_template = template.detach().float().contiguous()
        self.last_pose_R = None
        self.last_status = None

    def __call__(self, joints_mm: torch.Tensor) -> torch.Tensor:
        if self.joints_template.device != joints_mm.device and joints_mm.is_cuda:
            self.joints_template = self.joints_template.to(joints_mm.device)
        pose_R, align, status = hand_ik(joints_mm, self.joints_template)
        self.last_pose_R, self.last_status = pose_R, status
        if isinstance(self.mano_layer, ManoSkin):   # the un-alignment runs inside the skin launch: one launch and one rounding fewer
            return self.mano_layer(pose_R, align=align, joints=False)[0]
        vertices = self.mano_layer(pose_R)[0]
        return rigid_unapply(vertices, align)
