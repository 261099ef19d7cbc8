"""The reference's reprojection (/root/reference/src/utils/camera.py:25-44) as one device launch instead of a Python loop
over batch x views with a torch.inverse per turn (``hmv_project_joints``, include/handmv.h).  No CPU path."""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def get_2d_joints_from_3d_joints(joints_3d, root_idx, intrinsics, extrinsics, bboxes=None):
    """joints_3d [B, 21, 3]: absolute joints in camera `root_idx` (metres); intrinsics [B, V, 4] = fx, fy, cx, cy; extrinsics
    [B, V, 4, 4] (any invertible matrices: the inverse is general, like torch.inverse) -> [B, V, 21, 2] image pixels.
    bboxes [B, V, 4] (not a reference argument): also apply batch_joints_img_to_cropped_joints with its default image_size of
    256, which is what handmvnet.py:332 does to the result."""
    if not isinstance(joints_3d, torch.Tensor) or not joints_3d.is_cuda:
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: joints_3d must be a CUDA(HIP) tensor (no CPU fallback)")
    dev = joints_3d.device
    j = joints_3d.detach().contiguous().float()
    it = intrinsics.detach().to(dev).contiguous().float()
    ex = extrinsics.detach().to(dev).contiguous().float()
    if j.dim() != 3 or j.shape[1:] != (21, 3):
        raise ValueError("joints_3d must be [B, 21, 3]")
    B = j.shape[0]
    if it.dim() != 3 or it.shape[0] != B or it.shape[2] != 4:
        raise ValueError("intrinsics must be [B, V, 4]")
    V = it.shape[1]
    if tuple(ex.shape) != (B, V, 4, 4):
        raise ValueError("extrinsics must be [B, V, 4, 4]")
    bb = None
    if bboxes is not None:
        bb = bboxes.detach().to(dev).contiguous().float()
        if tuple(bb.shape) != (B, V, 4):
            raise ValueError("bboxes must be [B, V, 4]")
    out = torch.empty(B, V, 21, 2, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        rc = _lib.load().hmv_project_joints(dev.index if dev.index is not None else torch.cuda.current_device(), j.data_ptr(), B, V,
                                            int(root_idx), it.data_ptr(), ex.data_ptr(), bb.data_ptr() if bb is not None else None,
                                            out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc)
    return out
