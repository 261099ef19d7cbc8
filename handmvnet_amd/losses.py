"""Device-side mirror of what the reference's evaluation step needs for its loss
(/root/reference/src/models/handmvnet.py:279-351 -> models/losses/loss.py, models/utils.py:123-131, utils/camera.py,
datasets/utils.py:86-143, datasets/ho3d.py:155-166).

``pose_losses`` is the one call ``HandMvNet._calculate_loss`` makes (``hmv_pose_losses``, include/handmv.h): every term and the
total from device pointers, the result left on the device.  ``target_heatmaps`` builds the dataset's ground-truth heat maps from
label joints; ``PoseLoss`` carries the two criteria handmvnet.py calls (``smooth_l1_loss`` / ``bce_loss`` are called nowhere
in it and are not provided).  Everything runs on the tensors' device and the current stream; there is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib

TERMS = ("heatmap_loss", "joints_2d_loss", "joints_3d_loss", "g2d_loss", "p2d_loss", "loss")   # layout of the result vector


def _device_f32(name: str, t, dev=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if dev is None:
        if not t.is_cuda:
            raise _lib.HandMvError(f"handmvnet_amd losses run on MI355X only: {name} must be a CUDA(HIP) tensor (no CPU fallback)")
        dev = t.device
    return t.detach().to(dev).contiguous().float()


def _index(dev: torch.device) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def target_heatmaps(joints_crop_img: torch.Tensor, image_size: int, heatmap_size, sigma: int = 2) -> torch.Tensor:
    """joints_crop_img [..., 21, 2] (device) -> fp32 [..., 21, h, w]: per joint generate_heatmap on a zero image_size^2 image ->
    ToTensor (float64) -> Resize((h, w), antialias=True) -> fp32, as datasets/ho3d.py:155-166 builds inputs["heatmap"].
    heatmap_size: an int or (h, w).  A label whose Gaussian misses the image entirely gives a zero map (the reference raises there)."""
    j = _device_f32("joints_crop_img", joints_crop_img)
    if j.dim() < 2 or j.shape[-2:] != (21, 2):
        raise ValueError("joints_crop_img must be [..., 21, 2]")
    if int(sigma) != sigma:
        raise ValueError("sigma must be an integer (the reference uses 2)")
    h, w = (int(heatmap_size),) * 2 if isinstance(heatmap_size, int) else (int(heatmap_size[0]), int(heatmap_size[1]))
    n = j.numel() // 42
    out = torch.empty(tuple(j.shape[:-1]) + (h, w), device=j.device, dtype=torch.float32)
    with torch.cuda.device(j.device):
        rc = _lib.load().hmv_op_target_heatmaps(_index(j.device), j.data_ptr(), n, int(image_size), h, w, int(sigma), out.data_ptr(),
                                                ctypes.c_void_p(torch.cuda.current_stream(j.device).cuda_stream))
    _lib.check(rc)
    return out


def build_loss_args(pred_heatmap, pred_joints_2d, pred_joints_cam, gt_joints_2d, gt_joints_cam, weights: dict, target_heatmap=None,
                    image_size: Optional[int] = None, sigma: int = 2, joints_mask=None, mask_invisible_joints: bool = False,
                    root_joint=None, root_idx: int = 0, intrinsic=None, extrinsic=None, bbox=None, want_projected: bool = True):
    """The hmv_loss_args of one call -> (args, device, projected or None, the tensors its pointers refer to).  Arguments as
    pose_losses; run_loss_args launches it (split so that the ABI tests can damage one field in between)."""
    hm = _device_f32("pred_heatmap", pred_heatmap)
    if hm.dim() != 5 or hm.shape[2] != 21:
        raise ValueError("pred_heatmap must be [B, V, 21, h, w]")
    dev = hm.device
    B, V, _, h, w = hm.shape
    p2 = _device_f32("pred_joints_2d", pred_joints_2d)
    pc = _device_f32("pred_joints_cam", pred_joints_cam)
    g2, gc = _device_f32("gt_joints_2d", gt_joints_2d, dev), _device_f32("gt_joints_cam", gt_joints_cam, dev)
    if tuple(p2.shape) != (B, V, 21, 2) or g2.shape != p2.shape:
        raise ValueError(f"pred / gt joints_2d must be [{B}, {V}, 21, 2]")
    if tuple(pc.shape) != (B, 21, 3) or gc.shape != pc.shape:
        raise ValueError(f"pred / gt joints_cam must be [{B}, 21, 3]")
    a = _lib.HmvLossArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvLossArgs)
    a.B, a.V, a.hm_h, a.hm_w = B, V, h, w
    a.w_heatmap, a.w_joints_2d, a.w_joints_3d = float(weights["heatmap"]), float(weights["joints_2d"]), float(weights["joints_3d"])
    a.pred_heatmap, a.pred_joints_2d, a.gt_joints_2d = hm.data_ptr(), p2.data_ptr(), g2.data_ptr()
    a.pred_joints_cam, a.gt_joints_cam = pc.data_ptr(), gc.data_ptr()
    keep = [hm, p2, pc, g2, gc]   # the tensors whose pointers the struct carries
    if target_heatmap is not None:
        tg = _device_f32("target_heatmap", target_heatmap, dev)
        if tg.shape != hm.shape:
            raise ValueError(f"target_heatmap must have the predicted map's shape {tuple(hm.shape)}, not {tuple(tg.shape)}")
        a.target_heatmap = tg.data_ptr()
        keep.append(tg)
    else:
        if image_size is None:
            raise TypeError("image_size is required when the target heat maps are synthesised from the label joints")
        a.image_size, a.sigma = int(image_size), int(sigma)
    if joints_mask is not None:
        mk = joints_mask.detach().to(dev).reshape(B, V, 21).ne(0).to(torch.uint8).contiguous()
        a.joints_mask, a.mask_invisible_joints = mk.data_ptr(), int(bool(mask_invisible_joints))
        keep.append(mk)
    projected = None
    if "g2d" in weights:
        a.with_projection, a.root_idx = 1, int(root_idx)
        a.w_g2d, a.w_p2d = float(weights["g2d"]), float(weights["p2d"])
        it = _device_f32("intrinsic", intrinsic, dev).reshape(B, V, 4)
        ex = _device_f32("extrinsic", extrinsic, dev).reshape(B, V, 4, 4)
        bb = _device_f32("bbox", bbox, dev).reshape(B, V, 4)
        a.intrinsic, a.extrinsic, a.bbox = it.data_ptr(), ex.data_ptr(), bb.data_ptr()
        keep += [it, ex, bb]
        if root_joint is not None:
            rj = _device_f32("root_joint", root_joint, dev).reshape(-1, 1, 3).expand(B, 1, 3).contiguous()   # broadcast like the reference's add
            a.root_joint = rj.data_ptr()
            keep.append(rj)
        if want_projected:
            projected = torch.empty(B, V, 21, 2, device=dev, dtype=torch.float32)
            a.projected = projected.data_ptr()
    lib = _lib.load()
    scratch = torch.empty(max(int(lib.hmv_pose_losses_scratch_bytes(B, V)) // 8, 1), device=dev, dtype=torch.float64)
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
    keep.append(scratch)
    return a, dev, projected, keep


def run_loss_args(args, dev: torch.device, view_present: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hmv_pose_losses -- with `view_present` (device uint8 [B, V]) hmv_pose_losses_views -- on `dev`'s current stream -> the device
    fp32 [6] result (order of TERMS).  Nothing synchronises."""
    result = torch.empty(6, device=dev, dtype=torch.float32)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if view_present is None:
            rc = _lib.load().hmv_pose_losses(_index(dev), ctypes.byref(args), result.data_ptr(), stream)
        else:
            rc = _lib.load().hmv_pose_losses_views(_index(dev), ctypes.byref(args), view_present.data_ptr(), result.data_ptr(), stream)
    _lib.check(rc)
    return result


def device_view_mask(view_mask, B: int, V: int, dev: torch.device) -> torch.Tensor:
    """view_mask (bool [B, V] tensor on any device, or array-like; True = the view is present) -> the device uint8 [B, V] the ragged
    entries read.  No synchronisation: that every sample has a present view is the caller's precondition (forward_views checks it)."""
    m = view_mask if isinstance(view_mask, torch.Tensor) else torch.as_tensor(np.asarray(view_mask))
    if tuple(m.shape) != (B, V):
        raise ValueError(f"view_mask must have shape [{B}, {V}], got {list(m.shape)}")
    return m.detach().to(dev).ne(0).to(torch.uint8).contiguous()


def pose_losses(*args, view_mask=None, **kwargs):
    """One hmv_pose_losses call.  pred_heatmap [B, V, 21, h, w], *_joints_2d [B, V, 21, 2], *_joints_cam [B, 21, 3] (metres).
    weights: train_params["loss_weights"] (heatmap, joints_2d, joints_3d and optionally g2d + p2d: then root_joint [B, 3],
    intrinsic, extrinsic and bbox are read).  target_heatmap None: the targets are synthesised from gt_joints_2d, image_size, sigma.
    -> (result, projected): result device fp32 [6] in the order of TERMS, projected [B, V, 21, 2] or None.  Labels on the host are
    moved to the predictions' device; nothing synchronises.
    view_mask (bool [B, V] on any device, or array-like; True = present): a ragged view set, hmv_pose_losses_views -- every term is
    the mean over samples of the sample's own value over its present views (include/handmv.h); the tensors keep the full [B, V]
    layout, rows of absent views are not read, `projected` is zero there.  Every sample needs a present view (not checked here: that
    would synchronise; a sample without one makes the view-dependent terms NaN).  None: the uniform call."""
    a, dev, projected, keep = build_loss_args(*args, **kwargs)
    present = None if view_mask is None else device_view_mask(view_mask, a.B, a.V, dev)
    result = run_loss_args(a, dev, present)
    del present
    del keep   # temporaries were allocated on the stream the kernels run on: the caching allocator reuses them in stream order
    return result, projected


class PoseLoss:
    """models/losses/loss.py:4-17 for the shapes handmvnet.py passes: heat maps [..., 21, h, w] to mse_loss, joints [..., 21, 2]
    or [..., 21, 3] to l1_loss.  0-dim device tensors; fp64 sums in a fixed order."""

    @staticmethod
    def _pair(preds, labels, stacked_dim):
        p = _device_f32("preds", preds)
        g = _device_f32("labels", labels, p.device)
        if stacked_dim:
            g = g.unsqueeze(stacked_dim).expand_as(p).contiguous()
        if g.shape != p.shape:
            raise ValueError(f"preds {tuple(p.shape)} and labels {tuple(g.shape)} differ in shape")
        return p, g

    @staticmethod
    def mse_loss(preds, labels, stacked_dim=None, weight=1.):
        p, g = PoseLoss._pair(preds, labels, stacked_dim)
        if p.dim() < 3 or p.shape[-3] != 21:
            raise ValueError("mse_loss takes heat maps [..., 21, h, w]")
        h, w = p.shape[-2:]
        n = p.numel() // (21 * h * w)
        z2, z3 = torch.zeros(n, 1, 21, 2, device=p.device), torch.zeros(n, 21, 3, device=p.device)
        r, _ = pose_losses(p.reshape(n, 1, 21, h, w), z2, z3, z2, z3, {"heatmap": weight, "joints_2d": 0., "joints_3d": 0.},
                           target_heatmap=g.reshape(n, 1, 21, h, w))
        return r[0]

    @staticmethod
    def l1_loss(preds, labels, stacked_dim=None, weight=1.):
        p, g = PoseLoss._pair(preds, labels, stacked_dim)
        if p.dim() < 2 or p.shape[-2] != 21 or p.shape[-1] not in (2, 3):
            raise ValueError("l1_loss takes joints [..., 21, 2] or [..., 21, 3]")
        n = p.numel() // (21 * p.shape[-1])
        zh = torch.zeros(n, 1, 21, 1, 1, device=p.device)
        if p.shape[-1] == 2:
            z3 = torch.zeros(n, 21, 3, device=p.device)
            r, _ = pose_losses(zh, p.reshape(n, 1, 21, 2), z3, g.reshape(n, 1, 21, 2), z3,
                               {"heatmap": 0., "joints_2d": weight, "joints_3d": 0.}, target_heatmap=zh)
            return r[1]
        z2 = torch.zeros(n, 1, 21, 2, device=p.device)
        r, _ = pose_losses(zh, z2, p.reshape(n, 21, 3), z2, g.reshape(n, 21, 3), {"heatmap": 0., "joints_2d": 0., "joints_3d": weight},
                           target_heatmap=zh)
        return r[2]
