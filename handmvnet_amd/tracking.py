"""Sequences without dataset boxes: the crop window of frame t + 1 is the box around the hand found in frame t.

The reference takes its windows from the labels (datasets/ho3d.py:103); a recorded or live multi-camera sequence has none.  It does
have the two pieces that turn one step's 2D joints into the next step's windows,
    batch_cropped_joints_to_joints_img   datasets/utils.py:146-162 (used at handmvnet.py:237)
    points2d_to_bbox                     datasets/utils.py:5-27
and here they are one device launch (csrc/track.hip, include/handmv.h "sequences"), so that a sequence runs with nothing on the host:

    joints_to_frame / next_crop_boxes   the op on its own, device tensors in and out
    SequenceTracker                     persistent buffers + hmv_forward_frames_track: one call (one replayed hipGraph) per time step
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .frames import IMAGENET_MEAN, IMAGENET_STD
from .spec import heatmap_size_of

STATUS_MOVED, STATUS_ABSENT, STATUS_KEPT = 0, 1, 2   # include/handmv.h: hmv_op_next_crop_boxes


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def next_crop_boxes(joints_crop_img: torch.Tensor, crop_boxes: torch.Tensor, image_size: int, margin: int = 0, square: bool = True,
                    present=None):
    """joints_crop_img fp32 [..., 21, 2] (crop pixels, as forward() returns them) and the windows they were found in, crop_boxes int
    [..., 4] -> (crop_boxes int32 [..., 4], bbox fp32 [..., 4], joints_img fp32 [..., 21, 2], status int32 [...]): the next windows
    (points2d_to_bbox of the frame-space joints, `margin` and `square` as there), the same numbers as fp32, the frame-space joints and
    per slot 0 = moved, 1 = absent (`present` [...] is zero there: window kept, zero joints), 2 = kept (a non-finite or absurd joint,
    or a window beyond 65536 px: the reference raises, the device reports).  Device tensors in, device tensors out, on the current
    stream, no host copy."""
    if not isinstance(joints_crop_img, torch.Tensor) or joints_crop_img.dim() < 2 or tuple(joints_crop_img.shape[-2:]) != (21, 2):
        raise ValueError("joints_crop_img must be a [..., 21, 2] tensor")
    lead = tuple(joints_crop_img.shape[:-2])
    if not isinstance(crop_boxes, torch.Tensor) or tuple(crop_boxes.shape) != lead + (4,):
        raise ValueError(f"crop_boxes must be a {list(lead + (4,))} tensor, one window per row of joints")
    if crop_boxes.dtype.is_floating_point or crop_boxes.dtype == torch.bool:
        raise ValueError("crop_boxes must be an integer tensor (x1, y1, x2, y2 in frame pixels)")
    if present is not None and (not isinstance(present, torch.Tensor) or tuple(present.shape) != lead):
        raise ValueError(f"present must be a {list(lead)} tensor")
    if int(image_size) <= 0:
        raise ValueError("image_size must be positive")
    if int(margin) < 0:
        raise ValueError("margin must not be negative")
    if not joints_crop_img.is_cuda or not crop_boxes.is_cuda or (present is not None and not present.is_cuda):
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: joints_crop_img, crop_boxes and present must be CUDA(HIP) tensors "
                               "(no CPU fallback)")
    dev = joints_crop_img.device
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    jc = joints_crop_img.contiguous().float()
    boxes = crop_boxes.to(dev).to(torch.int32).contiguous()
    pres = None if present is None else (present.to(dev) != 0).to(torch.uint8).contiguous()
    out_boxes = torch.empty(lead + (4,), device=dev, dtype=torch.int32)
    out_bbox = torch.empty(lead + (4,), device=dev, dtype=torch.float32)
    out_img = torch.empty(lead + (21, 2), device=dev, dtype=torch.float32)
    status = torch.empty(lead, device=dev, dtype=torch.int32)
    if n == 0:
        return out_boxes, out_bbox, out_img, status
    with torch.cuda.device(dev):
        rc = _lib.load().hmv_op_next_crop_boxes(dev.index if dev.index is not None else torch.cuda.current_device(), n, jc.data_ptr(),
                                                boxes.data_ptr(), pres.data_ptr() if pres is not None else None, int(image_size),
                                                int(margin), int(bool(square)), out_boxes.data_ptr(), out_bbox.data_ptr(),
                                                out_img.data_ptr(), status.data_ptr(), _stream(dev))
    _lib.check(rc)
    return out_boxes, out_bbox, out_img, status


def joints_to_frame(joints_crop_img: torch.Tensor, crop_boxes: torch.Tensor, image_size: int) -> torch.Tensor:
    """Frame-space joints [..., 21, 2] of crop-space joints found in the windows crop_boxes [..., 4]:
    batch_cropped_joints_to_joints_img in the reference's fp32 operation order."""
    return next_crop_boxes(joints_crop_img, crop_boxes, image_size)[2]


class SequenceTracker:
    """Runs a model over a multi-camera sequence whose crop windows follow the hand.

        tracker = SequenceTracker(model, crop_boxes0, {"intrinsic": K})      # the first windows are the caller's
        for frames in sequence:                                              # uint8 [B, V, Hf, Wf, 3], device or pinned host
            out = tracker.step(frames)

    The tracker owns every buffer the engine sees -- a frame staging buffer (allocated at the first step), the int32 windows, their
    fp32 copy (`bbox` of the crop-FoV columns), the intrinsics, the three outputs, joints_img and status -- and presents the same
    pointers at every step: with model.set_graphs(True) a steady sequence is one replayed hipGraph per time step, the window update
    included (include/handmv.h: hmv_forward_frames_track).  Nothing synchronises and nothing but the frames crosses to the device.

    step() returns a dict of VIEWS OF THE TRACKER'S OWN BUFFERS, valid until the next step() (clone what must outlive it):
        joints_crop_img [B, V, 21, 2], joints_cam [B, 21, 3], heatmap [B, V, 21, h, w]   as forward_frames()
        joints_img      [B, V, 21, 2]   the 2D joints in frame pixels
        status          [B, V] int32    0 = window moved, 1 = view absent (window kept), 2 = window kept (non-finite / absurd joints)
        crop_boxes      [B, V, 4] int32 the windows the NEXT step will use
        crop_boxes_used [B, V, 4] int32 the windows this step ran on (the one extra device copy per step, enqueued before the call)
    step(frames, view_mask=...) runs a ragged step (forward_frames(view_mask=), always eager): the windows of absent views stay where
    they are until the view returns.
    """

    def __init__(self, model, crop_boxes0, cam_params=None, margin: int = 0, square: bool = True, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 device=None):
        boxes0 = torch.as_tensor(crop_boxes0)
        if boxes0.dim() != 3 or boxes0.shape[1] != model.num_views or boxes0.shape[2] != 4 or boxes0.shape[0] < 1:
            raise ValueError(f"crop_boxes0 must be [b, {model.num_views}, 4]")
        if boxes0.dtype.is_floating_point or boxes0.dtype == torch.bool:
            raise ValueError("crop_boxes0 must be an integer tensor (x1, y1, x2, y2 in frame pixels)")
        if int(margin) < 0:
            raise ValueError("margin must not be negative")
        if device is None:
            device = boxes0.device if boxes0.is_cuda else torch.device("cuda", torch.cuda.current_device())
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.HandMvError("handmvnet_amd runs on MI355X only: a SequenceTracker lives on a CUDA(HIP) device (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.model, self.device = model, dev
        self.margin, self.square = int(margin), bool(square)
        self._mean, self._std = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        b, v = int(boxes0.shape[0]), int(boxes0.shape[1])
        self.batch, self.num_views = b, v
        self.image_size = size = int(model.cfg.image_size)
        self._need_cam = "crop" in model.cfg.pos_enc
        self._boxes = boxes0.to(dev).to(torch.int32).contiguous().clone()
        self._bbox = self._boxes.float() if self._need_cam else None
        self._intr = None
        if self._need_cam:
            if cam_params is None:
                raise TypeError("pos_enc contains 'crop': cam_params['intrinsic'] is required")
            self._intr = cam_params["intrinsic"].to(dev).reshape(-1, 4).contiguous().float().clone()
            if self._intr.shape[0] != b * v:
                raise RuntimeError("intrinsic must hold one row per frame")
        hs = tuple(heatmap_size_of(model.cfg, size, size))
        self._out = {"joints_crop_img": torch.zeros(b, v, 21, 2, device=dev), "joints_cam": torch.zeros(b, 21, 3, device=dev),
                     "heatmap": torch.zeros((b, v, 21) + hs, device=dev)}
        self._joints_img = torch.zeros(b, v, 21, 2, device=dev)
        self._status = torch.zeros(b, v, device=dev, dtype=torch.int32)
        self._used = self._boxes.clone()
        self._frames = None

    @property
    def crop_boxes(self) -> torch.Tensor:
        """The windows the next step will use: int32 [B, V, 4], the tracker's own buffer."""
        return self._boxes

    def reset(self, crop_boxes0) -> None:
        """New first windows into the same buffers (a new sequence, or a re-detection from outside)."""
        boxes0 = torch.as_tensor(crop_boxes0)
        if tuple(boxes0.shape) != tuple(self._boxes.shape) or boxes0.dtype.is_floating_point:
            raise ValueError(f"crop_boxes0 must be an integer {list(self._boxes.shape)} tensor")
        self._boxes.copy_(boxes0.to(torch.int32), non_blocking=True)
        if self._bbox is not None:
            self._bbox.copy_(self._boxes)

    def step(self, frames: torch.Tensor, view_mask=None) -> dict:
        model, dev, b, v, out = self.model, self.device, self.batch, self.num_views, self._out
        model._check_frames(frames)
        if tuple(frames.shape[:2]) != (b, v):
            raise ValueError(f"frames must hold {b} x {v} views like the tracker's windows, got {list(frames.shape[:2])}")
        if self._frames is None:
            self._frames = torch.empty(tuple(frames.shape), device=dev, dtype=torch.uint8)
        elif tuple(frames.shape) != tuple(self._frames.shape):
            raise ValueError(f"frame size {list(frames.shape[2:4])} differs from the first step's {list(self._frames.shape[2:4])}")
        if not frames.is_cuda and not frames.is_pinned():
            raise _lib.HandMvError("handmvnet_amd runs on MI355X only: frames must be a CUDA(HIP) tensor or pinned host memory")
        mask = counts = None
        if view_mask is not None:
            mask, counts = model._host_view_mask(view_mask, b, v)
        size = (self.image_size, self.image_size)
        src = (self._frames, int(frames.shape[2]), int(frames.shape[3]), self._boxes)
        tail = (self.margin, int(self.square), self._joints_img, self._status)
        model._engine(*size, dev.index)   # (made, or refused, before anything is enqueued)
        self._frames.copy_(frames, non_blocking=True)   # copies run on the current stream of the tensors' own device, like the call
        self._used.copy_(self._boxes)
        if mask is None:
            model._call("hmv_forward_frames_track", *size, dev, b, *src, self._mean, self._std, self._bbox, self._intr,
                        out["joints_crop_img"], out["joints_cam"], out["heatmap"], *tail)
        else:   # hmv_forward_frames_views_track: the packed rows of the present frames, scattered back into the tracker's full buffers
            table, idx = model._present_table(mask, dev)
            bb = it = None
            if self._need_cam:
                bb, it = self._bbox.view(-1, 4).index_select(0, idx), self._intr.index_select(0, idx)
            model._call_views("hmv_forward_frames_views_track", size, dev, mask, counts, idx, src + (table, self._mean, self._std), bb, it,
                              tail=tail, into=out)
            if self._bbox is not None:
                self._bbox.copy_(self._boxes)   # the full fp32 copy follows the windows (the entry updated the packed rows)
        return {"joints_crop_img": out["joints_crop_img"], "joints_cam": out["joints_cam"], "heatmap": out["heatmap"],
                "joints_img": self._joints_img, "status": self._status, "crop_boxes": self._boxes, "crop_boxes_used": self._used}
