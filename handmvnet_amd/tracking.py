"""Sequences without dataset boxes: the crop window of frame t + 1 is the box around the hand found in frame t.

The reference takes its windows from the labels (datasets/ho3d.py:103); a recorded or live multi-camera sequence has none.  It does
have the two pieces that turn one step's 2D joints into the next step's windows,
    batch_cropped_joints_to_joints_img   datasets/utils.py:146-162 (used at handmvnet.py:237)
    points2d_to_bbox                     datasets/utils.py:5-27
and here they are one device launch (csrc/track.hip, include/handmv.h "sequences"), so that a sequence runs with nothing on the host:

    joints_to_frame / next_crop_boxes   the op on its own, device tensors in and out
    SequenceTracker                     persistent buffers + hmv_forward_frames_track: one call (one replayed hipGraph) per time step

That is the single-view rule: a camera that loses the hand loses its window.  reproject_crop_boxes (hmv_op_reproject_crop_boxes, the
same file) moves the windows of ALL cameras to where one 3D pose projects -- get_2d_joints_from_3d_joints (utils/camera.py:25-44) then
points2d_to_bbox -- and SequenceTracker(windows="reprojected") closes that loop on the device: forward + own-joints windows,
triangulation of the views' 2D joints, reprojection of the pose into every camera.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .frames import IMAGENET_MEAN, IMAGENET_STD
from .spec import heatmap_size_of

STATUS_MOVED, STATUS_ABSENT, STATUS_KEPT = 0, 1, 2   # include/handmv.h: hmv_op_next_crop_boxes
SOURCE_OWN, SOURCE_REPROJECTED = 0, 1                # include/handmv.h: hmv_op_reproject_crop_boxes
MAX_VIEWS = 16                                       # hmv_op_triangulate's


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


def _reproject_launch(dev, B, V, margin, square, require_all, points3d, point_status, frame_cam, intr, ext, joints_img, boxes, bbox,
                      status, source, reproj, gap) -> None:
    """The raw entry, in place on boxes / bbox / status: every tensor is contiguous, of its dtype and on `dev` (or None where the
    entry takes NULL)."""
    a = _lib.HmvReprojectBoxesArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvReprojectBoxesArgs)
    a.B, a.V, a.margin, a.square, a.require_all = B, V, int(margin), int(bool(square)), int(bool(require_all))
    for name, t in (("points3d", points3d), ("point_status", point_status), ("frame_cam", frame_cam), ("intrinsic", intr),
                    ("extrinsic", ext), ("joints_img", joints_img), ("crop_boxes", boxes), ("bbox", bbox), ("status", status),
                    ("source", source), ("joints_reproj", reproj), ("gap", gap)):
        if t is not None:
            setattr(a, name, t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hmv_op_reproject_crop_boxes(dev.index if dev.index is not None else torch.cuda.current_device(),
                                                           ctypes.byref(a), _stream(dev)))


def reproject_crop_boxes(points3d: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor, crop_boxes: torch.Tensor,
                         status: torch.Tensor, *, point_status=None, frame_cam=None, joints_img=None, margin: int = 0,
                         square: bool = True, require_all: bool = False):
    """The windows of every camera from one 3D pose (one launch; include/handmv.h: hmv_op_reproject_crop_boxes).
      points3d     [B, 21, 3] fp32 device tensor, metres, in the frame of camera frame_cam[b]
      intrinsics   [B, V, 4] (fx, fy, cx, cy);  extrinsics [B, V, 4, 4] camera-to-world, as get_2d_joints_from_3d_joints takes them
      crop_boxes   integer [B, V, 4] and status [B, V] (0 moved / 1 absent / 2 kept): what the own-joints rule (next_crop_boxes) left
      point_status None, or [B, 21]: triangulate()'s status per joint -- a sample whose root (require_all: any joint) was not
                   triangulated keeps its windows
      frame_cam    None (camera 0), an int, or [B] camera indices (list, array, device tensor)
      joints_img   None, or [B, V, 21, 2]: the views' own 2D joints in frame pixels, for `gap` only
    Returns NEW tensors (crop_boxes int32 [B, V, 4], bbox fp32 [B, V, 4], status int32 [B, V], source int32 [B, V], joints_reproj fp32
    [B, V, 21, 2], gap fp32 [B, V]); the inputs are not modified.  source 1: the window is points2d_to_bbox(margin, square) of the 21
    projections (every joint in front of the camera, finite, a window of at most 65536 px), status 2 became 0, an absent view's 1 stayed;
    source 0: window and status are the inputs'.  joints_reproj is NaN for a sample that keeps its windows; gap is the mean distance
    of joints_img from joints_reproj over the joints where the incoming status is 0, NaN elsewhere and without joints_img."""
    if not isinstance(points3d, torch.Tensor) or points3d.dim() != 3 or tuple(points3d.shape[1:]) != (21, 3):
        raise ValueError("points3d must be a [B, 21, 3] tensor")
    B = int(points3d.shape[0])
    if not isinstance(intrinsics, torch.Tensor) or intrinsics.dim() != 3 or int(intrinsics.shape[0]) != B or int(intrinsics.shape[2]) != 4:
        raise ValueError(f"intrinsics must be a [{B}, V, 4] tensor (fx, fy, cx, cy)")
    V = int(intrinsics.shape[1])
    if B < 1 or not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"reproject_crop_boxes needs B >= 1 and 1 <= V <= {MAX_VIEWS}; got B = {B}, V = {V}")
    if not isinstance(extrinsics, torch.Tensor) or tuple(extrinsics.shape) != (B, V, 4, 4):
        raise ValueError(f"extrinsics must be a [{B}, {V}, 4, 4] tensor")
    if not isinstance(crop_boxes, torch.Tensor) or tuple(crop_boxes.shape) != (B, V, 4):
        raise ValueError(f"crop_boxes must be a [{B}, {V}, 4] tensor")
    if crop_boxes.dtype.is_floating_point or crop_boxes.dtype == torch.bool:
        raise ValueError("crop_boxes must be an integer tensor (x1, y1, x2, y2 in frame pixels)")
    if not isinstance(status, torch.Tensor) or tuple(status.shape) != (B, V) or status.dtype.is_floating_point or status.dtype == torch.bool:
        raise ValueError(f"status must be an integer [{B}, {V}] tensor")
    if point_status is not None and (not isinstance(point_status, torch.Tensor) or tuple(point_status.shape) != (B, 21)
                                     or point_status.dtype.is_floating_point):
        raise ValueError(f"point_status must be an integer [{B}, 21] tensor")
    if joints_img is not None and (not isinstance(joints_img, torch.Tensor) or tuple(joints_img.shape) != (B, V, 21, 2)):
        raise ValueError(f"joints_img must be a [{B}, {V}, 21, 2] tensor")
    if int(margin) < 0:
        raise ValueError("margin must not be negative")
    if not points3d.is_cuda:
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: points3d must be a CUDA(HIP) tensor (no CPU fallback)")
    dev = points3d.device
    fc = None
    if frame_cam is not None:
        if isinstance(frame_cam, torch.Tensor) and frame_cam.is_cuda:
            fc = frame_cam.detach().to(dev).to(torch.int32).contiguous()   # device data: an index outside [0, V) keeps the sample's windows
        else:
            host = np.asarray(frame_cam.detach().cpu().numpy() if isinstance(frame_cam, torch.Tensor) else frame_cam)
            if host.dtype.kind not in "iu" or host.ndim > 1:
                raise ValueError("frame_cam must be an integer camera index or one per sample")
            host = np.broadcast_to(host, (B,)) if host.ndim == 0 else host
            if host.shape != (B,) or ((host < 0) | (host >= V)).any():
                raise ValueError(f"frame_cam must hold {B} camera indices in [0, {V})")
            fc = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(dev)
        if fc.numel() != B:
            raise ValueError(f"frame_cam must hold {B} entries, one per sample")
    p3 = points3d.detach().float().contiguous()
    it = intrinsics.detach().to(dev).float().contiguous()
    ex = extrinsics.detach().to(dev).float().contiguous()
    ps = None if point_status is None else point_status.detach().to(dev).to(torch.int32).contiguous()
    ji = None if joints_img is None else joints_img.detach().to(dev).float().contiguous()
    boxes = crop_boxes.detach().to(dev).to(torch.int32).contiguous().clone()
    bbox = boxes.float()
    st = status.detach().to(dev).to(torch.int32).contiguous().clone()
    source = torch.empty((B, V), device=dev, dtype=torch.int32)
    reproj = torch.empty((B, V, 21, 2), device=dev, dtype=torch.float32)
    gap = torch.empty((B, V), device=dev, dtype=torch.float32)
    _reproject_launch(dev, B, V, margin, square, require_all, p3, ps, fc, it, ex, ji, boxes, bbox, st, source, reproj, gap)
    del p3, it, ex, ps, ji, fc   # allocated on the stream the kernel runs on: the caching allocator reuses them in stream order
    return boxes, bbox, st, source, reproj, gap


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

    windows="joints" (the default) is the rule above: every camera follows its own 2D joints.  windows="reprojected" follows the hand in
    space: cam_params must also hold "extrinsic" [B, V, 4, 4], camera-to-world with the translation in metres, and a step is
        1. the call above (own-joints windows, joints_img, status: the fallback, and graph replay of it works as ever);
        2. one triangulate launch on the same stream over the tracker's joints_img, with present = view_mask AND status == 0 computed
           on the device and the result in the frame of camera 0 (a ragged sample: of its first present view).  `ransac`, `refit` and
           `confidence` are forward_absolute's (confidence: the peaks and select launches go first);
        3. the pose: pose="fused" is joints_cam + joints_tri[:, :1] and needs the root triangulated; pose="triangulated" is joints_tri
           and needs every joint triangulated;
        4. one reproject_crop_boxes launch in place on the windows, bbox and status: every camera of a sample with such a pose gets the
           window of its projection -- the camera that was fooled and the absent one (status stays 1) included.
    The launches of 2 - 4 are eager, a few elementwise torch ops on [B, V]-sized tensors among them; nothing synchronises, nothing is
    read back.  The dict gains, all views of the tracker's own buffers:
        source        [B, V] int32      0 = the window is the own-joints rule's, 1 = the reprojection's
        joints_reproj [B, V, 21, 2]     the pose projected into every camera, frame pixels (NaN for a sample without a pose)
        reproj_gap    [B, V]            the mean distance of joints_img from joints_reproj (NaN unless the view's status was 0)
        joints_tri    [B, 21, 3], tri_status [B, 21] int32, joints_abs [B, 21, 3] (joints_cam + joints_tri[:, :1])
    """

    def __init__(self, model, crop_boxes0, cam_params=None, margin: int = 0, square: bool = True, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 device=None, windows: str = "joints", pose: str = "fused", ransac=None, refit: bool = True, confidence=None):
        if windows not in ("joints", "reprojected"):
            raise ValueError('windows must be "joints" or "reprojected"')
        if pose not in ("fused", "triangulated"):
            raise ValueError('pose must be "fused" or "triangulated"')
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
        self.windows, self.pose = windows, pose
        if windows == "reprojected":
            from .triangulation import parse_gate, parse_ransac
            if cam_params is None or "intrinsic" not in cam_params or "extrinsic" not in cam_params:
                raise ValueError('windows="reprojected" needs cam_params["intrinsic"] and cam_params["extrinsic"]')
            if not 1 <= v <= MAX_VIEWS:
                raise ValueError(f'windows="reprojected" takes 1 .. {MAX_VIEWS} views')
            intr, ext = torch.as_tensor(cam_params["intrinsic"]), torch.as_tensor(cam_params["extrinsic"])
            if intr.numel() != b * v * 4 or ext.numel() != b * v * 16:
                raise ValueError(f"intrinsic must hold [{b}, {v}, 4] and extrinsic [{b}, {v}, 4, 4] values")
            self._rig_intr = intr.to(dev).reshape(b, v, 4).contiguous().float().clone()
            self._rig_ext = ext.to(dev).reshape(b, v, 4, 4).contiguous().float().clone()
            table, self._threshold = parse_ransac(v, ransac)
            if table is not None and not isinstance(table, torch.Tensor):
                table = torch.from_numpy(np.ascontiguousarray(np.asarray(table)))
            self._table = None if table is None else table.to(dev).to(torch.int32).contiguous()   # (triangulate() checks its shape)
            self._refit = bool(refit) and table is not None
            self._gate = parse_gate(confidence)
            self._tri = torch.zeros(b, 21, 3, device=dev)
            self._tri_status = torch.zeros(b, 21, device=dev, dtype=torch.int32)
            self._abs = torch.zeros(b, 21, 3, device=dev)
            self._source = torch.zeros(b, v, device=dev, dtype=torch.int32)
            self._reproj = torch.zeros(b, v, 21, 2, device=dev)
            self._gap = torch.zeros(b, v, device=dev)
            self._present = torch.zeros(b, v, device=dev, dtype=torch.bool)
            self._frame_cam = torch.zeros(b, device=dev, dtype=torch.int32)
            self._frame_cam_set = False

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
            if self._bbox is not None and self.windows == "joints":
                self._bbox.copy_(self._boxes)   # the full fp32 copy follows the windows (the entry updated the packed rows)
        res = {"joints_crop_img": out["joints_crop_img"], "joints_cam": out["joints_cam"], "heatmap": out["heatmap"],
               "joints_img": self._joints_img, "status": self._status, "crop_boxes": self._boxes, "crop_boxes_used": self._used}
        if self.windows == "reprojected":
            self._reproject(mask, res)
        return res

    def _reproject(self, mask, res) -> None:
        """Steps 2 - 4 of a windows="reprojected" step, behind the forward on the current stream: triangulate the views' own 2D
        joints, project the pose into every camera, move the windows.  mask: the step's host view mask or None."""
        from .triangulation import triangulate
        dev, b, v, out = self.device, self.batch, self.num_views, self._out
        if mask is None:
            torch.eq(self._status, 0, out=self._present)
            if self._frame_cam_set:   # (a ragged step left its samples' first present views there)
                self._frame_cam.zero_()
                self._frame_cam_set = False
        else:
            host = torch.from_numpy(mask.astype(np.uint8)).to(dev, non_blocking=True)
            torch.logical_and(host, self._status == 0, out=self._present)
            self._frame_cam.copy_(torch.from_numpy(mask.argmax(axis=1).astype(np.int32)), non_blocking=True)   # the first present view
            self._frame_cam_set = True
        extra = {}
        if self._gate is not None:   # the peaks launch on the step's own heat maps; the select launch runs inside triangulate()
            from .confidence import heatmap_peaks
            conf = heatmap_peaks(out["heatmap"])[0]
            extra = dict(confidences=conf, confidence_threshold=self._gate[0], confidence_step=self._gate[1], carry=self._gate[2])
        triangulate(self._joints_img, self._rig_intr, self._rig_ext, present=self._present, subsets=self._table,
                    threshold=self._threshold, refit=self._refit, frame_cam=self._frame_cam, out=(self._tri, self._tri_status), **extra)
        torch.add(out["joints_cam"], self._tri[:, :1], out=self._abs)
        fused = self.pose == "fused"
        _reproject_launch(dev, b, v, self.margin, self.square, not fused, self._abs if fused else self._tri, self._tri_status,
                          self._frame_cam, self._rig_intr, self._rig_ext, self._joints_img, self._boxes, self._bbox, self._status,
                          self._source, self._reproj, self._gap)
        if mask is not None and self._bbox is not None:
            self._bbox.copy_(self._boxes)   # the full fp32 copy follows the windows, after the launch that moved them last
        res.update(source=self._source, joints_reproj=self._reproj, reproj_gap=self._gap, joints_tri=self._tri,
                   tri_status=self._tri_status, joints_abs=self._abs)
