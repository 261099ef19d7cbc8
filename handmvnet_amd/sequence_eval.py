"""Evaluating a sequence whose crop windows follow the hand (tracking.py), on the device.

Under a ``SequenceTracker`` the windows are the tracker's own, so 2D labels expressed in the dataset's boxes do not belong to the
predictions: every view-dependent number (2D MPJPE, the heat-map, 2D and reprojection loss terms) needs the labels in the windows a
step actually ran on.  And the number one wants from a tracker, the jitter of its output, is the reference's sequence metric
``PoseMetrics.mka`` (models/metrics.py:36-49), which no step-wise evaluation computes.  Both are device work here
(csrc/seq_eval.hip, include/handmv.h "sequence evaluation"):

    labels_to_windows    frame-space label joints -> crop pixels of given windows: batch_joints_img_to_cropped_joints
                         (datasets/utils.py:124-143) to the bits of the reference's fp32 run, plus per slot how many visible joints
                         fell outside the window
    SequenceEvaluator    tracker step + labels into its windows + EpochEvaluator.add + one hmv_seq_eval_add per time step; nothing is
                         copied to the host until compute()

2D numbers of such an evaluation are in crop pixels of the FOLLOWED windows, not of dataset boxes.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .evaluation import STEPS, EpochEvaluator, finish_state
from .losses import _index, device_view_mask

STATUS_MAPPED, STATUS_ABSENT, STATUS_EMPTY = 0, 1, 2   # include/handmv.h: hmv_op_labels_to_windows
_SUMS = 12                                             # doubles per lane (include/handmv.h: hmv_seq_eval_add)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def labels_to_windows(joints_img: torch.Tensor, crop_boxes: torch.Tensor, image_size: int, joints_img_mask=None, present=None):
    """joints_img fp32 [..., 21, 2] (frame pixels) and the windows crop_boxes int [..., 4] a step ran on ->
    (joints_crop_img fp32 [..., 21, 2], mask uint8 [..., 21], info int32 [..., 3]): the labels in crop pixels of the windows, the
    joint mask of the result (non-zero = do not use: joints_img_mask [..., 21] was non-zero, or the slot's status is not 0) and per
    slot {status, outside, visible}: status 0 = mapped, 1 = absent (`present` [...] is zero there), 2 = empty window (x2 <= x1 or
    y2 <= y1; the reference divides by zero); a slot of status 1 or 2 has zero joints and a full mask.  visible counts the unmasked
    joints of a mapped slot, outside those of them that are non-finite or not in 0 <= c < image_size on either axis.  Device tensors
    in, device tensors out, on the current stream, no host copy."""
    if not isinstance(joints_img, torch.Tensor) or joints_img.dim() < 2 or tuple(joints_img.shape[-2:]) != (21, 2):
        raise ValueError("joints_img must be a [..., 21, 2] tensor")
    if not joints_img.dtype.is_floating_point:
        raise ValueError("joints_img must be a floating-point tensor (frame pixels)")
    lead = tuple(joints_img.shape[:-2])
    if not isinstance(crop_boxes, torch.Tensor) or tuple(crop_boxes.shape) != lead + (4,):
        raise ValueError(f"crop_boxes must be a {list(lead + (4,))} tensor, one window per row of joints")
    if crop_boxes.dtype.is_floating_point or crop_boxes.dtype == torch.bool:
        raise ValueError("crop_boxes must be an integer tensor (x1, y1, x2, y2 in frame pixels)")
    if joints_img_mask is not None and (not isinstance(joints_img_mask, torch.Tensor) or tuple(joints_img_mask.shape) != lead + (21,)):
        raise ValueError(f"joints_img_mask must be a {list(lead + (21,))} tensor")
    if present is not None and (not isinstance(present, torch.Tensor) or tuple(present.shape) != lead):
        raise ValueError(f"present must be a {list(lead)} tensor")
    if int(image_size) <= 0:
        raise ValueError("image_size must be positive")
    if not all(t.is_cuda for t in (joints_img, crop_boxes, joints_img_mask, present) if t is not None):
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: joints_img, crop_boxes, joints_img_mask and present must be "
                               "CUDA(HIP) tensors (no CPU fallback)")
    dev = joints_img.device
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    ji = joints_img.detach().contiguous().float()
    boxes = crop_boxes.to(dev).to(torch.int32).contiguous()
    hidden = None if joints_img_mask is None else joints_img_mask.detach().to(dev).ne(0).to(torch.uint8).contiguous()
    pres = None if present is None else present.detach().to(dev).ne(0).to(torch.uint8).contiguous()
    crop = torch.empty(lead + (21, 2), device=dev, dtype=torch.float32)
    mask = torch.empty(lead + (21,), device=dev, dtype=torch.uint8)
    info = torch.empty(lead + (3,), device=dev, dtype=torch.int32)
    if n == 0:
        return crop, mask, info
    with torch.cuda.device(dev):
        rc = _lib.load().hmv_op_labels_to_windows(_index(dev), n, ji.data_ptr(), boxes.data_ptr(),
                                                  pres.data_ptr() if pres is not None else None,
                                                  hidden.data_ptr() if hidden is not None else None, int(image_size), crop.data_ptr(),
                                                  mask.data_ptr(), info.data_ptr(), _stream(dev))
    _lib.check(rc)
    return crop, mask, info


def pool_sums(sums: torch.Tensor, unlabelled_steps: int = 0) -> torch.Tensor:
    """sums [B * 12] or [B, 12] (any device) -> the 11 doubles a multi-rank evaluation adds up: the lane-pooled sums [1 .. 10], then
    the lane-steps that carried no labels (host knowledge: whether [4] means anything must not differ between ranks)."""
    pooled = sums.reshape(-1, _SUMS)[:, 1:11].sum(0)
    return torch.cat([pooled, torch.tensor([float(unlabelled_steps)], dtype=pooled.dtype, device=pooled.device)])


def reduce_pooled(pooled: torch.Tensor, group=None) -> torch.Tensor:
    """ONE all_reduce(SUM) of pool_sums' vector, in place.  Any tensor on any backend (gloo drives it on the CPU)."""
    dist.all_reduce(pooled, op=dist.ReduceOp.SUM, group=group)
    return pooled


def finish_sequence(sums, pooled, labelled: bool, mode: str) -> dict:
    """The sequence numbers from host copies of a rank's sums ([B, 12]) and of the (reduced) pool_sums vector; `labelled`: at least one
    labelled step was added anywhere.  Raises ValueError when no step was added."""
    s = np.asarray(sums, np.float64).reshape(-1, _SUMS)
    p = np.concatenate([[0.0], np.asarray(pooled, np.float64).reshape(-1)])      # [1 .. 10] indexed like a lane's sums, [11] unlabelled
    if p.size != _SUMS:
        raise ValueError(f"the pooled vector has {_SUMS - 1} elements, not {p.size - 1}")
    if not p[1] > 0:
        raise ValueError("empty evaluation: no step was added")
    nan = float("nan")
    out = {f"{mode}_mka": float(1000 * p[3] / p[2]) if p[2] > 0 else nan,
           f"{mode}_mka_gt": (float(1000 * p[4] / p[2]) if p[2] > 0 else nan) if labelled and not p[11] > 0 else None,
           f"{mode}_mka_per_sequence": [float(1000 * r[3] / r[2]) if r[2] > 0 else nan for r in s]}
    slots = p[5] + p[6] + p[7]
    for k, name in enumerate(("window_moved", "window_absent", "window_kept")):
        out[name] = float(p[5 + k] / slots) if slots > 0 else nan
    out["empty_windows"] = int(p[8])
    out["labels_outside_window"] = (float(p[10] / p[9]) if p[9] > 0 else nan) if labelled else None
    return out


class SequenceEvaluator:
    """An evaluation epoch over sequences that a SequenceTracker follows: raw frames and frame-space labels in, the epoch's numbers in
    the followed windows out, plus jitter and window-quality counts, with one readback at the end.

        ev = SequenceEvaluator(tracker, cam_params)
        for frames, labels in sequence:
            out = ev.step(frames, labels)      # labels may be None; view_mask= as tracker.step
        ev.reduce()                            # only under torch.distributed
        numbers = ev.compute()

    labels: {"joints_img": [B, V, 21, 2] frame pixels, "joints_cam": [B, 21, 3] millimetres as the dataset gives it (NOT modified),
    optionally "root_joint" [B, 3] millimetres, "root_idx", "joints_img_mask" [B, V, 21]}.  The B samples of the tracker's batch are B
    concurrent sequences ("lanes").  One step enqueues, on the current stream and copying nothing to the host: tracker.step; the labels
    into out["crop_boxes_used"] (on a ragged step the view mask is `present`); EpochEvaluator.add with inputs = {joints_crop_img,
    joints_cam / 1000, root_joint / 1000, root_idx, joints_img_mask = the mapped mask, bboxes = crop_boxes_used as fp32}; one
    hmv_seq_eval_add with the tracker's status and the slot info just written.  The inputs never carry "heatmap" (dataset maps are in
    the wrong window): by EpochEvaluator.add's rule the loss terms are computed exactly when model.heatmap_targets == "joints", with
    targets synthesised from the window-space labels, and are None otherwise.  A step with labels=None adds only to the sequence sums:
    jitter of the predictions and the status counts.  The millimetre-to-metre division runs on the device.

    cam_params is what the loss reads (intrinsic, extrinsic of the reprojection terms): with "g2d" among the model's loss weights it
    must carry "extrinsic" (TypeError otherwise).  The states live on the tracker's device and belong to the stream the steps run on."""

    def __init__(self, tracker, cam_params=None, mode: str = "test"):
        model = tracker.model
        if "g2d" in model.train_params.get("loss_weights", {}) and (cam_params is None or "extrinsic" not in cam_params
                                                            or "intrinsic" not in cam_params):
            raise TypeError('"g2d" is among the loss weights: cam_params["intrinsic"] and cam_params["extrinsic"] are required')
        self.tracker, self.model, self.mode, self.cam_params = tracker, model, mode, cam_params
        self.device = dev = tracker.device
        self.batch, self.num_views = tracker.batch, tracker.num_views
        lib = _lib.load()
        self._epoch = EpochEvaluator(model, mode)
        self.sums = torch.zeros(int(lib.hmv_seq_eval_sums_doubles(self.batch)), device=dev, dtype=torch.float64)
        self.history = torch.zeros(int(lib.hmv_seq_eval_history_floats(self.batch)), device=dev, dtype=torch.float32)
        self._restart = torch.zeros(self.batch, device=dev, dtype=torch.uint8)
        self._restart_pending = False
        self._unlabelled_steps = 0
        self._reduced: Optional[torch.Tensor] = None

    @property
    def state(self) -> Optional[torch.Tensor]:
        """The epoch state of the labelled steps (EpochEvaluator's), None before the first one."""
        return self._epoch.state

    def restart(self, crop_boxes0, lanes=None) -> None:
        """New sequences: tracker.reset(crop_boxes0), and the next step tells hmv_seq_eval_add that the lanes `lanes` (indices into
        the batch; default all) begin anew, so that no acceleration is taken across the cut.  Everything else keeps accumulating."""
        flags = np.zeros(self.batch, np.uint8)
        if lanes is None:
            flags[:] = 1
        else:
            idx = np.asarray(list(lanes), np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= self.batch):
                raise ValueError(f"lanes must be indices into the batch of {self.batch}")
            flags[idx] = 1
        self.tracker.reset(crop_boxes0)
        if self._restart_pending:   # two restarts without a step between them: both hold
            self._restart.bitwise_or_(torch.from_numpy(flags).to(self.device))
        else:
            self._restart.copy_(torch.from_numpy(flags))
        self._restart_pending = True

    def _check_labels(self, labels: dict) -> None:
        b, v = self.batch, self.num_views
        for key, shape in (("joints_img", (b, v, 21, 2)), ("joints_cam", (b, 21, 3))):
            if key not in labels:
                raise ValueError(f"labels must carry {key!r}")
            t = labels[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or not t.dtype.is_floating_point:
                raise ValueError(f"labels[{key!r}] must be a floating-point {list(shape)} tensor")
        m = labels.get("joints_img_mask")
        if m is not None and (not isinstance(m, torch.Tensor) or tuple(m.shape) != (b, v, 21)):
            raise ValueError(f"labels['joints_img_mask'] must be a {[b, v, 21]} tensor")
        r = labels.get("root_joint")
        if r is not None and (not isinstance(r, torch.Tensor) or r.numel() != b * 3):
            raise ValueError(f"labels['root_joint'] must hold {b} x 3 numbers")

    def step(self, frames: torch.Tensor, labels: Optional[dict] = None, view_mask=None) -> dict:
        """One time step; returns tracker.step's dictionary (views of the tracker's buffers, valid until the next step).  ValueError
        for labels of the wrong shape or type, before anything is launched."""
        if labels is not None:
            self._check_labels(labels)
        dev, b, v = self.device, self.batch, self.num_views
        out = self.tracker.step(frames, view_mask=view_mask)
        self._reduced = None
        keep = []
        a = _lib.HmvSeqEvalArgs()
        a.struct_size = ctypes.sizeof(_lib.HmvSeqEvalArgs)
        a.B, a.V = b, v
        a.pred_joints_cam, a.track_status = out["joints_cam"].data_ptr(), out["status"].data_ptr()
        if labels is None:
            self._unlabelled_steps += 1
        else:
            present = None if view_mask is None else device_view_mask(view_mask, b, v, dev)
            hidden = labels.get("joints_img_mask")
            crop, mask, info = labels_to_windows(labels["joints_img"].to(dev), out["crop_boxes_used"], self.tracker.image_size,
                                                 None if hidden is None else hidden.to(dev), present)
            inputs = {"joints_crop_img": crop, "joints_cam": labels["joints_cam"].detach().to(dev).float() / 1000,
                      "joints_img_mask": mask, "bboxes": out["crop_boxes_used"].float()}
            if labels.get("root_joint") is not None:
                inputs["root_joint"] = labels["root_joint"].detach().to(dev).float() / 1000
            if "root_idx" in labels:
                inputs["root_idx"] = labels["root_idx"]
            mine = dict(out)   # the loss adds its projection to the dictionary it is given: not to the tracker's
            if present is None:
                self._epoch.add(mine, inputs, self.cam_params)
            else:
                self._epoch.add(mine, inputs, self.cam_params, view_mask=present)
            gc = inputs["joints_cam"].contiguous()
            a.gt_joints_cam, a.slot_info = gc.data_ptr(), info.data_ptr()
            keep += [gc, info, present]
        if self._restart_pending:
            a.restart = self._restart.data_ptr()
        a.sums, a.sums_doubles = self.sums.data_ptr(), self.sums.numel()
        a.history, a.history_floats = self.history.data_ptr(), self.history.numel()
        with torch.cuda.device(dev):
            rc = _lib.load().hmv_seq_eval_add(_index(dev), ctypes.byref(a), _stream(dev))
        _lib.check(rc)
        if self._restart_pending:
            self._restart.zero_()           # behind the launch that read it, in stream order
            self._restart_pending = False
        del keep   # allocated on the stream the kernel runs on: the caching allocator reuses them in stream order
        return out

    def reduce(self, group=None) -> None:
        """Two all_reduce(SUM): the epoch state, and the lane-pooled sums [1 .. 10] (with the count of unlabelled lane-steps behind
        them).  The per-sequence list stays local to the rank.  Call it after the last step: a later step drops the reduced sums."""
        self._epoch.reduce(group)
        self._reduced = reduce_pooled(pool_sums(self.sums, self._unlabelled_steps * self.batch), group)

    def compute(self) -> dict:
        """ONE device->host copy of both states, the rest on the host.  With at least one labelled step: everything
        EpochEvaluator.compute returns (2D numbers in crop pixels of the followed windows).  Always:
          {mode}_mka               jitter of the predictions in millimetres, 1000 x sum[3] / sum[2] pooled over lanes (and restarts);
                                   NaN when no lane reached three steps
          {mode}_mka_gt            the labels' own jitter, from [4]; None unless EVERY step (of every rank, after reduce()) carried
                                   labels: a step without them leaves the label history stale, and [4] would mix sequences
          {mode}_mka_per_sequence  one value per lane (this rank's)
          window_moved / window_absent / window_kept   fractions of slot-steps with tracker status 0 / 1 / 2
          empty_windows            slot-steps whose window was empty (count)
          labels_outside_window    sum[10] / sum[9]: the fraction of visible label joints outside the window their step ran on;
                                   None without labelled steps
        Raises ValueError when no step was added."""
        n_state, n_sums = self._epoch.state_doubles, self.batch * _SUMS
        state = self._epoch.state if self._epoch.state is not None else torch.zeros(n_state, device=self.device, dtype=torch.float64)
        pooled = self._reduced if self._reduced is not None else pool_sums(self.sums, self._unlabelled_steps * self.batch)
        host = torch.cat([state, self.sums, pooled]).cpu().numpy()
        labelled = bool(host[0] > 0)
        seq = finish_sequence(host[n_state:n_state + n_sums], host[n_state + n_sums:], labelled, self.mode)   # raises for an empty one
        out = finish_state(host[:n_state], self._epoch.thr_min, self._epoch.thr_max, STEPS, self.mode) if labelled else {}
        out.update(seq)
        return out

    def reset(self) -> None:
        """An empty evaluation again (zero states are one); the tracker is not touched."""
        self._epoch.reset()
        self.sums.zero_()
        self.history.zero_()
        self._restart.zero_()
        self._restart_pending, self._unlabelled_steps, self._reduced = False, 0, None
