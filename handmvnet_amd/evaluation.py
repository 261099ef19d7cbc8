"""A whole evaluation epoch on the device: what ``trainer.validate`` / ``trainer.test`` hand back in the reference
(eval.py: one set of epoch numbers, dumped as val.json / test.json), without a host round trip per step.

``EpochEvaluator.step(batch)`` enqueues the forward, the loss (``HandMvNet._calculate_loss``) and ONE accumulation launch
(``hmv_eval_add``, include/handmv.h) that adds the step into an fp64 state vector on the device; nothing is copied to the host and
nothing synchronises, so the next step's launches queue up under this step's kernels.  ``reduce()`` is one all-reduce of that
vector, ``compute()`` one device->host copy followed by a handful of divisions.

The epoch value.  For every quantity it is

    sum over steps and ranks of (B x the step's value)  /  sum of B,

the batch-size-weighted mean that Lightning's ``self.log(..., on_epoch=True)`` produces from the per-step values the reference logs.
MPJPE, PA-MPJPE, 2D MPJPE and the PCK curve are linear in the rows, so for them this equals the value on the pooled split and does
not depend on how the split is cut into batches and ranks; AUC is the trapezoid of that pooled curve (linear in the curve as well).
Ragged view sets.  A batch may carry ``batch["view_mask"]`` (bool [B, V], True = the view is present; keep it on the HOST, where
``forward_views`` reads it).  The step then runs ``forward_views``, the ragged loss (``hmv_pose_losses_views``) and the ragged
accumulation (``hmv_eval_add_views``): still one loss call and one accumulation launch, nothing copied to the host.  The value of a
view-dependent quantity on such a batch is the mean over its samples of the value the reference logs for that sample alone over its
present views, so the epoch value again does not depend on the cut into batches and ranks; for a full mask it is the uniform value.
``view_mask_from_joints`` derives the mask from the ``joints_img_mask`` a reference batch already carries.

Lightning is not a dependency of this package, so the ``_epoch`` / ``_step`` suffixes its loggers add to a key logged with both
``on_step`` and ``on_epoch`` cannot be pinned and are not reproduced: the keys are the names the reference passes to ``self.log``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .losses import TERMS, _device_f32, _index, device_view_mask

STEPS = 20       # thresholds of the PCK curve (handmvnet.py:359-363)
_SCALARS = 14    # state[0 .. 14): counts and sums, then the steps + 1 histogram bins (include/handmv.h: "State layout")


def view_mask_from_joints(joints_img_mask):
    """joints_img_mask [..., V, 21] (True = the joint is invisible; tensor or array) -> view mask [..., V], True = the view is present:
    a view is absent when none of its joints is visible, the dataset's own rule for feeding a black image (datasets/ho3d.py:138-140)."""
    if isinstance(joints_img_mask, torch.Tensor):
        return ~joints_img_mask.bool().all(-1)
    return ~np.asarray(joints_img_mask).astype(bool).all(-1)


def reduce_state(state: torch.Tensor, group=None) -> torch.Tensor:
    """ONE all_reduce(SUM) of an epoch state, in place: afterwards every rank holds the sums over all ranks.  The state is additive
    element by element, so this is all a multi-rank epoch needs.  Any tensor on any backend (gloo drives it on the CPU)."""
    dist.all_reduce(state, op=dist.ReduceOp.SUM, group=group)
    return state


def finish_state(state, thr_min: float, thr_max: float, steps: int, mode: str) -> dict:
    """The epoch's numbers from a state vector on the host (15 + steps doubles), under the names the reference logs.
    Raises ValueError for an empty epoch."""
    s = np.asarray(state, dtype=np.float64).reshape(-1)
    if s.size != _SCALARS + 1 + steps:
        raise ValueError(f"an epoch state with {steps} thresholds has {_SCALARS + 1 + steps} elements, not {s.size}")
    if not s[0] > 0:
        raise ValueError("empty epoch: no step was added")
    thr = torch.linspace(thr_min, thr_max, steps).numpy()                       # fp32, as metrics.py:106 builds them
    pck = np.cumsum(s[_SCALARS:_SCALARS + steps]).astype(np.float32) / np.float32(s[2])
    auc, one = np.float32(0), np.float32(0)                                      # fp32 trapezoid (metrics.py:114-121)
    for i in range(1, steps):
        dx = thr[i] - thr[i - 1]
        auc += dx * (pck[i] + pck[i - 1]) * np.float32(0.5)
        one += dx
    out = {f"{mode}_mpjpe": float(s[3] / s[2] * 1000), f"{mode}_pa_mpjpe": float(s[4] / s[2] * 1000), f"{mode}_mpjpe2d": float(s[6] / s[5]),
           f"{mode}_pck_j": pck.tolist(), f"{mode}_auc_j": float(auc),
           f"{mode}_norm_auc_j": float(auc / one) if steps > 1 else float("nan"), "thresholds": thr.tolist()}
    for i, term in enumerate(TERMS):
        out[f"{mode}/{term}"] = float(s[8 + i] / s[7]) if s[7] > 0 else None
    out[f"{mode}/root_3d_loss"] = 0.0 if s[7] > 0 else None                      # the constant of a root-relative model
    out["samples"], out["steps"] = int(s[0]), int(s[1])
    return out


class EpochEvaluator:
    """Accumulates evaluation steps of `model` (a HandMvNet) on the device; see the module docstring for the epoch value.

        ev = EpochEvaluator(model, "test")
        for batch in loader: ev.step(batch)
        ev.reduce()                      # only under torch.distributed
        numbers = ev.compute()

    The state lives on the device of the first step (a zeroed fp64 tensor of hmv_eval_state_doubles(20) elements) and belongs to
    the stream the steps run on."""

    def __init__(self, model, mode: str = "test"):
        self.model, self.mode = model, mode
        self.thr_min, self.thr_max = float(model.auc_thresh[0]), float(model.auc_thresh[1])
        self.state_doubles = int(_lib.load().hmv_eval_state_doubles(STEPS))
        self.state: Optional[torch.Tensor] = None

    def _state_on(self, dev: torch.device) -> torch.Tensor:
        if self.state is None:
            self.state = torch.zeros(self.state_doubles, device=dev, dtype=torch.float64)
        elif self.state.device != dev:
            raise ValueError(f"this epoch's state is on {self.state.device}, the step on {dev}")
        return self.state

    def add(self, out: dict, inputs: dict, cam_params, view_mask=None) -> None:
        """One step from the forward's `out` and the labels as _eval_step passes them (joints_cam / root_joint in metres): the loss
        when the batch carries loss labels, then one hmv_eval_add on the current stream.  Returns nothing; nothing reaches the host.
        view_mask (bool [B, V], True = present): `out` is forward_views' and the step is a ragged one -- the ragged loss and
        hmv_eval_add_views; rows of absent views are not read."""
        pc = _device_f32("out['joints_cam']", out["joints_cam"])
        dev = pc.device
        p2 = _device_f32("out['joints_crop_img']", out["joints_crop_img"], dev)
        gc = _device_f32("inputs['joints_cam']", inputs["joints_cam"], dev)
        g2 = _device_f32("inputs['joints_crop_img']", inputs["joints_crop_img"], dev)
        if pc.dim() != 3 or tuple(pc.shape[1:]) != (21, 3) or gc.shape != pc.shape:
            raise ValueError("joints_cam must be [B, 21, 3] in the output and in the labels")
        B = pc.shape[0]
        if p2.dim() != 4 or p2.shape[0] != B or tuple(p2.shape[2:]) != (21, 2) or g2.shape != p2.shape:
            raise ValueError(f"joints_crop_img must be [{B}, V, 21, 2] in the output and in the labels")
        V = p2.shape[1]
        keep = [pc, p2, gc, g2]
        a = _lib.HmvEvalArgs()
        a.struct_size = ctypes.sizeof(_lib.HmvEvalArgs)
        a.B, a.V, a.steps, a.thr_min, a.thr_max = B, V, STEPS, self.thr_min, self.thr_max
        a.pred_joints_cam, a.gt_joints_cam, a.pred_joints_2d, a.gt_joints_2d = pc.data_ptr(), gc.data_ptr(), p2.data_ptr(), g2.data_ptr()
        if "joints_img_mask" in inputs:   # _calculate_mpjpe masks whatever train_params["mask_invisible_joints"] says
            mk = inputs["joints_img_mask"].detach().to(dev).reshape(B, V, 21).ne(0).to(torch.uint8).contiguous()
            a.joints_mask = mk.data_ptr()
            keep.append(mk)
        if "heatmap" in inputs or self.model.heatmap_targets == "joints":   # _eval_step's rule
            if view_mask is None:
                self.model._calculate_loss(out, inputs, cam_params, mode=self.mode)
            else:
                self.model._calculate_loss(out, inputs, cam_params, mode=self.mode, view_mask=view_mask)
            loss = self.model.last_loss_vector
            a.loss_result = loss.data_ptr()
            keep.append(loss)
        state = self._state_on(dev)
        a.state, a.state_doubles = state.data_ptr(), state.numel()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            if view_mask is None:
                rc = _lib.load().hmv_eval_add(_index(dev), ctypes.byref(a), stream)
            else:
                present = device_view_mask(view_mask, B, V, dev)
                keep.append(present)
                rc = _lib.load().hmv_eval_add_views(_index(dev), ctypes.byref(a), present.data_ptr(), stream)
        _lib.check(rc)
        del keep   # allocated on the stream the kernel runs on: the caching allocator reuses them in stream order

    def step(self, batch: dict) -> dict:
        """forward + add for one batch of the reference's DataLoader layout; like the reference's test_step it converts
        inputs["joints_cam"] / ["root_joint"] from mm to metres IN PLACE.  Returns the forward's output dictionary."""
        inputs = batch["data"]
        view_mask = batch.get("view_mask")
        if view_mask is None:
            out = self.model.forward(inputs["rgb"], inputs["bboxes"], batch["cam_params"])
        else:   # raises ValueError for a sample without a present view, before anything is launched
            out = self.model.forward_views(inputs["rgb"], view_mask, inputs["bboxes"], batch["cam_params"])
        inputs["joints_cam"] /= 1000
        if "root_joint" in inputs:
            inputs["root_joint"] /= 1000
        if view_mask is None:
            self.add(out, inputs, batch["cam_params"])
        else:
            self.add(out, inputs, batch["cam_params"], view_mask=view_mask)
        return out

    def reduce(self, group=None) -> None:
        """One all_reduce(SUM) of the state over `group`: afterwards every rank holds the global sums.  A rank that saw no batch
        takes part with a zero state."""
        if self.state is None:
            self._state_on(torch.device("cuda", torch.cuda.current_device()))
        reduce_state(self.state, group)

    def compute(self) -> dict:
        """ONE device->host copy of the state, the rest on the host (finish_state).  {mode}_mpjpe / {mode}_pa_mpjpe in millimetres,
        {mode}_mpjpe2d in crop pixels, {mode}_pck_j (list), {mode}_auc_j, {mode}_norm_auc_j, thresholds (list), {mode}/heatmap_loss
        ... {mode}/p2d_loss, {mode}/root_3d_loss, {mode}/loss (None when no step carried a loss), samples, steps.
        Raises ValueError for an empty epoch."""
        host = np.zeros(self.state_doubles) if self.state is None else self.state.cpu().numpy()
        return finish_state(host, self.thr_min, self.thr_max, STEPS, self.mode)

    def reset(self) -> None:
        """An empty epoch again (a zero state is one)."""
        if self.state is not None:
            self.state.zero_()
