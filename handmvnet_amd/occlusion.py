"""Occlusion sweeps from raw frames: which patch of which camera's window the 3D prediction rests on, and what happens when the hand is
partly hidden in one camera -- at the cost of one clean per-frame pass plus one occluded frame per (variant, sample) instead of a full
forward per variant.

The occluder is the reference's ``OcclusionAugmentation`` (datasets/augment.py:102-129): one cell of a patch grid on the cropped uint8
window is zeroed before ToTensor / Resize / Normalize.  Here it is a rectangle (rx1, ry1, rx2, ry2) in window pixels from the window's
top-left corner, half-open, clipped to the window (include/handmv.h); the reference's patch (patch_size p, row r, column c) is
(c p, r p, (c + 1) p, (r + 1) p).  The per-frame stage does not depend on the other views, so ``HandMvNet.forward_frames_occlusions`` /
``hmv_forward_frames_occlusions`` prepare and push through the backbone only the occluded frame of each variant and reuse the clean token
rows of the other cameras; the fusion blocks and the decoder run per variant.

The rule that defines every number: variant o's outputs and epoch values are what ``forward_frames`` / ``evaluate`` give on the same
batches when, in camera occ_view[o]'s frames, the frame pixels under the rectangle are zeroed.  ``OcclusionSweepEvaluator`` reaches that by
construction: per step one ``forward_frames_occlusions`` call, then per variant the same ``EpochEvaluator.add`` on that variant's
composed output -- the same launches on the same bits in the same fp64 order.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .evaluation import STEPS, EpochEvaluator, finish_state, reduce_state


def cell_rects(crop_boxes: torch.Tensor, grid: int, row: int, col: int) -> torch.Tensor:
    """The rectangles of cell (row, col) of a grid x grid occluder layout on every window of `crop_boxes` (int [..., 4] = x1, y1, x2,
    y2): int32 [..., 4] on the boxes' device, computed there with integer ops (no host copy).  p = min(cw, ch) // grid and the rect is
    (col p, row p, (col + 1) p, (row + 1) p): since grid p <= min(cw, ch), every such cell is a patch the reference's class can draw with
    patch_size = p.  A window smaller than `grid` (or an empty one) gives p = 0, an empty rectangle, hence the clean result.  (Sides are
    taken as at most 65536 px, the widest window the frame preparation accepts: wider ones are black views whatever the rectangle.)"""
    grid, row, col = int(grid), int(row), int(col)
    if grid < 1:
        raise ValueError(f"grid must be at least 1, got {grid}")
    if not (0 <= row < grid and 0 <= col < grid):
        raise ValueError(f"cell ({row}, {col}) is outside the {grid} x {grid} grid")
    if not isinstance(crop_boxes, torch.Tensor) or crop_boxes.is_floating_point() or crop_boxes.shape[-1:] != (4,):
        raise ValueError("crop_boxes must be an int tensor [..., 4]")
    bx = crop_boxes.to(torch.int64)
    cw, ch = bx[..., 2] - bx[..., 0], bx[..., 3] - bx[..., 1]
    p = torch.div(torch.minimum(cw, ch).clamp(min=0, max=1 << 16), grid, rounding_mode="floor")
    return torch.stack((col * p, row * p, (col + 1) * p, (row + 1) * p), dim=-1).to(torch.int32)


def grid_variants(V: int, grid: int, cameras: Optional[Sequence[int]] = None) -> List[Tuple[int, int, int]]:
    """The variants of a sweep as (camera, row, col), camera-major, then row-major, over `cameras` (None: all V, in order).  ValueError
    for V < 1, grid < 1, no camera, a camera that is no integer, outside [0, V) or named twice."""
    V, grid = int(V), int(grid)
    if V < 1:
        raise ValueError(f"grid_variants needs V >= 1, got V = {V}")
    if grid < 1:
        raise ValueError(f"grid must be at least 1, got {grid}")
    if cameras is None:
        cams = list(range(V))
    else:
        if isinstance(cameras, torch.Tensor):
            cameras = cameras.detach().cpu().numpy()
        cams = []
        for i, c in enumerate(np.asarray(cameras).tolist() if isinstance(cameras, np.ndarray) else list(cameras)):
            if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer, float, np.floating)) or int(c) != c:
                raise ValueError(f"cameras[{i}]: camera indices must be integers")
            if not 0 <= int(c) < V:
                raise ValueError(f"cameras[{i}]: camera {int(c)} is outside [0, {V})")
            if int(c) in cams:
                raise ValueError(f"cameras[{i}]: camera {int(c)} is named twice")
            cams.append(int(c))
        if not cams:
            raise ValueError("a sweep needs at least one camera")
    return [(c, r, k) for c in cams for r in range(grid) for k in range(grid)]


def sensitivity_maps(clean: dict, per_variant: Sequence[dict], variants: Sequence[Tuple[int, int, int]], V: int, grid: int) -> dict:
    """Per scalar key of `clean` a [V, grid, grid] float array of value(variant) - value(clean) at [camera, row, col]; cells of cameras
    not swept are NaN, and so is a key that is None on either side.  Lists (the PCK curve, the thresholds) and the sample / step counts
    are left out."""
    if len(per_variant) != len(variants):
        raise ValueError("one result dict per variant")
    out = {}
    for key, v0 in clean.items():
        if key in ("samples", "steps") or isinstance(v0, (list, tuple, bool)):
            continue
        if v0 is not None and not isinstance(v0, (int, float, np.integer, np.floating)):
            continue
        m = np.full((int(V), int(grid), int(grid)), np.nan)
        for (c, r, k), res in zip(variants, per_variant):
            v = res.get(key)
            if v0 is not None and v is not None:
                m[c, r, k] = float(v) - float(v0)
        out[key] = m
    return out


class OcclusionSweepEvaluator:
    """EpochEvaluator for the clean batches and every cell of a grid x grid occluder on every camera of `cameras` at once: an fp64 state
    [1 + n_occ][state] on the device (row 0 clean), one forward_frames_occlusions call per step.

        ev = OcclusionSweepEvaluator(model, grid=4)
        for batch in loader: ev.step(batch)
        ev.reduce()                      # only under torch.distributed: ONE all-reduce of the whole state
        numbers = ev.compute()           # ONE readback: {"variants", "clean", "per_variant", "sensitivity"}

    Batches bring raw frames: batch["data"]["frames"] (uint8 [B, V, Hf, Wf, 3]) and ["crop_boxes"] (int [B, V, 4]).  Nothing is copied
    to the host per step."""

    def __init__(self, model, grid: int = 4, cameras=None, mode: str = "test"):
        self.model, self.mode, self.grid = model, mode, int(grid)
        self.variants = grid_variants(model.num_views, grid, cameras)
        self.occ_view = np.array([c for c, _, _ in self.variants], dtype=np.int32)
        self._rows = [EpochEvaluator(model, mode) for _ in range(1 + len(self.variants))]   # each accumulates into its row of self.state
        self.state_doubles = self._rows[0].state_doubles
        self.state: Optional[torch.Tensor] = None

    def _state_on(self, dev: torch.device) -> torch.Tensor:
        if self.state is None:
            self.state = torch.zeros(len(self._rows), self.state_doubles, device=dev, dtype=torch.float64)
            for ev, row in zip(self._rows, self.state):
                ev.state = row
        elif self.state.device != dev:
            raise ValueError(f"this epoch's state is on {self.state.device}, the step on {dev}")
        return self.state

    def rects(self, crop_boxes: torch.Tensor) -> torch.Tensor:
        """The sweep's rectangles for one batch of windows [B, V, 4]: int32 [n_occ, B, 4], made on the windows' device."""
        cells = {}
        rows = []
        for c, r, k in self.variants:
            if (r, k) not in cells:
                cells[(r, k)] = cell_rects(crop_boxes, self.grid, r, k)
            rows.append(cells[(r, k)][:, c])
        return torch.stack(rows, dim=0)

    def add(self, out: dict, inputs: dict, cam_params) -> None:
        """One step from forward_frames_occlusions' `out` and the labels as _eval_step passes them (joints_cam / root_joint in metres):
        the clean output into state row 0, then per variant its composed output -- joints_cam[1 + o], and the clean joints_crop_img /
        heatmap with camera occ_view[o]'s slice replaced by the variant's -- into row 1 + o, each through EpochEvaluator.add."""
        cam = out["joints_cam"]
        n = len(self.variants)
        if cam.dim() != 4 or cam.shape[0] != 1 + n:
            raise ValueError(f"out['joints_cam'] must be forward_frames_occlusions' [{1 + n}, B, 21, 3]")
        self._state_on(cam.device)
        crop, hm = out["joints_crop_img"], out["heatmap"]
        self._rows[0].add({"joints_cam": cam[0], "joints_crop_img": crop, "heatmap": hm}, inputs, cam_params)
        for o, (c, _, _) in enumerate(self.variants):
            crop_o, hm_o = crop.clone(), hm.clone()
            crop_o[:, c] = out["joints_crop_img_occ"][o]
            hm_o[:, c] = out["heatmap_occ"][o]
            self._rows[1 + o].add({"joints_cam": cam[1 + o], "joints_crop_img": crop_o, "heatmap": hm_o}, inputs, cam_params)

    def step(self, batch: dict) -> dict:
        """forward_frames_occlusions + add for one batch; like the reference's test_step it converts inputs["joints_cam"] /
        ["root_joint"] from mm to metres IN PLACE.  The windows serve as the reprojection loss's bboxes when inputs["bboxes"] is
        absent.  Returns the forward's output dictionary."""
        if batch.get("view_mask") is not None:
            raise ValueError("an occlusion sweep takes full-view batches: batch['view_mask'] must be absent")
        inputs = batch["data"]
        frames, boxes = inputs["frames"], inputs["crop_boxes"]
        boxes = boxes.to(frames.device)
        out = self.model.forward_frames_occlusions(frames, boxes, self.occ_view, self.rects(boxes), batch["cam_params"])
        inputs["joints_cam"] /= 1000
        if "root_joint" in inputs:
            inputs["root_joint"] /= 1000
        if "bboxes" not in inputs:
            inputs = dict(inputs, bboxes=boxes.float())
        self.add(out, inputs, batch["cam_params"])
        return out

    def reduce(self, group=None) -> None:
        """ONE all_reduce(SUM) of the whole [1 + n_occ][state] tensor; a rank that saw no batch takes part with a zero state."""
        if self.state is None:
            self._state_on(torch.device("cuda", torch.cuda.current_device()))
        reduce_state(self.state, group)

    def finish(self, host) -> dict:
        """compute() from a host copy of the state [1 + n_occ][state]."""
        ev = self._rows[0]
        host = np.asarray(host, dtype=np.float64).reshape(len(self._rows), self.state_doubles)
        res = [finish_state(row, ev.thr_min, ev.thr_max, STEPS, self.mode) for row in host]
        return {"variants": list(self.variants), "clean": res[0], "per_variant": res[1:],
                "sensitivity": sensitivity_maps(res[0], res[1:], self.variants, self.model.num_views, self.grid)}

    def compute(self) -> dict:
        """ONE device->host copy of the state.  "variants": the (camera, row, col) list; "clean" and "per_variant": EpochEvaluator
        .compute()'s dict on the clean and on each variant's frames; "sensitivity": sensitivity_maps() of them.  Raises ValueError for an
        empty epoch."""
        host = np.zeros((len(self._rows), self.state_doubles)) if self.state is None else self.state.cpu().numpy()
        return self.finish(host)

    def reset(self) -> None:
        """An empty epoch again."""
        if self.state is not None:
            self.state.zero_()
