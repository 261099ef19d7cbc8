"""Camera-subset sweeps: the camera ablation ("how does accuracy change with the number and placement of cameras, which k of the V to
keep") at the cost of one backbone pass per step instead of one per subset.

Everything up to the per-frame token rows does not depend on which other views are present, so ``HandMvNet.forward_subsets`` /
``hmv_forward_subsets`` (include/handmv.h) run it once on the full batch and repeat only the positional encoding, the fusion blocks
and the decoder per subset.  One subset table serves the whole batch -- that is what an ablation is.

The rule that defines every number: subset s's outputs and epoch values are what ``forward_views`` / ``evaluate`` give on the same
batches with ``view_mask`` equal to subset s on every sample.  ``SubsetSweepEvaluator`` reaches that by construction: per step one
``forward_subsets`` call, then per subset the ragged loss and accumulation entries ``EpochEvaluator`` runs (``hmv_pose_losses_views``,
``hmv_eval_add_views``) with that subset's mask broadcast over the batch, on that subset's slice of ``joints_cam`` -- the same launches
on the same bits in the same fp64 order.
"""
from __future__ import annotations

import itertools
from typing import List, Optional, Sequence

import numpy as np
import torch

from .evaluation import STEPS, EpochEvaluator, finish_state, reduce_state


def k_of_n(V: int, k: int) -> List[List[int]]:
    """All subsets of k of the V cameras as sorted index lists, in lexicographic order (C(V, k) of them)."""
    V, k = int(V), int(k)
    if V < 1 or not 1 <= k <= V:
        raise ValueError(f"k_of_n needs 1 <= k <= V, got V = {V}, k = {k}")
    return [list(c) for c in itertools.combinations(range(V), k)]


def as_subset_table(subsets, V: int) -> np.ndarray:
    """A sweep's subsets as the host uint8 table [S, V] hmv_forward_subsets reads (1 = the camera is present).  `subsets`: a bool / 0-1
    array, tensor or nested list of shape [S, V], or a sequence of camera-index lists.  ValueError for no subset, an empty subset, a
    camera outside [0, V), a camera named twice, or a mask whose width is not V.  Duplicate subsets are allowed."""
    V = int(V)
    if isinstance(subsets, torch.Tensor):
        subsets = subsets.detach().cpu().numpy()
    is_mask = isinstance(subsets, np.ndarray) and subsets.ndim == 2
    if not is_mask and not isinstance(subsets, np.ndarray):
        rows = [list(r) if not isinstance(r, (torch.Tensor, np.ndarray)) else np.asarray(r).tolist() for r in subsets]
        # a nested list of bools of width V is a mask; lists of ints are camera indices
        is_mask = bool(rows) and all(len(r) > 0 and all(isinstance(v, (bool, np.bool_)) for v in r) for r in rows)
        if is_mask:
            if any(len(r) != V for r in rows):
                raise ValueError(f"a subset mask must have {V} columns (one per camera)")
            subsets = np.array(rows, dtype=bool)
    if is_mask:
        mask = np.asarray(subsets)
        if mask.shape[1] != V:
            raise ValueError(f"a subset mask must have {V} columns (one per camera), got {mask.shape[1]}")
        table = (mask != 0).astype(np.uint8)
    else:
        if isinstance(subsets, np.ndarray):
            raise ValueError(f"subsets must be a [S, {V}] mask or a sequence of camera-index lists")
        table = np.zeros((len(rows), V), dtype=np.uint8)
        for s, cams in enumerate(rows):
            for c in cams:
                if isinstance(c, (bool, np.bool_)) or int(c) != c:
                    raise ValueError(f"subset {s}: camera indices must be integers")
                if not 0 <= int(c) < V:
                    raise ValueError(f"subset {s}: camera {int(c)} is outside [0, {V})")
                if table[s, int(c)]:
                    raise ValueError(f"subset {s}: camera {int(c)} is named twice")
                table[s, int(c)] = 1
    if table.shape[0] == 0:
        raise ValueError("a sweep needs at least one subset")
    empty = np.flatnonzero(table.sum(axis=1) == 0)
    if empty.size:
        raise ValueError(f"subset {int(empty[0])} has no camera")
    return np.ascontiguousarray(table)


def subset_lists(table: np.ndarray) -> List[List[int]]:
    """The camera-index lists of a subset table."""
    return [np.flatnonzero(row).tolist() for row in np.asarray(table)]


def by_count(per_subset: Sequence[dict], subsets: Sequence[Sequence[int]]) -> dict:
    """Per view count k, the plain mean over the subsets with k cameras of every scalar entry of their result dicts (lists such as the
    PCK curve are left out; an entry that is None for one of the subsets is None), plus "subsets": how many were averaged."""
    if len(per_subset) != len(subsets):
        raise ValueError("one result dict per subset")
    out = {}
    for k in sorted({len(s) for s in subsets}):
        rows = [r for r, s in zip(per_subset, subsets) if len(s) == k]
        mean = {}
        for key, v0 in rows[0].items():
            vals = [r[key] for r in rows]
            if all(v is None for v in vals) or any(v is None for v in vals):
                mean[key] = None
            elif isinstance(v0, (int, float, np.integer, np.floating)) and not isinstance(v0, bool):
                mean[key] = float(sum(float(v) for v in vals) / len(vals))
        mean["subsets"] = len(rows)
        out[k] = mean
    return out


class SubsetSweepEvaluator:
    """EpochEvaluator for S camera subsets at once: an fp64 state [S][state] on the device, one forward_subsets call per step.

        ev = SubsetSweepEvaluator(model, k_of_n(8, 4), "test")
        for batch in loader: ev.step(batch)
        ev.reduce()                      # only under torch.distributed: ONE all-reduce of the whole state
        numbers = ev.compute()           # ONE readback: {"subsets", "per_subset", "by_count"}

    Batches are uniform full-view batches (no batch["view_mask"]).  Nothing is copied to the host per step."""

    def __init__(self, model, subsets, mode: str = "test"):
        self.model, self.mode = model, mode
        self.table = as_subset_table(subsets, model.num_views)
        self.subsets = subset_lists(self.table)
        self._masks = self.table.astype(bool)
        self._masks_dev: Optional[torch.Tensor] = None
        self._rows = [EpochEvaluator(model, mode) for _ in self.subsets]   # each accumulates into its row of self.state
        self.state_doubles = self._rows[0].state_doubles
        self.state: Optional[torch.Tensor] = None

    def _state_on(self, dev: torch.device) -> torch.Tensor:
        if self.state is None:
            self.state = torch.zeros(len(self.subsets), self.state_doubles, device=dev, dtype=torch.float64)
            for ev, row in zip(self._rows, self.state):
                ev.state = row
        elif self.state.device != dev:
            raise ValueError(f"this epoch's state is on {self.state.device}, the step on {dev}")
        return self.state

    def add(self, out: dict, inputs: dict, cam_params) -> None:
        """One step from forward_subsets' `out` and the labels as _eval_step passes them (joints_cam / root_joint in metres): per
        subset the ragged loss (when the batch carries loss labels) and one hmv_eval_add_views into that subset's state row."""
        cam = out["joints_cam"]
        if cam.dim() != 4 or cam.shape[0] != len(self.subsets):
            raise ValueError(f"out['joints_cam'] must be forward_subsets' [{len(self.subsets)}, B, 21, 3]")
        self._state_on(cam.device)
        if self._masks_dev is None:   # the one upload of the epoch; the per-subset masks below are device views of it
            self._masks_dev = torch.from_numpy(self._masks).to(cam.device)
        B, V = cam.shape[1], self._masks.shape[1]
        for s, ev in enumerate(self._rows):
            one = {"joints_cam": cam[s], "joints_crop_img": out["joints_crop_img"], "heatmap": out["heatmap"]}
            ev.add(one, inputs, cam_params, view_mask=self._masks_dev[s].expand(B, V))

    def step(self, batch: dict) -> dict:
        """forward_subsets + add for one batch of the reference's DataLoader layout; like the reference's test_step it converts
        inputs["joints_cam"] / ["root_joint"] from mm to metres IN PLACE.  Returns the forward's output dictionary."""
        if batch.get("view_mask") is not None:
            raise ValueError("a sweep takes full-view batches: the subsets name the cameras, batch['view_mask'] must be absent")
        inputs = batch["data"]
        out = self.model.forward_subsets(inputs["rgb"], self.table, inputs["bboxes"], batch["cam_params"])
        inputs["joints_cam"] /= 1000
        if "root_joint" in inputs:
            inputs["root_joint"] /= 1000
        self.add(out, inputs, batch["cam_params"])
        return out

    def reduce(self, group=None) -> None:
        """ONE all_reduce(SUM) of the whole [S][state] tensor; a rank that saw no batch takes part with a zero state."""
        if self.state is None:
            self._state_on(torch.device("cuda", torch.cuda.current_device()))
        reduce_state(self.state, group)

    def compute(self) -> dict:
        """ONE device->host copy of the state.  "subsets": the camera-index lists; "per_subset": per subset EpochEvaluator.compute()'s
        dict; "by_count": by_count() of those.  Raises ValueError for an empty epoch."""
        S = len(self.subsets)
        host = np.zeros((S, self.state_doubles)) if self.state is None else self.state.cpu().numpy()
        ev = self._rows[0]
        per = [finish_state(host[s], ev.thr_min, ev.thr_max, STEPS, self.mode) for s in range(S)]
        return {"subsets": [list(s) for s in self.subsets], "per_subset": per, "by_count": by_count(per, self.subsets)}

    def reset(self) -> None:
        """An empty epoch again."""
        if self.state is not None:
            self.state.zero_()
