"""Reference-view sweeps: every camera of a rig as the reference view, at the cost of one backbone pass per step.

The model treats the first view it is fed as special: the cross-attention block takes its queries from it, ``joints_cam`` comes out
root-relative in its camera frame, and the sinusoidal positions count the other views in feed order.  Everything up to the per-frame
token rows does not depend on the feed order, so ``HandMvNet.forward_orders`` / ``hmv_forward_orders`` (include/handmv.h) run it
once on the full batch and repeat only the positional encoding, the fusion blocks and the decoder per order.

The rule that defines every number: an order is a list of k distinct cameras (1 <= k <= V), the first one the reference view, and
order s's ``joints_cam`` holds the bits ``forward_views`` returns for the batch with its views permuted by that order --
``x[:, order]``, ``bbox[:, order]``, ``intrinsic[:, order]`` in the first k view slots under a mask of k leading ``True``.  A sorted
order is a subset (``forward_subsets``' bits); the identity order over all V cameras has ``forward()``'s.

V reference views give V estimates of the same hand.  ``pose_consensus`` (``hmv_op_pose_consensus``, one launch) rotates them into
one camera's frame by the extrinsics and returns their mean or geometric median, the per-joint spread -- the only uncertainty signal
this model can produce -- and each estimate's distance from the consensus.  ``ReferenceSweepEvaluator`` answers "which camera should
be the reference view on this rig" over an epoch.

For the learnable-query fusion the sweep is defined by the same rule; the alignment takes whatever ``ref_cam`` the caller passes
(by default each order's first camera), and which frame that model's output is in is a property of its training, not of the engine.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .evaluation import STEPS, EpochEvaluator, finish_state, reduce_state

MODES = {"mean": 0, "median": 1}


def each_reference(V: int) -> List[List[int]]:
    """V orders over all V cameras: order c is camera c followed by the other cameras ascending."""
    V = int(V)
    if V < 1:
        raise ValueError(f"each_reference needs V >= 1, got {V}")
    return [[c] + [v for v in range(V) if v != c] for c in range(V)]


def rotations(V: int) -> List[List[int]]:
    """The V cyclic shifts of the cameras: order c is c, c + 1, ..., V - 1, 0, ..., c - 1."""
    V = int(V)
    if V < 1:
        raise ValueError(f"rotations needs V >= 1, got {V}")
    return [[(c + i) % V for i in range(V)] for c in range(V)]


def as_order_table(orders, V: int) -> np.ndarray:
    """A sweep's orders as the host int32 table [S, V] hmv_forward_orders reads: each row lists its cameras from the left and is padded
    with -1.  `orders`: a sequence of camera-index lists, or an integer array / tensor [S, <= V] already padded with -1.  ValueError
    for no order, an empty order, a camera outside [0, V), a camera named twice in one order, a non-negative entry after a -1, or a
    row longer than V.  Duplicate orders are allowed."""
    V = int(V)
    if isinstance(orders, torch.Tensor):
        orders = orders.detach().cpu().numpy()
    if isinstance(orders, np.ndarray):
        if orders.ndim != 2 or orders.dtype.kind not in "iu":
            raise ValueError(f"orders must be a sequence of camera-index lists or an integer [S, <= {V}] table padded with -1")
        rows = orders.tolist()
    else:
        rows = [np.asarray(r).tolist() if isinstance(r, (torch.Tensor, np.ndarray)) else list(r) for r in orders]
    if not rows:
        raise ValueError("a sweep needs at least one order")
    table = np.full((len(rows), V), -1, dtype=np.int32)
    for s, row in enumerate(rows):
        if len(row) > V:
            raise ValueError(f"order {s} has {len(row)} entries, the rig has {V} cameras")
        k, padded = 0, False
        for c in row:
            if isinstance(c, (bool, np.bool_)) or int(c) != c:
                raise ValueError(f"order {s}: camera indices must be integers")
            c = int(c)
            if c == -1:
                padded = True
                continue
            if not 0 <= c < V:
                raise ValueError(f"order {s}: camera {c} is outside [0, {V})")
            if padded:
                raise ValueError(f"order {s}: camera {c} comes after a -1")
            if c in table[s, :k]:
                raise ValueError(f"order {s}: camera {c} is named twice")
            table[s, k] = c
            k += 1
        if k == 0:
            raise ValueError(f"order {s} has no camera")
    return np.ascontiguousarray(table)


def order_lists(table: np.ndarray) -> List[List[int]]:
    """The camera-index lists of an order table."""
    return [[int(c) for c in row if c >= 0] for row in np.asarray(table)]


def pose_consensus(poses, ref_cam, extrinsic, target: int = 0, mode: str = "mean", iterations: int = 16,
                   outputs=("aligned", "consensus", "spread", "deviation")) -> dict:
    """S root-relative estimates of the same hands, estimate s in camera ref_cam[s]'s frame, in camera `target`'s frame and reduced
    (hmv_op_pose_consensus: one launch, fp64 arithmetic in a documented order, nothing copied to the host).
      poses      [S, B, 21, 3] device tensor (forward_orders' joints_cam)
      ref_cam    S camera indices: a list / array (one small upload) or an int32 device tensor; a value outside [0, V) in a DEVICE
                 tensor cannot be refused and makes that estimate's outputs NaN
      extrinsic  [B, V, 4, 4], the reference's convention world = E [x; 1]
      mode       "mean" or "median" (the geometric median: `iterations` Weiszfeld steps from the mean, no early exit)
    Returns the requested `outputs` as fp32 device tensors: "aligned" [S, B, 21, 3], "consensus" [B, 21, 3], "spread" [B, 21] (the
    root mean square over s of |aligned_s - consensus|, in the poses' unit), "deviation" [S, B] (the mean over joints of
    |aligned_s - consensus|).  A singular extrinsic gives non-finite values, as hmv_project_joints does."""
    if mode not in MODES:
        raise ValueError('mode must be "mean" or "median"')
    if not isinstance(poses, torch.Tensor) or poses.dim() != 4 or tuple(poses.shape[2:]) != (21, 3):
        raise ValueError("poses must be a [S, B, 21, 3] tensor")
    if not poses.is_cuda:
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: poses must be a CUDA(HIP) tensor (no CPU fallback)")
    dev = poses.device
    S, B = int(poses.shape[0]), int(poses.shape[1])
    p = poses.detach().float().contiguous()
    e = extrinsic.detach().to(dev).float().contiguous()
    if e.dim() != 4 or e.shape[0] != B or tuple(e.shape[2:]) != (4, 4):
        raise ValueError(f"extrinsic must be [{B}, V, 4, 4]")
    V = int(e.shape[1])
    if isinstance(ref_cam, torch.Tensor) and ref_cam.is_cuda:
        rc = ref_cam.detach().to(dev).to(torch.int32).contiguous()
    else:
        host = np.asarray(ref_cam.detach().cpu().numpy() if isinstance(ref_cam, torch.Tensor) else ref_cam)
        if host.ndim != 1 or host.dtype.kind not in "iu":
            raise ValueError("ref_cam must hold one integer camera index per estimate")
        bad = np.flatnonzero((host < 0) | (host >= V))
        if bad.size:
            raise ValueError(f"ref_cam[{int(bad[0])}] = {int(host[bad[0]])} is outside [0, {V})")
        rc = torch.from_numpy(host.astype(np.int32)).to(dev)
    if rc.numel() != S:
        raise ValueError(f"ref_cam must hold {S} entries, one per estimate")
    unknown = set(outputs) - {"aligned", "consensus", "spread", "deviation"}
    if unknown or not outputs:
        raise ValueError(f"outputs must name some of aligned, consensus, spread, deviation (got {sorted(unknown) or 'none'})")
    shapes = {"aligned": (S, B, 21, 3), "consensus": (B, 21, 3), "spread": (B, 21), "deviation": (S, B)}
    out = {k: torch.empty(shapes[k], device=dev, dtype=torch.float32) for k in shapes if k in outputs}
    a = _lib.HmvConsensusArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvConsensusArgs)
    a.S, a.B, a.V, a.target_cam, a.mode, a.iterations = S, B, V, int(target), MODES[mode], int(iterations)
    a.poses, a.ref_cam, a.extrinsic = p.data_ptr(), rc.data_ptr(), e.data_ptr()
    for k, t in out.items():
        setattr(a, k, t.data_ptr())
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().hmv_op_pose_consensus(idx, ctypes.byref(a), stream))
    del p, e, rc   # allocated on the stream the kernel runs on: the caching allocator reuses them in stream order
    return out


class ReferenceSweepEvaluator:
    """EpochEvaluator for S reference-view orders and their consensus at once: an fp64 state [S + 1][state] on the device, one
    forward_orders call and one pose_consensus call per step.

        ev = ReferenceSweepEvaluator(model, each_reference(8), "test")
        for batch in loader: ev.step(batch)
        ev.reduce()                      # only under torch.distributed: ONE all-reduce of the whole state
        numbers = ev.compute()           # ONE readback: {"orders", "per_order", "consensus", "best_reference"}

    orders=None: each_reference(model.num_views).  consensus: "mean" or "median".  Every estimate is rotated into the frame of camera
    inputs["root_idx"] (0 when the batch has none), the frame the labels are in; row s accumulates the rotated estimate of order s,
    row S the consensus, each through the loss and hmv_eval_add entries EpochEvaluator runs on a full-view batch.  Batches are uniform
    full-view batches (no batch["view_mask"]) and carry cam_params["extrinsic"].  Nothing is copied to the host per step.

    With the learnable-query fusion the numbers are defined by the same rule; which frame that model's output is in is a property of
    its training, not of the engine."""

    def __init__(self, model, orders=None, mode: str = "test", consensus: str = "mean"):
        if consensus not in MODES:
            raise ValueError('consensus must be "mean" or "median"')
        self.model, self.mode, self.consensus = model, mode, consensus
        self.table = as_order_table(each_reference(model.num_views) if orders is None else orders, model.num_views)
        self.orders = order_lists(self.table)
        self._ref_host = np.ascontiguousarray(self.table[:, 0])
        self._ref_dev: Optional[torch.Tensor] = None
        self._rows = [EpochEvaluator(model, mode) for _ in range(len(self.orders) + 1)]   # each accumulates into its row of self.state
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

    def add(self, out: dict, inputs: dict, cam_params) -> dict:
        """One step from forward_orders' `out` and the labels as _eval_step passes them (joints_cam / root_joint in metres): one
        pose_consensus call, then per order and for the consensus the loss (when the batch carries loss labels) and one hmv_eval_add
        into that row of the state.  Returns pose_consensus' dict."""
        cam = out["joints_cam"]
        S = len(self.orders)
        if cam.dim() != 4 or cam.shape[0] != S:
            raise ValueError(f"out['joints_cam'] must be forward_orders' [{S}, B, 21, 3]")
        if cam_params is None or "extrinsic" not in cam_params:
            raise ValueError("a reference-view sweep needs cam_params['extrinsic']")
        self._state_on(cam.device)
        if self._ref_dev is None:   # the one upload of the epoch
            self._ref_dev = torch.from_numpy(self._ref_host).to(cam.device)
        target = 0
        if "root_idx" in inputs:
            root_idx = inputs["root_idx"]
            target = int(root_idx[0]) if hasattr(root_idx, "__len__") else int(root_idx)
        res = pose_consensus(cam, self._ref_dev, cam_params["extrinsic"], target=target, mode=self.consensus)
        for s, ev in enumerate(self._rows):
            one = {"joints_cam": res["aligned"][s] if s < S else res["consensus"], "joints_crop_img": out["joints_crop_img"],
                   "heatmap": out["heatmap"]}
            ev.add(one, inputs, cam_params)
        return res

    def step(self, batch: dict) -> dict:
        """forward_orders + add for one batch of the reference's DataLoader layout; like the reference's test_step it converts
        inputs["joints_cam"] / ["root_joint"] from mm to metres IN PLACE.  Returns the forward's output dictionary."""
        if batch.get("view_mask") is not None:
            raise ValueError("a sweep takes full-view batches: the orders name the cameras, batch['view_mask'] must be absent")
        inputs = batch["data"]
        out = self.model.forward_orders(inputs["rgb"], self.table, inputs["bboxes"], batch["cam_params"])
        inputs["joints_cam"] /= 1000
        if "root_joint" in inputs:
            inputs["root_joint"] /= 1000
        self.add(out, inputs, batch["cam_params"])
        return out

    def reduce(self, group=None) -> None:
        """ONE all_reduce(SUM) of the whole [S + 1][state] tensor; a rank that saw no batch takes part with a zero state."""
        if self.state is None:
            self._state_on(torch.device("cuda", torch.cuda.current_device()))
        reduce_state(self.state, group)

    def compute(self) -> dict:
        """ONE device->host copy of the state.  "orders": the camera-index lists; "per_order": per order EpochEvaluator.compute()'s
        dict for its rotated estimate; "consensus": that dict for the consensus pose; "best_reference": the index of the order with
        the lowest {mode}_mpjpe, the lowest index among equals.  Raises ValueError for an empty epoch."""
        S = len(self.orders)
        host = np.zeros((S + 1, self.state_doubles)) if self.state is None else self.state.cpu().numpy()
        ev = self._rows[0]
        rows = [finish_state(host[s], ev.thr_min, ev.thr_max, STEPS, self.mode) for s in range(S + 1)]
        key = f"{self.mode}_mpjpe"
        best = min(range(S), key=lambda s: (rows[s][key], s))
        return {"orders": [list(o) for o in self.orders], "per_order": rows[:S], "consensus": rows[S], "best_reference": best}

    def reset(self) -> None:
        """An empty epoch again."""
        if self.state is not None:
            self.state.zero_()
