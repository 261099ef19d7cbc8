"""Attention maps of the fusion blocks, read per camera.

The engine hands out what the reference returns from ``MultiHeadAttention.forward(x, return_attention=True)`` and
``MultiHeadAttentionLearnableQuery.forward(x, return_attention=True)`` (layers.py:202-237, 267-301): ``attn[b, h, i, j]``, and the
share of it per view, ``share[b, h, i, r] = sum of attn over the 21 keys of the view of rank r`` (``HandMvNet.forward_attention``,
include/handmv.h: hmv_set_attention_capture).  This module holds what sits on top of that: the index of the cross block, the move from
view ranks to camera slots for ragged view sets, and an accumulator over an evaluation run.  Nothing here is a hot path: torch ops on
small device tensors, one readback at the end.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch


def cross_block_index(model_params: dict) -> int:
    """The fusion block whose 21 outputs draw on the views: block (fusion_layers - 1) // 2 of CrossAttentionFusion (fusion.py:16-22),
    block 2 -- the probe block -- of CrossAttentionFusionLearnableQuery, which always has five (fusion.py:39-45)."""
    if model_params["fusion"] == "cross_attn_learnable_query":
        return 2
    layers = int(model_params.get("fusion_layers", 5))
    if layers < 1 or layers % 2 == 0:
        raise ValueError(f"fusion_layers must be a positive odd number, got {layers}")
    return (layers - 1) // 2


def share_to_cameras(share_by_rank: torch.Tensor, view_mask=None, num_views: Optional[int] = None) -> torch.Tensor:
    """[b, 8, Tq, R] by view RANK -> [b, 8, Tq, V] by CAMERA SLOT: the column of rank r of sample b moves to the r-th present camera
    of view_mask[b] (bool [b, V], True = present; tensor, array or nested list, read on the host); absent cameras are 0.
    view_mask None: every camera is present and rank = slot (V = num_views or R)."""
    if share_by_rank.dim() != 4:
        raise ValueError("share_by_rank must be [b, heads, Tq, ranks]")
    b, nh, tq, R = share_by_rank.shape
    if view_mask is None:
        V = R if num_views is None else int(num_views)
        if V < R:
            raise ValueError(f"{R} ranks do not fit {V} cameras")
        out = share_by_rank.new_zeros(b, nh, tq, V)
        out[..., :R] = share_by_rank
        return out
    mask = view_mask.detach().cpu().numpy() if isinstance(view_mask, torch.Tensor) else np.asarray(view_mask)
    mask = mask.astype(bool)
    if mask.ndim != 2 or mask.shape[0] != b:
        raise ValueError(f"view_mask must have shape [{b}, V], got {list(mask.shape)}")
    V = mask.shape[1]
    counts = mask.sum(axis=1)
    if (counts > R).any():
        raise ValueError(f"a sample has {int(counts.max())} present views, the share has {R} ranks")
    # src[b, v] = rank of camera v among sample b's present ones; absent cameras read an appended zero column (index R)
    src = np.where(mask, np.cumsum(mask, axis=1) - 1, R).astype(np.int64)
    idx = torch.from_numpy(src).to(share_by_rank.device)[:, None, None, :].expand(b, nh, tq, V)
    padded = torch.cat([share_by_rank, share_by_rank.new_zeros(b, nh, tq, 1)], dim=-1)
    return padded.gather(-1, idx)


class ViewAttentionMeter:
    """Accumulates ``out["view_attention"]`` ([b, 21, V]: per output joint, the share of the cross block's attention that goes to each
    camera slot, averaged over heads) over the batches of a run, on the device; ``compute()`` reads back once.

    query_view: True for ``cross_attn``, whose cross block takes its queries from the first present camera of a sample -- that camera's
    own share is 0 by construction -- so the meter also counts how often each camera was that one."""

    def __init__(self, num_views: int, query_view: bool = True):
        self.num_views = int(num_views)
        self.query_view = bool(query_view)
        self._sum: Optional[torch.Tensor] = None        # [21, V] float64
        self._present: Optional[torch.Tensor] = None    # [V] float64
        self._query: Optional[torch.Tensor] = None      # [V] float64
        self._samples = 0

    def add(self, out, view_mask=None) -> None:
        va = out["view_attention"] if isinstance(out, dict) else out
        if va.dim() != 3 or va.shape[1] != 21 or va.shape[2] != self.num_views:
            raise ValueError(f"view_attention must be [b, 21, {self.num_views}], got {list(va.shape)}")
        b, dev = va.shape[0], va.device
        if view_mask is None:
            present = torch.ones(b, self.num_views, dtype=torch.float64, device=dev)
        else:
            present = (view_mask if isinstance(view_mask, torch.Tensor) else torch.as_tensor(np.asarray(view_mask))).to(dev).to(torch.float64)
            if tuple(present.shape) != (b, self.num_views):
                raise ValueError(f"view_mask must have shape [{b}, {self.num_views}], got {list(present.shape)}")
        if self._sum is None:
            self._sum = torch.zeros(21, self.num_views, dtype=torch.float64, device=dev)
            self._present = torch.zeros(self.num_views, dtype=torch.float64, device=dev)
            self._query = torch.zeros(self.num_views, dtype=torch.float64, device=dev)
        self._sum += (va.to(torch.float64) * present[:, None, :]).sum(0)
        self._present += present.sum(0)
        first = (present.cumsum(1) == 1) & (present > 0)      # the first present camera of every sample
        self._query += first.to(torch.float64).sum(0)
        self._samples += b

    def compute(self) -> Dict[str, object]:
        """{"per_joint_camera": [21, V] mean share over the samples in which the camera is present (nan for a camera never present),
        "per_camera": [V] its mean over the joints, "present": [V] samples per camera, "samples": their number, and for cross_attn
        "query_view_fraction": [V] the fraction of samples in which the camera supplied the queries}."""
        if self._sum is None:
            raise RuntimeError("ViewAttentionMeter.compute() before any add()")
        state = torch.cat([self._sum.reshape(-1), self._present, self._query]).cpu().numpy()   # the one readback
        V = self.num_views
        s, present, query = state[:21 * V].reshape(21, V), state[21 * V:22 * V], state[22 * V:]
        with np.errstate(invalid="ignore", divide="ignore"):
            per = s / present[None, :]
        res = {"per_joint_camera": per, "per_camera": per.mean(0), "present": present, "samples": self._samples}
        if self.query_view:
            res["query_view_fraction"] = query / max(self._samples, 1)
        return res
