"""CPU restatement (numpy, float64) of the RAGGED evaluation-step losses and epoch state -- TEST INFRASTRUCTURE ONLY.

The rule (include/handmv.h, hmv_pose_losses_views): the value of any loss term or metric on a ragged batch is the mean, over the
batch's samples, of the value the reference logs for that sample alone (batch 1) over that sample's present views only.  So nothing
here restates a formula: the ragged loss is built from loss_oracle.losses and loss_oracle.project (both pinned to the real reference
by tests/golden/loss_cases.npz) called per sample, the ragged epoch state from epoch_oracle.accumulate called per sample.
Only tests/ may import this file.
"""
from __future__ import annotations

import functools

import numpy as np

import epoch_oracle as eo
import loss_oracle as lo

VIEW_TERMS = ("heatmap_loss", "joints_2d_loss", "g2d_loss", "p2d_loss")   # the terms that depend on the view mask


# ---------------------------------------------------------------- the masks of the ragged tests (cases of tests/golden/loss_cases.npz)
@functools.lru_cache(maxsize=None)
def case_mask(name: str) -> np.ndarray:
    """bool [B, V], True = the view is present.  Shared and cached: callers must not write into it."""
    if name == "vii_many":   # 38 x 8 = 304 frame slots > 256 lanes: every strided loop of the one-workgroup kernels wraps
        rng = np.random.default_rng(3)
        p = rng.random((38, 8)) < 0.6
        p[np.arange(38), rng.integers(0, 8, 38)] = True      # one forced present view per sample
        p[0] = True                                          # sample 0 is full
        p[1] = False
        p[1, 7] = True                                       # sample 1 has only view 7
        return p
    return np.array({"i_flag_on": [[1, 0, 1], [0, 0, 1]],
                     "iii_9x13": [[1, 0, 1, 1], [0, 1, 0, 0]],   # root camera (1) absent in sample 0; a single-view sample
                     "v_three": [[1, 0], [0, 1]],
                     "vi_sheared": [[1, 1, 0], [1, 0, 1]]}[name], bool)


MASKED_CASES = ("i_flag_on", "iii_9x13", "v_three", "vi_sheared", "vii_many")


# ---------------------------------------------------------------- the loss
def losses(pred_hm, target_hm, pred_2d, gt_2d, pred_cam, gt_cam, weights: dict, view_mask, mask=None, mask_invisible_joints=False,
           root_joint=None, root_idx=0, intrinsic=None, extrinsic=None, bbox=None):
    """Arguments as loss_oracle.losses in the full [B, V] layout, plus view_mask bool [B, V].
    -> (dict of the six TERMS, projected [B, V, 21, 2] float64 with zeros for absent views, or None)."""
    view_mask = np.asarray(view_mask, bool)
    B, V = view_mask.shape
    assert view_mask.any(axis=1).all(), "every sample needs a present view"
    plain = {k: weights[k] for k in ("heatmap", "joints_2d", "joints_3d")}
    with_proj = "g2d" in weights
    out = {t: 0.0 for t in lo.TERMS}
    projected = np.zeros((B, V, lo.NJ, 2), np.float64) if with_proj else None
    for b in range(B):
        P = np.flatnonzero(view_mask[b])
        one = slice(b, b + 1)
        terms, _ = lo.losses(np.asarray(pred_hm)[one][:, P], np.asarray(target_hm)[one][:, P], np.asarray(pred_2d)[one][:, P],
                             np.asarray(gt_2d)[one][:, P], np.asarray(pred_cam)[one], np.asarray(gt_cam)[one], plain,
                             None if mask is None else np.asarray(mask)[one][:, P], mask_invisible_joints)
        for t in ("heatmap_loss", "joints_2d_loss", "joints_3d_loss"):
            out[t] += terms[t] / B
        if with_proj:   # the sample's FULL camera table (the root camera may be absent), then the present rows
            rj = np.asarray(root_joint, np.float64).reshape(-1, 1, 3) if root_joint is not None else np.zeros((B, 1, 3))
            rj = np.broadcast_to(rj, (B, 1, 3))
            proj = lo.project(np.asarray(pred_cam, np.float64)[one] + rj[one], root_idx, np.asarray(intrinsic)[one],
                              np.asarray(extrinsic)[one], np.asarray(bbox)[one])[0]
            projected[b, P] = proj[P]
            out["g2d_loss"] += float(np.mean(np.abs(proj[P] - np.asarray(gt_2d, np.float64)[b, P]))) * weights["g2d"] / B
            out["p2d_loss"] += float(np.mean(np.abs(proj[P] - np.asarray(pred_2d, np.float64)[b, P]))) * weights["p2d"] / B
    out["loss"] = out["heatmap_loss"] + out["joints_2d_loss"] + out["joints_3d_loss"] + out["g2d_loss"] + out["p2d_loss"]
    return out, projected


def case_losses(name: str, view_mask):
    """losses() on a case of loss_oracle.loss_case."""
    c = lo.loss_case(name)
    return losses(c["pred_hm"], c["target"], c["pred_2d"], c["gt_2d"], c["pred_cam"], c["gt_cam"], c["weights"], view_mask, c["mask"],
                  c["flag"], c["root_joint"], c["root_idx"], c["intr"], c["extr"], c["bbox"])


# ---------------------------------------------------------------- the epoch state
def accumulate(state, pred_cam, gt_cam, pred_2d, gt_2d, view_mask, mask=None, loss=None, thr_min=0.0, thr_max=0.02, steps=20):
    """Adds one ragged step in place (layout: include/handmv.h).  Each sample goes through epoch_oracle.accumulate alone, over its
    present views; [5] counts rows in units of a full sample (V * 21 per sample) and the sample's 2D sum is scaled by V / v_b, so
    [6] / [5] is the mean over samples of the per-sample 2D MPJPE."""
    view_mask = np.asarray(view_mask, bool)
    B, V = view_mask.shape
    assert pred_2d.shape[:2] == (B, V) and view_mask.any(axis=1).all()
    for b in range(B):
        P = np.flatnonzero(view_mask[b])
        one = eo.new_state(steps)
        eo.accumulate(one, pred_cam[b:b + 1], gt_cam[b:b + 1], pred_2d[b:b + 1][:, P], gt_2d[b:b + 1][:, P],
                      None if mask is None else np.asarray(mask)[b:b + 1][:, P], None, thr_min, thr_max, steps)
        state[[0, 2, 3, 4]] += one[[0, 2, 3, 4]]
        state[eo.SCALARS:] += one[eo.SCALARS:]
        state[5] += V * eo.NJ
        state[6] += one[6] * V / len(P)
    state[1] += 1
    if loss is not None:
        state[7] += B
        for i, term in enumerate(lo.TERMS):
            state[8 + i] += B * float(loss[term])
    return state


def mpjpe2d(pred_2d, gt_2d, view_mask, mask=None) -> float:
    """The rule spelled out for the 2D metric: mean over samples of the reference's mpjpe on the sample's present views."""
    from oracle import metrics_oracle as mo
    view_mask = np.asarray(view_mask, bool)
    vals = []
    for b in range(view_mask.shape[0]):
        P = np.flatnonzero(view_mask[b])
        keep = np.ones((len(P), eo.NJ, 1), np.float32) if mask is None else (~np.asarray(mask, bool)[b, P])[..., None].astype(np.float32)
        vals.append(mo.mpjpe(pred_2d[b, P] * keep, gt_2d[b, P] * keep))
    return float(np.mean(vals))
