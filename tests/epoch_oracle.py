"""CPU restatement (numpy) of the evaluation-epoch state that hmv_eval_add accumulates -- TEST INFRASTRUCTURE ONLY.

The layout is include/handmv.h's ("State layout"); every entry is built from oracle.metrics_oracle (mpjpe, pa_mpjpe, the fp32
comparison of pck) and, for the loss slots, from the dictionaries tests/loss_oracle.py returns.  Only tests/ may import this file.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import metrics_oracle as mo  # noqa: E402

import loss_oracle as lo  # noqa: E402

NJ = 21
SCALARS = 14


def new_state(steps: int = 20) -> np.ndarray:
    return np.zeros(SCALARS + 1 + steps, np.float64)


def histogram(pred, gt, thr_min, thr_max, steps) -> np.ndarray:
    """steps + 1 integer bins: rows whose FIRST threshold with dist <= thr is thr[i] (the comparison of mo.pck: fp32 distances
    against fp32 thresholds), and a last bin for the rows beyond thr_max."""
    thr = mo.linspace_f32(thr_min, thr_max, steps)
    d = pred.astype(np.float32) - gt.astype(np.float32)
    dist = np.sqrt((d * d).sum(axis=-1, dtype=np.float32))
    within = np.array([int((dist <= t).sum()) for t in thr] + [dist.size], np.int64)   # cumulative, thresholds ascend
    return np.diff(np.concatenate([[0], within]))


def accumulate(state, pred_cam, gt_cam, pred_2d, gt_2d, mask=None, loss=None, thr_min=0.0, thr_max=0.02, steps=20):
    """Adds one step in place.  pred_cam / gt_cam [B, 21, 3], pred_2d / gt_2d [B, V, 21, 2], mask [B, V, 21] bool (True = invisible)
    or None, loss: a dictionary with the six lo.TERMS (what lo.losses returns) or None for a step without loss labels."""
    B, V = pred_2d.shape[:2]
    assert state.size == SCALARS + 1 + steps and pred_cam.shape == (B, NJ, 3)
    rows3, rows2 = B * NJ, B * V * NJ
    keep = np.ones((B, V, NJ, 1), np.float32) if mask is None else (~np.asarray(mask, bool))[..., None].astype(np.float32)
    state[0] += B
    state[1] += 1
    state[2] += rows3
    state[3] += mo.mpjpe(pred_cam, gt_cam) * rows3
    state[4] += mo.pa_mpjpe(pred_cam, gt_cam) * rows3
    state[5] += rows2
    state[6] += mo.mpjpe(pred_2d * keep, gt_2d * keep) * rows2     # zeroed on both sides, still counted (models/utils.py:123-131)
    if loss is not None:
        state[7] += B
        for i, term in enumerate(lo.TERMS):
            state[8 + i] += B * float(loss[term])
    state[SCALARS:] += histogram(pred_cam, gt_cam, thr_min, thr_max, steps)
    return state


def finish(state, thr_min=0.0, thr_max=0.02, steps=20) -> dict:
    """The epoch's numbers from a state, by the reference's formulas: means in float64, the PCK curve and the trapezoid in fp32."""
    thr = mo.linspace_f32(thr_min, thr_max, steps)
    cum = np.cumsum(state[SCALARS:SCALARS + steps])
    pck = cum.astype(np.float32) / np.float32(state[2])
    dx = thr[1:] - thr[:-1]
    auc = float(np.sum(dx * (pck[1:] + pck[:-1]) * np.float32(0.5), dtype=np.float32))
    one = float(np.sum(dx, dtype=np.float32))
    out = {"mpjpe": state[3] / state[2] * 1000, "pa_mpjpe": state[4] / state[2] * 1000, "mpjpe2d": state[6] / state[5],
           "pck": pck, "thr": thr, "auc": auc, "norm_auc": auc / one, "samples": int(state[0]), "steps": int(state[1])}
    for i, term in enumerate(lo.TERMS):
        out[term] = state[8 + i] / state[7] if state[7] > 0 else None
    return out
