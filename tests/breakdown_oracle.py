"""CPU restatement (numpy) of what hmv_eval_breakdown_add accumulates and of its record rows -- TEST INFRASTRUCTURE ONLY.

The layouts are include/handmv.h's ("evaluation breakdown").  Every entry is oracle.metrics_oracle's mpjpe / compute_similarity_transform
or tests/epoch_oracle.histogram applied to one joint column or one camera slice.  Only tests/ may import this file.
"""
from __future__ import annotations

import numpy as np

import epoch_oracle as eo
from epoch_oracle import mo

NJ = 21
HEADER = 4


def doubles(V: int, steps: int = 20) -> int:
    return HEADER + 2 * NJ + NJ * (steps + 1) + V * (1 + 2 * NJ)


def new_state(V: int, steps: int = 20) -> np.ndarray:
    return np.zeros(doubles(V, steps), np.float64)


def slices(state, V: int, steps: int = 20) -> dict:
    """Views into a state: J3 [21], JPA [21], H [21, steps + 1], CN [V], C2 [V, 21], CV [V, 21]."""
    assert state.size == doubles(V, steps)
    at, out = HEADER, {}
    for name, shape in (("J3", (NJ,)), ("JPA", (NJ,)), ("H", (NJ, steps + 1)), ("CN", (V,)), ("C2", (V, NJ)), ("CV", (V, NJ))):
        n = int(np.prod(shape))
        out[name] = state[at:at + n].reshape(shape)
        at += n
    return out


def _keep(shape, mask):
    return np.ones(shape + (1,), np.float32) if mask is None else (~np.asarray(mask, bool))[..., None].astype(np.float32)


def accumulate(state, pred_cam, gt_cam, pred_2d, gt_2d, mask=None, present=None, thr_min=0.0, thr_max=0.02, steps=20):
    """Adds one step in place.  Shapes as epoch_oracle.accumulate; present [B, V] bool (True = the view is there) or None.  An
    absent slot is never read (its inputs may be NaN) and adds nothing."""
    B, V = pred_2d.shape[:2]
    s = slices(state, V, steps)
    if state[1] == 0:
        state[2], state[3] = V, steps
    state[0] += B
    state[1] += 1
    aligned = mo.compute_similarity_transform(pred_cam, gt_cam)
    for j in range(NJ):
        s["J3"][j] += mo.mpjpe(pred_cam[:, j], gt_cam[:, j]) * B
        s["JPA"][j] += mo.mpjpe(aligned[:, j], gt_cam[:, j]) * B
        s["H"][j] += eo.histogram(pred_cam[:, j], gt_cam[:, j], thr_min, thr_max, steps)
    here = np.ones((B, V), bool) if present is None else np.asarray(present, bool)
    keep = _keep((B, V, NJ), mask)
    for v in range(V):
        rows = here[:, v]
        n = int(rows.sum())
        s["CN"][v] += n
        if n == 0:
            continue
        p, g = (pred_2d[rows, v] * keep[rows, v]), (gt_2d[rows, v] * keep[rows, v])       # zeroed on both sides (models/utils.py:123-131)
        for j in range(NJ):
            s["C2"][v, j] += mo.mpjpe(p[:, j], g[:, j]) * n
            s["CV"][v, j] += int(keep[rows, v, j, 0].sum())
    return state


def record_rows(pred_cam, gt_cam, pred_2d, gt_2d, mask=None, present=None) -> np.ndarray:
    """[B, 4 + V] float64: mpjpe, pa_mpjpe (metres), the sample's 2D MPJPE over its present views, v_b, the 2D error per camera (NaN
    for an absent one; the sample's own value is NaN without any view)."""
    B, V = pred_2d.shape[:2]
    aligned = mo.compute_similarity_transform(pred_cam, gt_cam)
    here = np.ones((B, V), bool) if present is None else np.asarray(present, bool)
    keep = _keep((B, V, NJ), mask)
    out = np.full((B, 4 + V), np.nan)
    for b in range(B):
        out[b, 0] = mo.mpjpe(pred_cam[b], gt_cam[b])
        out[b, 1] = mo.mpjpe(aligned[b], gt_cam[b])
        out[b, 3] = here[b].sum()
        for v in np.flatnonzero(here[b]):
            out[b, 4 + v] = mo.mpjpe(pred_2d[b, v] * keep[b, v], gt_2d[b, v] * keep[b, v])
        if here[b].any():
            out[b, 2] = mo.mpjpe(pred_2d[b, here[b]] * keep[b, here[b]], gt_2d[b, here[b]] * keep[b, here[b]])
    return out
