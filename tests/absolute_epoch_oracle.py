"""CPU restatement (numpy) of what hmv_eval_absolute_add accumulates -- TEST INFRASTRUCTURE ONLY.

The layout is include/handmv.h's ("absolute evaluation").  The two fp32 sums of the world distance -- joints_cam + the triangulated
root, and the label's joints_cam + root_joint -- are made in float32 exactly as the kernel makes them; everything after them
(differences, norms, sums) is float64.  Only tests/ may import this file.
"""
from __future__ import annotations

import numpy as np

NJ = 21
FIXED = 155   # header (8), W, T, TN (21 each), S (84)


def doubles(V: int) -> int:
    return FIXED + 1 + 3 * V


def new_state(V: int) -> np.ndarray:
    return np.zeros(doubles(V), np.float64)


def slices(state, V: int) -> dict:
    """Views into a state: W, T, TN [21], S [21, 4], R, RN [V], H [V + 1]."""
    assert state.size == doubles(V)
    at, out = 8, {}
    for name, shape in (("W", (NJ,)), ("T", (NJ,)), ("TN", (NJ,)), ("S", (NJ, 4)), ("R", (V,)), ("RN", (V,)), ("H", (V + 1,))):
        n = int(np.prod(shape))
        out[name] = state[at:at + n].reshape(shape)
        at += n
    return out


def located(tri, status) -> np.ndarray:
    """[B] bool: the root joint has status 0 and three finite coordinates."""
    return (np.asarray(status)[:, 0] == 0) & np.isfinite(np.asarray(tri)[:, 0]).all(-1)


def _norm(a, b):
    return np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(-1))


def world_distance(pred_cam, tri, gt_cam, gt_root) -> np.ndarray:
    """[B, 21] float64: |(pred_cam + tri[:, :1]) - (gt_cam + gt_root)| with both sums in float32."""
    pred_cam, tri, gt_cam = (np.asarray(a, np.float32) for a in (pred_cam, tri, gt_cam))
    gt_root = np.asarray(gt_root, np.float32).reshape(-1, 1, 3)
    with np.errstate(invalid="ignore"):
        return _norm(pred_cam + tri[:, :1], gt_cam + gt_root)


def accumulate(state, pred_cam, tri, status, gt_cam, gt_root, reproj=None, inliers=None, V=None):
    """Adds one step in place and returns the state.  pred_cam, tri, gt_cam [B, 21, 3]; status [B, 21]; gt_root [B, 3] or [B, 1, 3];
    reproj [B, V, 21] or None; inliers [B, 21] or None; V is read from reproj, from the state's length otherwise."""
    tri, gt_cam = np.asarray(tri, np.float32), np.asarray(gt_cam, np.float32)
    status = np.asarray(status)
    gt_root = np.asarray(gt_root, np.float32).reshape(-1, 1, 3)
    B = tri.shape[0]
    if V is None:
        V = reproj.shape[1] if reproj is not None else (state.size - FIXED - 1) // 3
    if state[2] not in (0, V):
        raise ValueError("this state was begun with another V")
    s = slices(state, V)
    found = located(tri, status)
    state[0] += B
    state[1] += 1
    state[2] = V
    state[3] += found.sum()
    w = world_distance(pred_cam, tri, gt_cam, gt_root)
    with np.errstate(invalid="ignore"):
        t = _norm(tri, gt_cam + gt_root)
        root = _norm(tri[:, 0], gt_root[:, 0])
    cols = w[found].sum(0) if found.any() else np.zeros(NJ)
    s["W"] += cols
    state[4] += cols.sum()
    state[5] += root[found].sum()
    ok = (status == 0) & np.isfinite(tri).all(-1)
    s["T"] += np.where(ok, t, 0.0).sum(0)
    s["TN"] += ok.sum(0)
    clamped = np.where((status < 0) | (status > 3), 3, status)
    for k in range(4):
        s["S"][:, k] += (clamped == k).sum(0)
    good = status == 0
    if reproj is not None:
        e = np.asarray(reproj, np.float32).astype(np.float64)
        use = good[:, None, :] & np.isfinite(e)
        s["R"] += np.where(use, e, 0.0).sum((0, 2))
        s["RN"] += use.sum((0, 2))
    if inliers is not None:
        k = np.clip(np.asarray(inliers).astype(np.int64), 0, V)
        s["H"] += np.bincount(k[good], minlength=V + 1)
    return state


def finish(state) -> dict:
    """The epoch's numbers in the state's own units (metres, pixels), float64; None for a ratio with a zero count."""
    state = np.asarray(state, np.float64)
    V = (state.size - FIXED - 1) // 3
    s = slices(state, V)

    def over(total, count):
        return float(total / count) if count > 0 else None

    n = state[3]
    return {"w_mpjpe": over(state[4], n * NJ), "root_err": over(state[5], n), "w_mpjpe_per_joint": [over(x, n) for x in s["W"]],
            "tri_mpjpe": over(s["T"].sum(), s["TN"].sum()), "tri_mpjpe_per_joint": [over(x, c) for x, c in zip(s["T"], s["TN"])],
            "tri_status_counts": s["S"].astype(np.int64).tolist(), "tri_reproj_per_camera": [over(x, c) for x, c in zip(s["R"], s["RN"])],
            "tri_reproj": over(s["R"].sum(), s["RN"].sum()), "tri_inlier_hist": s["H"].astype(np.int64).tolist(),
            "located": int(n), "lost": int(state[0] - n)}
