"""CPU restatement (numpy) of the vertex state that hmv_eval_vertices_add accumulates and of its record rows -- TEST INFRASTRUCTURE
ONLY.

The layout is include/handmv.h's ("vertex evaluation").  Both meshes are divided by unit_div in fp32; the distance is fp32 like
epoch_oracle.histogram's, with the roundings csrc/pose_rows.h pins for distance_3 -- sqrt(fma(d1, d1, d0 * d0) + d2 * d2) -- so that the
fp64 sums here and on the device are sums of the SAME fp32 terms (tests/test_vertices_epoch_oracle.py holds the bins to
epoch_oracle.histogram's on the fixture).  Sums are float64, sample after sample in feed order; the alignment is
oracle.metrics_oracle.compute_similarity_transform.  A sample with a non-zero status is skipped: it counts in [4] and nowhere else.
Only tests/ may import this file.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import metrics_oracle as mo  # noqa: E402

SCALARS = 8


def doubles(n_verts: int, steps: int = 20) -> int:
    return SCALARS + steps + 1 + 2 * n_verts


def scratch_bytes(B: int, n_verts: int, steps: int = 20) -> int:
    return B * (8 * (steps + 4) + 12 * n_verts)


def new_state(n_verts: int, steps: int = 20) -> np.ndarray:
    return np.zeros(doubles(n_verts, steps), np.float64)


def slices(state, steps: int = 20) -> dict:
    nv = (state.size - doubles(0, steps)) // 2
    at = SCALARS + steps + 1
    return {"H": state[SCALARS:at], "PV": state[at:at + nv], "PVA": state[at + nv:at + 2 * nv]}


def divided(x, unit_div) -> np.ndarray:
    """x / unit_div in fp32, correctly rounded (numpy's fp32 division is)."""
    return np.asarray(x, np.float32) / np.float32(unit_div)


def distance_f32(p, g) -> np.ndarray:
    """|p - g| over the last axis in fp32 with distance_3's roundings; the fused multiply-add through fma_f32."""
    d = p.astype(np.float32) - g.astype(np.float32)
    sq0 = d[..., 0] * d[..., 0]
    sq2 = d[..., 2] * d[..., 2]
    with np.errstate(invalid="ignore"):
        return np.sqrt(fma_f32(d[..., 1], d[..., 1], sq0) + sq2)


def fma_f32(a, b, c) -> np.ndarray:
    """fl32(a * b + c) with ONE rounding, for fp32 arrays.  The product of two fp32 values is exact in float64; the float64 sum s is
    rounded, and its error e is exact (the two-sum of Knuth).  Rounding s to fp32 can only go wrong when s sits exactly half way
    between two fp32 values -- a value float64 holds, so the first rounding cannot step over it -- and the true sum does not: there
    the sign of e decides, where ties-to-even would have."""
    x = a.astype(np.float64) * b.astype(np.float64)
    y = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = x + y
        t = s - x
        e = (x - (s - t)) + (y - t)
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        toward = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = np.isfinite(s) & (s != r64) & ((r64 + toward.astype(np.float64)) * 0.5 == s)
        up = np.maximum(r, toward)
        down = np.minimum(r, toward)
        return np.where(tie & (e > 0), up, np.where(tie & (e < 0), down, r)).astype(np.float32)


def bins(dist, thr_min, thr_max, steps) -> np.ndarray:
    """steps + 1 integer bins of fp32 distances, epoch_oracle.histogram's rule: the first threshold with dist <= thr, the last bin for
    the rest (a NaN lands there)."""
    thr = mo.linspace_f32(thr_min, thr_max, steps)
    with np.errstate(invalid="ignore"):
        within = np.array([int((dist <= t).sum()) for t in thr] + [dist.size], np.int64)
    return np.diff(np.concatenate([[0], within]))


def aligned_svd(p, g) -> np.ndarray:
    """[n] float64 distances that remain after the similarity alignment of one mesh: the reference's route.  A mesh with a non-finite
    coordinate gives NaN throughout (numpy's SVD raises on one; the reference's and the device's propagate it)."""
    if not (np.isfinite(p).all() and np.isfinite(g).all()):
        return np.full(p.shape[0], np.nan)
    y =mo.compute_similarity_transform(p[None], g[None])[0]
    return np.linalg.norm(y - g.astype(np.float64), axis=-1)


def aligned_eig(p, g) -> np.ndarray:
    """The same by a second float64 route: V and the squared singular values from the eigen-decomposition of K^T K, U = K V / s."""
    S1, S2 = p.astype(np.float64).T, g.astype(np.float64).T
    mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = (X1 ** 2).sum()
    K = X1 @ X2.T
    w, V = np.linalg.eigh(K.T @ K)
    order = np.argsort(-w)
    V, s = V[:, order], np.sqrt(np.maximum(w[order], 0.0))
    U = (K @ V) / s
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ V.T))
    R = V @ Z @ U.T
    scale = np.trace(R @ K) / var1
    t = mu2 - scale * (R @ mu1)
    return np.linalg.norm((scale * (R @ S1) + t - S2).T, axis=-1)


def synth_case(n_verts: int, B: int, seed: int):
    """Seeded meshes in millimetres, float32 [B, n_verts, 3]: labels scattered over a hand's 80 mm (never coplanar for n_verts >= 5),
    predictions a slightly turned, scaled and shifted copy plus 5 mm of noise per coordinate -- distances from about 2 to 30 mm, so
    the 20 bins up to 20 mm and the one beyond all fill."""
    rng = np.random.default_rng([seed, n_verts, B])
    gt = rng.standard_normal((B, n_verts, 3)) * 40 + rng.uniform(-200, 200, (B, 1, 3))
    a = rng.uniform(-0.08, 0.08, B)
    R = np.zeros((B, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1
    mid = gt.mean(1, keepdims=True)
    pred = (gt - mid) @ R.transpose(0, 2, 1) * rng.uniform(0.95, 1.05, (B, 1, 1)) + mid + rng.uniform(-4, 4, (B, 1, 3))
    pred = pred + rng.standard_normal(pred.shape) * 5
    return pred.astype(np.float32), gt.astype(np.float32)


def route_difference(pred, gt, unit_div=1000.0) -> float:
    """The largest relative difference, over the samples, between the aligned sums of the two float64 routes."""
    worst = 0.0
    for b in range(pred.shape[0]):
        p, g = divided(pred[b], unit_div), divided(gt[b], unit_div)
        one, two = aligned_svd(p, g).sum(), aligned_eig(p, g).sum()
        worst = max(worst, abs(one - two) / abs(one))
    return worst


def sample_values(pred, gt, unit_div=1000.0, aligned=aligned_svd):
    """One sample: (dist fp32 [n], pa_dist float64 [n]) of the divided meshes."""
    p, g = divided(pred, unit_div), divided(gt, unit_div)
    with np.errstate(invalid="ignore"):
        return distance_f32(p, g), aligned(p, g)


def accumulate(state, pred, gt, status=None, thr_min=0.0, thr_max=0.02, steps=20, unit_div=1000.0, records=None, record_base=0,
               aligned=aligned_svd):
    """Adds one step in place, sample after sample.  pred / gt [B, n, 3]; status [B] or None; records: float32 [cap, 2] or None."""
    B, n = pred.shape[:2]
    assert state.size == doubles(n, steps) and gt.shape == pred.shape == (B, n, 3)
    s = slices(state, steps)
    if state[1] == 0:
        state[2], state[3] = n, steps
    state[1] += 1
    for b in range(B):
        if status is not None and status[b] != 0:
            state[4] += 1
            if records is not None:
                records[record_base + b] = np.nan
            continue
        dist, pa = sample_values(pred[b], gt[b], unit_div, aligned)
        d64 = dist.astype(np.float64)
        state[0] += 1
        state[5] += n
        state[6] += d64.sum()
        state[7] += pa.sum()
        s["H"] += bins(dist, thr_min, thr_max, steps)
        s["PV"] += d64
        s["PVA"] += pa
        if records is not None:
            records[record_base + b] = (np.float32(d64.sum() / n), np.float32(pa.sum() / n))
    return state


def step_values(pred, gt, thr_min=0.0, thr_max=0.02, steps=20, unit_div=1000.0) -> dict:
    """What one step on its own gives: the per-step values the reference logs for `vertices / unit_div`."""
    return finish(accumulate(new_state(pred.shape[1], steps), pred, gt, None, thr_min, thr_max, steps, unit_div), thr_min, thr_max, steps)


def finish(state, thr_min=0.0, thr_max=0.02, steps=20) -> dict:
    """The epoch's mesh numbers by the reference's formulas: means in float64, the PCK curve and the trapezoid in fp32; mirrors
    handmvnet_amd.evaluation.finish_vertices."""
    s = slices(state, steps)
    thr = mo.linspace_f32(thr_min, thr_max, steps)
    pck = np.cumsum(s["H"][:steps]).astype(np.float32) / np.float32(state[5])
    dx = thr[1:] - thr[:-1]
    auc = float(np.sum(dx * (pck[1:] + pck[:-1]) * np.float32(0.5), dtype=np.float32))
    one = float(np.sum(dx, dtype=np.float32))
    return {"mpvpe": state[6] / state[5] * 1000, "pa_mpvpe": state[7] / state[5] * 1000, "pck": pck, "thr": thr, "auc": auc,
            "norm_auc": auc / one if steps > 1 else float("nan"), "vertex_err": s["PV"] / state[0] * 1000,
            "vertex_pa_err": s["PVA"] / state[0] * 1000, "samples": int(state[0]), "skipped": int(state[4])}
