"""CPU restatement (numpy, float64) of the reference's evaluation-step losses -- TEST INFRASTRUCTURE ONLY.

Follows /root/reference/src/models/handmvnet.py:279-351 (_calculate_loss, root-relative), models/losses/loss.py:4-17,
models/utils.py:123-131 (mask_joints), utils/camera.py:4-60 (reprojection), datasets/utils.py:86-143 (generate_heatmap,
batch_joints_img_to_cropped_joints) and datasets/ho3d.py:155-166 (hm_transform: ToTensor -> Resize(antialias=True), whose
separable triangle filter is aten's `_compute_indices_min_size_weights_aa` evaluated in double).  Pinned to outputs of the real
reference by tests/golden/loss_cases.npz (tests/golden/make_loss_fixture.py) in tests/test_loss_oracle.py.
"""
from __future__ import annotations

import functools
import os

import numpy as np

NJ = 21
TERMS = ("heatmap_loss", "joints_2d_loss", "joints_3d_loss", "g2d_loss", "p2d_loss", "loss")


# ---------------------------------------------------------------- portable generator (fixture <-> tests)
def hash_uniform(seed: int, n: int) -> np.ndarray:
    """n float64 values in [0, 1) from the splitmix64 counter hash of (seed, index): integer arithmetic only, so the fixture
    generator and the tests draw the same numbers on every platform and numpy version."""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def pred_heatmap_from(target: np.ndarray, seed: int) -> np.ndarray:
    """A 'predicted' heat map near `target` (fp32, same shape): what the fixture's heat-map terms were computed on."""
    u = hash_uniform(seed, target.size).reshape(target.shape)
    return (0.8 * target.astype(np.float64) + 0.05 * (u - 0.5)).astype(np.float32)


def densify(idx: np.ndarray, val: np.ndarray, shape) -> np.ndarray:
    """The fixture keeps the reference's (sparse) target maps as flat indices + fp32 values."""
    out = np.zeros(int(np.prod(shape)), np.float32)
    out[idx.astype(np.int64)] = val
    return out.reshape(shape)


# ---------------------------------------------------------------- the fixture (tests/golden/loss_cases.npz)
WEIGHT_KEYS = ("heatmap", "joints_2d", "joints_3d", "g2d", "p2d")


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_cases.npz"))


def case_names(kind: str):
    """kind "hm": the target-map cases; "loss": the loss cases."""
    return sorted({k.split(".")[1] for k in fixture().files if k.startswith(kind + ".")})


@functools.lru_cache(maxsize=None)
def map_case(name: str):
    """-> dict: S, h, w, joints [7, 21, 2], valid [7, 21] (False: the reference cannot build this map), ref [7, 21, h, w] fp32."""
    fx = fixture()
    S, h, w = (int(v) for v in fx[f"hm.{name}.shape"])
    joints = fx[f"hm.{name}.joints"]
    return dict(S=S, h=h, w=w, joints=joints, valid=fx[f"hm.{name}.valid"],
                ref=densify(fx[f"hm.{name}.idx"], fx[f"hm.{name}.val"], joints.shape[:-1] + (h, w)))


@functools.lru_cache(maxsize=None)
def loss_case(name: str):
    """-> dict of one loss case: the inputs (target / pred_hm rebuilt densely), ref32 / ref64 [6] in the order of TERMS, the
    reference's projections.  Shared and cached: callers must not write into the arrays."""
    fx, k = fixture(), f"loss.{name}."
    B, V, S, h, w, root_idx, has_mask, flag, seed = (int(v) for v in fx[k + "dims"])
    c = {n: fx[k + n] for n in ("extr", "intr", "root_joint", "gt_cam", "pred_cam", "bbox", "gt_2d", "pred_2d", "ref32", "ref64")}
    c.update(B=B, V=V, S=S, h=h, w=w, root_idx=root_idx, flag=bool(flag), mask=fx[k + "mask"] if has_mask else None)
    c["weights"] = {n: float(v) for n, v in zip(WEIGHT_KEYS, fx[k + "weights"]) if not np.isnan(v)}
    c["target"] = densify(fx[k + "tgt_idx"], fx[k + "tgt_val"], (B, V, 21, h, w))
    c["pred_hm"] = pred_heatmap_from(c["target"], seed)
    for n in ("proj32", "proj64", "proj_img32", "proj_img64", "proj_maxdiff", "proj_img_maxdiff"):
        c[n] = fx[k + n] if k + n in fx.files else None
    return c


# ---------------------------------------------------------------- target heat maps
def aa_weights64(in_size: int, out_size: int):
    """Per output index: (first input index, normalised float64 weights) of the antialiased bilinear filter."""
    scale = float(in_size) / float(out_size)
    support = scale if scale >= 1.0 else 1.0
    invscale = 1.0 / scale if scale >= 1.0 else 1.0
    res = []
    for i in range(out_size):
        center = scale * (i + 0.5)
        xmin = max(int(center - support + 0.5), 0)
        xsize = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([max(0.0, 1.0 - abs((j + xmin - center + 0.5) * invscale)) for j in range(xsize)], np.float64)
        res.append((xmin, w / w.sum()))
    return res


def gaussian_1d(p: float, size: int, sigma: int = 2) -> np.ndarray:
    """One axis of generate_heatmap on `size` zero pixels: the 6 sigma + 1 taps around trunc(p), cropped to the image."""
    g = np.zeros(size, np.float64)
    c = int(np.float32(p))   # astype(np.int32): toward zero
    for k in range(6 * sigma + 1):
        x = c - 3 * sigma + k
        if 0 <= x < size:
            g[x] = np.exp(-float((k - 3 * sigma) ** 2) / (2.0 * sigma * sigma))
    return g


def target_profile(p: float, size: int, out_size: int, sigma: int = 2, weights=None) -> np.ndarray:
    g = gaussian_1d(p, size, sigma)
    weights = weights or aa_weights64(size, out_size)
    return np.array([float(np.dot(w, g[x0:x0 + len(w)])) for x0, w in weights], np.float64)


def target_heatmaps(joints: np.ndarray, image_size: int, h: int, w: int, sigma: int = 2) -> np.ndarray:
    """joints [..., 2] (x, y) -> float64 [..., h, w]: row profile x column profile.  Whole Gaussian outside the image: zeros."""
    j = np.asarray(joints, np.float32).reshape(-1, 2)
    wx, wy = aa_weights64(image_size, w), aa_weights64(image_size, h)
    out = np.empty((j.shape[0], h, w), np.float64)
    for i, (x, y) in enumerate(j):
        out[i] = np.outer(target_profile(y, image_size, h, sigma, wy), target_profile(x, image_size, w, sigma, wx))
    return out.reshape(np.asarray(joints).shape[:-1] + (h, w))


def gaussian_in_image(p: float, size: int, sigma: int = 2) -> bool:
    """False where generate_heatmap takes its early return (utils.py:103-105), which the dataset transform cannot digest."""
    c = int(np.float32(p))
    return not (c - 3 * sigma >= size or c + 3 * sigma + 1 < 0)


# ---------------------------------------------------------------- reprojection
def project(joints_abs, root_idx: int, intrinsic, extrinsic, bbox=None) -> np.ndarray:
    """get_2d_joints_from_3d_joints (+ batch_joints_img_to_cropped_joints with its default image_size 256 when bbox is given)."""
    X = np.asarray(joints_abs, np.float64)
    K, E = np.asarray(intrinsic, np.float64), np.asarray(extrinsic, np.float64)
    B, V = K.shape[:2]
    out = np.empty((B, V, X.shape[1], 2), np.float64)
    for b in range(B):
        hom = np.concatenate([X[b], np.ones((X.shape[1], 1))], axis=1)
        world = (E[b, root_idx] @ hom.T).T
        for i in range(V):
            cam = (np.linalg.inv(E[b, i]) @ world.T).T[:, :3] * 1000
            z = cam[:, 2] + 1e-6
            out[b, i, :, 0] = cam[:, 0] * K[b, i, 0] / z + K[b, i, 2]
            out[b, i, :, 1] = cam[:, 1] * K[b, i, 1] / z + K[b, i, 3]
    if bbox is not None:
        bb = np.asarray(bbox, np.float64)
        out = out - bb[:, :, None, :2]
        out[..., 0] *= 256.0 / (bb[:, :, None, 2] - bb[:, :, None, 0])
        out[..., 1] *= 256.0 / (bb[:, :, None, 3] - bb[:, :, None, 1])
    return out


# ---------------------------------------------------------------- the loss
def losses(pred_hm, target_hm, pred_2d, gt_2d, pred_cam, gt_cam, weights: dict, mask=None, mask_invisible_joints=False,
           root_joint=None, root_idx=0, intrinsic=None, extrinsic=None, bbox=None):
    """-> (dict of the six TERMS as floats, projected [B, V, 21, 2] float64 or None)."""
    f = lambda a: np.asarray(a, np.float64)   # noqa: E731
    out = {"heatmap_loss": float(np.mean((f(pred_hm) - f(target_hm)) ** 2)) * weights["heatmap"]}
    p2, g2 = f(pred_2d), f(gt_2d)
    if mask is not None and mask_invisible_joints:
        keep = (~np.asarray(mask, bool))[..., None]
        p2m, g2m = p2 * keep, g2 * keep
    else:
        p2m, g2m = p2, g2
    out["joints_2d_loss"] = float(np.mean(np.abs(p2m - g2m))) * weights["joints_2d"]
    out["joints_3d_loss"] = float(np.mean(np.abs(f(pred_cam) - f(gt_cam)))) * weights["joints_3d"]
    out["g2d_loss"] = out["p2d_loss"] = 0.0
    proj = None
    if "g2d" in weights:
        rj = f(root_joint).reshape(-1, 1, 3) if root_joint is not None else 0.0
        proj = project(f(pred_cam) + rj, root_idx, intrinsic, extrinsic, bbox)
        out["g2d_loss"] = float(np.mean(np.abs(proj - g2))) * weights["g2d"]
        out["p2d_loss"] = float(np.mean(np.abs(proj - p2))) * weights["p2d"]
    out["loss"] = out["heatmap_loss"] + out["joints_2d_loss"] + out["joints_3d_loss"] + out["g2d_loss"] + out["p2d_loss"]
    return out, proj
