"""Generates tests/golden/loss_cases.npz by running the REAL reference functions behind HandMvNet._calculate_loss
(/root/reference/src/models/handmvnet.py:279-351) on seeded inputs: models.losses.loss.PoseLoss, models.utils.mask_joints,
utils.camera.get_2d_joints_from_3d_joints and datasets.utils.{generate_heatmap, batch_joints_img_to_cropped_joints} (all import
with torch alone).  torchvision is absent, so hm_transform's ToTensor -> Resize(antialias=True) (datasets/ho3d.py:42-45) is spelled
with the torch call torchvision's tensor path makes, as make_frames_fixture.py does.  The glue between them is _calculate_loss's.

    python tests/golden/make_loss_fixture.py

Every term is stored twice: from fp32 inputs (the real thing) and from the same functions on float64 copies of those inputs
(default dtype float64, so that the buffers the functions allocate are float64 too).  Target maps are stored sparsely (flat index +
fp32 value); predicted heat maps are not stored at all: loss_oracle.pred_heatmap_from rebuilds them from the targets and a seed.
Runs only where the reference is present; the fixture is data.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/src")
from datasets.utils import batch_joints_img_to_cropped_joints, generate_heatmap  # noqa: E402
from models.losses.loss import PoseLoss  # noqa: E402
from models.utils import mask_joints  # noqa: E402
from utils.camera import get_2d_joints_from_3d_joints  # noqa: E402

import loss_oracle as lo  # noqa: E402

FULL = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}     # every release YAML
THREE = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0}


def ref_heatmap(pt, S, h, w):
    """ho3d.py:160-162 for one joint: float64 zeros -> generate_heatmap(sigma=2) -> ToTensor -> Resize(antialias=True); fp32 (ho3d.py:166)."""
    hm = generate_heatmap(np.zeros((S, S)), np.asarray(pt), sigma=2)
    t = torch.from_numpy(hm)[None, None]
    return F.interpolate(t, size=(h, w), mode="bilinear", antialias=True, align_corners=False)[0, 0].to(torch.float32).numpy()


def ref_targets(joints, S, h, w):
    """-> (dense fp32 [..., h, w], valid [...]): joints whose Gaussian misses the image make the reference fail; they stay zero."""
    flat = joints.reshape(-1, 2)
    out = np.zeros((flat.shape[0], h, w), np.float32)
    valid = np.array([lo.gaussian_in_image(x, S) and lo.gaussian_in_image(y, S) for x, y in flat])
    for i, pt in enumerate(flat):
        if valid[i]:
            out[i] = ref_heatmap(pt, S, h, w)
    return out.reshape(joints.shape[:-1] + (h, w)), valid.reshape(joints.shape[:-1])


def sparse(dense):
    flat = dense.reshape(-1)
    idx = np.flatnonzero(flat)
    return idx.astype(np.uint32), flat[idx]


# ---------------------------------------------------------------- target-map cases
MAP_CASES = {"s256_32": (256, 32, 32), "s128_16": (128, 16, 16), "s100_9x13": (100, 9, 13), "s96_12x20": (96, 12, 20)}


def map_positions(rng, S):
    edge = [-7.5, -6.2, -0.5, 0.0, 127.5, S - 0.1, S + 5.9, S + 6.1, -8.3]
    pts = [(x, y) for x in edge for y in edge]
    pts += [tuple(p) for p in rng.uniform(-12, S + 12, size=(66, 2))]      # 81 + 66 = 147 = 7 frames of 21
    return np.array(pts, np.float32).reshape(7, 21, 2)


# ---------------------------------------------------------------- loss cases
def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    """Camera-to-world 4x4 of a camera at `pos` whose +z axis points at `target`."""
    z = target - pos
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, 0], E[:3, 1], E[:3, 2], E[:3, 3] = x, y, z, pos
    return E


def make_inputs(rng, B, V, S, root_idx, shear_view=None):
    """Cameras on a ring 0.5-1.1 m from the hand, looking at it (every depth positive); everything fp32."""
    extr = np.empty((B, V, 4, 4))
    intr = np.empty((B, V, 4))
    world = np.empty((B, 21, 3))
    for b in range(B):
        hand = rng.uniform(-0.05, 0.05, 3)
        world[b] = hand + rng.standard_normal((21, 3)) * 0.04
        for i in range(V):
            ang = 2 * np.pi * (i + rng.uniform(-0.2, 0.2)) / max(V, 3)
            r = rng.uniform(0.5, 1.1)
            pos = hand + np.array([r * np.cos(ang), r * np.sin(ang), rng.uniform(-0.25, 0.25)])
            extr[b, i] = look_at(pos, hand + rng.uniform(-0.02, 0.02, 3))
            if shear_view is not None and i == shear_view:   # scaled, sheared, still invertible: only a GENERAL inverse undoes it
                A = np.eye(4)
                A[:3, :3] = np.diag([1.15, 0.9, 1.05]) + np.array([[0, 0.12, -0.07], [0.05, 0, 0.1], [-0.08, 0.04, 0]])
                A[3, :3] = 0.0
                extr[b, i] = extr[b, i] @ A
            intr[b, i] = [rng.uniform(570, 630), rng.uniform(570, 630), rng.uniform(300, 340), rng.uniform(220, 260)]
    extr, intr = extr.astype(np.float32), intr.astype(np.float32)
    abs_root = np.stack([(np.linalg.inv(extr[b, root_idx].astype(np.float64)) @ np.c_[world[b], np.ones(21)].T).T[:, :3] for b in range(B)])
    root_joint = abs_root[:, :1].astype(np.float32)                                   # [B, 1, 3] metres
    gt_cam = (abs_root - abs_root[:, :1]).astype(np.float32)
    pred_cam = (gt_cam + rng.standard_normal(gt_cam.shape) * 0.005).astype(np.float32)
    img = lo.project(gt_cam.astype(np.float64) + root_joint, root_idx, intr, extr)    # image pixels of the labels
    c = img.mean(axis=2)
    side = np.maximum(1.5 * (img.max(axis=2) - img.min(axis=2)).max(axis=-1), 60.0) * rng.uniform(0.9, 1.2, (B, V))
    bbox = np.concatenate([c - side[..., None] / 2, c + side[..., None] / 2], axis=-1).astype(np.float32)
    gt_2d = ((img - bbox[:, :, None, :2]) * (S / (bbox[:, :, None, 2:] - bbox[:, :, None, :2]))).astype(np.float32)
    gt_2d = np.clip(gt_2d, -5.0, S + 5.0).astype(np.float32)                          # every Gaussian touches the image
    pred_2d = (gt_2d + rng.standard_normal(gt_2d.shape) * 2.0).astype(np.float32)
    mask = rng.random((B, V, 21)) < 0.25
    return dict(extr=extr, intr=intr, root_joint=root_joint, gt_cam=gt_cam, pred_cam=pred_cam, bbox=bbox, gt_2d=gt_2d,
                pred_2d=pred_2d, mask=mask)


def ref_terms(d, pred_hm, tgt_hm, weights, num_views, root_idx, use_mask, flag, dtype):
    """_calculate_loss (handmvnet.py:279-351, root_relative) with the real component functions, on `dtype` copies of the inputs."""
    torch.set_default_dtype(dtype)
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)   # noqa: E731
        out = {"heatmap": t(pred_hm), "joints_crop_img": t(d["pred_2d"]), "joints_cam": t(d["pred_cam"])}
        inputs = {"heatmap": t(tgt_hm), "joints_crop_img": t(d["gt_2d"]), "joints_cam": t(d["gt_cam"]), "root_joint": t(d["root_joint"]),
                  "bboxes": t(d["bbox"]), "root_idx": [root_idx]}
        cam_params = {"intrinsic": t(d["intr"]), "extrinsic": t(d["extr"])}
        if use_mask:
            inputs["joints_img_mask"] = torch.from_numpy(d["mask"])
        losses = {}
        losses["heatmap_loss"] = PoseLoss.mse_loss(preds=out["heatmap"], labels=inputs["heatmap"], weight=weights["heatmap"])
        if "joints_img_mask" in inputs:
            m = inputs["joints_img_mask"]
            p2 = mask_joints(out["joints_crop_img"], m) if flag else out["joints_crop_img"]
            g2 = mask_joints(inputs["joints_crop_img"], m) if flag else inputs["joints_crop_img"]
        else:
            p2, g2 = out["joints_crop_img"], inputs["joints_crop_img"]
        losses["joints_2d_loss"] = PoseLoss.l1_loss(preds=p2, labels=g2, weight=weights["joints_2d"])
        losses["joints_3d_loss"] = PoseLoss.l1_loss(preds=out["joints_cam"], labels=inputs["joints_cam"], weight=weights["joints_3d"])
        losses["root_3d_loss"] = 0.
        losses["g2d_loss"] = 0.
        losses["p2d_loss"] = 0.
        proj = proj_img = None
        if "g2d" in weights:
            proj_img = get_2d_joints_from_3d_joints(out["joints_cam"] + inputs["root_joint"], inputs["root_idx"][0],
                                                    cam_params["intrinsic"], cam_params["extrinsic"])
            proj = batch_joints_img_to_cropped_joints(proj_img.view(-1, 21, 2), inputs["bboxes"].view(-1, 4)).view(-1, num_views, 21, 2)
            losses["g2d_loss"] = PoseLoss.l1_loss(preds=proj, labels=inputs["joints_crop_img"], weight=weights["g2d"])
            losses["p2d_loss"] = PoseLoss.l1_loss(preds=proj, labels=out["joints_crop_img"], weight=weights["p2d"])
        losses["loss"] = sum(losses.values())
        assert proj is None or proj.dtype == dtype
        terms = np.array([float(losses[k]) for k in lo.TERMS], np.float64)
        return terms, (proj.numpy() if proj is not None else None), (proj_img.numpy() if proj_img is not None else None)
    finally:
        torch.set_default_dtype(torch.float32)


LOSS_CASES = {   # name: B, V, S, h, w, root_idx, weights, mask present, flag, sheared view, seed
    "i_flag_on":   (2, 3, 256, 32, 32, 2, FULL, True, True, None, 101),      # mask present, flag on; root_idx = 2
    "i_flag_off":  (2, 3, 256, 32, 32, 2, FULL, True, False, None, 101),     # same inputs, flag off
    "ii_q256":     (1, 1, 128, 16, 16, 0, FULL, False, False, None, 102),    # 128-pixel config, crop mapping still x 256
    "iii_9x13":    (2, 4, 100, 9, 13, 1, FULL, True, True, None, 103),       # odd frame length 2457: unaligned map starts
    "iv_12x20":    (1, 2, 96, 12, 20, 0, FULL, False, False, None, 104),     # scales 8 and 4.8
    "v_three":     (2, 2, 128, 16, 16, 0, THREE, False, False, None, 105),   # no g2d key: three-term total
    "vi_sheared":  (2, 3, 128, 16, 16, 1, FULL, False, False, 1, 106),       # view 1 (the root camera too) is not rigid
    "vii_many":    (38, 8, 128, 16, 16, 3, FULL, True, True, None, 107),     # 304 frames: more than CUs
}


def main():
    out = {}
    rng = np.random.default_rng(20251017)
    for name, (S, h, w) in MAP_CASES.items():
        joints = map_positions(rng, S)
        dense, valid = ref_targets(joints, S, h, w)
        idx, val = sparse(dense)
        out[f"hm.{name}.joints"], out[f"hm.{name}.shape"] = joints, np.array([S, h, w], np.int32)
        out[f"hm.{name}.idx"], out[f"hm.{name}.val"], out[f"hm.{name}.valid"] = idx, val, valid
    for name, (B, V, S, h, w, root_idx, weights, use_mask, flag, shear, seed) in LOSS_CASES.items():
        d = make_inputs(np.random.default_rng(seed), B, V, S, root_idx, shear)
        tgt, valid = ref_targets(d["gt_2d"], S, h, w)
        assert valid.all()
        pred_hm = lo.pred_heatmap_from(tgt, seed)
        t32, p32, pi32 = ref_terms(d, pred_hm, tgt, weights, V, root_idx, use_mask, flag, torch.float32)
        t64, p64, pi64 = ref_terms(d, pred_hm, tgt, weights, V, root_idx, use_mask, flag, torch.float64)
        k = f"loss.{name}."
        out[k + "dims"] = np.array([B, V, S, h, w, root_idx, int(use_mask), int(flag), seed], np.int32)
        out[k + "weights"] = np.array([weights.get(n, np.nan) for n in ("heatmap", "joints_2d", "joints_3d", "g2d", "p2d")], np.float64)
        for n in ("extr", "intr", "root_joint", "gt_cam", "pred_cam", "bbox", "gt_2d", "pred_2d", "mask"):
            out[k + n] = d[n]
        out[k + "tgt_idx"], out[k + "tgt_val"] = sparse(tgt)
        out[k + "ref32"], out[k + "ref64"] = t32, t64
        if p32 is not None:
            assert np.isfinite(p64).all() and np.isfinite(p32).all()
            out[k + "proj32"], out[k + "proj64"] = p32.astype(np.float32), p64.astype(np.float64)
            out[k + "proj_img32"], out[k + "proj_img64"] = pi32.astype(np.float32), pi64.astype(np.float64)
            out[k + "proj_maxdiff"] = np.float64(np.abs(p32.astype(np.float64) - p64).max())            # max |f32 - f64|, crop pixels
            out[k + "proj_img_maxdiff"] = np.float64(np.abs(pi32.astype(np.float64) - pi64).max())    # ... image pixels
        print(name, t32, t64, out.get(k + "proj_maxdiff"))
    path = os.path.join(HERE, "loss_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
