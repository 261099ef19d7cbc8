"""Generates tests/golden/breakdown_cases.npz by running the REAL reference metrics (/root/reference/src/models/metrics.py,
models/utils.py:mask_joints) on one joint column or one camera slice at a time.

    python tests/golden/make_breakdown_fixture.py

The 3D inputs are those of metrics_cases.npz (not stored again): noise_5mm, similarity, mirrored, single_pose_7steps and the first 64
poses of many_poses.  Stored per case and joint j: PoseMetrics.mpjpe on column j, PoseMetrics.mpjpe of
compute_similarity_transform(p, g) on column j (the alignment is the whole pose's), PoseMetrics.pck on column j at every threshold.
Plus a seeded 2D case (B = 4, V = 3, about 20 % of the joints masked) with its inputs: PoseMetrics.mpjpe of the mask_joints(...)
slices per camera and per (camera, joint).  Runs only in the build container; the fixture is data.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")
from models.metrics import PoseMetrics  # noqa: E402
from models.utils import mask_joints  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"noise_5mm": None, "similarity": None, "mirrored": None, "single_pose_7steps": None, "many_poses": 64}


def main():
    src = np.load(os.path.join(HERE, "metrics_cases.npz"))
    out = {}
    for name, first in CASES.items():
        p, g = torch.from_numpy(src[f"{name}.pred"][:first]), torch.from_numpy(src[f"{name}.gt"][:first])
        lo, hi, steps = src[f"{name}.range"]
        thr = torch.linspace(float(lo), float(hi), int(steps))
        aligned = PoseMetrics.compute_similarity_transform(p, g)
        out[f"{name}.poses"] = np.int64(p.shape[0])
        out[f"{name}.mpjpe"] = np.array([PoseMetrics.mpjpe(p[:, j:j + 1], g[:, j:j + 1]).item() for j in range(21)], np.float64)
        out[f"{name}.pa_mpjpe"] = np.array([PoseMetrics.mpjpe(aligned[:, j:j + 1], g[:, j:j + 1]).item() for j in range(21)], np.float64)
        out[f"{name}.pck"] = np.array([[PoseMetrics.pck(p[:, j:j + 1], g[:, j:j + 1], t.item()).item() for t in thr] for j in range(21)],
                                      np.float64)
    rng = np.random.default_rng(11)
    g2 = (rng.random((4, 3, 21, 2)) * 128).astype(np.float32)
    p2 = g2 + rng.standard_normal(g2.shape).astype(np.float32) * 2
    mask = rng.random((4, 3, 21)) < 0.2
    mp, mg = mask_joints(torch.from_numpy(p2), torch.from_numpy(mask)), mask_joints(torch.from_numpy(g2), torch.from_numpy(mask))
    out["crop2d.pred"], out["crop2d.gt"], out["crop2d.mask"] = p2, g2, mask
    out["crop2d.per_camera"] = np.array([PoseMetrics.mpjpe(mp[:, v], mg[:, v]).item() for v in range(3)], np.float64)
    out["crop2d.per_camera_joint"] = np.array([[PoseMetrics.mpjpe(mp[:, v, j], mg[:, v, j]).item() for j in range(21)] for v in range(3)],
                                              np.float64)
    out["crop2d.pooled"] = np.float64(PoseMetrics.mpjpe(mp, mg).item())
    path = os.path.join(HERE, "breakdown_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
