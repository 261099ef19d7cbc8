"""Shared by the triangulation tests (test_triangulation_oracle.py, test_gpu_triangulation.py): golden/triangulation_cases.npz, its
bars and the inputs of its cases."""
import os

import numpy as np

from helpers import GOLDEN

FIX = np.load(os.path.join(GOLDEN, "triangulation_cases.npz"), allow_pickle=False)
THR = float(FIX["threshold"])
PLAIN = ["plain_v2", "plain_v5", "plain_v13", "plain_v5_mm"]


def unit_of(name):
    return "mm" if name.endswith("_mm") else "m"


def term(name):
    """16 x the deviation between two LAPACK drivers on this unit's cases: what float64 itself leaves open."""
    return 16 * float(FIX[f"svd_driver_deviation/{unit_of(name)}"])


def ransac_inputs(name):
    base = "ransac_v5_k3"
    kw = dict(points=FIX[f"{base}/points"], intrinsic=FIX[f"{base}/intr"], extrinsic=FIX[f"{base}/ext"], kind=1,
              subsets=FIX[f"{base}/table"], threshold=THR)
    if name == "masked_ransac":
        kw.update(present=FIX["masked/present"], joint_mask=FIX["masked/joint_mask"])
    return kw


def scattered(pts):
    """Every view's points moved by 400 px in a direction of its own: no three views agree on a point within a pixel."""
    ang = 2.4 * np.arange(pts.shape[1])
    return (pts + 400 * np.stack([np.cos(ang), np.sin(ang)], axis=-1)[None, :, None, :]).astype(np.float32)
