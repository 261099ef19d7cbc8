"""Generates tests/golden/absolute_epoch_cases.npz: seeded steps of an absolute evaluation with the REAL reference's numbers on them
(/root/reference/src/models/metrics.py: PoseMetrics.mpjpe; utils/triangulation.py:61-95: calculate_reprojection_error).

    python tests/golden/make_absolute_epoch_fixture.py

Per case the inputs of hmv_eval_absolute_add -- pred_cam, tri, status, gt_cam, gt_root, reproj, inliers -- where reproj and inliers
are calculate_reprojection_error's own outputs (float32) for the case's points `tri`, pixels and projection matrices, and `camera`
the reference's mean error per camera over the joints with status 0.  For `plain`, two cuts into steps with PoseMetrics.mpjpe per
step on joints_cam + root (the two sums made in float32 as handmvnet.py:412-413 makes them, then handed over in float64) and on the
root alone.  For `mixed`, the located / lost samples, the status counts and the inlier histogram, counted here entry by entry.
Cases: plain (B 5, V 3, all status 0), mixed (B 5, V 3: every status, a NaN root with status 2, a located sample with a status-1
joint, NaN reprojection entries, values outside the status and inlier ranges), one (B 1, V 1), wide (B 13, V 16).
Runs only in the build container; the fixture is data.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")
from models.metrics import PoseMetrics  # noqa: E402
from utils.triangulation import calculate_reprojection_error  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NJ = 21
THRESHOLD = 10.0


def rig(rng, B, V):
    """Projection matrices [B, V, 3, 4] into V cameras on an arc around the hand; camera 0 is the frame the points are in."""
    M = np.zeros((B, V, 3, 4))
    for b in range(B):
        for v in range(V):
            a = 0.0 if v == 0 else rng.uniform(-0.9, 0.9)
            R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            centre = np.array([0.0, 0.0, 0.6])
            t = centre - R @ centre + (0 if v == 0 else rng.uniform(-0.02, 0.02, 3))     # the hand stays in front of every camera
            K = np.array([[600.0 + 5 * v, 0, 320.0], [0, 600.0 + 5 * v, 240.0], [0, 0, 1.0]])
            M[b, v] = K @ np.concatenate([R, t[:, None]], 1)
    return M.astype(np.float32)


def case(seed, B, V):
    rng = np.random.default_rng(seed)
    gt_root = (rng.uniform(-0.05, 0.05, (B, 3)) + [0, 0, 0.6]).astype(np.float32)
    gt_cam = (rng.standard_normal((B, NJ, 3)) * 0.04).astype(np.float32)
    gt_cam[:, 0] = 0
    pred_cam = (gt_cam + rng.standard_normal((B, NJ, 3)) * 0.005).astype(np.float32)
    tri = (gt_cam + gt_root[:, None] + rng.standard_normal((B, NJ, 3)) * 0.003).astype(np.float32)
    M = rig(rng, B, V)
    hom = np.concatenate([gt_cam + gt_root[:, None], np.ones((B, NJ, 1), np.float32)], -1).astype(np.float64)
    proj = np.einsum("bvik,bjk->bvji", M.astype(np.float64), hom)
    px = (proj[..., :2] / proj[..., 2:3] + rng.standard_normal((B, V, NJ, 2)) * 1.0).astype(np.float32)
    return dict(pred_cam=pred_cam, tri=tri, status=np.zeros((B, NJ), np.int32), gt_cam=gt_cam, gt_root=gt_root, px=px, M=M)


def reference_reprojection(c):
    """reproj [B, V, 21] float32 and inliers [B, 21] int32 from the reference, and its mean per camera over the status-0 joints."""
    with np.errstate(invalid="ignore"):
        err, count = calculate_reprojection_error(torch.from_numpy(c["tri"]), torch.from_numpy(c["px"]), torch.from_numpy(c["M"]), THRESHOLD)
    c["reproj"], c["inliers"] = err.numpy().astype(np.float32), count.numpy().astype(np.int32)
    del c["px"], c["M"]


def camera_means(c):
    err = torch.from_numpy(c["reproj"]).double()
    good = torch.from_numpy(c["status"] == 0)
    out = []
    for v in range(err.shape[1]):
        e = err[:, v][good & torch.isfinite(err[:, v])]
        out.append(e.mean().item() if e.numel() else np.nan)
    return np.array(out, np.float64)


def step_values(c, lo, hi):
    """PoseMetrics.mpjpe of one step: the world positions (float32 sums, float64 from there) and the root alone."""
    p = torch.from_numpy(c["pred_cam"][lo:hi] + c["tri"][lo:hi, :1]).double()
    g = torch.from_numpy(c["gt_cam"][lo:hi] + c["gt_root"][lo:hi, None]).double()
    r = PoseMetrics.mpjpe(torch.from_numpy(c["tri"][lo:hi, :1]).double(), torch.from_numpy(c["gt_root"][lo:hi, None]).double())
    return PoseMetrics.mpjpe(p, g).item(), r.item()


def main():
    out = {}
    plain = case(61, 5, 3)
    reference_reprojection(plain)
    for i, cut in enumerate(((2, 3), (1, 1, 3))):
        at, w, r = 0, [], []
        for n in cut:
            a, b = step_values(plain, at, at + n)
            w.append(a)
            r.append(b)
            at += n
        out[f"plain.cut{i}"], out[f"plain.cut{i}.w_mpjpe"], out[f"plain.cut{i}.root_err"] = np.array(cut), np.array(w), np.array(r)

    mixed = case(62, 5, 3)
    st, tri = mixed["status"], mixed["tri"]
    st[1, :], tri[1, :] = 2, np.nan            # a lost sample: too few views, NaN root
    st[2, 5], tri[2, 5] = 1, 0.0               # located, one joint without an inlier: zeros, as the reference leaves it
    st[2, 9], tri[2, 9] = 3, np.inf            # located, one joint not finite
    st[3, 0], tri[3, 0] = 3, np.nan            # lost: the root is not finite; its other joints are fine
    st[4, 20] = 7                              # outside 0 .. 3: counts as 3
    st[4, 19] = -2
    tri[0, 3] = np.nan                         # status 0 with a point that is not finite: counts in S[.][0], not in T
    reference_reprojection(mixed)
    mixed["reproj"][0, 1, 7] = np.nan          # a view that was not usable for one joint
    mixed["reproj"][4, 2, :4] = np.nan
    mixed["inliers"][0, 1], mixed["inliers"][0, 2], mixed["inliers"][4, 4] = 9, -1, 1     # clamped to V, to 0
    found = [b for b in range(5) if st[b, 0] == 0 and np.isfinite(tri[b, 0]).all()]
    assert len(found) >= 3 and found == [0, 2, 4], found
    assert set(np.unique(st)) >= {0, 1, 2, 3} and np.isnan(mixed["reproj"]).any()
    counts = np.zeros((NJ, 4), np.int64)
    hist = np.zeros(4, np.int64)
    for b in range(5):
        for j in range(NJ):
            counts[j, st[b, j] if 0 <= st[b, j] <= 3 else 3] += 1
            if st[b, j] == 0:
                hist[min(max(int(mixed["inliers"][b, j]), 0), 3)] += 1
    out["mixed.located"], out["mixed.lost"], out["mixed.status_counts"], out["mixed.inlier_hist"] = np.int64(len(found)), np.int64(5 - len(found)), counts, hist

    one = case(63, 1, 1)
    reference_reprojection(one)
    wide = case(64, 13, 16)
    wide["status"][3, 4], wide["tri"][3, 4] = 1, 0.0
    wide["status"][11, 17], wide["tri"][11, 17] = 2, np.nan
    reference_reprojection(wide)

    for name, c in (("plain", plain), ("mixed", mixed), ("one", one), ("wide", wide)):
        for k, v in c.items():
            out[f"{name}.{k}"] = v
        out[f"{name}.camera"] = camera_means(c)
    path = os.path.join(HERE, "absolute_epoch_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
