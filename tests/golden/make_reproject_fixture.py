"""Generates tests/golden/reproject_cases.npz: the windows of every camera from one 3D pose, from the REAL reference functions
    get_2d_joints_from_3d_joints   (utils/camera.py:25-44) fed float64 tensors -- its joints_2d buffer is fp32, so what it returns is
                                   "fp64, rounded once", the device's rule
    points2d_to_bbox               (datasets/utils.py:5-27) on those projections
on seeded synthetic rigs (V = 3 and 4, B = 1 .. 3, the hand 0.3 - 0.8 m in front of the frame camera, margin 0 and 4).  Which slots
move is the rule of include/handmv.h (hmv_op_reproject_crop_boxes), evaluated here on the reference's own numbers: the depth is the
z of transform_joints_between_cameras (camera.py:4-22) in float64.

Every minimum and maximum projected coordinate of a slot whose joints all lie in front of its camera is at least 1e-3 px from an
integer (asserted; a rig that misses is drawn again): a last-bit difference in fp64 cannot move an integer edge.

    python tests/golden/make_reproject_fixture.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")
from datasets.utils import points2d_to_bbox  # noqa: E402
from utils.camera import get_2d_joints_from_3d_joints, transform_joints_between_cameras  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_WINDOW, MAX_COORD = 1 << 16, 1e9


def look_at(pos, target, roll):
    """Camera-to-world matrix of a camera at `pos` whose +z axis points at `target` (x right, y down), rolled about it."""
    z = target - pos
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    R = np.stack([c * x + s * y, -s * x + c * y, z], axis=1)
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, pos
    return E


def rig(rng, B, V, frame_cam):
    """Seeded rig: per sample V cameras on an arc around a hand; -> points3d [B, 21, 3] fp32 in camera frame_cam[b], intr, ext fp32."""
    p3, intr, ext = np.zeros((B, 21, 3), np.float32), np.zeros((B, V, 4), np.float32), np.zeros((B, V, 4, 4), np.float32)
    for b in range(B):
        centre = rng.uniform(-0.05, 0.05, 3)
        hand = centre + rng.uniform(-0.08, 0.08, (21, 3))
        for c in range(V):
            ang = rng.uniform(-1.0, 1.0)
            dist = rng.uniform(0.3, 0.8)
            pos = centre + dist * np.array([np.sin(ang), rng.uniform(-0.3, 0.3), -np.cos(ang)])
            ext[b, c] = look_at(pos, centre + rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.2, 0.2))
            f = rng.uniform(500.0, 700.0)
            intr[b, c] = [f, f * rng.uniform(0.97, 1.03), 320 + rng.uniform(-20, 20), 240 + rng.uniform(-20, 20)]
        E = ext[b, frame_cam[b]].astype(np.float64)
        p3[b] = (np.linalg.inv(E) @ np.concatenate([hand, np.ones((21, 1))], axis=1).T).T[:, :3]
    return p3, intr, ext


def reference(p3, intr, ext, frame_cam):
    """The reference's projections [B, V, 21, 2] fp32 and depth terms [B, V, 21] float64 (NaN rows for a sample with a NaN
    coordinate, which the reference would only smear)."""
    B, V = intr.shape[:2]
    j2d, z = np.full((B, V, 21, 2), np.nan, np.float32), np.full((B, V, 21), np.nan)
    for b in range(B):
        if not np.isfinite(p3[b]).all():
            continue
        t = [torch.from_numpy(a[b:b + 1].astype(np.float64)) for a in (p3, intr, ext)]
        j2d[b] = get_2d_joints_from_3d_joints(t[0], int(frame_cam[b]), t[1], t[2])[0].numpy()
        for c in range(V):
            cam = transform_joints_between_cameras(t[0][0], t[2][0, int(frame_cam[b])], t[2][0, c])
            z[b, c] = cam[:, 2].numpy() * 1000 + 1e-6
    assert j2d.dtype == np.float32
    return j2d, z


def expected(j2d, z, ok, boxes_in, status_in, margin, square):
    boxes, status, source = boxes_in.copy(), status_in.copy(), np.zeros(status_in.shape, np.int32)
    for b, c in np.ndindex(*status_in.shape):
        p = j2d[b, c]
        if not ok[b] or not (z[b, c] > 0).all() or not np.isfinite(p).all() or not (np.abs(p) < MAX_COORD).all():
            continue
        box = points2d_to_bbox(p, margin, square).astype(np.int64)
        if box[2] - box[0] > MAX_WINDOW or box[3] - box[1] > MAX_WINDOW:
            continue
        boxes[b, c], source[b, c] = box, 1
        status[b, c] = 0 if status[b, c] == 2 else status[b, c]
    return boxes.astype(np.int32), status, source


def away_from_integers(j2d, z):
    """Every extreme of a slot in front of its camera at least 1e-3 px from an integer; the depths at least 1 mm from zero."""
    for b, c in np.ndindex(*z.shape[:2]):
        if not np.isfinite(z[b, c]).all():
            continue
        if (np.abs(z[b, c]) < 1.0).any():
            return False
        if (z[b, c] > 0).all():
            p = j2d[b, c].astype(np.float64)
            ext = np.array([p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max()])
            if (np.abs(ext - np.round(ext)) < 1e-3).any():
                return False
    return True


def build(seed, B, V, margin, square, frame_cam=None, edit=None):
    for attempt in range(100):
        rng = np.random.default_rng(seed * 1000 + attempt)
        fc = np.zeros(B, np.int32) if frame_cam is None else np.asarray(frame_cam, np.int32)
        p3, intr, ext = rig(rng, B, V, fc)
        x1, y1 = rng.integers(-50, 400, (B, V)), rng.integers(-50, 300, (B, V))
        boxes_in = np.stack([x1, y1, x1 + rng.integers(20, 300, (B, V)), y1 + rng.integers(20, 300, (B, V))], axis=-1).astype(np.int32)
        case = dict(points3d=p3, intr=intr, ext=ext, frame_cam=fc, boxes_in=boxes_in, status_in=np.zeros((B, V), np.int32),
                    point_status=np.zeros((B, 21), np.int32))
        if edit is not None:
            edit(case, rng)
        j2d, z = reference(case["points3d"], case["intr"], case["ext"], fc)
        if away_from_integers(j2d, z):
            break
    else:
        raise AssertionError("no rig away from the integers in 100 draws")
    finite = np.isfinite(case["points3d"]).all(axis=(1, 2))
    ps = case["point_status"]
    out = dict(case, margin=np.int32(margin), square=np.int32(square), joints_2d=j2d, depth=z)
    with np.errstate(invalid="ignore"):
        noise = rng.normal(0, 3.0, j2d.shape).astype(np.float32)
    out["joints_img"] = np.where(np.isfinite(j2d), np.clip(j2d, -1e6, 1e6) + noise, np.float32(100.0)).astype(np.float32)
    for tag, ok in (("", finite & (ps[:, 0] == 0)), ("_all", finite & (ps == 0).all(axis=1))):
        out["ok" + tag] = ok
        out["boxes" + tag], out["status" + tag], out["source" + tag] = expected(j2d, z, ok, boxes_in, case["status_in"], margin, square)
    return out


def behind(case, rng):      # camera 1 of sample 0 moves into the hand: some joints behind it, that slot falls back alone
    E0 = case["ext"][0, 0].astype(np.float64)
    world = (E0 @ np.concatenate([case["points3d"][0].astype(np.float64), np.ones((21, 1))], axis=1).T).T[:, :3]
    E = case["ext"][0, 1].astype(np.float64)
    E[:3, 3] = world.mean(axis=0) + 0.01 * E[:3, 2]
    case["ext"][0, 1] = E


def statuses(case, rng):    # sample 0: root status 1; sample 1: status-0 root, joint 9 status 2; sample 2: all fine
    case["point_status"][0, 0] = 1
    case["point_status"][1, 9] = 2


def nan_coordinate(case, rng):
    case["points3d"][1, 13, 2] = np.nan


def slot_statuses(case, rng):   # an absent view (1 in, moved, still 1) and a kept one (2 becomes 0)
    case["status_in"][0, 1] = 1
    case["status_in"][1, 2] = 2
    case["status_in"][1, 0] = 1


def huge_window(case, rng):     # a focal length of 1e6 px: the hand spans far more than 65536 px, every coordinate below 1e9
    case["intr"][0, 2, :2] = [1.0e6, 1.0e6]


CASES = {
    "plain_v3":      dict(seed=1, B=2, V=3, margin=0, square=True),
    "plain_v4_m4":   dict(seed=2, B=3, V=4, margin=4, square=True),
    "frame_cam":     dict(seed=3, B=3, V=4, margin=0, square=True, frame_cam=[2, 0, 3]),
    "square_off":    dict(seed=4, B=2, V=3, margin=4, square=False),
    "one_sample":    dict(seed=5, B=1, V=4, margin=0, square=True, frame_cam=[1]),
    "behind":        dict(seed=6, B=2, V=3, margin=0, square=True, edit=behind),
    "point_status":  dict(seed=7, B=3, V=3, margin=4, square=True, edit=statuses),
    "nan":           dict(seed=8, B=2, V=4, margin=0, square=True, edit=nan_coordinate),
    "slot_status":   dict(seed=9, B=2, V=3, margin=4, square=True, edit=slot_statuses),
    "huge_window":   dict(seed=10, B=1, V=3, margin=0, square=True, edit=huge_window),
}


def main():
    out, parities = {}, set()
    for name, spec in CASES.items():
        res = build(**spec)
        for k, v in res.items():
            out[f"{name}.{k}"] = v
        if spec["square"]:
            for b, c in zip(*np.nonzero(res["source"])):
                p = res["joints_2d"][b, c]
                w, h = int(p[:, 0].max()) - int(p[:, 0].min()), int(p[:, 1].max()) - int(p[:, 1].min())
                parities.add((h > w, abs(h - w) % 2))
        print(name, "source", res["source"].tolist(), "status", res["status"].tolist())
    assert {(True, 1), (False, 1), (True, 0), (False, 0)} <= parities, parities      # the pad + 1 side on either axis
    s = out
    assert s["plain_v3.source"].all() and s["plain_v4_m4.source"].all() and s["frame_cam.source"].all()
    assert s["behind.source"].tolist() == [[1, 0, 1], [1, 1, 1]] and (s["behind.depth"][0, 1] < 0).any()
    assert s["point_status.source"].tolist() == [[0] * 3, [1] * 3, [1] * 3] and s["point_status.source_all"].tolist() == [[0] * 3, [0] * 3, [1] * 3]
    assert s["nan.source"].tolist() == [[1] * 4, [0] * 4]
    assert s["slot_status.source"].all() and s["slot_status.status"].tolist() == [[0, 1, 0], [1, 0, 0]]
    assert s["huge_window.source"].tolist() == [[1, 1, 0]] and np.abs(s["huge_window.joints_2d"]).max() < 1e9
    p = s["huge_window.joints_2d"][0, 2]
    assert p[:, 0].max() - p[:, 0].min() > MAX_WINDOW + 16
    path = os.path.join(HERE, "reproject_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
