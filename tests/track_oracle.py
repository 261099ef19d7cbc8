"""Numpy restatement of the window-following rule of include/handmv.h ("sequences"; csrc/track.hip): the reference's
batch_cropped_joints_to_joints_img (datasets/utils.py:146-162, torch fp32 as handmvnet.py:237 calls it) followed by points2d_to_bbox
(datasets/utils.py:5-27), plus the status codes a device op needs where the reference raises.  tests/test_track_oracle.py holds it
to a fixture written by the real reference functions (tests/golden/make_track_fixture.py); the GPU tests hold the kernel to it."""
import numpy as np

MAX_WINDOW = 1 << 16          # hmv_forward_frames reads a wider window as the black view
MAX_COORD = np.float32(1e9)   # beyond it int() of a coordinate no longer fits an int32


def joints_to_frame(joints_crop_img, crop_boxes, image_size):
    """[n, 21, 2] crop-space joints in the windows [n, 4] -> frame-space joints, every fp32 operation rounded on its own, in the
    reference's order: pts *= (x2 - x1) / S; pts += x1."""
    j = np.asarray(joints_crop_img, np.float32)
    b = np.asarray(crop_boxes).astype(np.float32)
    s = np.float32(image_size)
    with np.errstate(all="ignore"):
        wq = ((b[:, 2] - b[:, 0]) / s).astype(np.float32)
        hq = ((b[:, 3] - b[:, 1]) / s).astype(np.float32)
        x = (j[:, :, 0] * wq[:, None]).astype(np.float32) + b[:, None, 0]
        y = (j[:, :, 1] * hq[:, None]).astype(np.float32) + b[:, None, 1]
    return np.stack([x, y], axis=-1).astype(np.float32)


def points_to_box(points, margin=0, square=True):
    """points2d_to_bbox on one [21, 2] set of finite points: Python ints throughout."""
    x_min, y_min = int(points[:, 0].min()), int(points[:, 1].min())   # int(): truncation toward zero
    x_max, y_max = int(points[:, 0].max()), int(points[:, 1].max())
    w, h = x_max - x_min, y_max - y_min
    if square and h != w:
        diff = abs(h - w)
        pad = diff // 2
        lead = pad if diff % 2 == 0 else pad + 1
        if h > w:
            x_min, x_max = x_min - lead, x_max + pad
        else:
            y_min, y_max = y_min - lead, y_max + pad
    return [x_min - margin, y_min - margin, x_max + margin, y_max + margin]


def next_crop_boxes(joints_crop_img, crop_boxes, image_size, margin=0, square=True, present=None):
    """-> (crop_boxes int32 [n, 4], bbox fp32 [n, 4], joints_img fp32 [n, 21, 2], status int32 [n]);
    status 0 moved, 1 absent (window kept, zero joints), 2 kept (non-finite / |coordinate| >= 1e9 / new window beyond 65536 px)."""
    boxes = np.asarray(crop_boxes).astype(np.int32)
    n = boxes.shape[0]
    img = joints_to_frame(joints_crop_img, boxes, image_size)
    out = boxes.copy()
    status = np.zeros(n, np.int32)
    for i in range(n):
        if present is not None and not present[i]:
            status[i] = 1
            img[i] = 0
            continue
        with np.errstate(invalid="ignore"):
            ok = bool((np.abs(img[i]) < MAX_COORD).all())   # False for NaN and inf as well
        box = points_to_box(img[i], margin, square) if ok else None
        if box is None or box[2] - box[0] > MAX_WINDOW or box[3] - box[1] > MAX_WINDOW:
            status[i] = 2
            continue
        out[i] = box
    return out, out.astype(np.float32), img, status
