"""Generates tests/golden/track_cases.npz: next crop windows from the REAL reference functions,
    batch_cropped_joints_to_joints_img  (datasets/utils.py:146-162; torch fp32 tensors, as handmvnet.py:237 calls it)
    points2d_to_bbox                    (datasets/utils.py:5-27)
on hand-built edge cases and seeded random slots.  Per case: joints [n, 21, 2] fp32 (crop pixels), boxes [n, 4] int32, size, margin,
square, and the expected joints_img [n, 21, 2] fp32 and out [n, 4] int32.

    python tests/golden/make_track_fixture.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")
from datasets.utils import batch_cropped_joints_to_joints_img, points2d_to_bbox  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RNG = np.random.default_rng(20251)


def hand(xlo, xhi, ylo, yhi):
    """21 joints whose extremes are exactly (xlo, xhi) x (ylo, yhi): two corner joints, the rest seeded inside."""
    p = np.stack([RNG.uniform(xlo, xhi, 21), RNG.uniform(ylo, yhi, 21)], axis=-1)
    p[3], p[17] = (xlo, yhi), (xhi, ylo)
    return p.astype(np.float32)


def reference(joints, boxes, size, margin, square):
    img = batch_cropped_joints_to_joints_img(torch.from_numpy(joints), torch.from_numpy(boxes.astype(np.float32)), size).numpy()
    out = np.stack([points2d_to_bbox(p, margin, square) for p in img]).astype(np.int64)
    return img, out


W64 = [100, 50, 164, 114]        # a 64 px window at S = 64: scale exactly 1, X = u + 100, Y = v + 50
CASES = {   # name: (joints [n, 21, 2], boxes [n, 4], image_size, margin, square, check(w, h) on the truncated extents or None)
    "h_gt_w_even":  ([hand(10.3, 30.7, 5.2, 41.9)], [W64], 64, 0, True, lambda w, h: h > w and (h - w) % 2 == 0),
    "h_gt_w_odd":   ([hand(10.3, 30.7, 5.2, 40.9)], [W64], 64, 0, True, lambda w, h: h > w and (h - w) % 2 == 1),
    "w_gt_h_even":  ([hand(5.2, 41.9, 10.3, 30.7)], [W64], 64, 0, True, lambda w, h: w > h and (w - h) % 2 == 0),
    "w_gt_h_odd":   ([hand(5.2, 40.9, 10.3, 30.7)], [W64], 64, 20, True, lambda w, h: w > h and (w - h) % 2 == 1),
    "h_eq_w":       ([hand(10.3, 30.7, 5.2, 25.9)], [W64], 64, 0, True, lambda w, h: w == h),
    "square_false": ([hand(10.3, 30.7, 5.2, 40.9), hand(5.2, 40.9, 10.3, 30.7)], [W64, W64], 64, 20, False, lambda w, h: w != h),
    # frame coordinates -1.5 / -0.5 at the low edge: int() gives -1 / 0 where floor would give -2 / -1
    "negative_trunc": ([hand(38.5, 60.25, 29.5, 47.75), hand(39.5, 55.5, 28.5, 50.0)], [[-40, -30, 24, 34]] * 2, 64, 0, True, None),
    # joints that land exactly on integers: whole crop pixels at scale 1, halves at scale 2, multiples of 32 at scales 200 / 64 and 100 / 64
    "on_integers":  ([np.round(hand(3, 60, 7, 52)), np.round(hand(2, 61, 4, 40) * 2) / 2, np.round(hand(0, 224, 32, 192) / 32) * 32],
                     [W64, [10, 20, 138, 148], [30, 40, 230, 140]], 64, 0, True, None),
    "non_square_window": ([hand(20, 230, 15, 250), hand(-30.5, 280.25, 100, 140)], [[30, 40, 230, 140], [17, 3, 44, 92]], 256, 0, True, None),
    "empty_window": ([hand(10, 50, 10, 50), hand(0, 63, 0, 63), hand(5, 20, 5, 60)], [[50, 60, 50, 90], [80, 70, 60, 50], [7, 9, 7, 9]], 64, 20, True, None),
    # windows partly outside a 480 x 640 frame, on every side
    "outside_frame": ([hand(40, 200, 30, 220), hand(60, 250, 20, 180), hand(10, 240, 10, 240)],
                      [[-60, -40, 140, 160], [560, 400, 760, 600], [-100, 300, 740, 620]], 256, 20, True, None),
}
CASES["on_integers_256"] = ([np.round(hand(3, 250, 7, 200)), np.round(hand(8, 248, 16, 128) / 8) * 8], [[0, 0, 256, 256], [64, 32, 96, 64]], 256, 20, True, None)


def random_case(n, size, margin, square):
    x1, y1 = RNG.integers(-100, 600, n), RNG.integers(-100, 440, n)
    bw, bh = RNG.integers(1, 400, n), RNG.integers(1, 400, n)              # square or not, down to one pixel
    boxes = np.stack([x1, y1, x1 + bw, y1 + bh], axis=-1)
    lo, hi = RNG.uniform(-0.3 * size, 0.6 * size, (2, n)), RNG.uniform(0.7 * size, 1.3 * size, (2, n))   # may leave [0, S)
    joints = np.stack([hand(lo[0, i], hi[0, i], lo[1, i], hi[1, i]) for i in range(n)])
    return joints, boxes, size, margin, square, None


CASES["random_64_m0"] = random_case(65, 64, 0, True)
CASES["random_256_m20"] = random_case(65, 256, 20, True)
CASES["random_256_rect"] = random_case(40, 256, 0, False)
CASES["random_64_m20"] = random_case(40, 64, 20, True)


def main():
    out, slots = {}, 0
    for name, (joints, boxes, size, margin, square, check) in CASES.items():
        joints = np.ascontiguousarray(np.asarray(joints, np.float32))
        boxes = np.asarray(boxes, np.int64)
        img, new = reference(joints, boxes, size, margin, square)
        # no slot of the fixture is one the device would keep (status 2): coordinates are small and windows far below 65536 px
        assert np.isfinite(img).all() and np.abs(img).max() < 1e9, name
        assert (new[:, 2] - new[:, 0] <= 65536).all() and (new[:, 3] - new[:, 1] <= 65536).all(), name
        assert np.abs(new).max() < 2 ** 31
        if check is not None:
            for p in img:
                w = int(p[:, 0].max()) - int(p[:, 0].min())
                h = int(p[:, 1].max()) - int(p[:, 1].min())
                assert check(w, h), (name, w, h)
        if name == "negative_trunc":
            assert img[0, :, 0].min() == -1.5 and img[0, :, 1].min() == -0.5 and img[1, :, 0].min() == -0.5 and img[1, :, 1].min() == -1.5
            assert int(img[0, :, 0].min()) == -1 and int(np.floor(img[0, :, 0].min())) == -2
            assert int(img[1, :, 0].min()) == 0 and int(np.floor(img[1, :, 0].min())) == -1
        if name.startswith("on_integers"):
            assert (img == np.round(img)).all(), name
        out[f"{name}.joints"], out[f"{name}.boxes"] = joints, boxes.astype(np.int32)
        out[f"{name}.size"], out[f"{name}.margin"], out[f"{name}.square"] = np.int32(size), np.int32(margin), np.int32(square)
        out[f"{name}.joints_img"], out[f"{name}.out"] = img.astype(np.float32), new.astype(np.int32)
        if name.startswith("random"):
            slots += len(boxes)
    assert slots >= 200
    path = os.path.join(HERE, "track_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", slots, "random slots")


if __name__ == "__main__":
    main()
