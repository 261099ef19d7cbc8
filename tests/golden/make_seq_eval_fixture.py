"""Generates tests/golden/seq_eval_cases.npz from the REAL reference functions:
    batch_joints_img_to_cropped_joints  (datasets/utils.py:124-143) on fp32 torch tensors, the int windows converted to fp32
    PoseMetrics.mka                     (models/metrics.py:36-49) in fp32 and in float64
Mapping cases ("map_*"): joints [n, 21, 2] fp32 (frame pixels), boxes [n, 4] int32, size, mask uint8 [n, 21] (non-zero = invisible),
the reference's out [n, 21, 2] fp32, and outside / visible int32 [n] counted from that output in plain numpy; hand-built cases also
carry hand_outside / hand_visible, typed in below from how the case was built.  Empty windows and absent slots are this project's
rule, not the reference's: they are in tests/test_seq_eval_oracle.py, not here.
MKA cases ("mka_*"): preds fp32 [B, T, 21, 3], ref64 (the reference on preds.double()), ref32 (on fp32, for information), rel.

    python tests/golden/make_seq_eval_fixture.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")
from datasets.utils import batch_joints_img_to_cropped_joints  # noqa: E402
from models.metrics import PoseMetrics  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RNG = np.random.default_rng(20252)


def inside(box, lo=0.1, hi=0.9):
    """21 frame-space joints well inside the window (between `lo` and `hi` of its extent on both axes)."""
    x1, y1, x2, y2 = box
    f = RNG.uniform(lo, hi, (21, 2))
    return np.stack([x1 + f[:, 0] * (x2 - x1), y1 + f[:, 1] * (y2 - y1)], axis=-1).astype(np.float32)


def put(joints, where):
    """joints with the entries of `where` {joint: (X, Y)} replaced."""
    for k, xy in where.items():
        joints[k] = xy
    return joints


def hidden(*joints):
    m = np.zeros(21, np.uint8)
    m[list(joints)] = 1
    return m


NONE = np.zeros(21, np.uint8)
W64 = [100, 50, 164, 114]        # 64 px at S = 64: the scale is exactly 1, u = X - 100, v = Y - 50
NEG = [-40, -30, 88, 98]         # 128 px at S = 256, negative origin: the scale is exactly 2
W192 = [10, 20, 74, 84]          # 64 px at S = 192: 1 / 64 and 3 are exact
PX = [7, -3, 8, -2]              # one pixel at S = 320: the scale is exactly 320
RECT = [30, 40, 230, 140]        # 200 x 100: neither reciprocal is exact
THIN = [17, 3, 44, 92]           # 27 x 89

# name: (joints per slot, box per slot, mask per slot, image_size, hand-counted outside per slot, hand-counted visible per slot)
HAND = {
    # exactly on 0 (inside) and exactly on S (outside), half pixels, half a pixel before the origin
    "map_edges_64": ([put(np.floor(inside(W64)) + 0.5, {0: (100, 50), 1: (164, 60), 2: (110, 114), 3: (99.5, 70), 4: (163.5, 113.5)})],
                     [W64], [NONE], 64, [3], [21]),
    # masked joints that lie outside do not count; a slot with every joint masked
    "map_masked_256": ([put(inside(NEG), {5: (-41, 0), 6: (10, 98), 7: (88, 10)}), put(inside(NEG), {0: (200, 200), 9: (-100, 5)})],
                       [NEG, NEG], [hidden(5, 6), np.ones(21, np.uint8)], 256, [1, 0], [19, 0]),
    "map_exact_192": ([put(inside(W192), {0: (10, 20), 20: (74, 84), 11: (73.5, 83.5), 12: (9.75, 50)})], [W192], [hidden(12)], 192, [1], [20]),
    "map_one_pixel_320": ([put(inside(PX), {0: (7, -3), 1: (7.5, -2.5), 2: (8, -2.5), 3: (7.5, -2), 4: (6.5, -2.5)})], [PX], [NONE], 320,
                          [3], [21]),
    # non-square windows whose reciprocals round: the cases that tell reciprocal-then-multiply from fl(S / wf)
    "map_rect_192": ([inside(RECT), put(inside(THIN), {3: (50, 40), 8: (20, 100)}), inside(THIN)], [RECT, THIN, THIN],
                     [NONE, hidden(8), NONE], 192, [0, 1, 0], [21, 20, 21]),
    "map_rect_320": ([put(inside(RECT), {1: (20, 90), 2: (100, 30), 19: (240, 150)}), inside(THIN), inside([-60, -40, 140, 59])],
                     [RECT, THIN, [-60, -40, 140, 59]], [NONE, NONE, hidden(0, 1, 2)], 320, [3, 0, 0], [21, 21, 18]),
}


def random_case(n, size, masked):
    x1, y1 = RNG.integers(-100, 600, n), RNG.integers(-100, 440, n)
    bw, bh = RNG.integers(1, 400, n), RNG.integers(1, 400, n)              # square or not, down to one pixel
    boxes = np.stack([x1, y1, x1 + bw, y1 + bh], axis=-1)
    joints = np.stack([inside(b, -0.3, 1.3) for b in boxes])              # some joints leave the window
    joints[n // 2] = inside(boxes[n // 2])                                 # and one slot certainly has none outside
    mask = (RNG.uniform(0, 1, (n, 21)) < 0.3).astype(np.uint8) if masked else np.zeros((n, 21), np.uint8)
    if masked:
        mask[3] = 1                                                        # a slot with every joint masked
    return joints, boxes, mask, size


RANDOM = {"map_random_192": random_case(65, 192, False), "map_random_320": random_case(65, 320, True),
          "map_random_256": random_case(65, 256, True)}


def reference(joints, boxes, size):
    return batch_joints_img_to_cropped_joints(torch.from_numpy(joints), torch.from_numpy(boxes.astype(np.float32)), size).numpy()


def divide_form(joints, boxes, size):
    """fl(S / wf) for the scale: the order the reference does NOT use."""
    b, s = boxes.astype(np.float32), np.float32(size)
    d = joints - b[:, None, :2]
    return np.stack([d[..., 0] * (s / (b[:, 2] - b[:, 0]))[:, None], d[..., 1] * (s / (b[:, 3] - b[:, 1]))[:, None]], -1).astype(np.float32)


def counts(out, mask, size):
    seen = mask == 0
    off = ~((out >= 0) & (out < np.float32(size))).all(-1)
    return (seen & off).sum(1).astype(np.int32), seen.sum(1).astype(np.int32)


def main():
    out, slots, differs = {}, 0, {192: 0, 320: 0}
    cases = dict(HAND)
    cases.update({k: v + (None, None) for k, v in RANDOM.items()})
    all_out, all_vis = [], []
    for name, (joints, boxes, mask, size, hand_out, hand_vis) in cases.items():
        joints = np.ascontiguousarray(np.asarray(joints, np.float32))
        boxes, mask = np.asarray(boxes, np.int64), np.ascontiguousarray(np.asarray(mask, np.uint8))
        assert joints.shape == (len(boxes), 21, 2) and mask.shape == (len(boxes), 21), name
        ref = reference(joints, boxes, size)
        assert ref.dtype == np.float32 and np.isfinite(ref).all(), name
        n_out, n_vis = counts(ref, mask, size)
        if hand_out is not None:
            assert n_out.tolist() == hand_out and n_vis.tolist() == hand_vis, (name, n_out, n_vis)
            out[f"{name}.hand_outside"], out[f"{name}.hand_visible"] = np.asarray(hand_out, np.int32), np.asarray(hand_vis, np.int32)
        else:
            slots += len(boxes)
        if size in differs:
            differs[size] += int((ref.view(np.uint32) != divide_form(joints, boxes, size).view(np.uint32)).sum())
        out[f"{name}.joints"], out[f"{name}.boxes"], out[f"{name}.mask"] = joints, boxes.astype(np.int32), mask
        out[f"{name}.size"], out[f"{name}.out"] = np.int32(size), ref
        out[f"{name}.outside"], out[f"{name}.visible"] = n_out, n_vis
        all_out.append(n_out)
        all_vis.append(n_vis)
    # the edge cases land where they were put: exactly 0, exactly S, half pixels
    e = out["map_edges_64.out"][0]
    assert e[0].tolist() == [0, 0] and e[1, 0] == 64 and e[2, 1] == 64 and e[3, 0] == -0.5 and e[4].tolist() == [63.5, 63.5]
    assert (e[5:] * 2 % 2 == 1).all()
    p = out["map_one_pixel_320.out"][0]
    assert p[0].tolist() == [0, 0] and p[1].tolist() == [160, 160] and p[2, 0] == 320 and p[3, 1] == 320 and p[4, 0] == -160
    n_out, n_vis = np.concatenate(all_out), np.concatenate(all_vis)
    assert (n_out > 0).any() and (n_out == 0).any() and (n_vis == 0).any()
    assert slots == 195
    assert differs[192] > 0 and differs[320] > 0, differs      # the fixture can tell the two operation orders apart

    g = torch.Generator().manual_seed(20252)
    for name, shape in (("mka_3x7", (3, 7, 21, 3)), ("mka_2x3", (2, 3, 21, 3)), ("mka_1x2", (1, 2, 21, 3))):
        walk = torch.cumsum(torch.randn(shape, generator=g) * 2e-3, dim=1)                 # metres: a hand that drifts and jitters
        preds = (torch.randn(shape[0], 1, 21, 3, generator=g) * 0.05 + walk).float().contiguous()
        r32, r64 = PoseMetrics.mka(preds).numpy(), PoseMetrics.mka(preds.double()).numpy()
        out[f"{name}.preds"], out[f"{name}.ref32"], out[f"{name}.ref64"] = preds.numpy(), r32, r64
        if shape[1] >= 3:
            assert np.isfinite(r64).all()
            out[f"{name}.rel"] = np.abs(r32.astype(np.float64) - r64).max() / np.abs(r64).max()
            print(name, "fp32 vs float64 reference:", out[f"{name}.rel"])
        else:
            assert np.isnan(r64).all() and np.isnan(r32).all()                               # the mean of an empty tensor
    path = os.path.join(HERE, "seq_eval_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", slots, "random slots; coordinates that differ from fl(S / wf):", differs)


if __name__ == "__main__":
    main()
