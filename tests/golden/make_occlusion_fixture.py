"""Generates tests/golden/occlusion_cases.npz: the reference's OcclusionAugmentation (datasets/augment.py:102-129) on the cropped uint8
window, in front of its frame preparation (ho3d.py:35-40, 136-149), on small seeded frames.

OcclusionAugmentation and crop_and_pad_image are the REAL reference classes.  datasets/augment.py imports cv2 and torchvision at module
level, both absent here: empty stand-in modules go into sys.modules before the import.  They are never called -- only SampleAugmentor
uses them, and it is not built.  The module's `random` is replaced by a scripted object, so that (patch_size, row, column) are the
case's own and p = 1.0 always occludes.  ToTensor / Resize(antialias=True) / Normalize are spelled with the torch calls of
make_frames_fixture.py.

Per case: frames [n, h, w, 3] uint8, boxes [n, 4], patches [n, 3] = (patch_size, row, column), rects [n, 4] = the patch as a rectangle
in window pixels (column p, row p, (column + 1) p, (row + 1) p), size, out [n, 3, size, size] fp32.  The run also checks that zeroing
the same pixels in the FRAME and cropping afterwards gives the identical uint8 window (what the GPU tests' naive baseline rests on).

    python tests/golden/make_occlusion_fixture.py
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
for _name in ("cv2", "torchvision"):
    if _name not in sys.modules:
        _m = types.ModuleType(_name)
        sys.modules[_name] = _m
if not hasattr(sys.modules["torchvision"], "transforms"):
    sys.modules["torchvision"].transforms = types.ModuleType("torchvision.transforms")
    sys.modules["torchvision.transforms"] = sys.modules["torchvision"].transforms
sys.path.insert(0, "/root/reference/src")
from datasets import augment  # noqa: E402
from datasets.utils import crop_and_pad_image  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_frames_fixture import img_transform, smooth_frame  # noqa: E402


class Scripted:
    """random.random() / random.randint(a, b) of augment.py, answering from a script; a scripted value outside [a, b] is an error."""

    def __init__(self):
        self.queue = []

    def random(self):
        return 0.0

    def randint(self, a, b):
        v = self.queue.pop(0)
        assert a <= v <= b, (a, v, b)
        return v


CASES = {   # name: (frame h, w, output size, [(box, (patch_size, row, column)), ...])
    "inside":      (120, 160, 32, [([10, 20, 90, 100], (16, 2, 3)), ([40, 0, 160, 120], (8, 0, 14))]),          # p = 8: the last column
    "two_sides":   (96, 128, 48, [([-20, -30, 50, 40], (32, 0, 0)), ([100, 60, 170, 130], (16, 3, 3))]),        # the patch partly over padding
    "non_square":  (96, 128, 40, [([5, 7, 105, 57], (16, 2, 5)), ([5, 7, 105, 57], (24, 1, 0))]),                # 50 rows, 100 columns
    "upsample":    (96, 128, 64, [([30, 10, 62, 42], (8, 1, 2)), ([30, 10, 62, 42], (5, 3, 1))]),               # 32 -> 64: taps straddle the patch edge
    "odd_scale":   (200, 200, 56, [([3, 5, 190, 192], (64, 1, 1)), ([11, 13, 84, 86], (8, 8, 8))]),             # 187 -> 56 (3.34), p = 64; 73 % 8 != 0: last valid row / column
}


def main():
    rng = np.random.default_rng(5151)
    script = Scripted()
    augment.random = script
    out = {}
    for name, (h, w, size, items) in CASES.items():
        frames = np.stack([smooth_frame(rng, h, w) for _ in items])
        res, rects = [], []
        for f, (box, (p, r, c)) in zip(frames, items):
            window = crop_and_pad_image(f, box)
            script.queue = [p, r, c]
            occluded = np.asarray(augment.OcclusionAugmentation((p, p), p=1.0)(window))
            assert not script.queue and occluded.shape == window.shape
            rect = [c * p, r * p, (c + 1) * p, (r + 1) * p]
            assert r < window.shape[0] // p and c < window.shape[1] // p
            mine = window.copy()
            mine[rect[1]:rect[3], rect[0]:rect[2]] = 0
            assert np.array_equal(mine, occluded)
            zeroed = f.copy()   # the same pixels zeroed in the frame itself, then cropped: the identical window
            x1, y1 = box[0], box[1]
            zeroed[max(rect[1] + y1, 0):max(rect[3] + y1, 0), max(rect[0] + x1, 0):max(rect[2] + x1, 0)] = 0
            assert np.array_equal(crop_and_pad_image(zeroed, box), occluded)
            assert not np.array_equal(occluded, window) or not window[rect[1]:rect[3], rect[0]:rect[2]].any()
            res.append(img_transform(occluded, size))
            rects.append(rect)
        out[f"{name}.frames"] = frames
        out[f"{name}.boxes"] = np.array([b for b, _ in items], np.int32)
        out[f"{name}.patches"] = np.array([pt for _, pt in items], np.int32)
        out[f"{name}.rects"] = np.array(rects, np.int32)
        out[f"{name}.size"] = np.int32(size)
        out[f"{name}.out"] = np.stack(res).astype(np.float32)
    path = os.path.join(HERE, "occlusion_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
