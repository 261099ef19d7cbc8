"""CPU restatement (numpy) of the occluder of the frame preparation -- TEST INFRASTRUCTURE ONLY.

The reference's OcclusionAugmentation (datasets/augment.py:102-129) zeroes one cell of a patch grid on the cropped uint8 window before
ToTensor / Resize / Normalize.  Here the occluder is a rectangle (rx1, ry1, rx2, ry2) in window pixels from the window's top-left
corner, half-open, clipped to the window (include/handmv.h); built on oracle/frames_oracle.py's crop_and_pad / resize_aa.  Pinned by
tests/golden/occlusion_cases.npz (the real class with scripted randomness, tests/golden/make_occlusion_fixture.py).
"""
from __future__ import annotations

import numpy as np

from oracle import frames_oracle as fo


def patch_rect(p: int, row: int, col: int):
    """The reference's patch (patch_size p, row, column) as a rectangle in window pixels."""
    return [col * p, row * p, (col + 1) * p, (row + 1) * p]


def clip_rect(rect, cw: int, ch: int):
    """The rectangle clipped to [0, cw] x [0, ch], or None when nothing is left of it."""
    rx1, ry1, rx2, ry2 = (int(v) for v in rect)
    rx1, rx2 = min(max(rx1, 0), cw), min(max(rx2, 0), cw)
    ry1, ry2 = min(max(ry1, 0), ch), min(max(ry2, 0), ch)
    return None if rx2 <= rx1 or ry2 <= ry1 else (rx1, ry1, rx2, ry2)


def occluded_window(frame_hwc_u8: np.ndarray, box, rect) -> np.ndarray:
    """crop_and_pad_image, then the rectangle zeroed on the window (augment.py:125-126)."""
    win = fo.crop_and_pad(frame_hwc_u8, box)
    r = clip_rect(rect, win.shape[1], win.shape[0])
    if r is not None:
        win[r[1]:r[3], r[0]:r[2]] = 0
    return win


def zero_in_frame(frame_hwc_u8: np.ndarray, box, rect) -> np.ndarray:
    """A copy of the FRAME with the frame pixels under the (clipped) rectangle zeroed: cropping it gives occluded_window()'s window, so a
    plain preparation / forward on it is the naive baseline of an occluded one."""
    out = frame_hwc_u8.copy()
    x1, y1, x2, y2 = (int(v) for v in box)
    if x2 <= x1 or y2 <= y1:
        return out
    r = clip_rect(rect, x2 - x1, y2 - y1)
    if r is not None:
        h, w = out.shape[:2]
        ax, bx = min(max(r[0] + x1, 0), w), min(max(r[2] + x1, 0), w)
        ay, by = min(max(r[1] + y1, 0), h), min(max(r[3] + y1, 0), h)
        out[ay:by, ax:bx] = 0
    return out


def prepare_view_occluded(frame_hwc_u8: np.ndarray, box, rect, size: int) -> np.ndarray:
    """One view: [3, size, size] fp32 = img_transform(OcclusionAugmentation(crop_and_pad_image(frame, box)))."""
    x1, y1, x2, y2 = (int(v) for v in box)
    if x2 <= x1 or y2 <= y1:
        return fo.prepare_view(frame_hwc_u8, box, size)
    t = occluded_window(frame_hwc_u8, box, rect).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    t = fo.resize_aa(t, size, size)
    return (t - fo.MEAN[:, None, None]) / fo.STD[:, None, None]


def prepare_batch_occluded(frames: np.ndarray, boxes: np.ndarray, rects: np.ndarray, size: int) -> np.ndarray:
    """frames [..., Hf, Wf, 3] uint8, boxes [..., 4], rects [..., 4] int -> [..., 3, size, size] fp32."""
    lead = frames.shape[:-3]
    f = frames.reshape((-1,) + frames.shape[-3:])
    b, r = boxes.reshape(-1, 4), rects.reshape(-1, 4)
    out = np.stack([prepare_view_occluded(f[i], b[i], r[i], size) for i in range(f.shape[0])])
    return out.reshape(lead + (3, size, size))


def zero_batch(frames: np.ndarray, boxes: np.ndarray, rects: np.ndarray) -> np.ndarray:
    """zero_in_frame over a batch: frames [..., Hf, Wf, 3], boxes and rects [..., 4]."""
    f = frames.reshape((-1,) + frames.shape[-3:])
    b, r = boxes.reshape(-1, 4), rects.reshape(-1, 4)
    return np.stack([zero_in_frame(f[i], b[i], r[i]) for i in range(f.shape[0])]).reshape(frames.shape)
