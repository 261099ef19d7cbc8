"""Numpy restatement of the sequence-evaluation rules of include/handmv.h ("sequence evaluation"; csrc/seq_eval.hip):
  labels_to_windows   the reference's batch_joints_img_to_cropped_joints (datasets/utils.py:124-143, torch fp32) in its own operation
                      order, plus the status / outside / visible / mask rules a device op needs where the reference divides by zero
  mka                 PoseMetrics.mka (models/metrics.py:36-49) in float64
  accumulate          one time step into the running sums and the two-step history of hmv_seq_eval_add
tests/test_seq_eval_oracle.py holds it to a fixture written by the real reference functions (tests/golden/make_seq_eval_fixture.py);
the GPU tests hold the kernels to it."""
import numpy as np

NJ, SUMS = 21, 12


def map_to_windows(joints_img, crop_boxes, image_size):
    """[n, 21, 2] frame-space joints and windows [n, 4] -> crop-space joints, every fp32 operation rounded on its own, in the order
    torch runs datasets/utils.py:133-141: pts -= (x1, y1); pts *= widths.reciprocal() * image_size (a Python scalar over a tensor)."""
    j = np.asarray(joints_img, np.float32)
    b = np.asarray(crop_boxes).astype(np.float32)
    s, one = np.float32(image_size), np.float32(1)
    with np.errstate(all="ignore"):
        rw = ((one / (b[:, 2] - b[:, 0])).astype(np.float32) * s).astype(np.float32)
        rh = ((one / (b[:, 3] - b[:, 1])).astype(np.float32) * s).astype(np.float32)
        u = ((j[:, :, 0] - b[:, None, 0]).astype(np.float32) * rw[:, None]).astype(np.float32)
        v = ((j[:, :, 1] - b[:, None, 1]).astype(np.float32) * rh[:, None]).astype(np.float32)
    return np.stack([u, v], axis=-1).astype(np.float32)


def map_to_windows_divide(joints_img, crop_boxes, image_size):
    """The same with fl(S / wf) for the scale: NOT what torch computes (the fixture generator asserts that the two differ)."""
    j = np.asarray(joints_img, np.float32)
    b = np.asarray(crop_boxes).astype(np.float32)
    s = np.float32(image_size)
    with np.errstate(all="ignore"):
        rw, rh = (s / (b[:, 2] - b[:, 0])).astype(np.float32), (s / (b[:, 3] - b[:, 1])).astype(np.float32)
        u = ((j[:, :, 0] - b[:, None, 0]).astype(np.float32) * rw[:, None]).astype(np.float32)
        v = ((j[:, :, 1] - b[:, None, 1]).astype(np.float32) * rh[:, None]).astype(np.float32)
    return np.stack([u, v], axis=-1).astype(np.float32)


def labels_to_windows(joints_img, crop_boxes, image_size, joints_mask=None, present=None):
    """-> (joints_crop fp32 [n, 21, 2], mask uint8 [n, 21], info int32 [n, 3] = status, outside, visible).
    status 0 mapped, 1 absent (present[n] == 0), 2 empty window (x2 <= x1 or y2 <= y1); 1 and 2: zero row, mask all 1, counts 0."""
    boxes = np.asarray(crop_boxes).astype(np.int64)
    n = boxes.shape[0]
    hidden = np.zeros((n, NJ), bool) if joints_mask is None else np.asarray(joints_mask).reshape(n, NJ) != 0
    status = np.zeros(n, np.int32)
    status[(boxes[:, 2] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 1])] = 2
    if present is not None:
        status[np.asarray(present).reshape(n) == 0] = 1
    crop = map_to_windows(joints_img, boxes, image_size)
    crop[status != 0] = 0
    s = np.float32(image_size)
    with np.errstate(invalid="ignore"):
        inside = ((crop >= 0) & (crop < s)).all(-1)          # False for NaN and inf
    seen = ~hidden & (status == 0)[:, None]
    info = np.stack([status, (seen & ~inside).sum(1), seen.sum(1)], axis=-1).astype(np.int32)
    mask = (hidden | (status != 0)[:, None]).astype(np.uint8)
    return crop, mask, info


def acc_norms(p0, p1, p2):
    """||(p0 + p2) - 2 p1|| over the last axis, float64 from whatever comes in, in the reference's operation order."""
    p0, p1, p2 = (np.asarray(p, np.float64) for p in (p0, p1, p2))
    return np.sqrt((((p0 + p2) - 2.0 * p1) ** 2).sum(-1))


def mka(preds):
    """[B, T, n_pts, dim] -> float64 [B]; NaN for T < 3 (the mean of an empty tensor)."""
    p = np.asarray(preds, np.float64)
    if p.shape[1] < 3:
        return np.full(p.shape[0], np.nan)
    return acc_norms(p[:, :-2], p[:, 1:-1], p[:, 2:]).reshape(p.shape[0], -1).mean(-1)


def empty_state(B):
    """(sums float64 [B, 12], history float32 [B, 2, 2, 63]): zeros are an empty evaluation."""
    return np.zeros((B, SUMS), np.float64), np.zeros((B, 2, 2, NJ * 3), np.float32)


def accumulate(sums, history, pred, gt=None, track_status=None, slot_info=None, restart=None):
    """One time step, in place.  pred / gt [B, 21, 3]; track_status [B, V]; slot_info [B, V, 3]; restart [B].  Layout of sums per lane:
    [0] steps since the restart, [1] steps, [2] acceleration rows, [3] / [4] sum of ||acc|| of predictions / labels, [5..7] slot-steps
    of tracker status 0 / 1 / 2, [8] empty windows, [9] visible, [10] outside, [11] 0.  history[b, w, k]: w = 0 predictions, 1 labels;
    k = 0 the step before the previous one, 1 the previous one."""
    B = sums.shape[0]
    for b in range(B):
        since = 1.0 if restart is not None and restart[b] else sums[b, 0] + 1.0
        full = since >= 3
        for w, cur in enumerate((pred, gt)):
            if cur is None:
                continue
            c = np.asarray(cur[b], np.float32).reshape(NJ, 3)
            if full:
                sums[b, 3 + w] += acc_norms(history[b, w, 0].reshape(NJ, 3), history[b, w, 1].reshape(NJ, 3), c).sum()
            history[b, w, 0] = history[b, w, 1]
            history[b, w, 1] = c.reshape(-1)
        sums[b, 0] = since
        sums[b, 1] += 1
        sums[b, 2] += NJ if full else 0
        if track_status is not None:
            for k in range(3):
                sums[b, 5 + k] += int((np.asarray(track_status[b]) == k).sum())
        if slot_info is not None:
            si = np.asarray(slot_info[b]).reshape(-1, 3)
            sums[b, 8] += int((si[:, 0] == 2).sum())
            sums[b, 9] += int(si[:, 2].sum())
            sums[b, 10] += int(si[:, 1].sum())
    return sums, history
