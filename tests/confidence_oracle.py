"""numpy restatement of the two heat-map confidence rules (include/handmv.h "heat-map confidences"), for the tests.

peaks():  torch.max(scores.view(N, J, -1), 2) and the reference's heatmaps_to_coordinates (models/utils.py:65-82) -- the largest value,
          among equal values the lowest flat index (+0 == -0), a NaN beats every number and the first NaN wins.
select(): the camera selection of the reference's triangulate_dlt (utils/triangulation.py:227-236), with the threshold a Python float
          (a double) lowered by repeated subtraction, compared with the fp32 confidences in fp32.
"""
import numpy as np


def peaks(scores):
    """scores [..., J, h, w] fp32 -> maxval [..., J] fp32, index [..., J] int32, preds [..., J, 2] fp32."""
    scores = np.asarray(scores, dtype=np.float32)
    h, w = scores.shape[-2:]
    flat = scores.reshape(-1, h * w)
    maxval = np.empty(len(flat), dtype=np.float32)
    index = np.empty(len(flat), dtype=np.int32)
    for m, row in enumerate(flat):
        nan = np.flatnonzero(np.isnan(row))
        # np.argmax returns the first of equal maxima; it treats -0 == +0 as equal, as the comparison does
        index[m] = nan[0] if len(nan) else int(np.argmax(row))
        maxval[m] = row[index[m]]
    x, y = (index % w + 1).astype(np.float32), (index // w + 1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        on = (maxval > 0).astype(np.float32)
    preds = np.stack([x * on, y * on], axis=-1)
    lead = scores.shape[:-2]
    return maxval.reshape(lead), index.reshape(lead), preds.reshape(lead + (2,))


def levels(threshold=0.5, step=0.05):
    """The thresholds the loop can visit from `threshold`: down to and including the first one <= 0."""
    out, t = [float(threshold)], float(threshold)
    while t > 0:
        t -= float(step)
        out.append(t)
    return out


def select(conf, threshold=0.5, step=0.05, carry=False, present=None, joint_mask=None):
    """conf [B, V, J] fp32 -> dict(mask [B, V, J] uint8 (1 = left out), level [B, J] fp32, lowered, selected [B, J] int32)."""
    conf = np.asarray(conf, dtype=np.float32)
    B, V, J = conf.shape
    usable = np.ones((B, V, J), dtype=bool)
    if present is not None:
        usable &= np.asarray(present).reshape(B, V, 1) != 0
    if joint_mask is not None:
        usable &= np.asarray(joint_mask).reshape(B, V, J) == 0
    mask = np.ones((B, V, J), dtype=np.uint8)
    level = np.zeros((B, J), dtype=np.float32)
    lowered = np.zeros((B, J), dtype=np.int32)
    selected = np.zeros((B, J), dtype=np.int32)
    for b in range(B):
        t = float(threshold)
        for j in range(J):
            if not carry:
                t = float(threshold)
            while True:
                with np.errstate(invalid="ignore"):
                    sel = usable[b, :, j] & (conf[b, :, j] > np.float32(t))
                if t <= 0:
                    break
                if sel.sum() <= 1:
                    t -= float(step)
                    lowered[b, j] += 1
                else:
                    break
            mask[b, :, j] = ~sel
            level[b, j], selected[b, j] = np.float32(t), sel.sum()
    return {"mask": mask, "level": level, "lowered": lowered, "selected": selected}
