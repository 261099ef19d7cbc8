"""Heat-map confidences on the device (hmv_op_heatmap_peaks, hmv_op_confidence_select; include/handmv.h "heat-map confidences").

The peak of a joint's heat map says how sure the head was of that joint in that view.  ``heatmap_peaks`` reads it off the NCHW map
every forward returns, one launch, nothing copied to the host:

    out = model(x, bbox, cam_params)
    conf, index, preds = heatmap_peaks(out["heatmap"])             # [b, v, 21], [b, v, 21], [b, v, 21, 2]
    mask = confidence_mask(conf, threshold=0.5)                    # [b, v, 21] uint8, 1 = leave the view out for this joint
    X, status = triangulate(out["joints_crop_img"], K, E, bbox=bbox, image_size=256, joint_mask=mask)

``triangulate(..., confidences=conf)`` and ``HandMvNet.forward_absolute(..., confidence=0.5)`` do the last two steps, or all three.

The selection is the reference's triangulate_dlt (utils/triangulation.py:227-236): per joint, the views whose confidence exceeds a
threshold that is lowered by `step` until two views remain or the threshold reaches zero.  Two properties of the reference are kept
to the bit: the threshold is a double lowered by repeated subtraction and compared in fp32, and with ``carry=True`` it is never reset,
so every later joint of a sample starts from what an earlier one lowered it to.  ``carry=False`` restarts every joint.

One deliberate difference from the reference: where the threshold reaches zero with fewer than two views, the reference triangulates
from one camera or raises; here ``selected`` says so and the triangulation reports status 2 and NaN for that joint.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib

MAX_VIEWS, MAX_POINTS, MAX_LEVELS = 16, 64, 1024   # include/handmv.h: hmv_op_confidence_select
MAX_MAPS, MAX_PIXELS = 1 << 24, 1 << 20            # hmv_op_heatmap_peaks


def _stream_call(name: str, dev: torch.device, args) -> None:
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(getattr(_lib.load(), name)(idx, ctypes.byref(args), stream))


def heatmap_peaks(heatmap):
    """The maximum of every score map and where it lies (one launch): `heatmap` is a float32 [..., J, h, w] device tensor (a view
    that is not contiguous is made contiguous; any other dtype is refused). Returns maxval [..., J] fp32, index [..., J] int32 (flat y * w + x, 0-based) and preds [..., J, 2] fp32,
    the reference's 1-based (x, y) zeroed where maxval <= 0 (models/utils.py:73-81).  The rule is torch.max's: the largest value, the
    lowest index among equals, and a NaN beats every number -- a NaN in maxval reports a NaN in the map."""
    if not isinstance(heatmap, torch.Tensor) or heatmap.dim() < 3:
        raise ValueError("heatmap must be a [..., J, h, w] tensor")
    lead = tuple(int(s) for s in heatmap.shape[:-3])
    J, h, w = (int(s) for s in heatmap.shape[-3:])
    N = 1
    for s in lead:
        N *= s
    if N < 1 or J < 1 or h < 1 or w < 1:
        raise ValueError(f"heatmap [..., J, h, w] must hold at least one map, got {list(heatmap.shape)}")
    if N * J > MAX_MAPS or h * w > MAX_PIXELS:
        raise ValueError(f"heatmap may hold at most 2^24 maps of at most 2^20 pixels, got {list(heatmap.shape)}")
    if heatmap.dtype != torch.float32:   # every forward returns fp32 maps in every arithmetic mode; a conversion here would be a hidden copy
        raise ValueError(f"heatmap must be float32, got {heatmap.dtype}")
    if not heatmap.is_cuda:
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: heatmap must be a CUDA(HIP) tensor (no CPU fallback)")
    dev = heatmap.device
    hm = heatmap.detach().contiguous()   # (a view that is not contiguous is the one thing that is copied)
    maxval = torch.empty(lead + (J,), device=dev, dtype=torch.float32)
    index = torch.empty(lead + (J,), device=dev, dtype=torch.int32)
    preds = torch.empty(lead + (J, 2), device=dev, dtype=torch.float32)
    a = _lib.HmvPeaksArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvPeaksArgs)
    a.N, a.J, a.h, a.w = N, J, h, w
    a.heatmap, a.maxval, a.index, a.preds = hm.data_ptr(), maxval.data_ptr(), index.data_ptr(), preds.data_ptr()
    _stream_call("hmv_op_heatmap_peaks", dev, a)
    del hm   # allocated on the stream the kernel runs on: the caching allocator reuses it in stream order
    return maxval, index, preds


def heatmaps_to_coordinates(scores):
    """models/utils.py:65-82 on the device, same signature and return: scores [N, J, h, w] -> preds [N, J, 2] fp32, the 1-based
    (x, y) of every map's maximum, zeros where the maximum is not > 0."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 4:
        raise ValueError("Score maps should be 4-dim")
    return heatmap_peaks(scores)[2]


def check_schedule(threshold, step):
    """(threshold, step) as floats, refused as hmv_op_confidence_select refuses them."""
    try:
        threshold, step = float(threshold), float(step)
    except (TypeError, ValueError):
        raise ValueError("threshold and step must be numbers") from None
    if not math.isfinite(threshold) or not math.isfinite(step):
        raise ValueError("threshold and step must be finite")
    if step <= 0:
        raise ValueError("step must be > 0")
    if threshold / step > MAX_LEVELS:
        raise ValueError(f"threshold / step must not exceed {MAX_LEVELS} levels")
    return threshold, step


def confidence_mask(conf, threshold: float = 0.5, step: float = 0.05, carry: bool = False, present=None, joint_mask=None,
                    return_details: bool = False):
    """Which views to leave out for which joint (one launch): `conf` float32 [B, V, J] device tensor (heatmap_peaks' maxval), V <= 16,
    J <= 64.  Per joint the views with conf > threshold are kept; while fewer than two are, the threshold is lowered by `step`,
    down to the first level <= 0.  carry=True: the threshold is lowered per SAMPLE, never reset between its joints -- what the
    reference's triangulate_dlt does; carry=False: every joint starts from `threshold`.  present [B, V] (zero = absent) and
    joint_mask [B, V, J] (non-zero = do not use) as in triangulate(): such a view is neither kept nor counted.  A NaN confidence
    is never kept.
    Returns mask [B, V, J] uint8, 1 = leave the view out for this joint -- triangulate()'s joint_mask, the caller's already in it.
    return_details=True: a dict with `mask`, `level` [B, J] fp32 (the threshold that decided), `lowered` [B, J] int32 (decrements
    spent on the joint) and `selected` [B, J] int32 (views kept; below two, the joint cannot be triangulated)."""
    if not isinstance(conf, torch.Tensor) or conf.dim() != 3:
        raise ValueError("conf must be a [B, V, J] tensor")
    B, V, J = (int(s) for s in conf.shape)
    if B < 1 or not 1 <= V <= MAX_VIEWS or not 1 <= J <= MAX_POINTS:
        raise ValueError(f"conf [B, V, J] needs B >= 1, 1 <= V <= {MAX_VIEWS}, 1 <= J <= {MAX_POINTS}; got {list(conf.shape)}")
    threshold, step = check_schedule(threshold, step)
    for name, t, shape in (("present", present, (B, V)), ("joint_mask", joint_mask, (B, V, J))):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape):
            raise ValueError(f"{name} must be a {list(shape)} tensor")
    if conf.dtype != torch.float32:   # the comparison is made in fp32 on the confidences as they are: no conversion here
        raise ValueError(f"conf must be float32, got {conf.dtype}")
    if not conf.is_cuda:
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: conf must be a CUDA(HIP) tensor (no CPU fallback)")
    dev = conf.device
    cf = conf.detach().contiguous()
    pr = None if present is None else (present.detach().to(dev) != 0).to(torch.uint8).contiguous()
    jm = None if joint_mask is None else (joint_mask.detach().to(dev) != 0).to(torch.uint8).contiguous()
    mask = torch.empty((B, V, J), device=dev, dtype=torch.uint8)
    level = lowered = selected = None
    a = _lib.HmvConfidenceSelectArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvConfidenceSelectArgs)
    a.B, a.V, a.J, a.carry, a.threshold, a.step = B, V, J, int(bool(carry)), threshold, step
    a.conf, a.mask_out = cf.data_ptr(), mask.data_ptr()
    if pr is not None:
        a.present = pr.data_ptr()
    if jm is not None:
        a.joint_mask = jm.data_ptr()
    if return_details:
        level = torch.empty((B, J), device=dev, dtype=torch.float32)
        lowered = torch.empty((B, J), device=dev, dtype=torch.int32)
        selected = torch.empty((B, J), device=dev, dtype=torch.int32)
        a.level, a.lowered, a.selected = level.data_ptr(), lowered.data_ptr(), selected.data_ptr()
    _stream_call("hmv_op_confidence_select", dev, a)
    del cf, pr, jm
    if return_details:
        return {"mask": mask, "level": level, "lowered": lowered, "selected": selected}
    return mask
