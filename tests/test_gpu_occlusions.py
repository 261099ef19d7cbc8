"""Occlusion sweeps on the GPU: the occluder of the frame preparation (hmv_op_prepare_frames_occluded), HandMvNet
.forward_frames_occlusions / hmv_forward_frames_occlusions and evaluate_occlusions -- one clean per-frame pass, one occluded frame per
(variant, sample), the fusion tail per variant.

The rule that defines every number: variant o's outputs are the bits forward_frames gives when, in camera occ_view[o]'s frames, the
frame pixels under the rectangle are zeroed.  So the bars are equal bits against forward_frames / prepare_frames on zeroed copies of the
frames (occlusion_oracle.zero_batch; the fixture's generator checks that this is the reference's occluded window), plus, for the op,
the reference's fixture and the numpy oracle at the filter's own bar (5e-6 in normalised units, tests/test_gpu_frames.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import loss_oracle as lo
import occlusion_oracle as oo
from guards import Guards
from oracle import frames_oracle as fo
from views_cases import VIEWS_CASES
from views_helpers import load_views_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "occlusion_cases.npz"))
FIX_NAMES = sorted({k.split(".")[0] for k in FIX.files})
MODES = ["f32", "f32x3", "f16"]
DEV = torch.device("cuda:0")
NAME = "views_r18_v7"
OCC_KEYS = ("joints_cam", "joints_crop_img", "heatmap", "joints_crop_img_occ", "heatmap_occ")
I32 = (-2 ** 31, 2 ** 31 - 1)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared scenes are read-only arrays)


# ---------------------------------------------------------------- 1. the op: the reference's fixture and the numpy oracle
@pytest.mark.parametrize("name", FIX_NAMES)
def test_op_matches_the_reference_fixture(name):
    from handmvnet_amd.frames import prepare_frames
    got = prepare_frames(_dev(FIX[f"{name}.frames"]), _dev(FIX[f"{name}.boxes"]), int(FIX[f"{name}.size"]), occlusion=_dev(FIX[f"{name}.rects"]))
    assert tuple(got.shape) == FIX[f"{name}.out"].shape
    err = float(np.abs(got.cpu().numpy() - FIX[f"{name}.out"]).max())
    print(name, "max error", err)
    assert err < 5e-6


def _random_case(rng, n=3):
    hf, wf = int(rng.integers(8, 70)), int(rng.integers(8, 90))
    size = int(rng.choice([8, 16, 24, 32, 48]))
    frames = rng.integers(0, 256, (n, hf, wf, 3), dtype=np.uint8)
    x1, y1 = rng.integers(-30, wf + 10, n), rng.integers(-30, hf + 10, n)
    bw, bh = rng.integers(1, 120, n), rng.integers(1, 120, n)
    boxes = np.stack([x1, y1, x1 + bw, y1 + bh], axis=-1).astype(np.int32)
    # rectangles inside, partly outside and wholly outside the window
    rx, ry = rng.integers(-20, bw + 10), rng.integers(-20, bh + 10)
    rw, rh = rng.integers(0, bw + 20), rng.integers(0, bh + 20)
    rects = np.stack([rx, ry, rx + rw, ry + rh], axis=-1).astype(np.int32)
    return frames, boxes, rects, size


def test_op_matches_the_oracle_on_random_windows_and_rectangles():
    from handmvnet_amd.frames import prepare_frames
    rng = np.random.default_rng(77)
    worst = 0.0
    for _ in range(25):
        frames, boxes, rects, size = _random_case(rng)
        got = prepare_frames(_dev(frames), _dev(boxes), size, occlusion=_dev(rects)).cpu().numpy()
        err = float(np.abs(got - oo.prepare_batch_occluded(frames, boxes, rects, size)).max())
        assert err < 5e-6, (boxes.tolist(), rects.tolist(), size, err)
        worst = max(worst, err)
    print("worst", worst)


# ---------------------------------------------------------------- 2. the op: the bits of the plain preparation on zeroed frames
def test_op_has_the_bits_of_prepare_frames_on_zeroed_frames():
    from handmvnet_amd.frames import prepare_frames
    rng = np.random.default_rng(78)
    changed = hidden = 0
    for _ in range(40):
        frames, boxes, rects, size = _random_case(rng)
        zeroed = oo.zero_batch(frames, boxes, rects)
        got = prepare_frames(_dev(frames), _dev(boxes), size, occlusion=_dev(rects))
        want = prepare_frames(_dev(zeroed), _dev(boxes), size)
        assert torch.equal(got, want), (boxes.tolist(), rects.tolist(), size)
        # a window pixel that is hidden had a positive weight in some output pixel: the view changes iff a frame pixel was zeroed
        hidden += int((zeroed != frames).any())
        changed += int(not torch.equal(got, prepare_frames(_dev(frames), _dev(boxes), size)))
    assert hidden >= 10 and changed == hidden      # (a property of the seeded inputs: the rectangles do meet frame pixels)
    # the named cases, on one frame and one window that leaves the frame on two sides: 60 x 50 window, frame 48 x 64
    frame = rng.integers(1, 256, (48, 64, 3), dtype=np.uint8)
    box = [-10, 20, 50, 70]
    named = {"wholly outside": [60, 0, 90, 50], "left of the window": [-40, 5, 0, 30], "partly outside": [40, 10, 100, 90],
             "over the frame edge": [0, 10, 25, 40], "one pixel wide": [17, 0, 18, 50], "one pixel high": [0, 11, 60, 12],
             "one pixel": [33, 7, 34, 8], "empty": [20, 20, 20, 40], "inverted": [30, 30, 10, 10], "the window": [0, 0, 60, 50],
             "more than the window": [-5, -5, 500, 500]}
    n = len(named)
    frames, boxes, rects = np.stack([frame] * n), np.array([box] * n, np.int32), np.array(list(named.values()), np.int32)
    hides = [bool((z != frame).any()) for z in oo.zero_batch(frames, boxes, rects)]
    assert hides == [w not in ("wholly outside", "left of the window", "empty", "inverted") for w in named]
    for size in (16, 75):      # down- and up-sampling
        got = prepare_frames(_dev(frames), _dev(boxes), size, occlusion=_dev(rects))
        want = prepare_frames(_dev(oo.zero_batch(frames, boxes, rects)), _dev(boxes), size)
        clean = prepare_frames(_dev(frames), _dev(boxes), size)
        black = prepare_frames(_dev(frames[:1]), _dev(np.array([[5, 5, 5, 9]], np.int32)), size)      # the empty window's black view
        for i, what in enumerate(named):
            assert torch.equal(got[i], want[i]), (what, size)
            if what in ("wholly outside", "left of the window", "empty", "inverted"):
                assert torch.equal(got[i], clean[i]), (what, size)
            elif what in ("the window", "more than the window"):
                assert torch.equal(got[i], black[0]), (what, size)
            else:
                assert not torch.equal(got[i], clean[i]), (what, size)


# ---------------------------------------------------------------- 3. garbage rectangles
def test_garbage_rectangles_are_bounded_and_deterministic():
    """INT32_MIN / INT32_MAX mixes, on legal and on garbage windows, inside guard bands: every result is the one of the clipped
    rectangle, twice the same, inputs unchanged, bands intact."""
    from handmvnet_amd.frames import prepare_frames
    lo_, hi_ = I32
    rects = np.array([[lo_, lo_, hi_, hi_], [hi_, hi_, lo_, lo_], [lo_, 5, hi_, 6], [7, lo_, 8, hi_], [lo_, lo_, 0, 0], [hi_ - 1, 0, hi_, 40],
                      [lo_, lo_, lo_ + 1, hi_], [0, 0, hi_, hi_], [-1, -1, hi_, 3], [lo_, hi_, hi_, lo_], [3, 3, hi_, hi_], [lo_, lo_, 20, 20]], np.int32)
    n = len(rects)
    rng = np.random.default_rng(5)
    frames = rng.integers(1, 256, (n, 40, 56, 3), dtype=np.uint8)
    boxes = np.array([[-8, 4, 40, 52]] * n, np.int32)
    boxes[9] = [lo_, lo_, hi_, hi_]          # garbage windows under garbage rectangles: the black view
    boxes[10] = [0, 0, 2 ** 30, 2 ** 30]
    g = Guards(DEV)
    f, b, r = g.inp(_dev(frames)), g.inp(_dev(boxes)), g.inp(_dev(rects))
    out = g.out((n, 24, 24, 4))
    from handmvnet_amd import _lib
    m3, s3 = (ctypes.c_float * 3)(*fo.MEAN.tolist()), (ctypes.c_float * 3)(*fo.STD.tolist())
    runs = []
    for _ in range(2):
        out.fill_(float("nan"))
        rc = _lib.load().hmv_op_prepare_frames_occluded(0, f.data_ptr(), n, 40, 56, b.data_ptr(), r.data_ptr(), m3, s3, 24, 24, out.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        runs.append(out.clone())
    g.check()
    assert torch.equal(runs[0], runs[1]) and bool(torch.isfinite(runs[0]).all())
    got = runs[0][..., :3].permute(0, 3, 1, 2)
    assert bool((runs[0][..., 3] == 0).all())
    clipped = np.array([oo.clip_rect(q, 48, 48) or (0, 0, 0, 0) for q in rects], np.int32)
    want = prepare_frames(_dev(oo.zero_batch(frames, boxes, clipped)), _dev(boxes), 24)
    assert torch.equal(got, want)
    black = torch.from_numpy(((0 - fo.MEAN) / fo.STD)).to(DEV)[:, None, None]
    for i in (0, 7, 9, 10):
        assert torch.allclose(got[i], black.expand(3, 24, 24)), i


# ---------------------------------------------------------------- the model cases
def _build(name, mode, tp_over=None):
    from handmvnet_amd import HandMvNet
    case = load_views_case(name)
    tp, mp, dp = case["params"]
    m = HandMvNet(dict(tp, **(tp_over or {})), mp, dp)
    m.load_state_dict(case["sd"], strict=True)
    m.to("cuda").eval()
    if mode == "f16":
        m.half()
    elif mode == "f32x3":
        m.float32x3()
    return m


@functools.lru_cache(maxsize=None)
def _model(name, mode):
    return _build(name, mode)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """Seeded, slightly smoothed uint8 frames (120 x 160) with windows that may leave them, the case's intrinsics, and the variant
    list: two variants on one camera, another camera, a duplicate of the first, an empty one; different rectangles per sample."""
    spec = VIEWS_CASES[name]
    B, V = spec["B"], spec["V"]
    rng = np.random.default_rng(17 + V)
    frames = rng.integers(0, 256, (B, V, 120, 160, 3), dtype=np.uint8)
    frames = ((frames.astype(np.float32) + np.roll(frames, 1, 2) + np.roll(frames, 1, 3)) / 3).astype(np.uint8)
    side = rng.integers(50, 140, (B, V))
    x1, y1 = rng.integers(-20, 100, (B, V)), rng.integers(-20, 60, (B, V))
    boxes = np.stack([x1, y1, x1 + side, y1 + side], axis=-1).astype(np.int32)
    intr = load_views_case(name)["inputs"][2].copy()
    view = np.array([0, 0, V - 1, 0, 1], np.int32)
    rects = np.zeros((len(view), B, 4), np.int32)
    for o, c in enumerate(view):
        s = side[:, c]
        rx, ry = rng.integers(-10, s - 10), rng.integers(-10, s - 10)
        rects[o] = np.stack([rx, ry, rx + rng.integers(8, s // 2 + 8), ry + rng.integers(8, s // 2 + 8)], axis=-1)
    rects[3] = rects[0]               # a duplicate
    rects[4, :, 2] = rects[4, :, 0]   # empty rectangles: the clean result
    for a in (frames, boxes, intr, view, rects):
        a.setflags(write=False)
    return frames, boxes, intr, view, rects


def _np(out, keys=OCC_KEYS):
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in keys}


def _sweep_on(m, name, view=None, rects=None, sl=slice(None)):
    frames, boxes, intr, v0, r0 = _scene(name)
    view, rects = (v0 if view is None else view), (r0 if rects is None else rects)
    return _np(m.forward_frames_occlusions(_dev(frames[sl]), _dev(boxes[sl]), view, _dev(rects[:, sl]), {"intrinsic": _dev(intr[sl])}))


@functools.lru_cache(maxsize=None)
def _sweep(name, mode):
    out = _sweep_on(_model(name, mode), name)
    for a in out.values():
        a.setflags(write=False)
    return out


def _zeroed(name, c, rects_b):
    """The scene's frames with, in camera c, the frame pixels under sample b's rectangle zeroed."""
    frames, boxes = _scene(name)[:2]
    z = frames.copy()
    z[:, c] = oo.zero_batch(frames[:, c], boxes[:, c], rects_b)
    return z


# ---------------------------------------------------------------- 4. end to end: the bits of forward_frames on zeroed frames
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_every_variant_has_the_bits_of_forward_frames_on_zeroed_frames(name, mode):
    """Both cases carry 'crop' in pos_enc: the occluded frame's bbox and intrinsic rows are exercised."""
    m, got = _model(name, mode), _sweep(name, mode)
    frames, boxes, intr, view, rects = _scene(name)
    assert "crop" in m.cfg.pos_enc
    B, V = frames.shape[:2]
    hs = got["heatmap"].shape[-2:]
    assert got["joints_cam"].shape == (1 + len(view), B, 21, 3) and got["joints_crop_img_occ"].shape == (len(view), B, 21, 2)
    assert got["heatmap_occ"].shape == (len(view), B, 21) + hs
    cam = {"intrinsic": _dev(intr)}
    keys = ("joints_cam", "joints_crop_img", "heatmap")
    clean = _np(m.forward_frames(_dev(frames), _dev(boxes), cam), keys)
    assert np.array_equal(got["joints_cam"][0], clean["joints_cam"]), (name, mode)
    for k in ("joints_crop_img", "heatmap"):
        assert got[k].shape == clean[k].shape and np.array_equal(got[k], clean[k]), (name, mode, k)
    for o, c in enumerate(view):
        ref = _np(m.forward_frames(_dev(_zeroed(name, c, rects[o])), _dev(boxes), cam), keys)
        assert np.array_equal(got["joints_cam"][1 + o], ref["joints_cam"]), (name, mode, o, float(np.abs(got["joints_cam"][1 + o] - ref["joints_cam"]).max()))
        assert np.array_equal(got["joints_crop_img_occ"][o], ref["joints_crop_img"][:, c]), (name, mode, o)
        assert np.array_equal(got["heatmap_occ"][o], ref["heatmap"][:, c]), (name, mode, o)
    # the occluder is seen; the duplicate equals its original; empty rectangles give the clean batch
    assert not np.array_equal(got["joints_cam"][1], got["joints_cam"][0]) and not np.array_equal(got["joints_cam"][1], got["joints_cam"][2])
    assert np.array_equal(got["joints_cam"][4], got["joints_cam"][1]) and np.array_equal(got["heatmap_occ"][3], got["heatmap_occ"][0])
    assert np.array_equal(got["joints_cam"][5], got["joints_cam"][0])
    assert np.array_equal(got["joints_crop_img_occ"][4], got["joints_crop_img"][:, view[4]])
    assert np.array_equal(got["heatmap_occ"][4], got["heatmap"][:, view[4]])
    m.check_range()      # the sweep reports into the handle's range word like any forward; nothing clamps here


# ---------------------------------------------------------------- 5. reservation, order, poisoned workspace
@pytest.mark.parametrize("mode", MODES)
def test_bits_do_not_depend_on_the_reservation_or_the_order(mode):
    """Sample 0 alone under 2 V + 1 variants on a handle reserved for 1 sample (frame passes of V frames, tail passes of one virtual
    sample) and on one reserved for B (one frame pass): the same bits, and those of sample 0 in the full batch's sweep.  The full batch
    on a reservation of 2 B + 1 (tail passes that cut through a variant).  Permuted variants: permuted outputs, nothing else.  A
    poisoned workspace changes nothing."""
    frames, boxes, intr, view, rects = _scene(NAME)
    B, V = frames.shape[:2]
    want = _sweep(NAME, mode)
    reps = -(-(2 * V + 1) // len(view))
    view1, rects1 = np.tile(view, reps)[:2 * V + 1], np.tile(rects, (reps, 1, 1))[:2 * V + 1]
    one = slice(0, 1)
    outs = []
    for reserve in (1, B):
        m = _build(NAME, mode)
        m.reserve(reserve, 64, 64)
        outs.append(_sweep_on(m, NAME, view1, rects1, one))
        if reserve == 1:
            m.poison_workspace(0xFF)
            again = _sweep_on(m, NAME, view1, rects1, one)
            for k in OCC_KEYS:
                assert np.isfinite(again[k]).all() and np.array_equal(again[k], outs[0][k]), (mode, k)
            del m
    for k in OCC_KEYS:
        assert np.array_equal(outs[0][k], outs[1][k]), (mode, k)
    idx = np.arange(2 * V + 1) % len(view)
    assert np.array_equal(outs[0]["joints_cam"][1:, 0], want["joints_cam"][1 + idx, 0])
    assert np.array_equal(outs[0]["joints_cam"][0, 0], want["joints_cam"][0, 0])
    assert np.array_equal(outs[0]["heatmap_occ"][:, 0], want["heatmap_occ"][idx, 0])
    assert np.array_equal(outs[0]["joints_crop_img_occ"][:, 0], want["joints_crop_img_occ"][idx, 0])
    m.reserve(2 * B + 1, 64, 64)      # (the handle reserved for B)
    got = _sweep_on(m, NAME)
    for k in OCC_KEYS:
        assert np.array_equal(got[k], want[k]), (mode, k)
    perm = [2, 4, 0, 3, 1]
    got = _sweep_on(m, NAME, view[perm], rects[perm])
    assert np.array_equal(got["joints_cam"][1:], want["joints_cam"][1:][perm]) and np.array_equal(got["joints_cam"][0], want["joints_cam"][0])
    for k in ("joints_crop_img_occ", "heatmap_occ"):
        assert np.array_equal(got[k], want[k][perm]), (mode, k)
    m.poison_workspace(0xFF)
    again = _sweep_on(m, NAME)
    for k in OCC_KEYS:
        assert np.isfinite(again[k]).all() and np.array_equal(again[k], want[k]), (mode, k)
    del m


# ---------------------------------------------------------------- 6. launch arithmetic
def test_the_backbone_runs_twice_not_once_per_variant():
    """views_r18_v7 on a fresh handle (reservation B): a frame pass holds B V frames = 7 variants, so all occluded frames of 1, 2 and
    5 variants go through the backbone in ONE pass, and a tail pass holds one variant.  The launch count is (clean stage) + (occluded
    stage) + (1 + n) tails: n(5) - n(1) == 4 (n(2) - n(1)), and a variant costs less than half of a forward's launches."""
    m = _build(NAME, "f32")
    frames, boxes, intr, view, rects = _scene(NAME)
    cam = {"intrinsic": _dev(intr)}
    n = {}
    for k in (1, 2, 5):
        m.forward_frames_occlusions(_dev(frames), _dev(boxes), view[:k], _dev(rects[:k]), cam)
        n[k] = m.launch_count()
    m.forward_frames(_dev(frames), _dev(boxes), cam)
    forward = m.launch_count()
    torch.cuda.synchronize()
    tail = n[2] - n[1]
    print("launches", n, "forward", forward, "per variant", tail)
    assert tail > 0 and n[5] - n[1] == 4 * tail
    assert 2 * tail < forward
    # the profiling brackets: one around the clean stage and one per occluded pass, one per tail pass
    m.set_profiling(True)
    m.forward_frames_occlusions(_dev(frames), _dev(boxes), view, _dev(rects), cam)
    torch.cuda.synchronize()
    kernels = [r["kernel"] for r in m.profile_records()]
    m.set_profiling(False)
    assert kernels.count("occlusions_frames") == 2 and kernels.count("occlusions_tail") == 1 + len(view)
    del m


# ---------------------------------------------------------------- 7. ABI refusals
def test_raw_abi_refuses_before_any_launch():
    from handmvnet_amd import _lib
    lib = _lib.load()
    m, want = _model(NAME, "f32"), _sweep(NAME, "f32")
    frames, boxes, intr, view, rects = _scene(NAME)
    B, V = frames.shape[:2]
    n = len(view)
    hs = want["heatmap"].shape[-2:]
    h = m._engine(64, 64, 0)
    _sweep_on(m, NAME)
    launches = lib.hmv_launch_count(h)
    g = Guards(DEV)
    f, bx, rc_ = g.inp(_dev(frames)), g.inp(_dev(boxes)), g.inp(_dev(rects))
    bb, it = g.inp(_dev(boxes.astype(np.float32))), g.inp(_dev(intr))
    crop, cam, hm = g.out((B, V, 21, 2)), g.out((1 + n, B, 21, 3)), g.out((B, V, 21) + hs)
    crop_occ, hm_occ = g.out((n, B, 21, 2)), g.out((n, B, 21) + hs)
    outs = (crop, cam, hm, crop_occ, hm_occ)
    for t in outs:
        t.fill_(float("nan"))
    m3, s3 = (ctypes.c_float * 3)(*fo.MEAN.tolist()), (ctypes.c_float * 3)(*fo.STD.tolist())
    bad_std = (ctypes.c_float * 3)(0.2, 0.0, 0.2)
    views = (ctypes.c_int32 * n)(*view.tolist())

    def call(batch=B, frames_=f, fh=120, std=s3, bbox=bb, n_occ=n, occ_view=views, occ_rects=rc_, crop_=crop):
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return lib.hmv_forward_frames_occlusions(h, batch, ptr(frames_), fh, 160, bx.data_ptr(), m3, std, ptr(bbox), it.data_ptr(), n_occ,
                                                 occ_view, ptr(occ_rects), ptr(crop_), cam.data_ptr(), hm.data_ptr(), crop_occ.data_ptr(),
                                                 hm_occ.data_ptr(), None)
    outside, negative = (ctypes.c_int32 * n)(*([0] * (n - 1) + [V])), (ctypes.c_int32 * n)(*([-1] + [0] * (n - 1)))
    refused = {"n_occ = 0": dict(n_occ=0), "n_occ < 0": dict(n_occ=-3), "a null occ_view": dict(occ_view=None),
               "a null occ_rects": dict(occ_rects=None), "camera V": dict(occ_view=outside), "camera -1": dict(occ_view=negative),
               "(1 + n_occ) x batch too large": dict(n_occ=2 ** 31 - 1), "batch = 0": dict(batch=0), "null frames": dict(frames_=None),
               "frame_h = 0": dict(fh=0), "std = 0": dict(std=bad_std), "no bbox under 'crop'": dict(bbox=None),
               "a null joints_crop_img": dict(crop_=None)}
    for what, kw in refused.items():
        rc = call(**kw)
        assert rc == _lib.HMV_ERR_ARG and lib.hmv_last_error(h), (what, rc)
        assert lib.hmv_launch_count(h) == launches, what
    torch.cuda.synchronize()
    for t in outs:
        assert bool(torch.isnan(t).all())      # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    g.check()
    for t, k in zip(outs, ("joints_crop_img", "joints_cam", "heatmap", "joints_crop_img_occ", "heatmap_occ")):
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    # the two per-variant 2D outputs may be NULL
    cam.fill_(float("nan"))
    assert lib.hmv_forward_frames_occlusions(h, B, f.data_ptr(), 120, 160, bx.data_ptr(), m3, s3, bb.data_ptr(), it.data_ptr(), n, views,
                                             rc_.data_ptr(), crop.data_ptr(), cam.data_ptr(), hm.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    g.check()
    assert np.array_equal(cam.cpu().numpy(), want["joints_cam"])
    # the wrapper's own checks
    cp = {"intrinsic": _dev(intr)}
    with pytest.raises(ValueError, match=r"occ_view\[1\] = 7"):
        m.forward_frames_occlusions(_dev(frames), _dev(boxes), [0, V], _dev(rects[:2]), cp)
    with pytest.raises(ValueError, match="occ_rects"):
        m.forward_frames_occlusions(_dev(frames), _dev(boxes), [0, 1], _dev(rects[:3]), cp)
    with pytest.raises(ValueError, match="occ_view"):
        m.forward_frames_occlusions(_dev(frames), _dev(boxes), [], _dev(rects[:0]), cp)
    # no stages after a sweep, as after a ragged call
    m.capture_stages(True)
    try:
        _sweep_on(m, NAME)
        with pytest.raises(_lib.HandMvError, match="ragged"):
            m.read_stage("tokens")
    finally:
        m.capture_stages(False)


# ---------------------------------------------------------------- 8. epoch numbers
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}
ROOT_IDX = 1      # (the root camera, in 0 .. V - 1)
EVAL_NAME = "views_r50_lq_v3"
GRID, CAMERAS = 2, [2, 0]


@functools.lru_cache(maxsize=None)
def _labelled(mode):
    """views_r50_lq_v3 with loss weights, and synthetic labels around its own clean forward from the scene's frames (host arrays)."""
    model = _build(EVAL_NAME, mode, {"loss_weights": WEIGHTS, "mask_invisible_joints": True})
    frames, boxes, intr = _scene(EVAL_NAME)[:3]
    B, V = frames.shape[:2]
    rig = lo.loss_case("vii_many")
    assert rig["V"] >= V and rig["B"] >= B
    own = _np(model.forward_frames(_dev(frames), _dev(boxes), {"intrinsic": _dev(intr)}), ("joints_cam", "joints_crop_img", "heatmap"))
    S, hs = model.data_params["image_size"], own["heatmap"].shape[-1]
    rng = np.random.default_rng(23)
    gt_crop = np.clip(own["joints_crop_img"] + rng.standard_normal(own["joints_crop_img"].shape) * 2, -5, S + 5).astype(np.float32)
    d = dict(frames=frames, boxes=boxes, intr=intr, extr=np.ascontiguousarray(rig["extr"][:B, :V]), gt_crop=gt_crop,
             root_mm=(rig["root_joint"][:B] * 1000).astype(np.float32),
             gt_cam_mm=((own["joints_cam"] + rng.standard_normal(own["joints_cam"].shape) * 0.006) * 1000).astype(np.float32),
             jmask=rng.random((B, V, 21)) < 0.2, heat=lo.target_heatmaps(gt_crop, S, hs, hs).astype(np.float32))
    return model, d


def _batch(d, sl, frames=None):
    data = {"frames": _dev((d["frames"] if frames is None else frames)[sl]), "crop_boxes": _dev(d["boxes"][sl]),
            "joints_cam": _dev(d["gt_cam_mm"][sl]), "root_joint": _dev(d["root_mm"][sl]), "joints_crop_img": _dev(d["gt_crop"][sl]),
            "joints_img_mask": _dev(d["jmask"][sl]), "root_idx": torch.tensor([ROOT_IDX]), "heatmap": _dev(d["heat"][sl])}
    return {"data": data, "cam_params": {"intrinsic": _dev(d["intr"][sl]), "extrinsic": _dev(d["extr"][sl])}}


def _epoch_on_frames(model, d, slices, frames):
    """What an EpochEvaluator gives when fed forward_frames' output on `frames` (the windows as the loss's bboxes)."""
    from handmvnet_amd.evaluation import EpochEvaluator
    ev = EpochEvaluator(model, "test")
    for sl in slices:
        b = _batch(d, sl, frames)
        inputs = b["data"]
        out = model.forward_frames(inputs["frames"], inputs["crop_boxes"], b["cam_params"])
        inputs["joints_cam"] /= 1000
        inputs["root_joint"] /= 1000
        ev.add(out, dict(inputs, bboxes=inputs["crop_boxes"].float()), b["cam_params"])
    return ev.compute()


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_epoch_numbers_equal_an_epoch_on_zeroed_frames(mode):
    """Two steps of different batch size (3 and 2 samples), a 2 x 2 grid on cameras 2 and 0: every value of "clean" and of
    "per_variant"[o] equals the epoch on the clean / zeroed frames -- the same launches on the same bits, the same fp64 order: exact
    equality -- and "sensitivity" is their difference."""
    from handmvnet_amd.occlusion import OcclusionSweepEvaluator, grid_variants
    model, d = _labelled(mode)
    frames, boxes = d["frames"], d["boxes"]
    B, V = frames.shape[:2]
    slices = [slice(0, 3), slice(1, 3)]
    got = model.evaluate_occlusions([_batch(d, sl) for sl in slices], grid=GRID, cameras=CAMERAS)
    variants = grid_variants(V, GRID, CAMERAS)
    assert got["variants"] == variants and len(got["per_variant"]) == len(variants) == 8
    want_clean = _epoch_on_frames(model, d, slices, frames)
    assert want_clean["samples"] == 5 and want_clean["steps"] == 2 and want_clean["test/loss"] is not None
    assert got["clean"] == want_clean
    p = np.minimum(boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]) // GRID
    differs = 0
    for o, (c, r, k) in enumerate(variants):
        rects = np.stack([k * p[:, c], r * p[:, c], (k + 1) * p[:, c], (r + 1) * p[:, c]], axis=-1)
        z = frames.copy()
        z[:, c] = oo.zero_batch(frames[:, c], boxes[:, c], rects)
        want = _epoch_on_frames(model, d, slices, z)
        assert set(got["per_variant"][o]) == set(want)
        for key, v in want.items():
            assert got["per_variant"][o][key] == v, (mode, o, key, got["per_variant"][o][key], v)
        differs += int(want["test_mpjpe"] != want_clean["test_mpjpe"])
        for key, v in want.items():
            if isinstance(v, float) and key not in ("samples", "steps"):
                assert got["sensitivity"][key][c, r, k] == v - want_clean[key], (mode, o, key)
    assert differs >= 6      # (the cells do hide something)
    for key, mp in got["sensitivity"].items():
        assert mp.shape == (V, GRID, GRID) and np.isnan(mp[1]).all(), key
    # a second epoch after reset() repeats the first
    ev = OcclusionSweepEvaluator(model, grid=GRID, cameras=CAMERAS)
    for sl in slices:
        ev.step(_batch(d, sl))
    first = ev.compute()
    assert first["per_variant"] == got["per_variant"] and first["clean"] == got["clean"]
    ev.reset()
    for sl in slices:
        ev.step(_batch(d, sl))
    assert ev.compute()["per_variant"] == first["per_variant"]
