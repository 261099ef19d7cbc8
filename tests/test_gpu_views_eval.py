"""Ragged view sets through the evaluation path on the GPU: hmv_pose_losses_views, hmv_eval_add_views and hmv_forward_frames_views
through handmvnet_amd.losses / .evaluation / the model, against the per-sample oracle (tests/views_loss_oracle.py: the reference's
own numbers for each sample alone over its present views, averaged), the unchanged uniform entries, and themselves.

Tolerances, none from what the kernels return:
  * loss terms and epoch sums: REL = 2e-5 relative, the bar tests/test_gpu_losses.py derives for a mean summed in fp64 (the same
    arithmetic: fp64 sums of the same per-element values, other divisors);
  * projected joints: 2 fp32 ulps of max(|ref|, 1) (fp64 arithmetic, one rounding), exact zeros for absent views;
  * a full mask against the uniform entry, the two target forms, poisoned absent rows, repeats: equal bits;
  * counts of the epoch state: exact;
  * forward_frames with a mask against forward_views on the prepared batch: the bars of
    tests/test_gpu_frames.py::test_forward_frames_equals_forward_on_prepared_batch.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import epoch_oracle as eo
import loss_oracle as lo
import views_loss_oracle as vo
from helpers import rel_l2
from oracle import frames_oracle as fo
from oracle import metrics_oracle as mo
from views_helpers import load_views_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 2e-5
DEV = torch.device("cuda:0")
PER_VIEW = ("pred_hm", "target", "pred_2d", "gt_2d")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _tensors(name):
    """The device tensors of one fixture case, uploaded once and never written."""
    c = lo.loss_case(name)
    t = {n: _dev(c[n]) for n in ("pred_hm", "target", "pred_2d", "gt_2d", "pred_cam", "gt_cam", "root_joint", "intr", "extr", "bbox")}
    t["mask"] = _dev(c["mask"]) if c["mask"] is not None else None
    return t


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The ragged oracle of one case under its mask, computed once."""
    return vo.case_losses(name, vo.case_mask(name))


def _call(name, target="tensor", view_mask=None, tensors=None, **over):
    from handmvnet_amd.losses import pose_losses
    c, t = lo.loss_case(name), tensors or _tensors(name)
    kw = dict(weights=c["weights"], joints_mask=t["mask"], mask_invisible_joints=c["flag"], root_joint=t["root_joint"],
              root_idx=c["root_idx"], intrinsic=t["intr"], extrinsic=t["extr"], bbox=t["bbox"])
    if target == "joints":
        kw.update(image_size=c["S"], sigma=2)
    else:
        kw["target_heatmap"] = t["target"] if target == "tensor" else target
    kw.update(over)
    if view_mask is not None:
        kw["view_mask"] = view_mask
    res, proj = pose_losses(t["pred_hm"], t["pred_2d"], t["pred_cam"], t["gt_2d"], t["gt_cam"], **kw)
    return res.cpu().numpy(), (proj.cpu().numpy() if proj is not None else None)


# ---------------------------------------------------------------- 1. the ragged loss against the oracle
@pytest.mark.parametrize("name", vo.MASKED_CASES)
def test_ragged_loss_matches_the_oracle(name):
    from handmvnet_amd.losses import target_heatmaps
    c, m = lo.loss_case(name), vo.case_mask(name)
    want, wproj = _oracle(name)
    got, proj = _call(name, view_mask=m)
    for i, term in enumerate(lo.TERMS):
        print(f"{name} {term}: dev {got[i]!r} oracle {want[term]!r}")
        assert abs(float(got[i]) - want[term]) <= REL * abs(want[term]), term
    assert (proj is not None) == ("g2d" in c["weights"])
    if proj is not None:
        assert proj.shape == (c["B"], c["V"], 21, 2) and not proj[~m].any()
        ulp = np.spacing(np.maximum(np.abs(wproj[m]), 1.0).astype(np.float32)).astype(np.float64)
        worst = (np.abs(proj[m].astype(np.float64) - wproj[m]) / ulp).max()
        print(f"{name}: projected vs oracle: {worst:.3f} fp32 ulps")
        assert worst <= 2.0
    # the mask as a device tensor and as a nested list: the same call
    again, _ = _call(name, view_mask=_dev(m))
    assert again.tobytes() == got.tobytes()
    assert _call(name, view_mask=m.tolist())[0].tobytes() == got.tobytes()
    # synthesised targets: within REL of the oracle, and the bits of the call over the tensor this library builds from the labels
    own = target_heatmaps(_tensors(name)["gt_2d"], c["S"], (c["h"], c["w"]))
    a, pa = _call(name, target=own, view_mask=m)
    b, pb = _call(name, target="joints", view_mask=m)
    assert a.tobytes() == b.tobytes() and (pa is None or pa.tobytes() == pb.tobytes())
    assert abs(float(b[0]) - want["heatmap_loss"]) <= REL * want["heatmap_loss"]
    assert np.array_equal(b[1:5], got[1:5])


# ---------------------------------------------------------------- 2. a full mask is the uniform entry
@pytest.mark.parametrize("name", ["i_flag_on", "iii_9x13", "vii_many"])
def test_full_mask_equals_the_uniform_entry(name):
    c = lo.loss_case(name)
    ones = np.ones((c["B"], c["V"]), bool)
    for target in ("tensor", "joints"):
        uni, uproj = _call(name, target=target)
        rag, rproj = _call(name, target=target, view_mask=ones)
        assert rag.tobytes() == uni.tobytes(), (target, rag, uni)
        assert (uproj is None and rproj is None) or uproj.tobytes() == rproj.tobytes()


class _Labels:
    """Stands in for the model where only labels are fed (as in tests/test_gpu_eval_epoch.py): a 'loss' that is whatever the step carries."""
    auc_thresh = [0.0, 0.02]
    heatmap_targets = "batch"

    def _calculate_loss(self, out, inputs, cam_params, mode="test", view_mask=None):
        self.last_loss_vector = inputs["heatmap"]


def _add(ev, s, view_mask="own"):
    inputs = {"joints_cam": _dev(s["g"]), "joints_crop_img": _dev(s["g2"])}
    if s.get("mask") is not None:
        inputs["joints_img_mask"] = _dev(s["mask"])
    if s.get("loss") is not None:
        inputs["heatmap"] = _dev(s["loss"])
    out = {"joints_cam": _dev(s["p"]), "joints_crop_img": _dev(s["p2"])}
    vm = s["vm"] if isinstance(view_mask, str) else view_mask
    if vm is None:
        ev.add(out, inputs, None)
    else:
        ev.add(out, inputs, None, view_mask=vm)


@functools.lru_cache(maxsize=None)
def _epoch_steps():
    """Three steps of different B and V (the first with more samples, 1030, than the kernel keeps view counts for in LDS, and more rows
    than it has lanes), the second without loss labels, the third uniform (vm None).  Host arrays, never written."""
    rng = np.random.default_rng(41)
    steps = []
    for B, V, with_loss, ragged in ((1030, 3, True, True), (3, 8, False, True), (6, 8, True, False)):
        g3 = rng.standard_normal((B, 21, 3)).astype(np.float32) * 0.05
        p3 = g3 + rng.standard_normal(g3.shape).astype(np.float32) * 0.006
        g2 = (rng.random((B, V, 21, 2)) * 128).astype(np.float32)
        p2 = g2 + rng.standard_normal(g2.shape).astype(np.float32) * 2
        vm = None
        if ragged:
            vm = rng.random((B, V)) < 0.5
            vm[np.arange(B), rng.integers(0, V, B)] = True
            vm[0] = True
        steps.append(dict(p=p3, g=g3, p2=p2, g2=g2, mask=rng.random((B, V, 21)) < 0.2, vm=vm,
                          loss=(rng.random(6) * 10).astype(np.float32) if with_loss else None))
    return steps


def test_full_mask_epoch_state_equals_the_uniform_entry():
    from handmvnet_amd.evaluation import EpochEvaluator
    uni, rag = EpochEvaluator(_Labels(), "test"), EpochEvaluator(_Labels(), "test")
    for s in _epoch_steps():
        _add(uni, s, view_mask=None)
        _add(rag, s, view_mask=np.ones(s["p2"].shape[:2], bool))
    a, b = uni.state.cpu().numpy(), rag.state.cpu().numpy()
    assert a[0] == 1039 and a.tobytes() == b.tobytes(), (a, b)


# ---------------------------------------------------------------- 3. absent rows are not read
@pytest.mark.parametrize("name", ["iii_9x13", "vii_many"])
def test_absent_rows_are_not_read(name):
    c, m = lo.loss_case(name), vo.case_mask(name)
    clean = {target: _call(name, target=target, view_mask=m) for target in ("tensor", "joints")}
    t = dict(_tensors(name))
    absent = _dev(~m)
    for n in PER_VIEW:
        t[n] = t[n].clone()
        t[n][absent] = float("nan")
    jm = t["mask"].clone() if t["mask"] is not None else torch.zeros(c["B"], c["V"], 21, dtype=torch.bool, device=DEV)
    jm[absent] = True
    t["mask"] = jm if c["mask"] is not None else None
    for target in ("tensor", "joints"):
        got, proj = _call(name, target=target, view_mask=m, tensors=t)
        assert np.isfinite(got).all(), (target, got)
        assert got.tobytes() == clean[target][0].tobytes(), (target, got, clean[target][0])
        assert proj is None or proj.tobytes() == clean[target][1].tobytes()
    # the epoch entry: NaN joints and a set joint mask in the absent rows change nothing
    from handmvnet_amd.evaluation import EpochEvaluator
    s = dict(p=c["pred_cam"], g=c["gt_cam"], p2=c["pred_2d"], g2=c["gt_2d"], mask=c["mask"], vm=m)
    a = EpochEvaluator(_Labels(), "test")
    _add(a, s)
    dirty = dict(s, p2=c["pred_2d"].copy(), g2=c["gt_2d"].copy(),
                 mask=(c["mask"].copy() if c["mask"] is not None else np.zeros((c["B"], c["V"], 21), bool)))
    dirty["p2"][~m] = np.nan
    dirty["g2"][~m] = np.nan
    if c["mask"] is not None:
        dirty["mask"][~m] = True
    else:
        dirty["mask"] = None
    b = EpochEvaluator(_Labels(), "test")
    _add(b, dirty)
    sa, sb = a.state.cpu().numpy(), b.state.cpu().numpy()
    assert np.isfinite(sb).all() and sa.tobytes() == sb.tobytes()


# ---------------------------------------------------------------- 4. the per-sample property, through the UNIFORM entry
def test_ragged_result_is_the_mean_of_the_uniform_entry_per_sample():
    """vii_many: the UNIFORM entry on each sample's present slices (B = 1, V = v_b), averaged.  The three terms without cameras over
    all 38 samples; all six over the samples whose root camera is present -- the sample's own model sees its present cameras only, so
    only there can the uniform entry express the projection."""
    from handmvnet_amd.losses import pose_losses
    name = "vii_many"
    c, t, m = lo.loss_case(name), _tensors(name), vo.case_mask(name)
    plain = {k: c["weights"][k] for k in ("heatmap", "joints_2d", "joints_3d")}
    rows, with_root = [], []
    for b in range(c["B"]):
        P = np.flatnonzero(m[b])
        idx, one = _dev(P), slice(b, b + 1)
        root_present = bool(m[b, c["root_idx"]])
        kw = dict(weights=plain, target_heatmap=t["target"][one][:, idx], joints_mask=t["mask"][one][:, idx], mask_invisible_joints=c["flag"])
        if root_present:   # the root's index among the present cameras
            kw.update(weights=c["weights"], root_joint=t["root_joint"][one], root_idx=int(np.searchsorted(P, c["root_idx"])),
                      intrinsic=t["intr"][one][:, idx], extrinsic=t["extr"][one][:, idx], bbox=t["bbox"][one][:, idx])
        r, _ = pose_losses(t["pred_hm"][one][:, idx], t["pred_2d"][one][:, idx], t["pred_cam"][one], t["gt_2d"][one][:, idx], t["gt_cam"][one], **kw)
        rows.append(r)
        with_root.append(root_present)
    rows = torch.stack(rows).cpu().numpy().astype(np.float64)
    sub = np.flatnonzero(with_root)
    assert 1 < len(sub) < c["B"]
    got, _ = _call(name, view_mask=m)
    for i in (0, 1, 2):
        print(lo.TERMS[i], got[i], rows[:, i].mean())
        assert abs(float(got[i]) - rows[:, i].mean()) <= REL * rows[:, i].mean(), lo.TERMS[i]
    pick = _dev(sub)
    part = {n: (v.index_select(0, pick) if v is not None else None) for n, v in t.items()}
    got_sub, _ = _call(name, view_mask=m[sub], tensors=part)
    for i in (0, 1, 2, 3, 4):
        print("root present:", lo.TERMS[i], got_sub[i], rows[sub, i].mean())
        assert abs(float(got_sub[i]) - rows[sub, i].mean()) <= REL * rows[sub, i].mean(), lo.TERMS[i]
    assert abs(float(got_sub[5]) - rows[sub, :5].mean(0).sum()) <= REL * rows[sub, :5].mean(0).sum()
    # the order of the samples does not matter
    rev = {n: (v.flip(0).contiguous() if v is not None else None) for n, v in t.items()}
    flipped, _ = _call(name, view_mask=m[::-1].copy(), tensors=rev)
    for i in range(6):
        assert abs(float(flipped[i]) - float(got[i])) <= REL * abs(float(got[i])), lo.TERMS[i]


def test_more_samples_than_the_kernels_keep_counts_for():
    """B = 1030 > 1024: beyond that the one-workgroup kernels count a sample's mask row when they need it instead of reading the
    table in LDS.  Random data on the camera rig of i_flag_on, 3 x 5 maps; the loss against the oracle."""
    from handmvnet_amd.losses import pose_losses
    c = lo.loss_case("i_flag_on")
    B, V, h, w = 1030, c["V"], 3, 5
    rng = np.random.default_rng(77)
    tile = lambda a: np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:]))   # noqa: E731
    hm, tg = rng.random((B, V, 21, h, w), np.float32), rng.random((B, V, 21, h, w), np.float32)
    g2 = (rng.random((B, V, 21, 2)) * 200).astype(np.float32)
    p2 = g2 + rng.standard_normal(g2.shape).astype(np.float32) * 2
    gc = np.tile(c["gt_cam"], (B // 2, 1, 1)) + rng.standard_normal((B, 21, 3)).astype(np.float32) * 0.002
    pc = gc + rng.standard_normal(gc.shape).astype(np.float32) * 0.004
    jm = rng.random((B, V, 21)) < 0.2
    vm = rng.random((B, V)) < 0.5
    vm[np.arange(B), rng.integers(0, V, B)] = True
    assert not vm[1024:].all() and not vm[:, c["root_idx"]].all()
    extr, intr, bbox, rj = tile(c["extr"]), tile(c["intr"]), tile(c["bbox"]), tile(c["root_joint"])
    res, proj = pose_losses(_dev(hm), _dev(p2), _dev(pc), _dev(g2), _dev(gc), c["weights"], target_heatmap=_dev(tg), joints_mask=_dev(jm),
                            mask_invisible_joints=True, root_joint=_dev(rj), root_idx=c["root_idx"], intrinsic=_dev(intr),
                            extrinsic=_dev(extr), bbox=_dev(bbox), view_mask=vm)
    want, wproj = vo.losses(hm, tg, p2, g2, pc, gc, c["weights"], vm, jm, True, rj, c["root_idx"], intr, extr, bbox)
    got = res.cpu().numpy()
    for i, term in enumerate(lo.TERMS):
        print(f"{term}: dev {got[i]!r} oracle {want[term]!r}")
        assert abs(float(got[i]) - want[term]) <= REL * abs(want[term]), term
    proj = proj.cpu().numpy()
    assert not proj[~vm].any()
    ulp = np.spacing(np.maximum(np.abs(wproj[vm]), 1.0).astype(np.float32)).astype(np.float64)
    assert (np.abs(proj[vm].astype(np.float64) - wproj[vm]) / ulp).max() <= 2.0


# ---------------------------------------------------------------- 5. the epoch
def test_ragged_epoch_matches_the_oracle():
    from handmvnet_amd.evaluation import EpochEvaluator
    steps = _epoch_steps()
    states = []
    for _ in range(2):
        ev = EpochEvaluator(_Labels(), "test")
        for s in steps:
            _add(ev, s)
        states.append(ev.state.cpu().numpy())
        got = ev.compute()
    assert states[0].tobytes() == states[1].tobytes()               # two identical epochs: identical bits
    state = states[0]
    want_state = eo.new_state(20)
    for s in steps:
        loss = dict(zip(lo.TERMS, s["loss"])) if s["loss"] is not None else None
        if s["vm"] is None:
            eo.accumulate(want_state, s["p"], s["g"], s["p2"], s["g2"], s["mask"], loss)
        else:
            vo.accumulate(want_state, s["p"], s["g"], s["p2"], s["g2"], s["vm"], s["mask"], loss)
    assert np.array_equal(state[[0, 1, 2, 5, 7]], want_state[[0, 1, 2, 5, 7]])
    assert state[0] == 1039 and state[1] == 3 and state[5] == (1030 * 3 + 9 * 8) * 21 and state[7] == 1036
    assert np.array_equal(state[14:], want_state[14:]) and state[14:].sum() == 1039 * 21
    for i in (3, 4, 6):
        print(i, state[i], want_state[i])
        assert abs(state[i] - want_state[i]) <= REL * want_state[i], i
    assert np.allclose(state[8:14], want_state[8:14], rtol=1e-12, atol=0)   # B x an fp32 value, summed in fp64 on both sides
    want = eo.finish(want_state)
    for mine, theirs in (("test_mpjpe", "mpjpe"), ("test_pa_mpjpe", "pa_mpjpe"), ("test_mpjpe2d", "mpjpe2d")):
        assert got[mine] == pytest.approx(want[theirs], rel=REL), mine
    assert np.array_equal(np.array(got["test_pck_j"], np.float32), want["pck"])
    for term in lo.TERMS:
        assert got[f"test/{term}"] == pytest.approx(want[term], rel=1e-12), term
    # one ragged step alone: [6] / [5] is the mean over samples of the per-sample 2D MPJPE
    ev, s = EpochEvaluator(_Labels(), "test"), steps[1]
    _add(ev, s)
    per = [vo.mpjpe2d(s["p2"][b:b + 1], s["g2"][b:b + 1], s["vm"][b:b + 1], s["mask"][b:b + 1]) for b in range(len(s["p"]))]
    assert ev.compute()["test_mpjpe2d"] == pytest.approx(np.mean(per), rel=REL)


# ---------------------------------------------------------------- 6. frames
NAME = "views_r18_v7"
MODES = ["f32", "f16", "f32x3"]


def _build(mode, tp_over=None):
    from handmvnet_amd import HandMvNet
    case = load_views_case(NAME)
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
def _model(mode):
    return _build(mode)


@functools.lru_cache(maxsize=None)
def _frames():
    """uint8 frames 120 x 160 and random windows for views_r18_v7, built as tests/test_gpu_frames.py builds them."""
    case = load_views_case(NAME)
    b, v = case["spec"]["B"], case["spec"]["V"]
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, (b, v, 120, 160, 3), dtype=np.uint8)
    frames = ((frames.astype(np.float32) + np.roll(frames, 1, 2) + np.roll(frames, 1, 3)) / 3).astype(np.uint8)
    side = rng.integers(50, 140, (b, v))
    x1, y1 = rng.integers(-20, 100, (b, v)), rng.integers(-20, 60, (b, v))
    boxes = np.stack([x1, y1, x1 + side, y1 + side], axis=-1).astype(np.int32)
    return frames, boxes


def _np(out):
    return {k: out[k].cpu().numpy() for k in ("joints_cam", "joints_crop_img", "heatmap")}


@pytest.mark.parametrize("mode", MODES)
def test_forward_frames_with_a_mask_equals_forward_views_on_the_prepared_batch(mode):
    from test_gpu_parity import fp16_bounds
    case, m = load_views_case(NAME), _model(mode)
    frames, boxes = _frames()
    mask, size = case["mask"], case["spec"]["size"]
    cam = {"intrinsic": _dev(case["inputs"][2])}
    fused = _np(m.forward_frames(_dev(frames), _dev(boxes), cam, image_size=size, view_mask=mask))
    two_step = _np(m.forward_views(_dev(fo.prepare_batch(frames, boxes, size)), mask, _dev(boxes.astype(np.float32)), cam))
    half = mode == "f16"
    B, V = mask.shape
    assert fused["joints_crop_img"].shape == (B, V, 21, 2) and fused["heatmap"].shape == two_step["heatmap"].shape
    assert not fused["joints_crop_img"][~mask].any() and not fused["heatmap"][~mask].any()      # absent views: exact zeros
    assert np.isfinite(fused["joints_cam"]).all()
    # the bars of test_forward_frames_equals_forward_on_prepared_batch (fp16: the noise floor of the nearest tiny r18 case)
    tol = fp16_bounds("tiny_r18")["joints_cam"] if half else 1e-4
    assert rel_l2(fused["joints_cam"], two_step["joints_cam"]) < tol
    assert np.abs(fused["joints_crop_img"] - two_step["joints_crop_img"]).max() < (1.0 if half else 0.02)
    assert rel_l2(fused["heatmap"], two_step["heatmap"]) < (5e-3 if half else 1e-4)
    # a full mask: the bits of forward_frames without one
    ones = np.ones_like(mask)
    a = _np(m.forward_frames(_dev(frames), _dev(boxes), cam, image_size=size, view_mask=ones))
    b = _np(m.forward_frames(_dev(frames), _dev(boxes), cam, image_size=size))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (mode, k)


@pytest.mark.parametrize("mode", MODES)
def test_forward_frames_with_a_mask_at_an_odd_size(mode):
    """75 x 75 crops: the indexed kernel writes the space-to-depth stem layout with a half-empty last row / column pair."""
    case, m = load_views_case(NAME), _model(mode)
    frames, boxes = _frames()
    cam = {"intrinsic": _dev(case["inputs"][2])}
    a = _np(m.forward_frames(_dev(frames), _dev(boxes), cam, image_size=75, view_mask=case["mask"]))
    b = _np(m.forward_frames(_dev(frames), _dev(boxes), cam, image_size=75, view_mask=case["mask"]))
    for k in a:
        assert np.isfinite(a[k]).all() and a[k].tobytes() == b[k].tobytes(), (mode, k)
    assert a["joints_crop_img"][case["mask"]].any() and not a["joints_crop_img"][~case["mask"]].any()


def test_raw_frames_entry_refuses_before_any_launch():
    from handmvnet_amd import _lib
    lib = _lib.load()
    case, m = load_views_case(NAME), _model("f32")
    frames, boxes = _frames()
    size = case["spec"]["size"]
    fr, bx, intr = _dev(frames), _dev(boxes), _dev(case["inputs"][2])
    cam = {"intrinsic": intr}
    good = _np(m.forward_frames(fr, bx, cam, image_size=size, view_mask=case["mask"]))
    h = m._engine(size, size, 0)
    launches = lib.hmv_launch_count(h)
    B, V = case["mask"].shape
    crop = torch.full((B * V, 21, 2), float("nan"), device=DEV)
    cam_out = torch.full((B, 21, 3), float("nan"), device=DEV)
    table = torch.arange(B * V, dtype=torch.int32, device=DEV)
    bb, it = bx.reshape(-1, 4).float().contiguous(), intr.reshape(-1, 4).contiguous()
    m3, s3 = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    arr = lambda *c: (ctypes.c_int32 * len(c))(*c)   # noqa: E731

    def call(batch, counts, frames_ptr=fr.data_ptr(), std=s3):
        return lib.hmv_forward_frames_views(h, batch, counts, frames_ptr, 120, 160, bx.data_ptr(), table.data_ptr(), m3, std, bb.data_ptr(),
                                            it.data_ptr(), crop.data_ptr(), cam_out.data_ptr(), None, None)
    for what, rc in {"a count of 0": call(B, arr(7, 0, 2, 3, 5)), "a count above num_views": call(B, arr(7, 1, V + 1, 3, 5)),
                     "a null table": call(B, None), "B = 0": call(0, arr(7, 1, 2, 3, 5))}.items():
        msg = lib.hmv_last_error(h)
        assert rc == 1 and msg and b"hmv_forward_frames_views" in msg, (what, rc, msg)
        assert lib.hmv_launch_count(h) == launches, what
    assert call(B, arr(7, 1, 2, 3, 5), frames_ptr=None) == 1 and lib.hmv_launch_count(h) == launches          # hmv_forward_frames' refusals
    assert call(B, arr(7, 1, 2, 3, 5), std=(ctypes.c_float * 3)(0.2, 0.0, 0.2)) == 1 and lib.hmv_launch_count(h) == launches
    torch.cuda.synchronize()
    assert torch.isnan(crop).all() and torch.isnan(cam_out).all()      # nothing was launched
    again = _np(m.forward_frames(fr, bx, cam, image_size=size, view_mask=case["mask"]))
    for k in good:
        assert again[k].tobytes() == good[k].tobytes(), k
    with pytest.raises(ValueError, match="at least one present view"):
        m.forward_frames(fr, bx, cam, image_size=size, view_mask=np.zeros_like(case["mask"]))


# ---------------------------------------------------------------- 7. the model
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}
ROOT_IDX = 3


@functools.lru_cache(maxsize=None)
def _labelled():
    """views_r18_v7 with loss weights, and synthetic labels around its own ragged forward (host arrays, never written)."""
    case = load_views_case(NAME)
    model = _build("f32", {"loss_weights": WEIGHTS, "mask_invisible_joints": True})
    x, bbox, intr = case["inputs"]
    B, V = case["mask"].shape
    rig = lo.loss_case("vii_many")
    assert rig["V"] >= V and not case["mask"][:, ROOT_IDX].all()      # the root camera is absent in some samples
    own = _np(model.forward_views(_dev(x), case["mask"], _dev(bbox), {"intrinsic": _dev(intr)}))
    S, hs = model.data_params["image_size"], own["heatmap"].shape[-1]
    rng = np.random.default_rng(9)
    gt_crop = np.clip(own["joints_crop_img"] + rng.standard_normal(own["joints_crop_img"].shape) * 2, -5, S + 5).astype(np.float32)
    d = dict(rgb=x, bboxes=bbox, intr=intr, extr=np.ascontiguousarray(rig["extr"][:B, :V]), gt_crop=gt_crop,
             root_mm=(rig["root_joint"][:B] * 1000).astype(np.float32),
             gt_cam_mm=((own["joints_cam"] + rng.standard_normal(own["joints_cam"].shape) * 0.006) * 1000).astype(np.float32),
             jmask=rng.random((B, V, 21)) < 0.2, heat=lo.target_heatmaps(gt_crop, S, hs, hs).astype(np.float32))
    return model, case["mask"], d, own


def _batch(d, sl=slice(None), view_mask=None):
    data = {"rgb": _dev(d["rgb"][sl]), "bboxes": _dev(d["bboxes"][sl]), "joints_cam": _dev(d["gt_cam_mm"][sl]),
            "root_joint": _dev(d["root_mm"][sl]), "joints_crop_img": _dev(d["gt_crop"][sl]), "joints_img_mask": _dev(d["jmask"][sl]),
            "root_idx": torch.tensor([ROOT_IDX]), "heatmap": _dev(d["heat"][sl])}
    batch = {"data": data, "cam_params": {"intrinsic": _dev(d["intr"][sl]), "extrinsic": _dev(d["extr"][sl])}}
    if view_mask is not None:
        batch["view_mask"] = torch.from_numpy(view_mask[sl].copy())
    return batch


NUMBERS = ("test_mpjpe", "test_pa_mpjpe", "test_mpjpe2d") + tuple(f"test/{t}" for t in lo.TERMS)


def test_test_step_on_a_ragged_batch():
    model, mask, d, own = _labelled()
    first = _batch(d, view_mask=mask)
    res = model.test_step(first, 0)
    gt_m, root = first["data"]["joints_cam"].cpu().numpy(), first["data"]["root_joint"].cpu().numpy()      # converted in place
    assert np.allclose(gt_m, d["gt_cam_mm"] / np.float32(1000), rtol=1e-6)
    want, _ = vo.losses(own["heatmap"], d["heat"], own["joints_crop_img"], d["gt_crop"], own["joints_cam"], gt_m, WEIGHTS, mask, d["jmask"], True,
                        root, ROOT_IDX, d["intr"], d["extr"], d["bboxes"])
    for n in lo.TERMS:
        got = float(model.last_losses[f"test/{n}"])
        print(f"{n}: dev {got!r} oracle {want[n]!r}")
        assert np.isfinite(want[n]) and abs(got - want[n]) <= REL * abs(want[n]), n
    assert res["loss"].item() == float(model.last_losses["test/loss"]) == float(model.last_loss_vector[5])
    met = res["metrics"]
    assert float(met["test_mpjpe2d"]) == pytest.approx(vo.mpjpe2d(own["joints_crop_img"], d["gt_crop"], mask, d["jmask"]), rel=REL)
    assert float(met["test_mpjpe"]) == pytest.approx(mo.mpjpe(own["joints_cam"], gt_m) * 1000, rel=REL)
    assert float(met["test_pa_mpjpe"]) == pytest.approx(mo.pa_mpjpe(own["joints_cam"], gt_m) * 1000, rel=REL)
    # a sample without a present view: forward_views' ValueError, before anything is launched
    none = mask.copy()
    none[2] = False
    bad = _batch(d, view_mask=none)
    with pytest.raises(ValueError, match="at least one present view"):
        model.test_step(bad, 0)
    assert np.array_equal(bad["data"]["joints_cam"].cpu().numpy(), d["gt_cam_mm"])      # not even the labels were converted
    with pytest.raises(ValueError, match="at least one present view"):
        model.evaluate([_batch(d, view_mask=none)])


def test_evaluate_does_not_depend_on_the_cut_of_a_ragged_split():
    model, mask, d, _ = _labelled()
    whole = model.evaluate([_batch(d, view_mask=mask)])
    step = model.test_step(_batch(d, view_mask=mask), 0)
    assert whole["samples"] == 5 and whole["steps"] == 1
    for k in ("test_mpjpe", "test_pa_mpjpe", "test_mpjpe2d"):
        assert whole[k] == pytest.approx(float(step["metrics"][k]), rel=REL), k
    for t in lo.TERMS:
        assert whole[f"test/{t}"] == pytest.approx(float(model.last_losses[f"test/{t}"]), rel=1e-6), t
    for cut in ((2, 3), (1, 4)):
        at, batches = 0, []
        for n in cut:
            batches.append(_batch(d, slice(at, at + n), view_mask=mask))
            at += n
        got = model.evaluate(batches)
        assert got["samples"] == 5 and got["steps"] == 2
        for k in NUMBERS:
            print(cut, k, got[k], whole[k])
            assert got[k] == pytest.approx(whole[k], rel=REL), (cut, k)
        assert got["test_pck_j"] == whole["test_pck_j"]


def test_a_batch_without_the_key_takes_the_old_path():
    """evaluate() on batches without "view_mask" against an explicit loop over forward + EpochEvaluator.add, the parent's loop: equal bits."""
    from handmvnet_amd.evaluation import EpochEvaluator
    model, mask, d, _ = _labelled()
    cuts = (slice(0, 2), slice(2, 5))
    got = model.evaluate([_batch(d, sl) for sl in cuts])
    ev = EpochEvaluator(model, "test")
    for sl in cuts:
        b = _batch(d, sl)
        out = model.forward(b["data"]["rgb"], b["data"]["bboxes"], b["cam_params"])
        b["data"]["joints_cam"] /= 1000
        b["data"]["root_joint"] /= 1000
        ev.add(out, b["data"], b["cam_params"])
    assert got == ev.compute()
    ragged = model.evaluate([_batch(d, sl, view_mask=mask) for sl in cuts])
    assert ragged["test_mpjpe2d"] != got["test_mpjpe2d"] and ragged["test/heatmap_loss"] != got["test/heatmap_loss"]


def test_view_mask_from_joints_selects_the_ragged_path():
    from handmvnet_amd.evaluation import EpochEvaluator, view_mask_from_joints
    model, mask, d, _ = _labelled()
    jm = d["jmask"].copy()
    jm[1, 4] = True                                   # sample 1 sees no joint in view 4: the dataset feeds a black image there
    vm = view_mask_from_joints(torch.from_numpy(jm))
    want = np.ones_like(mask)
    want[1, 4] = False
    assert vm.numpy().tolist() == want.tolist()
    d2 = dict(d, jmask=jm)
    a, b = EpochEvaluator(model, "test"), EpochEvaluator(model, "test")
    batch = _batch(d2)
    batch["view_mask"] = vm
    out = a.step(batch)
    assert not out["joints_crop_img"][1, 4].any() and not out["heatmap"][1, 4].any() and out["joints_crop_img"][1, 3].any()
    b.step(_batch(d2, view_mask=want))
    assert a.state.cpu().numpy().tobytes() == b.state.cpu().numpy().tobytes()
    plain = EpochEvaluator(model, "test")
    plain.step(_batch(d2))
    assert plain.state.cpu().numpy()[6] != a.state.cpu().numpy()[6]
