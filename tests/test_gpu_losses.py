"""GPU parity of the evaluation-step losses (handmvnet_amd/csrc/losses.hip through handmvnet_amd.losses / .camera / the model)
against outputs of the real reference (tests/golden/loss_cases.npz, stored from fp32 and from float64 runs).

Tolerances, each from the arithmetic and none from what the kernels return:
  * target maps: the kernel and the float64 reference evaluate the same expression in fp64 (a few 1e-16 apart), so only the final
    fp32 rounding can flip: |dev - ref| <= 2^-23 |ref| + 1e-12;
  * projection: <= 2 fp32 ulps of max(|ref|, 1) from the float64 reference (fp64 arithmetic, one rounding); from the fp32 reference
    <= 2 x that run's own stored max |f32 - f64|;
  * loss terms: 2e-5 relative to the float64 reference -- the bar tests/test_gpu_metrics.py sets for a mean the reference sums in
    fp32 and the kernel in fp64; against the fp32 reference that plus the reference's own |f32 - f64|;
  * the synthesised-target form and repeated calls: equal bits.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import loss_oracle as lo
from helpers import load_case

pytestmark = pytest.mark.gpu

MAP_NAMES, LOSS_NAMES = lo.case_names("hm"), lo.case_names("loss")
REL = 2e-5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _tensors(name):
    """The device tensors of one fixture case, uploaded once and never written."""
    c = lo.loss_case(name)
    t = {n: _dev(c[n]) for n in ("pred_hm", "target", "pred_2d", "gt_2d", "pred_cam", "gt_cam", "root_joint", "intr", "extr", "bbox")}
    t["mask"] = _dev(c["mask"]) if c["mask"] is not None else None
    return t


def _kwargs(name, target="tensor", **over):
    c, t = lo.loss_case(name), _tensors(name)
    kw = dict(weights=c["weights"], joints_mask=t["mask"], mask_invisible_joints=c["flag"], root_joint=t["root_joint"],
              root_idx=c["root_idx"], intrinsic=t["intr"], extrinsic=t["extr"], bbox=t["bbox"])
    if isinstance(target, torch.Tensor):
        kw["target_heatmap"] = target
    elif target == "joints":
        kw.update(image_size=c["S"], sigma=2)
    else:
        kw["target_heatmap"] = t["target"]
    kw.update(over)
    return (t["pred_hm"], t["pred_2d"], t["pred_cam"], t["gt_2d"], t["gt_cam"]), kw


def _run(name, target="tensor", **over):
    from handmvnet_amd.losses import pose_losses
    args, kw = _kwargs(name, target, **over)
    res, proj = pose_losses(*args, **kw)
    return res.cpu().numpy(), proj


@pytest.mark.parametrize("name", MAP_NAMES)
def test_target_maps_match_reference(name):
    from handmvnet_amd.losses import target_heatmaps
    m = lo.map_case(name)
    got = target_heatmaps(_dev(m["joints"]), m["S"], (m["h"], m["w"])).cpu().numpy()
    assert got.shape == m["ref"].shape and got.dtype == np.float32
    valid, ref = m["valid"], m["ref"].astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)[valid]
    print(f"{name}: max |dev - ref| = {err.max():.3e}, elements that differ: {(err > 0).sum()} of {err.size}")
    assert np.all(err <= 2.0 ** -23 * np.abs(ref[valid]) + 1e-12)
    assert (~valid).sum() > 0 and np.all(got[~valid] == 0)      # whole Gaussian outside the image (S + 6.1, -8.3): zero maps
    assert got[valid].max() > 0.1


@pytest.mark.parametrize("name", [n for n in LOSS_NAMES if "g2d" in lo.loss_case(n)["weights"] and n != "i_flag_off"])
def test_projection_matches_reference(name):
    from handmvnet_amd.camera import get_2d_joints_from_3d_joints
    c, t = lo.loss_case(name), _tensors(name)
    joints_abs = t["pred_cam"] + t["root_joint"]          # the fp32 add the fp32 reference does (handmvnet.py:325)
    for bbox, r64, r32, d in ((None, c["proj_img64"], c["proj_img32"], c["proj_img_maxdiff"]),
                              (t["bbox"], c["proj64"], c["proj32"], c["proj_maxdiff"])):
        got = get_2d_joints_from_3d_joints(joints_abs, c["root_idx"], t["intr"], t["extr"], bbox).cpu().numpy()
        assert got.shape == (c["B"], c["V"], 21, 2)
        e32 = np.abs(got.astype(np.float64) - r32).max()
        print(f"{name}: vs fp32 reference {e32:.3e} px (its own f32 - f64: {float(d):.3e})")
        assert e32 <= 2 * float(d)
    # the float64 reference added pred_cam + root_joint in float64, so its operand is not the fp32 sum above: the loss entry takes
    # the two separately and adds them in fp64 as well -- compare its `projected`
    _, proj = _run(name)
    got = proj.cpu().numpy()
    ulp = np.spacing(np.maximum(np.abs(c["proj64"]), 1.0).astype(np.float32)).astype(np.float64)
    worst = (np.abs(got.astype(np.float64) - c["proj64"]) / ulp).max()
    print(f"{name}: projected vs float64 reference: {worst:.3f} fp32 ulps")
    assert worst <= 2.0


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_loss_terms_match_reference(name):
    c = lo.loss_case(name)
    got, proj = _run(name)
    assert (proj is not None) == ("g2d" in c["weights"])
    for i, term in enumerate(lo.TERMS):
        r64, r32 = float(c["ref64"][i]), float(c["ref32"][i])
        print(f"{name} {term}: dev {got[i]!r} ref64 {r64!r} ref32 {r32!r}")
        assert abs(float(got[i]) - r64) <= REL * abs(r64), term
        assert abs(float(got[i]) - r32) <= REL * abs(r32) + abs(r32 - r64), term


@pytest.mark.parametrize("name", ["i_flag_on", "iii_9x13", "iv_12x20", "vii_many"])
def test_synthesised_targets_give_the_bits_of_the_tensor_path(name):
    from handmvnet_amd.losses import target_heatmaps
    c, t = lo.loss_case(name), _tensors(name)
    own = target_heatmaps(t["gt_2d"], c["S"], (c["h"], c["w"]))
    a, _ = _run(name, target=own)
    b, _ = _run(name, target="joints")
    assert a.tobytes() == b.tobytes()
    assert abs(float(b[0]) - float(c["ref64"][0])) <= REL * float(c["ref64"][0])     # and it is the right number
    # an unaligned view of the same values (frame bases off the 16-byte grid) takes the scalar loads: same bits again
    flat = torch.empty(t["pred_hm"].numel() + 1, device="cuda:0")
    flat[1:] = t["pred_hm"].reshape(-1)
    args, kw = _kwargs(name, "joints")
    from handmvnet_amd.losses import pose_losses
    shifted = flat[1:].view_as(t["pred_hm"])
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    r, _ = pose_losses(shifted, *args[1:], **kw)
    assert r.cpu().numpy().tobytes() == b.tobytes()


def test_losses_are_deterministic():
    name = "vii_many"
    first, _ = _run(name)
    x = torch.randn(512, 512, device="cuda:0")
    for _ in range(2):
        y = x @ x                                              # unrelated work on the stream in between
        again, _ = _run(name)
        assert again.tobytes() == first.tobytes()
    assert torch.isfinite(y).all()


def test_mask_semantics():
    on, _ = _run("i_flag_on")
    off, _ = _run("i_flag_off")
    none, _ = _run("i_flag_on", joints_mask=None)
    assert off.tobytes() == none.tobytes()                     # flag off with a mask present = no mask
    assert on[1] != off[1] and np.array_equal(on[[0, 2, 3, 4]], off[[0, 2, 3, 4]])     # g2d / p2d are unmasked, like the reference
    c = lo.loss_case("i_flag_on")
    full, _ = _run("i_flag_on", joints_mask=torch.ones(c["B"], c["V"], 21, dtype=torch.bool, device="cuda:0"))
    assert full[1] == 0.0
    assert full[5] == pytest.approx(float(full[0]) + float(full[2]) + float(full[3]) + float(full[4]), rel=1e-6)


def test_pose_loss_criteria():
    from handmvnet_amd.losses import PoseLoss
    c, t = lo.loss_case("iii_9x13"), _tensors("iii_9x13")
    f = lambda a: np.asarray(a, np.float64)   # noqa: E731
    mse = PoseLoss.mse_loss(t["pred_hm"], t["target"], weight=10.)
    assert mse.dim() == 0 and mse.is_cuda
    assert mse.item() == pytest.approx(10 * np.mean((f(c["pred_hm"]) - f(c["target"])) ** 2), rel=REL)
    assert PoseLoss.l1_loss(t["pred_2d"], t["gt_2d"]).item() == pytest.approx(np.mean(np.abs(f(c["pred_2d"]) - f(c["gt_2d"]))), rel=REL)
    assert PoseLoss.l1_loss(t["pred_cam"], t["gt_cam"], weight=1000.).item() == \
        pytest.approx(1000 * np.mean(np.abs(f(c["pred_cam"]) - f(c["gt_cam"]))), rel=REL)
    # stacked_dim: one label set for every view
    lab = t["gt_2d"][:, 0]
    want = np.mean(np.abs(f(c["pred_2d"]) - f(c["gt_2d"])[:, :1]))
    assert PoseLoss.l1_loss(t["pred_2d"], lab, stacked_dim=1).item() == pytest.approx(want, rel=REL)


def test_bad_arguments():
    from handmvnet_amd import _lib
    from handmvnet_amd.camera import get_2d_joints_from_3d_joints
    from handmvnet_amd.losses import build_loss_args, pose_losses, run_loss_args, target_heatmaps
    name = "ii_q256"
    c, t = lo.loss_case(name), _tensors(name)
    args, kw = _kwargs(name)
    with pytest.raises(_lib.HandMvError, match="pred_heatmap"):
        pose_losses(args[0].cpu(), *args[1:], **kw)                                   # no CPU path
    with pytest.raises(_lib.HandMvError, match="CUDA"):
        target_heatmaps(t["gt_2d"].cpu(), c["S"], 16)
    with pytest.raises(_lib.HandMvError, match="CUDA"):
        get_2d_joints_from_3d_joints(t["pred_cam"].cpu(), 0, t["intr"], t["extr"])
    with pytest.raises(_lib.HandMvError, match="B must"):
        pose_losses(*(a[:0] for a in args), **{**kw, "target_heatmap": t["target"][:0], "bbox": t["bbox"][:0], "intrinsic": t["intr"][:0],
                                               "extrinsic": t["extr"][:0], "root_joint": None})
    with pytest.raises(_lib.HandMvError, match="V must"):
        pose_losses(args[0][:, :0], args[1][:, :0], args[2], args[3][:, :0], args[4],
                    **{**kw, "target_heatmap": t["target"][:, :0], "bbox": t["bbox"][:, :0], "intrinsic": t["intr"][:, :0],
                       "extrinsic": t["extr"][:, :0]})
    with pytest.raises(_lib.HandMvError, match="root_idx"):
        pose_losses(*args, **{**kw, "root_idx": c["V"]})
    with pytest.raises(_lib.HandMvError, match="root_idx"):
        get_2d_joints_from_3d_joints(t["pred_cam"], c["V"], t["intr"], t["extr"])
    for field, value, word in (("gt_joints_2d", None, "gt_joints_2d"), ("scratch_bytes", 8 * c["B"] * c["V"] - 1, "scratch_bytes"),
                               ("struct_size", ctypes.sizeof(_lib.HmvLossArgs) - 8, "struct_size")):
        a, dev, _, keep = build_loss_args(*args, **kw)
        setattr(a, field, value)
        with pytest.raises(_lib.HandMvError, match=word):
            run_loss_args(a, dev)
    good, _ = pose_losses(*args, **kw)                                                # and the library still works afterwards
    assert abs(good[5].item() - float(c["ref64"][5])) <= REL * float(c["ref64"][5])


def _rig(V):
    """extrinsics + root joint of a fixture rig with V views (sample 0), metres."""
    c = lo.loss_case("iii_9x13")
    assert c["V"] == V
    return c["extr"][:1], c["root_joint"][:1], c["root_idx"]


def test_evaluation_step_returns_the_loss():
    """cfg1_r50_v4_128 through test_step with loss labels: the loss of the engine's own forward, checked against the numpy oracle."""
    from handmvnet_amd import HandMvNet
    cfg, (tp, mp, dp), sd, (x, bbox, intr), fx = load_case("cfg1_r50_v4_128")
    weights = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}
    tp = dict(tp, loss_weights=weights, mask_invisible_joints=True)
    model = HandMvNet(tp, mp, dp)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    B, V, S, hs = x.shape[0], x.shape[1], dp["image_size"], dp["heatmap_size"]
    extr, root_m, root_idx = _rig(V)
    own = model(_dev(x), _dev(bbox), {"intrinsic": _dev(intr)})
    own = {k: v.cpu().numpy() for k, v in own.items()}
    assert own["heatmap"].shape == (B, V, 21, hs, hs)
    rng = np.random.default_rng(5)
    gt_cam_mm = ((own["joints_cam"] + rng.standard_normal(own["joints_cam"].shape) * 0.006) * 1000).astype(np.float32)
    gt_crop = np.clip(own["joints_crop_img"] + rng.standard_normal(own["joints_crop_img"].shape) * 2, -5, S + 5).astype(np.float32)
    mask = rng.random((B, V, 21)) < 0.2
    root_mm = (root_m * 1000).astype(np.float32)
    heat = lo.target_heatmaps(gt_crop, S, hs, hs).astype(np.float32)

    def batch(with_loss_labels=True, heatmap=True):
        data = {"rgb": _dev(x), "bboxes": _dev(bbox), "joints_cam": _dev(gt_cam_mm), "root_joint": _dev(root_mm),
                "joints_crop_img": _dev(gt_crop), "joints_img_mask": _dev(mask)}
        cam = {"intrinsic": _dev(intr)}
        if with_loss_labels:
            data["root_idx"] = torch.tensor([root_idx])
            cam["extrinsic"] = torch.from_numpy(extr.copy())          # left on the host: moved like the other labels
            if heatmap:
                data["heatmap"] = torch.from_numpy(heat.copy())
        return {"data": data, "cam_params": cam}

    first = batch()
    res = model.test_step(first, 0)
    # the labels as the step converted them in place (mm -> m on the device)
    gt_m, root = first["data"]["joints_cam"].cpu().numpy(), first["data"]["root_joint"].cpu().numpy()
    assert np.allclose(gt_m, gt_cam_mm / np.float32(1000), rtol=1e-6)
    want, proj = lo.losses(own["heatmap"], heat, own["joints_crop_img"], gt_crop, own["joints_cam"], gt_m, weights, mask, True,
                           root, root_idx, intr, extr, bbox)
    assert res["loss"].dim() == 0 and res["loss"].is_cuda
    names = {f"test/{n}" for n in ("heatmap_loss", "joints_2d_loss", "joints_3d_loss", "root_3d_loss", "g2d_loss", "p2d_loss")}
    assert names <= set(model.last_losses) and set(model.last_losses) - names == {"test/loss"}
    assert model.last_losses["test/root_3d_loss"] == 0.0
    for n in lo.TERMS:
        got = float(model.last_losses[f"test/{n}"])
        print(f"{n}: dev {got!r} oracle {want[n]!r}")
        assert np.isfinite(want[n]) and abs(got - want[n]) <= REL * abs(want[n]), n
    assert res["loss"].item() == float(model.last_losses["test/loss"])
    # _calculate_loss itself: the projected joints land in `out`
    out = model(_dev(x), _dev(bbox), {"intrinsic": _dev(intr)})
    b = batch()
    b["data"]["joints_cam"] /= 1000
    b["data"]["root_joint"] /= 1000
    total = model._calculate_loss(out, b["data"], b["cam_params"], mode="val")
    assert tuple(out["projected_joints_crop_img"].shape) == (B, V, 21, 2) and "val/g2d_loss" in model.last_losses
    assert total.item() == res["loss"].item()
    pj = out["projected_joints_crop_img"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(pj - proj) <= 2 * np.spacing(np.maximum(np.abs(proj), 1).astype(np.float32)))
    # targets synthesised in the kernel from the label joints: no "heatmap" key, the same loss
    model.heatmap_targets = "joints"
    syn = model.test_step(batch(heatmap=False), 0)
    # (the kernel's targets and the oracle's `heat` may differ in the last fp32 bit of isolated pixels, 6e-8 relative, and the
    # result is rounded to fp32 once more)
    assert abs(syn["loss"].item() - res["loss"].item()) <= 1e-6 * abs(res["loss"].item())
    model.heatmap_targets = "batch"
    # a batch without loss labels: "loss" None as before, and the same metrics as the step with them
    plain = model.test_step(batch(with_loss_labels=False), 0)
    assert plain["loss"] is None
    assert set(plain["metrics"]) == set(res["metrics"])
    for k, v in plain["metrics"].items():
        a, b2 = res["metrics"][k], v
        assert (a.item() == b2.item()) if isinstance(a, torch.Tensor) else (a == b2), k
    # "g2d" configured but no extrinsic: KeyError, like the reference
    bad = batch()
    del bad["cam_params"]["extrinsic"]
    with pytest.raises(KeyError):
        model.test_step(bad, 0)
