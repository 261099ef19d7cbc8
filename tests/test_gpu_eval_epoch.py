"""The evaluation epoch on the GPU (hmv_eval_add through handmvnet_amd.evaluation.EpochEvaluator and HandMvNet.evaluate) against
  (1) the numpy restatement of its state (tests/epoch_oracle.py, built on oracle.metrics_oracle),
  (2) itself under other cuts of the same poses into batches,
  (3) the per-step results of the existing test_step, weighted by batch size.

Tolerances: PCK values, thresholds and histogram counts are exact (fp32 comparisons of fp32 distances, integer counts); mpjpe /
pa_mpjpe / mpjpe2d within 2e-5 relative of the oracle (the bar tests/test_gpu_metrics.py derives for fp64 against fp32 summation);
fp64 sums of the same terms in another order within 1e-12; against per-step values that were each rounded to fp32 once (6e-8),
1e-6.
"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

import epoch_oracle as eo
import loss_oracle as lo
from helpers import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(ROOT, "tests", "golden", "metrics_cases.npz"))
SMALL = ("noise_5mm", "similarity", "mirrored")     # 16 + 8 + 8 poses, thresholds 0 .. 0.02
V2 = 2                                               # views of the invented 2D joints


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class _Labels:
    """Stands in for the model where only labels are fed: dexycb thresholds, and a 'loss' that is whatever the step carries."""
    auc_thresh = [0.0, 0.02]
    heatmap_targets = "batch"

    def _calculate_loss(self, out, inputs, cam_params, mode="test"):
        self.last_loss_vector = inputs["heatmap"]    # the step's invented device float[6]


@functools.lru_cache(maxsize=None)
def _steps():
    """The steps of the oracle test, built once and never written: many_poses as 1 + 2 + 5 + 1092 poses (the last larger than the
    workgroup), then the three small cases; invented 2D joints, ~20 % of them masked; every other step carries a loss vector."""
    rng = np.random.default_rng(31)
    cuts, at = [], 0
    for n in (1, 2, 5, 1092):
        cuts.append((FIX["many_poses.pred"][at:at + n], FIX["many_poses.gt"][at:at + n]))
        at += n
    assert at == FIX["many_poses.pred"].shape[0] == 1100
    cuts += [(FIX[f"{n}.pred"], FIX[f"{n}.gt"]) for n in SMALL]
    steps = []
    for i, (p, g) in enumerate(cuts):
        g2 = (rng.random((p.shape[0], V2, 21, 2)) * 128).astype(np.float32)
        p2 = g2 + rng.standard_normal(g2.shape).astype(np.float32) * 2
        mask = rng.random((p.shape[0], V2, 21)) < 0.2
        loss = (rng.random(6) * 10).astype(np.float32) if i % 2 == 0 else None
        steps.append(dict(p=p, g=g, p2=p2, g2=g2, mask=mask, loss=loss))
    return steps


def _feed(ev, steps, with_mask=True):
    for s in steps:
        inputs = {"joints_cam": _dev(s["g"]), "joints_crop_img": _dev(s["g2"])}
        if with_mask:
            inputs["joints_img_mask"] = _dev(s["mask"])
        if s.get("loss") is not None:
            inputs["heatmap"] = _dev(s["loss"])
        ev.add({"joints_cam": _dev(s["p"]), "joints_crop_img": _dev(s["p2"])}, inputs, None)


def test_epoch_matches_the_oracle():
    from handmvnet_amd.evaluation import EpochEvaluator
    steps = _steps()
    ev = EpochEvaluator(_Labels(), "test")
    _feed(ev, steps)
    got = ev.compute()
    state = ev.state.cpu().numpy()
    want_state = eo.new_state(20)
    for s in steps:
        loss = dict(zip(lo.TERMS, s["loss"])) if s["loss"] is not None else None
        eo.accumulate(want_state, s["p"], s["g"], s["p2"], s["g2"], s["mask"], loss)
    want = eo.finish(want_state)
    print({k: got[k] for k in ("test_mpjpe", "test_pa_mpjpe", "test_mpjpe2d", "test_auc_j")}, want["mpjpe"], want["pa_mpjpe"], want["mpjpe2d"])
    assert got["samples"] == want["samples"] == 1132 and got["steps"] == want["steps"] == 7
    assert np.array_equal(state[[0, 1, 2, 5, 7]], want_state[[0, 1, 2, 5, 7]])
    assert np.array_equal(state[14:].astype(np.int64), want_state[14:].astype(np.int64)) and np.all(state[14:] == np.round(state[14:]))
    assert state[14:].sum() == 1132 * 21
    assert got["test_mpjpe"] == pytest.approx(want["mpjpe"], rel=2e-5)
    assert got["test_pa_mpjpe"] == pytest.approx(want["pa_mpjpe"], rel=2e-5)
    assert got["test_mpjpe2d"] == pytest.approx(want["mpjpe2d"], rel=2e-5)
    assert np.array_equal(np.array(got["test_pck_j"], np.float32), want["pck"])
    assert np.array_equal(np.array(got["thresholds"], np.float32), want["thr"])
    assert got["test_auc_j"] == pytest.approx(want["auc"], rel=1e-6) and got["test_norm_auc_j"] == pytest.approx(want["norm_auc"], rel=1e-6)
    for term in lo.TERMS:                       # B x an fp32 value, summed in fp64 on both sides
        assert got[f"test/{term}"] == pytest.approx(want[term], rel=1e-12), term
    assert got["test/root_3d_loss"] == 0.0
    # without a mask every 2D joint counts with its distance
    plain = EpochEvaluator(_Labels(), "test")
    _feed(plain, steps[4:], with_mask=False)
    ps, ws = plain.state.cpu().numpy(), eo.new_state(20)
    for s in steps[4:]:
        eo.accumulate(ws, s["p"], s["g"], s["p2"], s["g2"], None, None)
    assert ps[6] == pytest.approx(ws[6], rel=2e-5) and ps[5] == ws[5] == 32 * V2 * 21


def test_the_cut_into_batches_does_not_matter():
    from handmvnet_amd.evaluation import EpochEvaluator
    whole = {k: np.concatenate([s[k] for s in _steps()[4:]]) for k in ("p", "g", "p2", "g2", "mask")}
    assert whole["p"].shape[0] == 32
    states = []
    for cut in ((1, 2, 29), (16, 16), (32,)):
        ev, at = EpochEvaluator(_Labels(), "val"), 0
        for n in cut:
            _feed(ev, [{k: v[at:at + n] for k, v in whole.items()}])
            at += n
        states.append(ev.state.cpu().numpy())
        assert states[-1][0] == 32 and states[-1][1] == len(cut)
    for s in states[1:]:
        assert np.array_equal(s[14:], states[0][14:])                       # the histogram: identical
        assert np.array_equal(s[[0, 2, 5]], states[0][[0, 2, 5]])
        assert np.allclose(s[[3, 4, 6]], states[0][[3, 4, 6]], rtol=1e-12, atol=0)


@functools.lru_cache(maxsize=None)
def _cfg1():
    """cfg1_r50_v4_128 built as tests/test_gpu_losses.py::test_evaluation_step_returns_the_loss builds it, its labels for B = 2 and
    the three steps of the end-to-end tests as host arrays (never written)."""
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.losses import target_heatmaps
    from handmvnet_amd.synth import synth_inputs
    cfg, (tp, mp, dp), sd, _, _ = load_case("cfg1_r50_v4_128")
    weights = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}
    tp = dict(tp, loss_weights=weights, mask_invisible_joints=True)
    model = HandMvNet(tp, mp, dp)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    B, S, hs = 2, dp["image_size"], dp["heatmap_size"]
    x, bbox, intr = synth_inputs(cfg, B, 13, 128)
    c = lo.loss_case("iii_9x13")
    assert c["V"] == x.shape[1] == 4
    extr, root_mm = np.repeat(c["extr"][:1], B, 0), np.repeat(c["root_joint"][:1] * 1000, B, 0).astype(np.float32)
    own = model(_dev(x), _dev(bbox), {"intrinsic": _dev(intr)})
    own = {k: v.cpu().numpy() for k, v in own.items()}
    rng = np.random.default_rng(7)
    steps = []
    for sl, with_loss, noise in ((slice(0, 2), True, 0.006), (slice(1, 2), True, 0.003), (slice(0, 2), False, 0.012)):
        cam = own["joints_cam"][sl]
        crop = own["joints_crop_img"][sl]
        gt_crop = np.clip(crop + rng.standard_normal(crop.shape) * 2, -5, S + 5).astype(np.float32)
        d = dict(rgb=x[sl], bboxes=bbox[sl], intr=intr[sl], extr=extr[sl], root_mm=root_mm[sl], gt_crop=gt_crop,
                 gt_cam_mm=((cam + rng.standard_normal(cam.shape) * noise) * 1000).astype(np.float32),
                 mask=rng.random(crop.shape[:3]) < 0.2, with_loss=with_loss, root_idx=c["root_idx"])
        d["heat"] = target_heatmaps(_dev(gt_crop), S, hs).cpu().numpy()
        steps.append(d)
    return model, steps


def _batch(d, root_idx_as_tensor=False):
    """A fresh device-resident batch of one step (the step converts its labels in place)."""
    data = {"rgb": _dev(d["rgb"]), "bboxes": _dev(d["bboxes"]), "joints_cam": _dev(d["gt_cam_mm"]), "root_joint": _dev(d["root_mm"]),
            "joints_crop_img": _dev(d["gt_crop"]), "joints_img_mask": _dev(d["mask"])}
    cam = {"intrinsic": _dev(d["intr"])}
    if d["with_loss"]:
        data["root_idx"] = torch.tensor([d["root_idx"]]) if root_idx_as_tensor else int(d["root_idx"])
        data["heatmap"] = _dev(d["heat"])
        cam["extrinsic"] = _dev(d["extr"])
    return {"data": data, "cam_params": cam}


def test_epoch_equals_the_weighted_mean_of_test_steps():
    from handmvnet_amd.evaluation import EpochEvaluator
    model, steps = _cfg1()
    ev = EpochEvaluator(model, "test")
    mine = [_batch(d) for d in steps]
    for b in mine:
        out = ev.step(b)
        assert set(out) >= {"joints_cam", "joints_crop_img", "heatmap"}
    got = ev.compute()
    for b, d in zip(mine, steps):                                    # converted to metres in place, like the reference
        assert np.allclose(b["data"]["joints_cam"].cpu().numpy(), d["gt_cam_mm"] / np.float32(1000), rtol=1e-6)
        assert np.allclose(b["data"]["root_joint"].cpu().numpy(), d["root_mm"] / np.float32(1000), rtol=1e-6)
    # the parent's loop on fresh copies of the same batches
    per_step = []
    for d in steps:
        r = model.test_step(_batch(d, root_idx_as_tensor=True), 0)
        assert (r["loss"] is not None) == d["with_loss"]
        per_step.append((d["rgb"].shape[0], r["metrics"], dict(model.last_losses) if d["with_loss"] else None))
    n = sum(b for b, _, _ in per_step)
    assert got["samples"] == n == 5 and got["steps"] == 3
    for key in ("test_mpjpe", "test_pa_mpjpe", "test_mpjpe2d"):
        want = sum(b * float(m[key]) for b, m, _ in per_step) / n
        print(key, got[key], want)
        assert got[key] == pytest.approx(want, rel=1e-6), key
    counts = sum(np.round(np.array(m["test_pck_j"], np.float64) * b * 21) for b, m, _ in per_step)   # already cumulative per step
    assert np.array_equal(np.array(got["test_pck_j"], np.float32), counts.astype(np.float32) / np.float32(n * 21))
    assert 0 < got["test_pck_j"][-1] <= 1 and got["test_auc_j"] > 0
    n_loss = sum(b for b, _, l in per_step if l is not None)
    assert n_loss == 3
    for term in lo.TERMS:
        want = sum(b * float(l[f"test/{term}"]) for b, _, l in per_step if l is not None) / n_loss
        assert got[f"test/{term}"] == pytest.approx(want, rel=1e-12), term
    assert got["test/root_3d_loss"] == 0.0
    # the loop itself: HandMvNet.evaluate is step, step, step, compute
    assert model.evaluate([_batch(d) for d in steps], mode="test") == got
    val = model.evaluate([_batch(d) for d in steps[:1]], mode="val")
    assert val["val_mpjpe"] == pytest.approx(float(per_step[0][1]["test_mpjpe"]), rel=1e-6) and "val/loss" in val


def test_steps_make_no_host_round_trip():
    """Two add calls and one step under torch's sync debug mode: any synchronising call raises.  The C entry is checked by reading."""
    from handmvnet_amd.evaluation import EpochEvaluator
    src = open(os.path.join(ROOT, "handmvnet_amd", "csrc", "eval_epoch.hip")).read()
    assert "hipMemcpy" not in src and "Synchronize" not in src
    model, steps = _cfg1()
    ev = EpochEvaluator(model, "test")
    ev.step(_batch(steps[0]))                                                 # warm up: engine, code objects, the state
    torch.cuda.synchronize()
    batches = [_batch(steps[0]), _batch(steps[1], root_idx_as_tensor=True), _batch(steps[2])]
    outs = []
    for b in batches[:2]:                                                     # what add() is handed: a forward and labels in metres
        outs.append(model(b["data"]["rgb"], b["data"]["bboxes"], b["cam_params"]))
        b["data"]["joints_cam"] /= 1000
        b["data"]["root_joint"] /= 1000
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except (NotImplementedError, RuntimeError) as e:
        print(f"sync debug mode is not available in this build ({e!r}): the round-trip assertion is skipped")
        return
    try:
        ev.add(outs[0], batches[0]["data"], batches[0]["cam_params"])
        ev.add(outs[1], batches[1]["data"], batches[1]["cam_params"])
        ev.step(batches[2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = ev.compute()
    assert got["samples"] == 2 + 2 + 1 + 2 and got["steps"] == 4


def test_determinism_reset_and_streams():
    from handmvnet_amd.evaluation import EpochEvaluator
    steps = _steps()[3:]                                                      # 1092, 16, 8, 8 poses
    ev = EpochEvaluator(_Labels(), "test")
    _feed(ev, steps)
    first = ev.state.cpu().numpy().copy()
    ev.reset()
    assert not ev.state.cpu().numpy().any()
    with pytest.raises(ValueError, match="empty epoch"):
        ev.compute()
    x = torch.randn(256, 256, device="cuda:0")
    y = x @ x                                                                 # unrelated work on the stream in between
    _feed(ev, steps)
    assert ev.state.cpu().numpy().tobytes() == first.tobytes() and torch.isfinite(y).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = EpochEvaluator(_Labels(), "test")
        _feed(other, steps)
        got = other.state.cpu().numpy()
    torch.cuda.synchronize()
    assert got.tobytes() == first.tobytes()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_reduce_over_rccl_world_of_one():
    from handmvnet_amd.evaluation import EpochEvaluator
    ev = EpochEvaluator(_Labels(), "test")
    _feed(ev, _steps()[4:])
    before = ev.state.cpu().numpy().copy()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        ev.reduce()
        torch.cuda.synchronize()
        assert ev.state.cpu().numpy().tobytes() == before.tobytes()
        idle = EpochEvaluator(_Labels(), "test")                              # a rank without batches still joins the collective
        idle.reduce()
        assert idle.state.is_cuda and not idle.state.cpu().numpy().any()
    finally:
        dist.destroy_process_group()
