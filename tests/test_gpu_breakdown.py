"""The evaluation breakdown on the GPU (hmv_eval_breakdown_add, directly and through EpochEvaluator(breakdown=True, records=n) and
HandMvNet.evaluate) against
  (1) the numpy restatement of its state and record rows (tests/breakdown_oracle.py, pinned to the reference by test_breakdown_oracle.py),
  (2) the pooled state of the same steps (hmv_eval_add), which it must leave alone and add up to,
  (3) itself: other cuts into batches, a full view mask, a second run.

Tolerances: integer slices (header, H, CN, CV) exact; J3 / JPA / C2 within 2e-5 relative of the oracle, the project's bar for fp64
against fp32 distances (tests/test_gpu_metrics.py); fp64 sums of the same terms in another order within 1e-12; a record value within
1e-6 of the oracle's: at most five fp32 roundings inside a distance (2.1e-7, halved by the root for three of them) and one of the mean.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import breakdown_oracle as bo
from helpers import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(ROOT, "tests", "golden", "metrics_cases.npz"))
SMALL = ("noise_5mm", "similarity", "mirrored")     # 16 + 8 + 8 poses, thresholds 0 .. 0.02
V2 = 2
POISON = 777.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class _Labels:
    """Stands in for the model where only labels are fed (as in tests/test_gpu_eval_epoch.py); no step carries a loss."""
    auc_thresh = [0.0, 0.02]
    heatmap_targets = "batch"


def _invent(rng, p, g, V, masked):
    g2 = (rng.random((p.shape[0], V, 21, 2)) * 128).astype(np.float32)
    p2 = g2 + rng.standard_normal(g2.shape).astype(np.float32) * 2
    mask = rng.random((p.shape[0], V, 21)) < 0.2
    return dict(p=p, g=g, p2=p2, g2=g2, mask=mask if masked else None)


@functools.lru_cache(maxsize=None)
def _steps():
    """Built once and never written: many_poses as 1 + 2 + 5 + 1092 poses (the last above one workgroup's lanes and above four
    staged chunks), then the three small cases; invented 2D joints for two views; a joint mask on every other step."""
    rng = np.random.default_rng(47)
    cuts, at = [], 0
    for n in (1, 2, 5, 1092):
        cuts.append((FIX["many_poses.pred"][at:at + n], FIX["many_poses.gt"][at:at + n]))
        at += n
    cuts += [(FIX[f"{n}.pred"], FIX[f"{n}.gt"]) for n in SMALL]
    return [_invent(rng, p, g, V2, i % 2 == 0) for i, (p, g) in enumerate(cuts)]


@functools.lru_cache(maxsize=None)
def _oracle(first=0):
    """The oracle's state and record rows of _steps()[first:], computed once."""
    steps = _steps()[first:]
    state = bo.new_state(V2)
    for s in steps:
        bo.accumulate(state, s["p"], s["g"], s["p2"], s["g2"], s["mask"])
    rows = np.concatenate([bo.record_rows(s["p"], s["g"], s["p2"], s["g2"], s["mask"]) for s in steps])
    state.setflags(write=False)
    rows.setflags(write=False)
    return state, rows


def _feed(ev, steps):
    for s in steps:
        inputs = {"joints_cam": _dev(s["g"]), "joints_crop_img": _dev(s["g2"])}
        if s["mask"] is not None:
            inputs["joints_img_mask"] = _dev(s["mask"])
        ev.add({"joints_cam": _dev(s["p"]), "joints_crop_img": _dev(s["p2"])}, inputs, None)


def _add(s, state, records=None, base=0, present=None, steps=20, thr=(0.0, 0.02)):
    """One hmv_eval_breakdown_add on the current stream; returns the status.  The tensors live until the synchronising readback."""
    from handmvnet_amd import _lib
    B, V = s["p2"].shape[:2]
    t = [_dev(s[k]) for k in ("p", "g", "p2", "g2")]
    a = _lib.HmvEvalBreakdownArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvEvalBreakdownArgs)
    a.B, a.V, a.steps, a.thr_min, a.thr_max = B, V, steps, thr[0], thr[1]
    a.pred_joints_cam, a.gt_joints_cam, a.pred_joints_2d, a.gt_joints_2d = (x.data_ptr() for x in t)
    if s.get("mask") is not None:
        t.append(_dev(s["mask"].astype(np.uint8)))
        a.joints_mask = t[-1].data_ptr()
    if present is not None:
        t.append(_dev(np.asarray(present).astype(np.uint8)))
        a.view_present = t[-1].data_ptr()
    a.state, a.state_doubles = state.data_ptr(), state.numel()
    if records is not None:
        a.records, a.record_capacity, a.record_base = records.data_ptr(), records.shape[0], base
    rc = _lib.load().hmv_eval_breakdown_add(0, ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _zeros(V, steps=20):
    return torch.zeros(bo.doubles(V, steps), device="cuda:0", dtype=torch.float64)


def _table(rows, V):
    return torch.full((rows, 4 + V), POISON, device="cuda:0")


def _compare_state(got, want, V, steps=20):
    g, w = bo.slices(got, V, steps), bo.slices(want, V, steps)
    assert got[:4].tolist() == want[:4].tolist()
    for name in ("H", "CN", "CV"):
        assert np.array_equal(g[name], w[name]), name
    for name in ("J3", "JPA", "C2"):
        rel = np.abs(g[name] - w[name]) / np.where(w[name] > 0, w[name], 1.0)
        print(name, "worst relative difference", rel.max())
        assert rel.max() <= 2e-5, name
        assert ((g[name] == 0) == (w[name] == 0)).all(), name


def _compare_rows(got, want):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    rel = np.abs(got[ok] - want[ok]) / np.where(want[ok] > 0, want[ok], 1.0)
    print("records: worst relative difference", rel.max())
    assert rel.max() <= 1e-6


def test_state_and_records_match_the_oracle():
    from handmvnet_amd.evaluation import EpochEvaluator, finish_breakdown
    steps = _steps()
    ev = EpochEvaluator(_Labels(), "test", breakdown=True, records=1140)
    _feed(ev, steps)
    want_state, want_rows = _oracle()
    state = ev.breakdown_state.cpu().numpy()
    assert state[:4].tolist() == [1132, 7, V2, 20] and bo.slices(state, V2)["H"].sum() == 1132 * 21
    _compare_state(state, want_state, V2)
    table = ev.record_table.cpu().numpy()
    _compare_rows(table[:1132].astype(np.float64), want_rows)
    assert np.isnan(table[1132:]).all() and ev.record_rows == 1132
    rec = ev.records()
    assert set(rec) == {"mpjpe", "pa_mpjpe", "mpjpe2d", "views", "mpjpe2d_per_camera"} and rec["views"].tolist() == [V2] * 1132
    assert rec["mpjpe"] == pytest.approx(want_rows[:, 0] * 1000, rel=1e-6) and rec["mpjpe2d_per_camera"].shape == (1132, V2)
    got, want = ev.compute(), finish_breakdown(want_state, 0.0, 0.02, 20, "test")
    assert got["test_pck_per_joint"] == want["test_pck_per_joint"] and got["visible_joints"] == want["visible_joints"]
    assert got["test_mpjpe_per_joint"] == pytest.approx(want["test_mpjpe_per_joint"], rel=2e-5)
    assert got["test_mpjpe2d_visible_per_camera"] == pytest.approx(want["test_mpjpe2d_visible_per_camera"], rel=2e-5)
    assert got["samples"] == 1132 and "test_mpjpe" in got                       # the pooled keys are still there


def test_pooled_state_is_untouched_and_is_the_sum_of_the_breakdown():
    from handmvnet_amd.evaluation import EpochEvaluator
    steps = _steps()
    on, off = EpochEvaluator(_Labels(), "test", breakdown=True, records=1132), EpochEvaluator(_Labels(), "test")
    _feed(on, steps)
    _feed(off, steps)
    pooled = on.state.cpu().numpy()
    assert pooled.tobytes() == off.state.cpu().numpy().tobytes()
    assert off.breakdown_state is None and off.record_table is None
    s = bo.slices(on.breakdown_state.cpu().numpy(), V2)
    assert np.array_equal(s["H"].sum(0), pooled[14:])                           # exactly
    for mine, theirs in ((s["J3"].sum(), pooled[3]), (s["JPA"].sum(), pooled[4]), (s["C2"].sum(), pooled[6])):
        print(mine, theirs, abs(mine - theirs) / theirs)
        assert mine == pytest.approx(theirs, rel=1e-12)
    assert (s["CN"] == 1132).all() and s["CN"].sum() * 21 == pooled[5]
    assert not set(off.compute()) & {"test_mpjpe_per_joint", "camera_samples"} and "test_mpjpe_per_joint" in on.compute()


def test_the_cut_into_batches_does_not_matter():
    from handmvnet_amd.evaluation import EpochEvaluator
    small = _steps()[4:]
    whole = {k: np.concatenate([s[k] if s[k] is not None else np.zeros(s["p2"].shape[:3], bool) for s in small]) for k in ("p", "g", "p2", "g2", "mask")}
    assert whole["p"].shape[0] == 32
    states, tables = [], []
    for cut in ((1, 2, 29), (16, 16), (32,)):
        ev, at = EpochEvaluator(_Labels(), "val", breakdown=True, records=32), 0
        for n in cut:
            _feed(ev, [{k: v[at:at + n] for k, v in whole.items()}])
            at += n
        states.append(ev.breakdown_state.cpu().numpy())
        tables.append(ev.record_table.cpu().numpy())
        assert states[-1][:4].tolist() == [32, len(cut), V2, 20]
    for st, tb in zip(states[1:], tables[1:]):
        a, b = bo.slices(st, V2), bo.slices(states[0], V2)
        for name in ("H", "CN", "CV"):
            assert np.array_equal(a[name], b[name]), name
        for name in ("J3", "JPA", "C2"):
            assert np.allclose(a[name], b[name], rtol=1e-12, atol=0), name
        assert tb.tobytes() == tables[0].tobytes()                              # a row does not depend on its batch


def test_ragged_steps():
    rng = np.random.default_rng(48)
    s = _invent(rng, FIX["noise_5mm.pred"][:5], FIX["noise_5mm.gt"][:5], 3, True)
    plain, full = (_zeros(3), _table(5, 3)), (_zeros(3), _table(5, 3))
    assert _add(s, *plain) == 0 and _add(s, *full, present=np.ones((5, 3), bool)) == 0
    assert plain[0].cpu().numpy().tobytes() == full[0].cpu().numpy().tobytes()
    assert plain[1].cpu().numpy().tobytes() == full[1].cpu().numpy().tobytes()
    present = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 0, 1], [1, 1, 0]], bool)
    poisoned = dict(s, p2=s["p2"].copy(), g2=s["g2"].copy())
    poisoned["p2"][~present] = np.nan                                           # an absent slot is not read
    poisoned["g2"][~present] = np.nan
    state, table = _zeros(3), _table(5, 3)
    assert _add(poisoned, state, table, present=present) == 0
    want = bo.accumulate(bo.new_state(3), s["p"], s["g"], s["p2"], s["g2"], s["mask"], present)
    got = state.cpu().numpy()
    assert np.isfinite(got).all() and bo.slices(got, 3)["CN"].tolist() == [3, 3, 3]
    _compare_state(got, want, 3)
    rows = table.cpu().numpy().astype(np.float64)
    _compare_rows(rows, bo.record_rows(s["p"], s["g"], s["p2"], s["g2"], s["mask"], present))
    assert np.array_equal(np.isnan(rows[:, 4:]), ~present) and rows[:, 3].tolist() == [2, 1, 3, 1, 2]


@pytest.mark.parametrize("name, steps, thr", [("single_pose_7steps", 7, (0.0, 0.02)), ("noise_5mm", 1, (0.004, 0.02)), ("mirrored", 7, (0.001, 0.012))])
def test_one_view_and_other_step_counts(name, steps, thr):
    rng = np.random.default_rng(49)
    s = _invent(rng, FIX[f"{name}.pred"], FIX[f"{name}.gt"], 1, True)
    state, table = _zeros(1, steps), _table(s["p"].shape[0], 1)
    assert state.numel() == 4 + 42 + 21 * (steps + 1) + 43
    assert _add(s, state, table, steps=steps, thr=thr) == 0
    want = bo.accumulate(bo.new_state(1, steps), s["p"], s["g"], s["p2"], s["g2"], s["mask"], None, thr[0], thr[1], steps)
    got = state.cpu().numpy()
    assert got[:4].tolist() == [s["p"].shape[0], 1, 1, steps]
    _compare_state(got, want, 1, steps)
    _compare_rows(table.cpu().numpy().astype(np.float64), bo.record_rows(s["p"], s["g"], s["p2"], s["g2"], s["mask"]))


def test_records_land_at_record_base_and_nowhere_else():
    from handmvnet_amd import _lib
    from handmvnet_amd.evaluation import EpochEvaluator, worst
    small = _steps()[4:]                                                        # 16 + 8 + 8 samples
    state, table = _zeros(V2), _table(40, V2)
    base = 3
    for s in small:
        assert _add(s, state, table, base=base) == 0
        base += s["p"].shape[0]
    rows = table.cpu().numpy()
    assert (rows[:3] == POISON).all() and (rows[35:] == POISON).all() and not (rows[3:35] == POISON).any()
    want = _oracle(4)[1]
    _compare_rows(rows[3:35].astype(np.float64), want)
    before = (state.cpu().numpy().tobytes(), rows.tobytes())
    assert _add(small[1], state, table, base=33) == _lib.HMV_ERR_ARG            # 33 + 8 > 40
    assert "exceeds record_capacity" in _lib.load().hmv_last_error(None).decode()
    assert (state.cpu().numpy().tobytes(), table.cpu().numpy().tobytes()) == before
    assert _add(small[1], state, table, base=32) == 0                           # the last row that fits
    # through the evaluator: the same rows, and the worst of them
    ev = EpochEvaluator(_Labels(), "test", records=32)                          # records alone run the launch as well
    _feed(ev, small)
    rec = ev.records()
    assert ev.record_table.cpu().numpy().tobytes() == rows[3:35].tobytes()
    for key, col in (("mpjpe", 0), ("pa_mpjpe", 1), ("mpjpe2d", 2)):
        assert worst(rec, key, 5) == np.argsort(-want[:, col], kind="stable")[:5].tolist(), key
    assert "test_mpjpe_per_joint" not in ev.compute()
    with pytest.raises(ValueError, match="record rows"):
        _feed(ev, small[:1])
    ev.reset()
    assert ev.record_rows == 0 and np.isnan(ev.record_table.cpu().numpy()).all() and not ev.breakdown_state.cpu().numpy().any()


def test_two_runs_give_the_same_bytes():
    from handmvnet_amd.evaluation import EpochEvaluator
    steps = _steps()[3:]                                                        # 1092, 16, 8, 8 poses
    runs = []
    for _ in range(2):
        ev = EpochEvaluator(_Labels(), "test", breakdown=True, records=1124)
        _feed(ev, steps)
        runs.append((ev.breakdown_state.cpu().numpy().tobytes(), ev.record_table.cpu().numpy().tobytes(), ev.state.cpu().numpy().tobytes()))
        _ = torch.randn(128, 128, device="cuda:0") @ torch.randn(128, 128, device="cuda:0")     # unrelated work in between
    assert runs[0] == runs[1]


@functools.lru_cache(maxsize=None)
def _tiny():
    """tiny_r18, the smallest configuration tests/golden/cases.py holds (two views, 64 x 64), and three label-only steps around its own
    predictions as host arrays (never written)."""
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.synth import synth_inputs
    cfg, (tp, mp, dp), sd, _, _ = load_case("tiny_r18")
    model = HandMvNet(dict(tp, mask_invisible_joints=True), mp, dp)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    x, bbox, intr = synth_inputs(cfg, 3, 12, 64)
    own = {k: v.cpu().numpy() for k, v in model(_dev(x), _dev(bbox), {"intrinsic": _dev(intr)}).items()}
    rng = np.random.default_rng(50)
    steps = []
    for sl, noise in ((slice(0, 2), 0.006), (slice(2, 3), 0.003), (slice(0, 3), 0.012)):
        cam, crop = own["joints_cam"][sl], own["joints_crop_img"][sl]
        steps.append(dict(rgb=x[sl], bboxes=bbox[sl], intr=intr[sl], pred_cam=cam, pred_crop=crop,
                          gt_crop=(crop + rng.standard_normal(crop.shape) * 2).astype(np.float32),
                          gt_cam_mm=((cam + rng.standard_normal(cam.shape) * noise) * 1000).astype(np.float32),
                          mask=rng.random(crop.shape[:3]) < 0.2))
    return model, steps


def _batch(d):
    return {"data": {"rgb": _dev(d["rgb"]), "bboxes": _dev(d["bboxes"]), "joints_cam": _dev(d["gt_cam_mm"]),
                     "joints_crop_img": _dev(d["gt_crop"]), "joints_img_mask": _dev(d["mask"])}, "cam_params": {"intrinsic": _dev(d["intr"])}}


def test_evaluate_end_to_end():
    from handmvnet_amd.evaluation import finish_breakdown, worst
    model, steps = _tiny()
    plain = model.evaluate([_batch(d) for d in steps])
    got = model.evaluate([_batch(d) for d in steps], breakdown=True, records=6)
    assert {k: got[k] for k in plain} == plain and "records" not in plain and "test_mpjpe_per_joint" not in plain
    # the loop users run today: test_step per batch, the outputs read back, the numpy breakdown on them
    want_state, want_rows, per_step = bo.new_state(2), [], []
    lo, hi = (float(t) for t in model.auc_thresh)                              # the thresholds of the case's data set
    for d in steps:
        b = _batch(d)
        per_step.append((d["rgb"].shape[0], model.test_step(b, 0)["metrics"]))
        out = model(b["data"]["rgb"], b["data"]["bboxes"], b["cam_params"])
        cam, crop = out["joints_cam"].cpu().numpy(), out["joints_crop_img"].cpu().numpy()
        gt_cam = b["data"]["joints_cam"].cpu().numpy()                         # metres by now: test_step converted it in place
        bo.accumulate(want_state, cam, gt_cam, crop, d["gt_crop"], d["mask"], None, lo, hi)
        want_rows.append(bo.record_rows(cam, gt_cam, crop, d["gt_crop"], d["mask"]))
    want, want_rows = finish_breakdown(want_state, lo, hi, 20, "test"), np.concatenate(want_rows)
    n = sum(b for b, _ in per_step)
    for key in ("test_mpjpe", "test_pa_mpjpe", "test_mpjpe2d"):
        assert got[key] == pytest.approx(sum(b * float(m[key]) for b, m in per_step) / n, rel=1e-6), key
    assert got["test_pck_per_joint"] == want["test_pck_per_joint"] and got["camera_samples"] == [6, 6]
    assert got["visible_joints"] == want["visible_joints"]
    for key in ("test_mpjpe_per_joint", "test_pa_mpjpe_per_joint", "test_auc_per_joint", "test_mpjpe2d_per_camera",
                "test_mpjpe2d_visible_per_camera"):
        print(key, got[key], want[key])
        assert got[key] == pytest.approx(want[key], rel=1e-6), key
    for key in ("test_mpjpe2d_per_camera_joint", "test_mpjpe2d_visible_per_camera_joint"):
        assert np.allclose(np.array(got[key], np.float64), np.array(want[key], np.float64), rtol=1e-6, atol=0), key
    assert np.mean(got["test_mpjpe_per_joint"]) == pytest.approx(got["test_mpjpe"], rel=1e-12)
    rec = got["records"]
    assert rec["views"].tolist() == [2] * 6 and rec["mpjpe2d_per_camera"].shape == (6, 2)
    assert rec["mpjpe"] == pytest.approx(want_rows[:, 0] * 1000, rel=1e-6) and rec["pa_mpjpe"] == pytest.approx(want_rows[:, 1] * 1000, rel=1e-6)
    assert rec["mpjpe2d"] == pytest.approx(want_rows[:, 2], rel=1e-6)
    assert worst(rec, "mpjpe", 3) == np.argsort(-want_rows[:, 0], kind="stable")[:3].tolist()
    only = model.evaluate([_batch(d) for d in steps], mode="val", records=6)
    assert "val_mpjpe_per_joint" not in only and only["records"]["mpjpe"].tolist() == rec["mpjpe"].tolist()


def test_a_step_with_other_views_raises_before_anything_is_launched():
    from handmvnet_amd.evaluation import EpochEvaluator
    rng = np.random.default_rng(51)
    steps = _steps()
    ev = EpochEvaluator(_Labels(), "test", breakdown=True, records=64)
    _feed(ev, steps[4:6])
    before = (ev.state.cpu().numpy().tobytes(), ev.breakdown_state.cpu().numpy().tobytes(), ev.record_table.cpu().numpy().tobytes())
    with pytest.raises(ValueError, match="2 views, the step has 3"):
        _feed(ev, [_invent(rng, FIX["mirrored.pred"], FIX["mirrored.gt"], 3, True)])
    torch.cuda.synchronize()
    assert (ev.state.cpu().numpy().tobytes(), ev.breakdown_state.cpu().numpy().tobytes(), ev.record_table.cpu().numpy().tobytes()) == before
    assert ev.record_rows == 24 and ev.compute()["samples"] == 24
    plain = EpochEvaluator(_Labels(), "test")                                   # without the switch V may change, as it always could
    _feed(plain, [steps[4], _invent(rng, FIX["mirrored.pred"], FIX["mirrored.gt"], 3, True)])
    assert plain.compute()["samples"] == 24
