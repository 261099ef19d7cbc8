"""Absolute evaluation on the GPU: hmv_eval_absolute_add against tests/absolute_epoch_oracle.py on golden/absolute_epoch_cases.npz,
then forward_absolute(details=True), EpochEvaluator(absolute=...) and HandMvNet.evaluate(absolute=...).

The bar for a sum: 2^-21 relative of the oracle's.  The oracle makes the kernel's two fp32 sums itself, the difference of two nearby
fp32 values is exact, so only the fp32 norm differs from float64: three multiplies, two adds and a square root stay under 3 ulp, one
bit is kept in hand; the fp64 accumulation adds nothing at that level.  Counts, the histogram and [0 .. 3] are exact.  Every raw call
runs on guarded buffers (tests/guards.py) with a state of exactly 156 + 3 V doubles.  Measured margins: DESIGN.md "Absolute evaluation"."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import absolute_epoch_oracle as ao
import triangulation_oracle as to
from guards import Guards
from helpers import load_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "absolute_epoch_cases.npz"))
KEYS = ("pred_cam", "tri", "status", "gt_cam", "gt_root", "reproj", "inliers")
DEV = torch.device("cuda:0")
BAR = 2.0 ** -21
SENTINEL = -12345.5
SUMS, COUNTS = ("W", "T", "R"), ("TN", "S", "RN", "H")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def case(name, lo=None, hi=None):
    return {k: FIX[f"{name}.{k}"][lo:hi] for k in KEYS}


def guarded_state(g, V, seed=None):
    state = g.out(ao.doubles(V), torch.float64)
    state.zero_()
    if seed is not None:
        state.copy_(_t(seed))
    return state


def add(g, c, state, V=None, reproj=True, inliers=True, v_checked=0):
    """One hmv_eval_absolute_add from numpy arrays on guarded device buffers; returns the status."""
    from handmvnet_amd import _lib
    a = _lib.HmvEvalAbsoluteArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvEvalAbsoluteArgs)
    a.B, a.V, a.v_checked = c["tri"].shape[0], c["reproj"].shape[1] if V is None else V, v_checked
    a.pred_joints_cam, a.joints_tri = g.inp(_t(c["pred_cam"])).data_ptr(), g.inp(_t(c["tri"])).data_ptr()
    a.tri_status = g.inp(_t(c["status"].astype(np.int32))).data_ptr()
    a.gt_joints_cam, a.gt_root = g.inp(_t(c["gt_cam"])).data_ptr(), g.inp(_t(c["gt_root"])).data_ptr()
    if reproj:
        a.reproj_err = g.inp(_t(c["reproj"][:, :a.V])).data_ptr()
    if inliers:
        a.inliers = g.inp(_t(c["inliers"].astype(np.int32))).data_ptr()
    a.state, a.state_doubles = state.data_ptr(), state.numel()
    rc = _lib.load().hmv_eval_absolute_add(0, ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc


def feed(name, cut, **kw):
    """The case in steps of `cut` rows through the entry, everything guarded; returns the state on the host."""
    V = FIX[f"{name}.reproj"].shape[1]
    g = Guards(DEV)
    state, at = guarded_state(g, V), 0
    for n in cut:
        assert add(g, case(name, at, at + n), state, **kw) == 0
        at += n
    g.check()
    return state.cpu().numpy()


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = case(name)
    state = ao.accumulate(ao.new_state(c["reproj"].shape[1]), *(c[k] for k in KEYS))
    state.setflags(write=False)
    return state


def worst_ratio(got, want, V):
    """Counts exact; returns the largest relative difference of a sum over the bar."""
    assert got[:4].tolist() == want[:4].tolist() and got[6:8].tolist() == [0, 0]
    g, w = ao.slices(got, V), ao.slices(want, V)
    for name in COUNTS:
        assert np.array_equal(g[name], w[name]), name
    worst = 0.0
    for name, a, b in [("[4]", got[4:5], want[4:5]), ("[5]", got[5:6], want[5:6])] + [(n, g[n], w[n]) for n in SUMS]:
        assert np.isfinite(a).all() and ((a == 0) == (b == 0)).all(), name
        rel = np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0)
        print(f"{name}: worst relative difference {rel.max():.3e} = {rel.max() / BAR:.3f} of the bar")
        worst = max(worst, rel.max() / BAR)
    return worst


# ---------------------------------------------------------------- 1. the state against the oracle, 2. on guarded buffers
@pytest.mark.parametrize("name", ["plain", "mixed", "one", "wide"])
def test_state_matches_the_oracle(name):
    B, V = FIX[f"{name}.reproj"].shape[:2]
    got = feed(name, (B,))
    assert got[:3].tolist() == [B, 1, V]
    ratio = worst_ratio(got, oracle(name), V)
    print(f"{name}: largest ratio to the 2^-21 bar {ratio:.3f}")
    assert ratio <= 1.0
    if name == "mixed":
        assert got[3] == FIX["mixed.located"] and got[0] - got[3] == FIX["mixed.lost"]
        assert np.array_equal(ao.slices(got, V)["S"], FIX["mixed.status_counts"]) and np.array_equal(ao.slices(got, V)["H"], FIX["mixed.inlier_hist"])


@pytest.mark.parametrize("name", ["mixed", "wide"])
def test_null_tables_leave_their_slices_alone(name):
    B, V = FIX[f"{name}.reproj"].shape[:2]
    seed = np.zeros(ao.doubles(V))
    seed[155:] = SENTINEL
    want = oracle(name)
    for reproj, inliers in ((False, False), (True, False), (False, True)):
        g = Guards(DEV)
        state = guarded_state(g, V, seed)
        assert add(g, case(name), state, reproj=reproj, inliers=inliers) == 0
        g.check()
        got = state.cpu().numpy()
        tail = got[155:].copy()
        if reproj:
            assert np.array_equal(tail[V:2 * V], want[155 + V:155 + 2 * V] + SENTINEL)      # RN: integers, exact
            tail[:2 * V] = SENTINEL
        if inliers:
            assert np.array_equal(tail[2 * V:], want[155 + 2 * V:] + SENTINEL)
            tail[2 * V:] = SENTINEL
        assert tail.tobytes() == seed[155:].tobytes(), (reproj, inliers)
        assert got[:155].tobytes() == feed(name, (B,))[:155].tobytes()                      # the fixed part does not depend on them


# ---------------------------------------------------------------- 3. the cut does not matter
def test_the_cut_does_not_matter_and_two_feeds_give_the_same_bytes():
    whole, cut = feed("wide", (13,)), feed("wide", (1, 5, 7))
    assert whole[:3].tolist() == [13, 1, 16] and cut[:3].tolist() == [13, 3, 16] and whole[3] == cut[3]
    a, b = ao.slices(whole, 16), ao.slices(cut, 16)
    for name in COUNTS:
        assert np.array_equal(a[name], b[name]), name
    assert np.allclose(whole[4:6], cut[4:6], rtol=1e-12, atol=0)
    for name in SUMS:
        assert np.allclose(a[name], b[name], rtol=1e-12, atol=0), name
    assert feed("wide", (1, 5, 7)).tobytes() == cut.tobytes() and feed("wide", (13,)).tobytes() == whole.tobytes()


# ---------------------------------------------------------------- 4. V is pinned
def test_a_step_with_another_v_is_refused_and_the_state_keeps_its_bytes():
    from handmvnet_amd import _lib
    g = Guards(DEV)
    state = guarded_state(g, 3)
    assert add(g, case("plain"), state) == 0
    before = state.cpu().numpy().tobytes()
    assert add(g, case("plain"), state, V=2) == _lib.HMV_ERR_ARG
    assert "state[2]" in _lib.load().hmv_last_error(None).decode()
    assert state.cpu().numpy().tobytes() == before
    # a caller that vouches for V is not checked on the host; the kernel still writes nothing to a state begun with another V
    assert add(g, case("plain"), state, V=2, v_checked=1) == 0
    assert state.cpu().numpy().tobytes() == before
    assert add(g, case("plain"), state, v_checked=1) == 0 and state.cpu().numpy()[:3].tolist() == [10, 2, 3]
    assert add(g, case("plain"), state) == 0 and state.cpu().numpy()[:3].tolist() == [15, 3, 3]
    g.check()


def test_a_vouched_feed_has_the_bytes_of_a_checked_one():
    assert feed("wide", (1, 5, 7), v_checked=1).tobytes() == feed("wide", (1, 5, 7)).tobytes()
    assert feed("mixed", (2, 3), v_checked=1).tobytes() == feed("mixed", (2, 3)).tobytes()


# ---------------------------------------------------------------- 5 .. 8. the model
@functools.lru_cache(maxsize=None)
def _tiny():
    """tiny_r18 (V = 2, 64 x 64) and two sets of synthetic inputs, of 3 and of 2 samples, each with a rigid rig in metres; device
    tensors, never written (the recipe of tests/test_gpu_triangulation.py)."""
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.synth import synth_inputs
    cfg, (tp, mp, dp), sd, _, _ = load_case("tiny_r18")
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    sets = []
    for B, seed in ((3, 3), (2, 4)):
        x, bbox, intr = (_t(a).to(DEV) for a in synth_inputs(cfg, B, 12, 64))
        E, _ = to.ring_rig(np.random.default_rng(seed), B, cfg.num_views)
        sets.append((x, bbox, {"intrinsic": intr, "extrinsic": _t(E).to(DEV)}))
    return m, sets


def _bits(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _batch(m, x, bbox, cp, seed=5, view_mask=None):
    """Labels in mm around the model's own predictions, with the label root where the triangulated one is (fresh tensors: a step
    converts them in place)."""
    rng = np.random.default_rng(seed)
    B = x.shape[0]
    own = m(x, bbox, cp)
    gt_cam = (_bits(own["joints_cam"]) + rng.standard_normal((B, 21, 3)) * 0.005) * 1000
    data = {"rgb": x, "bboxes": bbox, "joints_cam": _t(gt_cam.astype(np.float32)).to(DEV),
            "root_joint": _t((rng.uniform(-0.1, 0.1, (B, 1, 3)) + [0, 0, 1.2]).astype(np.float32) * 1000).to(DEV),
            "joints_crop_img": (own["joints_crop_img"] + 1.5).clone()}
    batch = {"data": data, "cam_params": cp}
    if view_mask is not None:
        batch["view_mask"] = view_mask
    return batch


def _batches(m, sets):
    return [_batch(m, *s, seed=5 + i) for i, s in enumerate(sets)]


def test_forward_absolute_details_adds_two_outputs_and_no_launch():
    from handmvnet_amd.triangulation import triangulate
    m, sets = _tiny()
    x, bbox, cp = sets[0]
    plain = {k: v.clone() for k, v in m.forward_absolute(x, bbox, cp).items()}
    n = m.launch_count()
    out = m.forward_absolute(x, bbox, cp, details=True)
    assert m.launch_count() == n
    assert set(out) == set(plain) | {"tri_reproj", "tri_inliers"}
    for k in plain:
        assert same_bits(_bits(out[k]), _bits(plain[k])), k
    res = triangulate(out["joints_crop_img"], cp["intrinsic"], cp["extrinsic"], bbox=bbox, image_size=m.data_params["image_size"],
                      frame_cam=0, return_details=True)
    assert out["tri_reproj"].shape == (3, 2, 21) and out["tri_reproj"].dtype == torch.float32
    assert out["tri_inliers"].shape == (3, 21) and out["tri_inliers"].dtype == torch.int32
    assert same_bits(_bits(out["tri_reproj"]), _bits(res["reproj_err"])) and same_bits(_bits(out["tri_inliers"]), _bits(res["inliers"]))
    assert same_bits(_bits(out["joints_tri"]), _bits(res["points3d"]))
    gated = m.forward_absolute(x, bbox, cp, confidence=0.3, details=True)         # with the confidence gate as well
    assert {"tri_reproj", "tri_inliers", "tri_views"} <= set(gated)


def test_evaluate_absolute_end_to_end():
    from handmvnet_amd.evaluation import EpochEvaluator, absolute_doubles, breakdown_doubles
    m, sets = _tiny()
    plain = m.evaluate(_batches(m, sets))
    got = m.evaluate(_batches(m, sets), absolute=True)
    assert got["lost"] == 0 and got["located"] == 5          # the condition under which the next bar means anything
    per_step = []
    m.absolute_root = "triangulate"
    try:
        for b in _batches(m, sets):
            per_step.append((b["data"]["rgb"].shape[0], m.test_step(b)["metrics"]))
    finally:
        m.absolute_root = None
    n = sum(b for b, _ in per_step)
    for key in ("test_w_mpjpe", "test_root_err"):
        want = sum(b * float(s[key]) for b, s in per_step) / n
        print(key, got[key], want, abs(got[key] - want) / want)
        assert np.isfinite(want) and abs(got[key] - want) <= 1e-5 * want, key
    assert {k: got[k] for k in plain} == plain and "test_w_mpjpe" not in plain
    assert np.mean(got["test_w_mpjpe_per_joint"]) == pytest.approx(got["test_w_mpjpe"], rel=1e-12)
    assert got["test_tri_status_counts"] == [[5, 0, 0, 0]] * 21 and got["test_tri_inlier_hist"] == [0, 0, 105]
    assert len(got["test_tri_reproj_per_camera"]) == 2 and all(v is not None and v >= 0 for v in got["test_tri_reproj_per_camera"])
    # the pooled state: the same bytes with and without the switch
    on, off = EpochEvaluator(m, "test", absolute=True), EpochEvaluator(m, "test")
    for ev in (on, off):
        for b in _batches(m, sets):
            ev.step(b)
    assert on.state.cpu().numpy().tobytes() == off.state.cpu().numpy().tobytes()
    assert off.absolute_state is None and on.absolute_state.numel() == absolute_doubles(2) and on.absolute_state[:3].tolist() == [5, 2, 2]
    # alongside the breakdown and the records: one state tensor, the three slices of it
    ev = EpochEvaluator(m, "test", breakdown=True, records=5, absolute={"ransac": (2, 25.0), "refit": True})
    for b in _batches(m, sets):
        ev.step(b)
    assert ev._both.numel() == ev.state_doubles + breakdown_doubles(2, 20) + absolute_doubles(2)
    store = ev._both.untyped_storage().data_ptr()
    assert all(s.untyped_storage().data_ptr() == store for s in (ev.state, ev.breakdown_state, ev.absolute_state))
    assert ev.state.cpu().numpy().tobytes() == off.state.cpu().numpy().tobytes()
    both = ev.compute()
    assert {"test_mpjpe", "test_mpjpe_per_joint", "test_w_mpjpe", "located"} <= set(both) and ev.records()["mpjpe"].shape == (5,)
    assert both["located"] + both["lost"] == 5
    ev.reset()
    assert not ev._both.cpu().numpy().any()


def test_a_ragged_batch_loses_the_sample_with_one_view():
    m, sets = _tiny()
    x, bbox, cp = sets[0]
    mask = np.array([[True, True], [False, True], [True, True]])
    got = m.evaluate([_batch(m, x, bbox, cp, view_mask=mask)], absolute=True)
    assert got["located"] == 2 and got["lost"] == 1
    assert [row[2] for row in got["test_tri_status_counts"]] == [1] * 21 and [row[0] for row in got["test_tri_status_counts"]] == [2] * 21
    out = m.forward_absolute(x, bbox, cp, view_mask=mask, details=True)
    labels = _batch(m, x, bbox, cp)["data"]
    labels["joints_cam"] /= 1000          # on the device and in place, as the step converts them
    labels["root_joint"] /= 1000
    keep = [0, 2]
    state = ao.accumulate(ao.new_state(2), *(_bits(out[k])[keep] for k in ("joints_cam", "joints_tri", "tri_status")),
                          _bits(labels["joints_cam"])[keep], _bits(labels["root_joint"])[keep],
                          _bits(out["tri_reproj"])[keep], _bits(out["tri_inliers"])[keep])
    want = ao.finish(state)
    for key, scale in (("w_mpjpe", 1000), ("root_err", 1000), ("tri_mpjpe", 1000), ("tri_reproj", 1)):
        print(key, got[f"test_{key}"], want[key] * scale)
        assert abs(got[f"test_{key}"] - want[key] * scale) <= BAR * want[key] * scale, key
    assert np.allclose(got["test_w_mpjpe_per_joint"], np.array(want["w_mpjpe_per_joint"]) * 1000, rtol=BAR, atol=0)
    assert got["test_tri_inlier_hist"] == want["tri_inlier_hist"] == [0, 0, 42]


def test_refusals_in_python():
    from handmvnet_amd.evaluation import EpochEvaluator
    m, sets = _tiny()
    x, bbox, cp = sets[0]
    ev = EpochEvaluator(m, "test", absolute=True)
    batch = _batch(m, x, bbox, cp)
    del batch["data"]["root_joint"]
    n = m.launch_count()
    with pytest.raises(ValueError, match="root_joint"):
        ev.step(batch)
    assert m.launch_count() == n and ev.state is None
    batch = _batch(m, x, bbox, cp)
    batch["cam_params"] = {"intrinsic": cp["intrinsic"]}
    n = m.launch_count()
    with pytest.raises(ValueError, match="extrinsic"):
        ev.step(batch)
    assert m.launch_count() == n and ev.state is None
    batch = _batch(m, x, bbox, cp)
    out = m(x, bbox, cp)
    with pytest.raises(ValueError, match="forward_absolute"):
        ev.add(out, batch["data"], cp)
    assert ev.state is None
    for bad in (1, "triangulate", {"threshold": 5.0}):
        with pytest.raises(ValueError, match="absolute must be"):
            m.evaluate([], absolute=bad)
