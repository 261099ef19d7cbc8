"""The absolute evaluation without a GPU: tests/absolute_epoch_oracle.py against golden/absolute_epoch_cases.npz (the reference's own
PoseMetrics.mpjpe and calculate_reprojection_error), evaluation.finish_absolute on hand-built states, and every refusal
hmv_eval_absolute_add makes before it touches HIP."""
import ctypes
import os

import numpy as np
import pytest

import absolute_epoch_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "absolute_epoch_cases.npz"))
KEYS = ("pred_cam", "tri", "status", "gt_cam", "gt_root", "reproj", "inliers")


def case(name, lo=None, hi=None):
    return [FIX[f"{name}.{k}"][lo:hi] for k in KEYS]


def feed(name, cut):
    V = FIX[f"{name}.reproj"].shape[1]
    state, at = ao.new_state(V), 0
    for n in cut:
        ao.accumulate(state, *case(name, at, at + n))
        at += n
    assert at == FIX[f"{name}.tri"].shape[0]
    return state


@pytest.mark.parametrize("cut", ["cut0", "cut1"])
def test_pooled_values_are_the_weighted_mean_of_the_references_steps(cut):
    sizes = FIX[f"plain.{cut}"]
    got = ao.finish(feed("plain", sizes))
    assert got["located"] == 5 and got["lost"] == 0
    for key in ("w_mpjpe", "root_err"):
        want = float((sizes * FIX[f"plain.{cut}.{key}"]).sum() / sizes.sum())
        print(key, got[key], want, abs(got[key] - want) / want)
        assert abs(got[key] - want) <= 1e-12 * want, key
    assert np.mean(got["w_mpjpe_per_joint"]) == pytest.approx(got["w_mpjpe"], rel=1e-12)


@pytest.mark.parametrize("name", ["plain", "mixed", "one", "wide"])
def test_the_reprojection_per_camera_is_the_references(name):
    B = FIX[f"{name}.tri"].shape[0]
    got = ao.finish(feed(name, (B,)))["tri_reproj_per_camera"]
    want = FIX[f"{name}.camera"]
    assert len(got) == want.size
    for g, w in zip(got, want):
        assert g is not None and abs(g - w) <= 1e-12 * w, (name, g, w)


def test_mixed_counts_are_exact():
    state = feed("mixed", (2, 3))
    got = ao.finish(state)
    assert got["located"] == int(FIX["mixed.located"]) == 3 and got["lost"] == int(FIX["mixed.lost"]) == 2
    assert np.array_equal(np.array(got["tri_status_counts"]), FIX["mixed.status_counts"])
    assert np.array_equal(np.array(got["tri_inlier_hist"]), FIX["mixed.inlier_hist"])
    assert state[:3].tolist() == [5, 2, 3] and np.isfinite(state).all()
    s = ao.slices(state, 3)
    assert s["S"].sum() == 5 * 21 and s["H"].sum() == s["S"][:, 0].sum()
    assert s["TN"].sum() == s["S"][:, 0].sum() - 1            # the status-0 joint whose point is NaN
    whole = feed("mixed", (5,))
    for name in ("TN", "S", "RN", "H"):
        assert np.array_equal(ao.slices(whole, 3)[name], s[name]), name
    assert whole[1] == 1 and np.allclose(whole[2:], state[2:], rtol=1e-12, atol=0)      # [1] counts the steps


def test_finish_absolute_on_hand_built_states():
    from handmvnet_amd import _lib
    from handmvnet_amd.evaluation import absolute_doubles, finish_absolute
    lib = _lib.load()
    for V in (1, 2, 16):
        assert absolute_doubles(V) == 156 + 3 * V == lib.hmv_eval_absolute_doubles(V) == ao.doubles(V)
    assert lib.hmv_eval_absolute_doubles(0) == 0 and lib.hmv_eval_absolute_doubles(17) == 0
    V = 2
    s = ao.new_state(V)
    s[0], s[1], s[2], s[3] = 4, 2, V, 3
    s[4], s[5] = 3 * 21 * 0.010, 3 * 0.020                     # metres: 10 mm per joint, 20 mm at the root
    v = ao.slices(s, V)
    v["W"][:] = 3 * 0.010
    v["T"][:], v["TN"][:] = 0.008, 2
    v["T"][20], v["TN"][20] = 0, 0
    v["S"][:, 0], v["S"][:, 2] = 3, 1
    v["R"][:], v["RN"][:] = [30.0, 0.0], [20, 0]
    v["H"][:] = [1, 2, 60]
    got = finish_absolute(s, "val")
    assert set(got) == {"val_w_mpjpe", "val_root_err", "val_w_mpjpe_per_joint", "val_tri_mpjpe", "val_tri_mpjpe_per_joint",
                        "val_tri_status_counts", "val_tri_reproj_per_camera", "val_tri_reproj", "val_tri_inlier_hist", "located", "lost"}
    assert got["val_w_mpjpe"] == pytest.approx(10.0, rel=1e-12) and got["val_root_err"] == pytest.approx(20.0, rel=1e-12)
    assert got["val_w_mpjpe_per_joint"] == pytest.approx([10.0] * 21, rel=1e-12)
    assert got["val_tri_mpjpe"] == pytest.approx(4.0, rel=1e-12)
    assert got["val_tri_mpjpe_per_joint"][:20] == pytest.approx([4.0] * 20, rel=1e-12) and got["val_tri_mpjpe_per_joint"][20] is None
    assert got["val_tri_status_counts"] == [[3, 0, 1, 0]] * 21
    assert got["val_tri_reproj_per_camera"] == [1.5, None] and got["val_tri_reproj"] == 1.5
    assert got["val_tri_inlier_hist"] == [1, 2, 60] and got["located"] == 3 and got["lost"] == 1
    # nothing located, no reprojection table
    s = ao.new_state(V)
    s[0], s[1], s[2] = 2, 1, V
    got = finish_absolute(s, "test")
    assert got["test_w_mpjpe"] is None and got["test_root_err"] is None and got["test_tri_mpjpe"] is None and got["test_tri_reproj"] is None
    assert got["test_w_mpjpe_per_joint"] == [None] * 21 and got["test_tri_reproj_per_camera"] == [None, None]
    assert got["located"] == 0 and got["lost"] == 2
    with pytest.raises(ValueError, match="empty epoch"):
        finish_absolute(ao.new_state(V), "test")
    with pytest.raises(ValueError, match=r"156 \+ 3 V"):
        finish_absolute(np.zeros(160), "test")
    s[2] = 3
    with pytest.raises(ValueError, match="V = 3"):
        finish_absolute(s, "test")
    # the oracle's finish and the package's agree on a real state
    state = feed("mixed", (5,))
    mine, theirs = finish_absolute(state, "test"), ao.finish(state)
    assert mine["test_w_mpjpe"] == pytest.approx(theirs["w_mpjpe"] * 1000, rel=1e-12)
    assert mine["test_tri_reproj_per_camera"] == pytest.approx(theirs["tri_reproj_per_camera"], rel=1e-12)
    assert mine["test_tri_inlier_hist"] == theirs["tri_inlier_hist"] and mine["test_tri_status_counts"] == theirs["tri_status_counts"]


def test_every_refusal_names_its_field_before_any_hip_call():
    from handmvnet_amd import _lib
    lib = _lib.load()
    fake = 0x1000                                               # never dereferenced: every call below is refused first

    def args(**kw):
        a = _lib.HmvEvalAbsoluteArgs()
        a.struct_size = ctypes.sizeof(_lib.HmvEvalAbsoluteArgs)
        a.B, a.V = 2, 3
        for f in ("pred_joints_cam", "joints_tri", "tri_status", "gt_joints_cam", "gt_root", "state"):
            setattr(a, f, fake)
        a.state_doubles = 156 + 9
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, text):
        assert lib.hmv_eval_absolute_add(0, None if a is None else ctypes.byref(a), None) == _lib.HMV_ERR_ARG, text
        assert text in lib.hmv_last_error(None).decode(), (text, lib.hmv_last_error(None))

    refused(None, "args is NULL")
    refused(args(struct_size=ctypes.sizeof(_lib.HmvEvalAbsoluteArgs) - 8), "struct_size")
    refused(args(B=0), "B must be")
    for V in (0, 17, -1):
        refused(args(V=V), "V must be in 1 .. 16")
    for f in ("pred_joints_cam", "joints_tri", "tri_status", "gt_joints_cam", "gt_root"):
        refused(args(**{f: None}), f"{f} is NULL")
    refused(args(state=None), "state is NULL")
    refused(args(state=fake + 4), "state is NULL or not 8-byte aligned")
    refused(args(state_doubles=156 + 8), "state_doubles")
    refused(args(V=16, state_doubles=156 + 47), "state_doubles")


def test_the_evaluator_refuses_other_values_of_absolute():
    from handmvnet_amd.evaluation import EpochEvaluator

    class Labels:
        auc_thresh = [0.0, 0.02]
        heatmap_targets = "batch"

    for bad in (1, "triangulate", None, {"threshold": 5.0}, ["ransac"]):
        with pytest.raises(ValueError, match="absolute must be"):
            EpochEvaluator(Labels(), "test", absolute=bad)
    for good in (False, True, {}, {"ransac": (2, 25.0), "refit": False, "confidence": 0.3}):
        EpochEvaluator(Labels(), "test", absolute=good)
