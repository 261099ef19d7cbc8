"""Ragged view sets in the evaluation path, without a GPU: the ragged oracle (tests/views_loss_oracle.py) against the real reference's
numbers, the condition that keeps the GPU tests from passing on an implementation that ignores the view mask, the [5] / [6] convention
of the epoch state, and the argument checks the new library entries make before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

import epoch_oracle as eo
import loss_oracle as lo
import views_loss_oracle as vo
from handmvnet_amd import _lib
from handmvnet_amd.evaluation import finish_state, view_mask_from_joints

REL = 2e-5   # the bar of tests/test_gpu_losses.py for a mean summed in fp64
HMV_ERR_ARG = 1


@pytest.mark.parametrize("name", lo.case_names("loss"))
def test_full_mask_reproduces_the_reference(name):
    """Every sample has the same number of elements, so the mean of the per-sample means is the reference's mean (float64: 1e-12)."""
    c = lo.loss_case(name)
    got, proj = vo.case_losses(name, np.ones((c["B"], c["V"]), bool))
    for i, term in enumerate(lo.TERMS):
        assert got[term] == pytest.approx(float(c["ref64"][i]), rel=1e-12, abs=1e-300), term
    if c["proj64"] is not None:
        assert np.allclose(proj, c["proj64"], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("name", vo.MASKED_CASES)
def test_the_masks_discriminate(name):
    """The ragged value of every view-dependent term differs from the full-mask value by at least 5 REL: an implementation that
    ignores the mask cannot pass the GPU tests."""
    c, m = lo.loss_case(name), vo.case_mask(name)
    assert m.shape == (c["B"], c["V"]) and m.any(axis=1).all() and not m.all()
    ragged, proj = vo.case_losses(name, m)
    full, _ = vo.case_losses(name, np.ones_like(m))
    terms = [t for t in vo.VIEW_TERMS if "g2d" in c["weights"] or t not in ("g2d_loss", "p2d_loss")]
    for t in terms:
        gap = abs(ragged[t] - full[t]) / abs(full[t])
        print(f"{name} {t}: ragged {ragged[t]!r} full {full[t]!r} gap {gap:.2e}")
        assert gap >= 5 * REL, t
    assert ragged["joints_3d_loss"] == pytest.approx(full["joints_3d_loss"], rel=1e-12)      # no view axis
    if proj is not None:
        assert not proj[~m].any() and np.isfinite(proj).all()


def test_what_the_masks_exercise():
    m = vo.case_mask("vii_many")
    root = lo.loss_case("vii_many")["root_idx"]
    assert m.shape == (38, 8) and m.size > 256 and m[0].all() and m[1].tolist() == [False] * 7 + [True]
    assert (~m[:, root]).any() and m[:, root].any()                   # the root camera is absent in some samples
    m3 = vo.case_mask("iii_9x13")
    assert not m3[0, lo.loss_case("iii_9x13")["root_idx"]] and m3[1].sum() == 1


def test_epoch_state_convention():
    """[6] / [5] of ragged steps is the mean over samples of the per-sample 2D MPJPE; a full mask gives the uniform state."""
    rng = np.random.default_rng(17)
    state, per_sample, n = eo.new_state(20), [], 0
    for B, V in ((3, 4), (5, 2), (1, 8)):
        g2 = (rng.random((B, V, 21, 2)) * 128).astype(np.float32)
        p2 = g2 + rng.standard_normal(g2.shape).astype(np.float32) * 3
        p3 = rng.standard_normal((B, 21, 3)).astype(np.float32) * 0.05
        g3 = p3 + rng.standard_normal(p3.shape).astype(np.float32) * 0.004
        jm = rng.random((B, V, 21)) < 0.2
        vm = rng.random((B, V)) < 0.5
        vm[np.arange(B), rng.integers(0, V, B)] = True
        vo.accumulate(state, p3, g3, p2, g2, vm, jm)
        for b in range(B):
            per_sample.append(vo.mpjpe2d(p2[b:b + 1], g2[b:b + 1], vm[b:b + 1], jm[b:b + 1]))
        n += B
        full, uni = eo.new_state(20), eo.new_state(20)
        vo.accumulate(full, p3, g3, p2, g2, np.ones((B, V), bool), jm)
        eo.accumulate(uni, p3, g3, p2, g2, jm)
        assert np.array_equal(full[[0, 1, 2, 5, 7]], uni[[0, 1, 2, 5, 7]]) and np.array_equal(full[14:], uni[14:])
        assert np.allclose(full, uni, rtol=1e-12, atol=0)
    assert state[0] == n == 9 and state[1] == 3 and state[5] == (3 * 4 + 5 * 2 + 1 * 8) * 21
    # with one V per epoch the quotient IS the mean of the per-sample values (below); steps of several V weigh a sample by its V,
    # as the uniform entry's row count does
    w = np.repeat([4, 2, 8], [3, 5, 1]).astype(np.float64)
    assert state[6] / state[5] == pytest.approx(np.sum(w * per_sample) / w.sum(), rel=1e-12)
    one = eo.new_state(20)
    g2 = (rng.random((6, 4, 21, 2)) * 128).astype(np.float32)
    p2 = g2 + rng.standard_normal(g2.shape).astype(np.float32) * 3
    g3 = rng.standard_normal((6, 21, 3)).astype(np.float32) * 0.05
    vm = rng.random((6, 4)) < 0.5
    vm[:, 1] = True
    vo.accumulate(one, g3 + rng.standard_normal(g3.shape).astype(np.float32) * 0.004, g3, p2, g2, vm)
    got = finish_state(one, 0.0, 0.02, 20, "test")
    assert got["test_mpjpe2d"] == pytest.approx(vo.mpjpe2d(p2, g2, vm), rel=1e-12)


# ---------------------------------------------------------------- argument checks, no HIP call
def _loss_args(**over):
    """A hmv_loss_args that passes every check (the pointers are never dereferenced on the host), with `over` applied."""
    a = _lib.HmvLossArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvLossArgs)
    a.B, a.V, a.hm_h, a.hm_w, a.image_size, a.sigma = 2, 3, 8, 8, 64, 2
    a.pred_heatmap = a.pred_joints_2d = a.gt_joints_2d = a.pred_joints_cam = a.gt_joints_cam = a.scratch = 4096
    a.scratch_bytes = 8 * 6
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _eval_args(**over):
    a = _lib.HmvEvalArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvEvalArgs)
    a.B, a.V, a.steps, a.thr_min, a.thr_max = 2, 4, 20, 0.0, 0.02
    a.pred_joints_cam = a.gt_joints_cam = a.pred_joints_2d = a.gt_joints_2d = a.state = 4096
    a.state_doubles = 35
    for k, v in over.items():
        setattr(a, k, v)
    return a


PRESENT, RESULT = ctypes.c_void_p(4096), ctypes.c_void_p(4096)


@pytest.mark.parametrize("over, present, word", [
    ({}, None, "view_present is NULL"), ({"struct_size": ctypes.sizeof(_lib.HmvLossArgs) - 8}, PRESENT, "struct_size"),
    ({"pred_heatmap": None}, PRESENT, "pred_heatmap is NULL"), ({"pred_joints_2d": None}, PRESENT, "pred_joints_2d is NULL"),
    ({"gt_joints_2d": None}, PRESENT, "gt_joints_2d is NULL"), ({"pred_joints_cam": None}, PRESENT, "pred_joints_cam is NULL"),
    ({"gt_joints_cam": None}, PRESENT, "gt_joints_cam is NULL"), ({"scratch": None}, PRESENT, "scratch is NULL"),
    ({"scratch_bytes": 8 * 6 - 1}, PRESENT, "scratch_bytes"), ({"B": 0}, PRESENT, "B must"), ({"V": 0}, PRESENT, "V must"),
    ({"with_projection": 1}, PRESENT, "intrinsic is NULL"),
    ({"with_projection": 1, "intrinsic": 4096, "extrinsic": 4096, "bbox": 4096, "root_idx": 3}, PRESENT, "root_idx")])
def test_ragged_loss_argument_checks_come_before_any_hip_call(over, present, word):
    """No GPU here: reaching hipSetDevice would give the HIP error code, not the argument one."""
    lib = _lib.load()
    assert lib.hmv_pose_losses_views(0, ctypes.byref(_loss_args(**over)), present, RESULT, None) == HMV_ERR_ARG
    msg = lib.hmv_last_error(None).decode()
    assert msg.startswith("hmv_pose_losses_views: ") and word in msg, msg


def test_ragged_loss_null_struct_and_result():
    lib = _lib.load()
    assert lib.hmv_pose_losses_views(0, None, PRESENT, RESULT, None) == HMV_ERR_ARG
    assert lib.hmv_last_error(None).decode() == "hmv_pose_losses_views: args is NULL"
    assert lib.hmv_pose_losses_views(0, ctypes.byref(_loss_args()), PRESENT, None, None) == HMV_ERR_ARG
    assert lib.hmv_last_error(None).decode() == "hmv_pose_losses_views: result is NULL"


@pytest.mark.parametrize("over, present, word", [
    ({}, None, "view_present is NULL"), ({"struct_size": ctypes.sizeof(_lib.HmvEvalArgs) - 8}, PRESENT, "struct_size"),
    ({"pred_joints_cam": None}, PRESENT, "pred_joints_cam is NULL"), ({"gt_joints_cam": None}, PRESENT, "gt_joints_cam is NULL"),
    ({"pred_joints_2d": None}, PRESENT, "pred_joints_2d is NULL"), ({"gt_joints_2d": None}, PRESENT, "gt_joints_2d is NULL"),
    ({"state": None}, PRESENT, "state is NULL"), ({"state": 4100}, PRESENT, "8-byte aligned"),
    ({"state_doubles": 34}, PRESENT, "state_doubles"), ({"steps": 257}, PRESENT, "steps must"), ({"B": 0}, PRESENT, "B must")])
def test_ragged_epoch_argument_checks_come_before_any_hip_call(over, present, word):
    lib = _lib.load()
    assert lib.hmv_eval_add_views(0, ctypes.byref(_eval_args(**over)), present, None) == HMV_ERR_ARG
    msg = lib.hmv_last_error(None).decode()
    assert msg.startswith("hmv_eval_add_views: ") and word in msg, msg


def test_the_uniform_entries_keep_their_own_name():
    lib = _lib.load()
    assert lib.hmv_eval_add(0, ctypes.byref(_eval_args(state=None)), None) == HMV_ERR_ARG
    assert lib.hmv_last_error(None).decode().startswith("hmv_eval_add: state is NULL")
    assert lib.hmv_pose_losses(0, ctypes.byref(_loss_args(scratch=None)), RESULT, None) == HMV_ERR_ARG
    assert lib.hmv_last_error(None).decode().startswith("hmv_pose_losses: scratch is NULL")


def test_forward_frames_views_without_a_handle():
    lib = _lib.load()
    counts = (ctypes.c_int32 * 1)(1)
    assert lib.hmv_forward_frames_views(None, 1, counts, None, 4, 4, None, None, None, None, None, None, None, None, None, None) == HMV_ERR_ARG


def test_view_mask_from_joints():
    jm = np.zeros((2, 3, 21), bool)
    jm[0, 1] = True             # no joint of view 1 is visible: the dataset feeds a black image there
    jm[1, 2, :20] = True        # one visible joint keeps the view
    want = [[True, False, True], [True, True, True]]
    got = view_mask_from_joints(jm)
    assert isinstance(got, np.ndarray) and got.dtype == bool and got.tolist() == want
    got_t = view_mask_from_joints(torch.from_numpy(jm))
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.bool and got_t.tolist() == want
