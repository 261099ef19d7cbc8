"""The numpy loss oracle (tests/loss_oracle.py) pinned to outputs of the real reference (tests/golden/loss_cases.npz), and the
argument checks of the loss entries that run before any HIP call.  No GPU.

Tolerances: the oracle and the float64 reference evaluate the same expressions in float64, so losses and projections agree to
1e-12 relative (summation order only); target maps are bit-equal after the fp32 cast where both scales are integers and within
one fp32 ulp otherwise.
"""
import ctypes

import numpy as np
import pytest

import loss_oracle as lo

MAP_NAMES, LOSS_NAMES = lo.case_names("hm"), lo.case_names("loss")
loss_case = lo.loss_case


def test_fixture_covers_the_cases():
    assert len(MAP_NAMES) == 4 and len(LOSS_NAMES) == 8
    assert lo.hash_uniform(7, 4).tolist() == pytest.approx([0.43174081, 0.1321804, 0.49900048, 0.14700725], abs=1e-8)
    c = loss_case("vii_many")
    assert c["B"] * c["V"] > 256 and c["mask"] is not None and c["flag"]
    assert "g2d" not in loss_case("v_three")["weights"]
    assert loss_case("i_flag_on")["root_idx"] == 2 and not loss_case("i_flag_off")["flag"]
    # the sheared rig really is not rigid: R^T R != I for the root view of case (vi)
    e = loss_case("vi_sheared")["extr"][0, 1, :3, :3].astype(np.float64)
    assert np.abs(e.T @ e - np.eye(3)).max() > 0.05


@pytest.mark.parametrize("name", MAP_NAMES)
def test_target_maps_match_reference(name):
    m = lo.map_case(name)
    S, h, w, joints, valid, ref = m["S"], m["h"], m["w"], m["joints"], m["valid"], m["ref"]
    got = lo.target_heatmaps(joints, S, h, w).astype(np.float32)
    assert 0 < (~valid).sum() < valid.size                       # both kinds of label are present
    assert np.all(got[~valid] == 0)                              # whole Gaussian outside the image: zero map (the reference raises)
    assert [lo.gaussian_in_image(v, S) for v in (-7.5, -6.2, S + 5.9, S + 6.1, -8.3)] == [True, True, True, False, False]
    assert np.all(lo.target_heatmaps(np.array([[-7.5, 10.0]], np.float32), S, h, w) == 0)   # c = -7: zero in the reference too
    if S % h == 0 and S % w == 0:
        assert np.array_equal(got[valid], ref[valid])
    else:
        assert np.all(np.abs(got[valid].astype(np.float64) - ref[valid]) <= np.spacing(np.abs(ref[valid])))


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_losses_match_reference_float64(name):
    c = loss_case(name)
    tgt = lo.target_heatmaps(c["gt_2d"], c["S"], c["h"], c["w"]).astype(np.float32)
    if c["S"] % c["h"] == 0 and c["S"] % c["w"] == 0:
        assert np.array_equal(tgt, c["target"])
    else:
        assert np.all(np.abs(tgt.astype(np.float64) - c["target"]) <= np.spacing(np.abs(c["target"])))
    terms, proj = lo.losses(c["pred_hm"], c["target"], c["pred_2d"], c["gt_2d"], c["pred_cam"], c["gt_cam"], c["weights"], c["mask"],
                            c["flag"], c["root_joint"], c["root_idx"], c["intr"], c["extr"], c["bbox"])
    for i, n in enumerate(lo.TERMS):
        assert terms[n] == pytest.approx(c["ref64"][i], rel=1e-12, abs=0), n
    if "g2d" in c["weights"]:
        assert np.abs(proj - c["proj64"]).max() <= 1e-12 * np.abs(c["proj64"]).max()
        img = lo.project(c["pred_cam"].astype(np.float64) + c["root_joint"], c["root_idx"], c["intr"], c["extr"])
        assert np.abs(img - c["proj_img64"]).max() <= 1e-12 * np.abs(c["proj_img64"]).max()
        assert 0 < c["proj_maxdiff"] < 1e-3       # the reference's own fp32 error on these rigs, in pixels
    else:
        assert proj is None and terms["g2d_loss"] == 0 and terms["p2d_loss"] == 0


# ---------------------------------------------------------------- the entries' argument checks (host side of libhandmv, no HIP call)
def _args():
    """An argument block that passes every check up to the device selection: the pointers are never dereferenced on the host."""
    from handmvnet_amd import _lib
    a = _lib.HmvLossArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvLossArgs)
    a.B, a.V, a.hm_h, a.hm_w, a.image_size, a.sigma = 2, 3, 16, 16, 128, 2
    for n in ("pred_heatmap", "target_heatmap", "pred_joints_2d", "gt_joints_2d", "pred_joints_cam", "gt_joints_cam", "scratch"):
        setattr(a, n, 4096)
    a.scratch_bytes = 8 * 6
    return a


@pytest.mark.parametrize("damage, word", [
    (lambda a: setattr(a, "struct_size", 64), "struct_size"), (lambda a: setattr(a, "B", 0), "B must"),
    (lambda a: setattr(a, "V", 0), "V must"), (lambda a: setattr(a, "pred_heatmap", None), "pred_heatmap"),
    (lambda a: setattr(a, "gt_joints_cam", None), "gt_joints_cam"), (lambda a: setattr(a, "scratch_bytes", 8 * 5), "scratch_bytes"),
    (lambda a: setattr(a, "scratch", None), "scratch"), (lambda a: setattr(a, "hm_w", 250), "hm_h + hm_w"),
    (lambda a: (setattr(a, "target_heatmap", None), setattr(a, "sigma", 0)), "sigma"),
    (lambda a: setattr(a, "with_projection", 1), "intrinsic"),
    (lambda a: ([setattr(a, n, 4096) for n in ("intrinsic", "extrinsic", "bbox")], setattr(a, "with_projection", 1),
                setattr(a, "root_idx", 3)), "root_idx"),
    (lambda a: setattr(a, "projected", 4096), "projected"),
])
def test_pose_losses_rejects_bad_arguments_before_touching_the_device(damage, word):
    from handmvnet_amd import _lib
    lib = _lib.load()
    assert ctypes.sizeof(_lib.HmvLossArgs) == 176
    assert lib.hmv_pose_losses_scratch_bytes(2, 3) == 48 and lib.hmv_pose_losses_scratch_bytes(0, 3) == 0
    a = _args()
    damage(a)
    assert lib.hmv_pose_losses(0, ctypes.byref(a), ctypes.c_void_p(4096), None) == 1      # HMV_ERR_ARG
    msg = lib.hmv_last_error(None).decode()
    assert msg.startswith("hmv_pose_losses: ") and word in msg, msg


def test_the_small_entries_reject_bad_arguments():
    from handmvnet_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    for args, word in (((0, None, 1, 128, 16, 16, 2, p, None), "joints"), ((0, p, 0, 128, 16, 16, 2, p, None), "n_frames"),
                       ((0, p, 1, 0, 16, 16, 2, p, None), "image_size"), ((0, p, 1, 128, 0, 16, 2, p, None), "hm_h"),
                       ((0, p, 1, 128, 16, 16, 9, p, None), "sigma"), ((0, p, 1, 128, 16, 16, 2, None, None), "out")):
        assert lib.hmv_op_target_heatmaps(*args) == 1
        assert word in lib.hmv_last_error(None).decode()
    for args, word in (((0, None, 1, 2, 0, p, p, None, p, None), "joints_abs"), ((0, p, 0, 2, 0, p, p, None, p, None), "B must"),
                       ((0, p, 1, 0, 0, p, p, None, p, None), "V must"), ((0, p, 1, 2, 2, p, p, None, p, None), "root_idx"),
                       ((0, p, 1, 2, -1, p, p, None, p, None), "root_idx"), ((0, p, 1, 2, 0, p, None, None, p, None), "extrinsic"),
                       ((0, p, 1, 2, 0, None, p, None, p, None), "intrinsic"), ((0, p, 1, 2, 0, p, p, None, None, None), "out")):
        assert lib.hmv_project_joints(*args) == 1
        assert word in lib.hmv_last_error(None).decode()
