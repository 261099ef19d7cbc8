"""Hand alignment and analytic IK without a GPU: the numpy oracle (tests/ik_oracle.py) against the fixture written by the reference's
own rigid_transform_3D and adaptive_IK (tests/golden/make_ik_fixture.py; the Rodrigues step there is pinned to the formula, not to
the transforms3d package), the two C entries' refusals, which come before any HIP call, the two symbols, and the refusals of
handmvnet_amd/ik.py that need no device.

Bar of the oracle: 16 x the fixture's f64_term, the measured spread between two LAPACK SVD drivers over the same cases -- the oracle
is the reference's arithmetic restated, and what may differ between the box that wrote the fixture and the one that runs this test is
the LAPACK build."""
import os
import re

import numpy as np
import pytest
import torch

import ik_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "ik_cases.npz"))
NAMES = sorted({k.split(".")[0] for k in FIX.files if "." in k})
TERM = 16 * float(FIX["f64_term"])
NEW_SYMBOLS = ["hmv_op_hand_ik", "hmv_op_rigid_unapply"]


def template_of(name):
    return FIX["template_" + str(FIX[f"{name}.template"])]


def test_fixture_holds_the_cases_the_rule_needs():
    assert NAMES == sorted(["posed_0", "posed_1", "posed_2", "straight", "mirrored", "planar", "nan_joint"])
    assert 0 < float(FIX["f64_term"]) < 1e-9                                    # measured, and far below one fp32 rounding
    assert [str(n) for n in FIX["batch_std"]] == ["posed_0", "straight", "mirrored", "nan_joint", "posed_1"]
    assert all(str(FIX[f"{n}.template"]) == "std" for n in FIX["batch_std"]) and str(FIX["planar.template"]) == "planar"
    assert FIX["template_std"].dtype == np.float32 and not FIX["template_planar"][:, 2].any() and FIX["template_std"][1:, 2].all()
    assert np.linalg.det(FIX["mirrored.pose_R"][0]) < -0.99                     # the reflection is kept ...
    assert np.linalg.det(FIX["planar.pose_R"][0]) > 0.99                        # ... and repaired where a singular value vanishes
    assert len(set(FIX["planar.joints"][[0, 1, 5, 9, 13, 17], 2].tolist())) == 1
    assert np.isnan(FIX["nan_joint.joints"]).sum() == 1 and np.isnan(FIX["nan_joint.pose_R"]).any()
    for n in NAMES:
        assert FIX[f"{n}.joints"].dtype == np.float32 and FIX[f"{n}.pose_R"].dtype == np.float64
        assert abs(np.linalg.det(FIX[f"{n}.ret_R"]) - 1) < 1e-12                # the alignment is always a proper rotation


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference_fixture(name):
    ret_R, ret_t, aligned, pose_R = io.align_and_ik(FIX[f"{name}.joints"], template_of(name))
    assert np.abs(ret_R - FIX[f"{name}.ret_R"]).max() <= TERM
    assert np.abs(ret_t.reshape(3) - FIX[f"{name}.ret_t"]).max() <= TERM * np.abs(FIX[f"{name}.ret_t"]).max()
    want_j, want_p = FIX[f"{name}.joints_to_mano"], FIX[f"{name}.pose_R"]
    assert (np.isnan(aligned) == np.isnan(want_j)).all() and (np.isnan(pose_R) == np.isnan(want_p)).all()
    assert np.nanmax(np.abs(aligned - want_j)) <= TERM * np.nanmax(np.abs(want_j))
    assert np.nanmax(np.abs(pose_R - want_p)) <= TERM
    pose, align, al, status = io.hand_ik(FIX[f"{name}.joints"][None], template_of(name))
    assert status.tolist() == [int(name == "nan_joint")]
    assert np.array_equal(align[0, :9].reshape(3, 3), ret_R) and np.array_equal(align[0, 9:], ret_t.reshape(3))


def test_oracle_unapply_undoes_the_alignment():
    rng = np.random.default_rng(4)
    names = [n for n in NAMES if n != "nan_joint"]
    align = np.stack([np.concatenate([FIX[f"{n}.ret_R"].reshape(9), FIX[f"{n}.ret_t"]]) for n in names])
    joints = np.stack([FIX[f"{n}.joints"] for n in names])
    aligned = np.stack([FIX[f"{n}.joints_to_mano"] for n in names]).astype(np.float32)
    back = io.rigid_unapply(aligned, align)
    assert np.abs(back - joints).max() <= 2.0 ** -22 * np.abs(joints).max()      # two fp32 roundings of ~600 mm coordinates
    pts = rng.uniform(-200, 200, (len(names), 5, 3)).astype(np.float32)
    want = np.stack([(FIX[f"{n}.ret_R"].T @ (pts[i].T.astype(np.float64) - FIX[f"{n}.ret_t"][:, None])).T for i, n in enumerate(names)])
    assert np.abs(io.rigid_unapply(pts, align) - want).max() <= TERM * 1000


def test_new_symbols_are_declared_and_exported():
    from handmvnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    declared = set(re.findall(r"\b(hmv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/handmv.h"
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), f"{sym} is not exported / bound"
    import handmvnet_amd
    for name in ("JointsToVertices", "hand_ik", "rigid_unapply"):
        assert callable(getattr(handmvnet_amd, name))


def test_raw_entries_refuse_bad_arguments_before_any_hip_call():
    """Both entries check their arguments in front of hipSetDevice: the refusals come back on a box without a GPU too."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    p = 4096   # never dereferenced
    for args, word in (((0, p, p, 0, p, p, None, p, None), b"n must be positive"),
                       ((0, p, p, -3, p, p, None, p, None), b"n must be positive"),
                       ((0, None, p, 2, p, p, None, p, None), b"joints is NULL"),
                       ((0, p, None, 2, p, p, None, p, None), b"template_joints"),
                       ((0, p, p, 2, None, p, None, p, None), b"pose_R"),
                       ((0, p, p, 2, p, None, None, p, None), b"align"),
                       ((0, p, p, 2, p, p + 4, None, p, None), b"align"),
                       ((0, p, p, 2, p, p, None, None, None), b"status")):
        assert lib.hmv_op_hand_ik(*args) == _lib.HMV_ERR_ARG
        msg = lib.hmv_last_error(None)
        assert b"hmv_op_hand_ik" in msg and word in msg, msg
    for args, word in (((0, p, p, 0, 21, p, None), b"n must be positive"),
                       ((0, p, p, 2, 0, p, None), b"n_pts"),
                       ((0, p, p, 2, -1, p, None), b"n_pts"),
                       ((0, None, p, 2, 21, p, None), b"points"),
                       ((0, p, None, 2, 21, p, None), b"align"),
                       ((0, p, p + 2, 2, 21, p, None), b"align"),
                       ((0, p, p, 2, 21, None, None), b"out")):
        assert lib.hmv_op_rigid_unapply(*args) == _lib.HMV_ERR_ARG
        msg = lib.hmv_last_error(None)
        assert b"hmv_op_rigid_unapply" in msg and word in msg, msg


def test_python_refusals_without_a_device():
    from handmvnet_amd import _lib
    from handmvnet_amd.ik import JointsToVertices, hand_ik, rigid_unapply
    T = torch.from_numpy(FIX["template_std"])
    with pytest.raises(ValueError):
        hand_ik(torch.zeros(2, 20, 3), T)
    with pytest.raises(ValueError):
        hand_ik(torch.zeros(2, 21, 3), T[:20])
    with pytest.raises(_lib.HandMvError, match="MI355X only"):
        hand_ik(torch.zeros(2, 21, 3), T)                                       # CPU tensors: no fallback
    with pytest.raises(ValueError):
        rigid_unapply(torch.zeros(2, 5, 2), torch.zeros(2, 12, dtype=torch.float64))
    with pytest.raises(ValueError):
        rigid_unapply(torch.zeros(2, 5, 3), torch.zeros(2, 12))                 # align is float64
    with pytest.raises(ValueError):
        rigid_unapply(torch.zeros(2, 5, 3), torch.zeros(3, 12, dtype=torch.float64))
    with pytest.raises(_lib.HandMvError, match="MI355X only"):
        rigid_unapply(torch.zeros(2, 5, 3), torch.zeros(2, 12, dtype=torch.float64))


def test_joints_to_vertices_constructor_checks_the_template():
    from handmvnet_amd.ik import JointsToVertices
    layer = lambda pose_R: (None, None)   # noqa: E731  (never called: the template is given)
    T = torch.from_numpy(FIX["template_std"])
    j2v = JointsToVertices(layer, template=T)
    assert torch.equal(j2v.joints_template, T) and j2v.last_pose_R is None and j2v.last_status is None
    bad = T.clone()
    bad[7] = bad[6]                                                             # joint 7 on its parent: a zero-length bone
    with pytest.raises(ValueError, match="zero-length bone.*joint 7"):
        JointsToVertices(layer, template=bad)
    bad = T.clone()
    bad[13] = bad[0]                                                            # a finger root on the wrist
    with pytest.raises(ValueError, match="zero-length bone"):
        JointsToVertices(layer, template=bad)
    bad = T.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        JointsToVertices(layer, template=bad)
    with pytest.raises(ValueError):
        JointsToVertices(layer, template=T[:20])
    with pytest.raises(TypeError):
        JointsToVertices(None, template=T)


def test_model_keeps_refusing_vertices_without_a_layer():
    from cases import CASES, case_params
    from handmvnet_amd import HandMvNet
    tp, mp, dp = case_params(CASES["tiny_r18"])
    model = HandMvNet(tp, dict(mp, get_vertices=True), dp)
    assert model.joints_to_vertices is None and model.get_vertices
    assert HandMvNet(tp, mp, dp).joints_to_vertices is None
