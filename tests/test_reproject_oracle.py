"""Windows from the reprojected pose without a GPU: the numpy oracle (tests/reproject_oracle.py) against the fixture written by the
real reference functions (tests/golden/make_reproject_fixture.py), the entry in the header, the library and the binding, and every
refusal of hmv_op_reproject_crop_boxes and of the Python layer, which come before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import reproject_oracle as ro
from handmvnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "reproject_cases.npz"))
NAMES = sorted({k.split(".")[0] for k in FIX.files})


def case(name):
    return {k.split(".", 1)[1]: FIX[k] for k in FIX.files if k.startswith(name + ".")}


def run_oracle(c, require_all=False, **over):
    kw = dict(point_status=c["point_status"], frame_cam=c["frame_cam"], joints_img=c["joints_img"], margin=int(c["margin"]),
              square=bool(c["square"]), require_all=require_all)
    kw.update(over)
    return ro.reproject_crop_boxes(c["points3d"], c["intr"], c["ext"], c["boxes_in"], c["status_in"], **kw)


def test_fixture_holds_the_cases_the_rule_needs():
    for need in ("plain_v3", "plain_v4_m4", "frame_cam", "square_off", "behind", "point_status", "nan", "slot_status", "huge_window"):
        assert need in NAMES
    assert {FIX[f"{n}.intr"].shape[1] for n in NAMES} == {3, 4} and {FIX[f"{n}.intr"].shape[0] for n in NAMES} == {1, 2, 3}
    assert {int(FIX[f"{n}.margin"]) for n in NAMES} == {0, 4} and {int(FIX[f"{n}.square"]) for n in NAMES} == {0, 1}
    assert (FIX["frame_cam.frame_cam"] != 0).any()
    parities = set()      # the odd difference of width and height: the pad + 1 side, on either axis
    for n in NAMES:
        c = case(n)
        for b, v in zip(*np.nonzero(c["source"])):
            p = c["joints_2d"][b, v]
            w, h = int(p[:, 0].max()) - int(p[:, 0].min()), int(p[:, 1].max()) - int(p[:, 1].min())
            parities.add((h > w, abs(h - w) % 2))
    assert {(True, 1), (False, 1)} <= parities
    assert (FIX["behind.depth"][0, 1] < 0).any() and FIX["behind.source"].tolist() == [[1, 0, 1], [1, 1, 1]]
    assert FIX["point_status.source"].tolist() != FIX["point_status.source_all"].tolist()
    assert np.isnan(FIX["nan.points3d"]).sum() == 1
    assert FIX["slot_status.status_in"].tolist() == [[0, 1, 0], [1, 0, 2]] and FIX["slot_status.status"].tolist() == [[0, 1, 0], [1, 0, 0]]
    assert FIX["huge_window.source"].tolist() == [[1, 1, 0]]


@pytest.mark.parametrize("name", NAMES)
def test_inputs_keep_every_edge_away_from_an_integer(name):
    """The condition that makes the integer windows immune to a last-bit difference in fp64: every extreme of a slot in front of its
    camera is at least 1e-3 px from an integer, every depth at least 1 mm from zero; re-checked from the stored values."""
    c = case(name)
    z, p = c["depth"], c["joints_2d"].astype(np.float64)
    for b, v in np.ndindex(*z.shape[:2]):
        if not np.isfinite(z[b, v]).all():
            continue
        assert (np.abs(z[b, v]) >= 1.0).all()
        if (z[b, v] > 0).all():
            ext = np.array([p[b, v, :, 0].min(), p[b, v, :, 0].max(), p[b, v, :, 1].min(), p[b, v, :, 1].max()])
            assert (np.abs(ext - np.round(ext)) >= 1e-3).all(), (name, b, v)


@pytest.mark.parametrize("require_all", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference_fixture(name, require_all):
    c = case(name)
    tag = "_all" if require_all else ""
    got = run_oracle(c, require_all)
    assert got["crop_boxes"].dtype == np.int32 and np.array_equal(got["crop_boxes"], c["boxes" + tag])
    assert np.array_equal(got["status"], c["status" + tag]) and np.array_equal(got["source"], c["source" + tag])
    assert np.array_equal(got["ok"], c["ok" + tag])
    assert np.array_equal(got["bbox"].view(np.uint32), c["boxes" + tag].astype(np.float32).view(np.uint32))
    want = c["joints_2d"].copy()
    want[~c["ok" + tag]] = np.nan
    assert ro.adjacent(got["joints_reproj"], want).all()
    moved = got["source"] == 1      # the other slots keep every byte of window and status
    assert np.array_equal(got["crop_boxes"][~moved], c["boxes_in"][~moved]) and np.array_equal(got["status"][~moved], c["status_in"][~moved])
    gap = got["gap"]
    defined = c["ok" + tag][:, None] & (c["status_in"] == 0)
    assert np.array_equal(np.isnan(gap), ~defined | np.isnan(got["joints_reproj"]).any(axis=(2, 3)))
    some = defined & (got["source"] == 1)
    assert (gap[some] > 0.5).all() and (gap[some] < 20).all()      # 3 px of noise per axis


def test_oracle_frame_cam_and_optional_inputs():
    c = case("plain_v4_m4")
    got = run_oracle(c, frame_cam=[0, 7, -1])
    assert got["ok"].tolist() == [True, False, False] and got["source"].tolist() == [[1] * 4, [0] * 4, [0] * 4]
    assert np.isnan(got["joints_reproj"][1:]).all() and np.isnan(got["gap"][1:]).all()
    got = run_oracle(c, point_status=None, frame_cam=None, joints_img=None)
    assert np.array_equal(got["crop_boxes"], c["boxes"]) and np.isnan(got["gap"]).all()


# ---------------------------------------------------------------- header, library, binding
def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    assert re.search(r"\bint\s+hmv_op_reproject_crop_boxes\s*\(", header)
    lib = _lib.load()
    assert hasattr(lib, "hmv_op_reproject_crop_boxes") and "hmv_op_reproject_crop_boxes" in _lib.SYMBOLS
    assert len(lib.hmv_op_reproject_crop_boxes.argtypes) == 3
    assert ctypes.sizeof(_lib.HmvReprojectBoxesArgs) == 6 * 4 + 12 * ctypes.sizeof(ctypes.c_void_p)
    fields = re.search(r"typedef struct hmv_reproject_boxes_args \{(.*?)\} hmv_reproject_boxes_args;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)\s*(?=[,;])", fields)
    assert names == [f[0] for f in _lib.HmvReprojectBoxesArgs._fields_] and names[0] == "struct_size"
    import handmvnet_amd
    assert callable(handmvnet_amd.reproject_crop_boxes)


def _args(**over):
    """A well-formed argument struct on fake non-null addresses: every refusal comes before the first HIP call, so none is read."""
    a = _lib.HmvReprojectBoxesArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvReprojectBoxesArgs)
    a.B, a.V, a.margin, a.square, a.require_all = 2, 4, 0, 1, 0
    for i, (name, _) in enumerate(_lib.HmvReprojectBoxesArgs._fields_[6:]):
        setattr(a, name, 0x1000 * (i + 1))
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over, text", [
    (dict(struct_size=0), b"struct_size"), (dict(struct_size=ctypes.sizeof(_lib.HmvReprojectBoxesArgs) - 8), b"struct_size"),
    (dict(B=0), b"B must"), (dict(B=-2), b"B must"), (dict(V=0), b"V must"), (dict(V=17), b"V must"), (dict(B=1 << 23), b"B * V"),
    (dict(margin=-1), b"margin"),
    (dict(points3d=None), b"points3d is NULL"), (dict(intrinsic=None), b"intrinsic is NULL"), (dict(extrinsic=None), b"extrinsic is NULL"),
    (dict(crop_boxes=None), b"crop_boxes is NULL"), (dict(status=None), b"status is NULL"), (dict(source=None), b"source is NULL"),
])
def test_raw_entry_refuses_bad_arguments_without_a_device(over, text):
    lib = _lib.load()
    rc = lib.hmv_op_reproject_crop_boxes(0, ctypes.byref(_args(**over)), None)
    msg = lib.hmv_last_error(None)
    assert rc == _lib.HMV_ERR_ARG and msg and b"hmv_op_reproject_crop_boxes" in msg and text in msg, (over, rc, msg)


def test_raw_entry_refuses_null_args():
    lib = _lib.load()
    assert lib.hmv_op_reproject_crop_boxes(0, None, None) == _lib.HMV_ERR_ARG
    assert b"args is NULL" in lib.hmv_last_error(None)


def test_python_refusals_come_before_the_library():
    from handmvnet_amd.tracking import SequenceTracker, reproject_crop_boxes
    p, k, e = torch.zeros(2, 21, 3), torch.ones(2, 4, 4), torch.eye(4).repeat(2, 4, 1, 1)
    boxes, st = torch.zeros(2, 4, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"\[B, 21, 3\]"):
        reproject_crop_boxes(torch.zeros(2, 20, 3), k, e, boxes, st)
    with pytest.raises(ValueError, match="intrinsics must be"):
        reproject_crop_boxes(p, torch.ones(2, 4, 3), e, boxes, st)
    with pytest.raises(ValueError, match="V <= 16"):
        reproject_crop_boxes(p, torch.ones(2, 17, 4), e, boxes, st)
    with pytest.raises(ValueError, match="extrinsics must be"):
        reproject_crop_boxes(p, k, e[:, :3], boxes, st)
    with pytest.raises(ValueError, match="crop_boxes must be a"):
        reproject_crop_boxes(p, k, e, boxes[:, :2], st)
    with pytest.raises(ValueError, match="integer tensor"):
        reproject_crop_boxes(p, k, e, boxes.float(), st)
    with pytest.raises(ValueError, match="status must be"):
        reproject_crop_boxes(p, k, e, boxes, st.float())
    with pytest.raises(ValueError, match="status must be"):
        reproject_crop_boxes(p, k, e, boxes, st[:1])
    with pytest.raises(ValueError, match="point_status must be"):
        reproject_crop_boxes(p, k, e, boxes, st, point_status=torch.zeros(2, 20, dtype=torch.int32))
    with pytest.raises(ValueError, match="joints_img must be"):
        reproject_crop_boxes(p, k, e, boxes, st, joints_img=torch.zeros(2, 4, 21))
    with pytest.raises(ValueError, match="margin"):
        reproject_crop_boxes(p, k, e, boxes, st, margin=-1)
    with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
        reproject_crop_boxes(p, k, e, boxes, st)

    class _Model:      # what SequenceTracker reads in front of its device check
        num_views = 4
    for kw, text in ((dict(windows="pose"), "windows must be"), (dict(pose="both"), "pose must be")):
        with pytest.raises(ValueError, match=text):
            SequenceTracker(_Model(), boxes, {"intrinsic": k, "extrinsic": e}, **kw)
