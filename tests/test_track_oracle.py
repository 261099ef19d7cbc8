"""Window following without a GPU: the numpy oracle (tests/track_oracle.py) against the fixture written by the real reference functions
(tests/golden/make_track_fixture.py), the three new C-ABI symbols, and the refusals of next_crop_boxes that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import track_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "track_cases.npz"))
NAMES = sorted({k.split(".")[0] for k in FIX.files})
NEW_SYMBOLS = ["hmv_op_next_crop_boxes", "hmv_forward_frames_track", "hmv_forward_frames_views_track"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixture_holds_the_cases_the_rule_needs():
    for need in ("h_gt_w_even", "h_gt_w_odd", "w_gt_h_even", "w_gt_h_odd", "h_eq_w", "square_false", "negative_trunc", "on_integers",
                 "non_square_window", "empty_window", "outside_frame"):
        assert need in NAMES
    assert {int(FIX[f"{n}.size"]) for n in NAMES} == {64, 256} and {int(FIX[f"{n}.margin"]) for n in NAMES} == {0, 20}
    assert sum(FIX[f"{n}.boxes"].shape[0] for n in NAMES if n.startswith("random")) >= 200


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference_fixture(name):
    boxes, bbox, img, status = to.next_crop_boxes(FIX[f"{name}.joints"], FIX[f"{name}.boxes"], int(FIX[f"{name}.size"]),
                                                  int(FIX[f"{name}.margin"]), bool(FIX[f"{name}.square"]))
    assert (status == 0).all()
    assert boxes.dtype == np.int32 and (boxes == FIX[f"{name}.out"]).all()
    assert (bits(img) == bits(FIX[f"{name}.joints_img"])).all()
    assert (bits(bbox) == bits(FIX[f"{name}.out"].astype(np.float32))).all()
    assert (bits(to.joints_to_frame(FIX[f"{name}.joints"], FIX[f"{name}.boxes"], int(FIX[f"{name}.size"]))) == bits(img)).all()


def test_oracle_status_codes():
    j, b = FIX["random_64_m0.joints"][:6].copy(), FIX["random_64_m0.boxes"][:6].copy()
    j[1, 4, 0] = np.nan
    j[2, 7, 1] = 1e12
    j[3, 0, 0], b[3] = 40000.0 * 64, [0, 0, 2, 2]          # frame x up to 80 000: a window wider than 65536 px
    present = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    boxes, bbox, img, status = to.next_crop_boxes(j, b, 64, 0, True, present)
    assert status.tolist() == [0, 2, 2, 2, 1, 0]
    assert (boxes[1:5] == b[1:5]).all() and (img[4] == 0).all() and np.isnan(img[1, 4, 0])
    ref = to.next_crop_boxes(FIX["random_64_m0.joints"][:6], FIX["random_64_m0.boxes"][:6], 64, 0, True)
    assert (boxes[[0, 5]] == ref[0][[0, 5]]).all() and (boxes[0] != b[0]).any()


def test_new_symbols_are_declared_and_exported():
    from handmvnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    declared = set(re.findall(r"\b(hmv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/handmv.h"
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), f"{sym} is not exported / bound"
    import handmvnet_amd
    for name in ("SequenceTracker", "next_crop_boxes", "joints_to_frame"):
        assert callable(getattr(handmvnet_amd, name))


def test_next_crop_boxes_refusals_without_a_device():
    from handmvnet_amd import _lib
    from handmvnet_amd.tracking import joints_to_frame, next_crop_boxes
    j, b = torch.zeros(2, 3, 21, 2), torch.zeros(2, 3, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        next_crop_boxes(torch.zeros(2, 3, 20, 2), b, 64)            # not 21 joints
    with pytest.raises(ValueError):
        next_crop_boxes(j, b[:, :2], 64)                            # one window per row of joints
    with pytest.raises(ValueError):
        next_crop_boxes(j, b.float(), 64)                           # windows are integers
    with pytest.raises(ValueError):
        next_crop_boxes(j, b, 64, present=torch.ones(2, 2))         # present has the leading shape
    with pytest.raises(ValueError):
        next_crop_boxes(j, b, 0)
    with pytest.raises(ValueError):
        next_crop_boxes(j, b, 64, margin=-1)
    with pytest.raises(_lib.HandMvError, match="MI355X only"):
        next_crop_boxes(j, b, 64)                                   # CPU tensors: no fallback
    with pytest.raises(_lib.HandMvError, match="MI355X only"):
        joints_to_frame(j, b, 64)


def test_raw_entry_refuses_bad_arguments_before_any_hip_call():
    """hmv_op_next_crop_boxes checks its arguments in front of hipSetDevice: the refusals come back on a box without a GPU too."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    p = 4096   # never dereferenced
    for args, word in (((0, 0, p, p, None, 64, 0, 1, p, None, None, None, None), b"n_slots"),
                       ((0, 4, p, p, None, 0, 0, 1, p, None, None, None, None), b"image_size"),
                       ((0, 4, p, p, None, 64, -1, 1, p, None, None, None, None), b"margin"),
                       ((0, 4, None, p, None, 64, 0, 1, p, None, None, None, None), b"required"),
                       ((0, 4, p, None, None, 64, 0, 1, p, None, None, None, None), b"required"),
                       ((0, 4, p, p, None, 64, 0, 1, None, None, None, None, None), b"required")):
        assert lib.hmv_op_next_crop_boxes(*args) == 1
        assert word in lib.hmv_last_error(None)
