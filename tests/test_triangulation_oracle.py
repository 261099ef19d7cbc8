"""Triangulation without a GPU: tests/triangulation_oracle.py against every expectation of golden/triangulation_cases.npz (the
reference's own functions, make_triangulation_fixture.py), candidate_table against itertools and random, the entry in the header, the
library and the binding, and every refusal of hmv_op_triangulate and of the Python layer, which come before any HIP call."""
import ctypes
import itertools
import os
import random
import re

import numpy as np
import pytest
import torch

import triangulation_oracle as to
from handmvnet_amd import _lib
from handmvnet_amd.triangulation import (batch_triangulate_dlt_ransac_torch, batch_triangulate_dlt_torch, candidate_table,
                                         triangulate)
from triangulation_helpers import FIX, PLAIN, THR, ransac_inputs, scattered, term

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close64(got, want, name):
    assert (np.isnan(got) == np.isnan(want)).all(), name
    with np.errstate(invalid="ignore"):
        d = float(np.nanmax(np.abs(got - want)))
    print(f"{name}: oracle vs the reference's float64 {d:.3e} (bar {term(name):.3e})")
    assert d <= term(name), (name, d)


# ---------------------------------------------------------------- the oracle against the fixture
@pytest.mark.parametrize("name", PLAIN)
def test_oracle_plain(name):
    got = to.triangulate(FIX[f"{name}/points"], FIX[f"{name}/intr"], FIX[f"{name}/ext"], kind=1)
    close64(got["points3d"], FIX[f"{name}/points3d"], name)
    V = FIX[f"{name}/points"].shape[1]
    assert not got["status"].any() and (got["winner"] == -1).all() and (got["inliers"] == V).all()
    assert np.isfinite(got["reproj_err"]).all() and got["reproj_err"].max() < 20      # 2 px of noise


@pytest.mark.parametrize("name", ["ransac_v5_k3", "masked_ransac"])
def test_oracle_ransac_winners_inliers_and_points(name):
    for refit in (False, True):
        got = to.triangulate(refit=refit, **ransac_inputs(name))
        for k in ("winner", "inliers", "status"):
            assert np.array_equal(got[k], FIX[f"{name}/{k}"]), (name, k, refit)
        close64(got["points3d"], FIX[f"{name}/points3d_refit" if refit else f"{name}/points3d"], name)
    assert float(FIX[f"{name}/threshold_margin"]) >= 1e-2
    ok = FIX[f"{name}/status"] == 0
    win = FIX[f"{name}/winner"][ok]
    assert len(set(win.tolist())) >= 3 and (win != 0).mean() >= 0.25      # a wrong tie-break would show
    assert float(FIX[f"{name}/ref_f32_deviation"]) < 1e-5


def test_oracle_masked_plain_and_crop():
    got = to.triangulate(FIX["plain_v5/points"], FIX["plain_v5/intr"], FIX["plain_v5/ext"], kind=1, present=FIX["masked/present"],
                         joint_mask=FIX["masked/joint_mask"])
    assert np.array_equal(got["status"], FIX["masked_plain/status"]) and (got["status"] == to.TOO_FEW).any()
    close64(got["points3d"], FIX["masked_plain/points3d"], "masked_plain")
    use = (FIX["masked/present"][:, :, None] != 0) & (FIX["masked/joint_mask"] == 0)
    assert np.array_equal(np.isnan(got["reproj_err"]), ~use | (got["status"] == to.TOO_FEW)[:, None, :])
    assert np.array_equal(got["inliers"], np.where(got["status"] == 0, use.sum(1), 0))
    boxes = FIX["crop/boxes"].astype(np.float32)
    size = int(FIX["crop/image_size"])
    assert np.array_equal(to.to_frame(FIX["crop/points"], boxes, size), FIX["crop/frame"])
    got = to.triangulate(FIX["crop/points"], FIX["plain_v5/intr"], FIX["plain_v5/ext"], kind=1, bbox=boxes, image_size=size)
    close64(got["points3d"], FIX["crop/points3d"], "crop")


def test_oracle_kinds_frame_and_statuses():
    pts, intr, ext = FIX["plain_v5/points"], FIX["plain_v5/intr"], FIX["plain_v5/ext"]
    c2w = np.linalg.inv(ext.astype(np.float64))
    a = to.triangulate(pts, intr, c2w, kind=0)["points3d"]
    b = to.triangulate(pts, intr, np.linalg.inv(c2w), kind=1)["points3d"]
    assert np.abs(a - b).max() <= term("plain_v5")
    world = to.triangulate(pts, intr, ext, kind=1)["points3d"]
    cam = to.triangulate(pts, intr, ext, kind=1, frame_cam=[2, 0, 4])["points3d"]
    for i, c in enumerate([2, 0, 4]):
        want = world[i] @ ext[i, c, :3, :3].astype(np.float64).T + ext[i, c, :3, 3]
        assert np.abs(cam[i] - want).max() < 1e-12
    got = to.triangulate(scattered(pts), intr, ext, kind=1, subsets=to.candidate_table(5, 3), threshold=1.0)
    assert (got["status"] == to.NO_INLIER).all() and not got["points3d"].any() and (got["winner"] == -1).all()
    assert not got["inliers"].any() and np.isfinite(got["reproj_err"]).all()      # the errors of the point that is written: 0, 0, 0
    one = np.zeros((3, 5), dtype=np.uint8)
    one[:, 3] = 1
    got = to.triangulate(pts, intr, ext, kind=1, present=one)
    assert (got["status"] == to.TOO_FEW).all() and np.isnan(got["points3d"]).all() and np.isnan(got["reproj_err"]).all()
    bad = pts.copy()
    bad[1, 2, 5, 0] = np.nan
    got = to.triangulate(bad, intr, ext, kind=1)
    assert got["status"][1, 5] == to.NOT_FINITE and got["status"].sum() == to.NOT_FINITE


# ---------------------------------------------------------------- candidate_table
def test_candidate_table_is_itertools_and_the_reference_s_shuffle():
    t = candidate_table(5, 3)
    assert t.dtype == np.int32 and t.flags["C_CONTIGUOUS"] and t.tolist() == [list(c) for c in itertools.combinations(range(5), 3)]
    assert candidate_table(8, 3).shape == (56, 3) and candidate_table(8, 3, n_iterations=20).shape == (20, 3)
    assert candidate_table(13, 4).shape == (100, 4)      # 715 combinations cut to the default n_iterations
    state = random.getstate()
    try:
        for seed in (0, 7, 12345):
            random.seed(seed)
            want = list(itertools.combinations(range(6), 3))
            random.shuffle(want)      # triangulation.py:25-26
            assert candidate_table(6, 3, seed=seed).tolist() == [list(c) for c in want]
            assert candidate_table(6, 3, n_iterations=7, seed=seed).tolist() == [list(c) for c in want[:7]]
    finally:
        random.setstate(state)
    before = random.getstate()
    candidate_table(6, 3, seed=3)
    assert random.getstate() == before      # the process-global state is not touched
    assert np.array_equal(candidate_table(5, 3, seed=int(FIX["seed"])), FIX["ransac_v5_k3/table"])
    assert np.array_equal(candidate_table(5, 3, seed=int(FIX["seed"])), to.candidate_table(5, 3, seed=int(FIX["seed"])))
    for V, k in ((4, 1), (4, 5), (1, 2)):
        with pytest.raises(ValueError, match="n_cams"):
            candidate_table(V, k)
    with pytest.raises(ValueError, match="n_iterations"):
        candidate_table(4, 2, n_iterations=0)


# ---------------------------------------------------------------- header, library, binding
def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    assert re.search(r"\bint\s+hmv_op_triangulate\s*\(", header)
    assert re.search(r"\}\s*hmv_triangulate_args\s*;", header)
    lib = _lib.load()
    assert hasattr(lib, "hmv_op_triangulate") and "hmv_op_triangulate" in _lib.SYMBOLS
    assert len(lib.hmv_op_triangulate.argtypes) == 3
    # 9 int32 fields, one float and 13 pointers, as the header lays them out
    assert ctypes.sizeof(_lib.HmvTriangulateArgs) == 10 * 4 + 13 * ctypes.sizeof(ctypes.c_void_p)
    fields = re.search(r"typedef struct hmv_triangulate_args \{(.*?)\} hmv_triangulate_args;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)\s*(?=[,;])", fields)
    assert names == [f[0] for f in _lib.HmvTriangulateArgs._fields_]
    import handmvnet_amd
    for name in ("triangulate", "candidate_table", "batch_triangulate_dlt_torch", "batch_triangulate_dlt_ransac_torch"):
        assert callable(getattr(handmvnet_amd, name))


def _args(**over):
    """A well-formed argument struct on fake non-null addresses: every refusal comes before the first HIP call, so none is read."""
    a = _lib.HmvTriangulateArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvTriangulateArgs)
    a.B, a.V, a.J, a.S, a.n_cams, a.image_size, a.extrinsic_kind, a.refit, a.threshold = 2, 5, 21, 10, 3, 256, 0, 1, 10.0
    a.points, a.bbox, a.intrinsic, a.extrinsic, a.present, a.joint_mask, a.subsets, a.frame_cam = (0x1000 * i for i in range(1, 9))
    a.points3d, a.reproj_err, a.inliers, a.winner, a.status = (0x1000 * i for i in range(9, 14))
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over, text", [
    (dict(struct_size=0), b"struct_size"), (dict(struct_size=ctypes.sizeof(_lib.HmvTriangulateArgs) - 8), b"struct_size"),
    (dict(B=0), b"B must"), (dict(B=-3), b"B must"), (dict(V=0), b"V must"), (dict(V=17), b"V must"), (dict(J=0), b"J must"),
    (dict(J=65), b"J must"), (dict(B=1 << 20), b"B * J"),
    (dict(points=None), b"points is NULL"), (dict(intrinsic=None), b"intrinsic"), (dict(extrinsic=None), b"extrinsic is NULL"),
    (dict(points3d=None), b"points3d"), (dict(status=None), b"status"),
    (dict(S=0), b"S must"), (dict(S=4097), b"S must"), (dict(n_cams=1), b"n_cams"), (dict(n_cams=6), b"n_cams"),
    (dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=float("inf")), b"threshold"),
    (dict(threshold=float("nan")), b"threshold"),
    (dict(image_size=0), b"image_size"), (dict(extrinsic_kind=2), b"extrinsic_kind"), (dict(extrinsic_kind=-1), b"extrinsic_kind"),
    (dict(refit=2), b"refit"), (dict(refit=-1), b"refit"), (dict(subsets=None, refit=2), b"refit"),
])
def test_triangulate_refuses_bad_arguments_without_a_device(over, text):
    lib = _lib.load()
    rc = lib.hmv_op_triangulate(0, ctypes.byref(_args(**over)), None)
    msg = lib.hmv_last_error(None)
    assert rc == _lib.HMV_ERR_ARG and msg and b"hmv_op_triangulate" in msg and text in msg, (over, rc, msg)


def test_triangulate_refuses_null_args():
    lib = _lib.load()
    assert lib.hmv_op_triangulate(0, None, None) == _lib.HMV_ERR_ARG
    assert b"args is NULL" in lib.hmv_last_error(None)


def test_python_refusals_come_before_the_library():
    p, k, e = torch.zeros(2, 4, 21, 2), torch.ones(2, 4, 4), torch.eye(4).repeat(2, 4, 1, 1)
    with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
        triangulate(p, k, e)
    with pytest.raises(ValueError, match=r"\[B, V, J, 2\]"):
        triangulate(p[0], k, e)
    with pytest.raises(ValueError, match="J <= 64|1 <= J"):
        triangulate(torch.zeros(2, 4, 65, 2), k, e)
    with pytest.raises(ValueError, match="V <= 16|1 <= V"):
        triangulate(torch.zeros(2, 17, 21, 2), k, e)
    with pytest.raises(ValueError, match="extrinsics must be"):
        triangulate(p, k, e[:, :3])
    with pytest.raises(ValueError, match="intrinsics must be"):
        triangulate(p, torch.ones(2, 4, 3), e)
    with pytest.raises(ValueError, match="extrinsic_kind"):
        triangulate(p, k, e, extrinsic_kind="w2c")
    with pytest.raises(ValueError, match="image_size"):
        triangulate(p, k, e, bbox=torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match="bbox must be"):
        triangulate(p, k, e, bbox=torch.zeros(2, 4), image_size=256)
    with pytest.raises(ValueError, match="present must be"):
        triangulate(p, k, e, present=torch.ones(2, 5))
    with pytest.raises(ValueError, match="joint_mask must be"):
        triangulate(p, k, e, joint_mask=torch.ones(2, 4))
    with pytest.raises(ValueError, match="2 .. V"):
        triangulate(p, k, e, subsets=[[0, 1, 2, 3, 0]])
    with pytest.raises(ValueError, match="integer"):
        triangulate(p, k, e, subsets=[[0.5, 1.0]])
    with pytest.raises(ValueError, match="threshold"):
        triangulate(p, k, e, subsets=[[0, 1]], threshold=0)
    # the drop-ins: the reference's [B, N, 3, 3] matrices, anything the device does not take is refused
    K = torch.zeros(2, 4, 3, 3)
    K[..., 0, 0] = K[..., 1, 1] = 600.0
    K[..., 2, 2] = 1.0
    skew = K.clone()
    skew[0, 1, 0, 1] = 0.5
    last = K.clone()
    last[1, 2, 2, 2] = 2.0
    for bad in (skew, last):
        with pytest.raises(ValueError, match="skew"):
            batch_triangulate_dlt_torch(p, bad, e)
        with pytest.raises(ValueError, match="skew"):
            batch_triangulate_dlt_ransac_torch(p, bad, e)
    with pytest.raises(ValueError, match=r"\[B, N, 3, 3\]"):
        batch_triangulate_dlt_torch(p, k, e)
    with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
        batch_triangulate_dlt_torch(p, K, e)
    with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
        batch_triangulate_dlt_ransac_torch(p, K, e, n_cams=2, seed=1)
    for f in (batch_triangulate_dlt_torch, batch_triangulate_dlt_ransac_torch):
        assert "1e-7" in f.__doc__ and "Deliberately different" in f.__doc__
    assert "random" in batch_triangulate_dlt_ransac_torch.__doc__
