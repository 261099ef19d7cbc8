"""Heat-map confidences without a GPU: tests/confidence_oracle.py against golden/confidence_cases.npz (the reference's own functions,
make_confidence_fixture.py) exactly, the twelve levels from 0.5, the entries in the header, the library and the binding, and every
refusal of hmv_op_heatmap_peaks, hmv_op_confidence_select and the Python layer, which come before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import confidence_oracle as co
from handmvnet_amd import _lib
from handmvnet_amd.confidence import confidence_mask, heatmap_peaks, heatmaps_to_coordinates
from handmvnet_amd.triangulation import triangulate, triangulate_dlt
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(GOLDEN, "confidence_cases.npz"), allow_pickle=False)
KEYS = ("mask", "level", "lowered", "selected")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the oracle against the fixture
@pytest.mark.parametrize("case", range(4))
def test_oracle_peaks_are_torch_max_and_the_reference_s_preds(case):
    got = co.peaks(FIX[f"peaks{case}/scores"])
    for k, a in zip(("maxval", "index", "preds"), got):
        assert same_bits(a, FIX[f"peaks{case}/{k}"]), (case, k)


def test_the_fixture_holds_the_edge_maps():
    s, idx, mx, preds = (FIX[f"peaks2/{k}"] for k in ("scores", "index", "maxval", "preds"))
    s, idx, mx, preds = s.reshape(-1, 576), idx.reshape(-1), mx.reshape(-1), preds.reshape(-1, 2)
    assert idx[0] == 0 and idx[1] == 575                                         # first and last index
    assert s[2, idx[2] + 1] == mx[2] and s[3, idx[3] + 64] == mx[3]              # ties a lane and 64 apart: the lowest index
    assert idx[4] == 5 and mx[4] == 0 and np.signbit(mx[4]) and s[4, 9] == 0 and not np.signbit(s[4, 9])   # -0 before +0: equal
    assert mx[5] < 0 and not preds[5].any()                                      # negatives only: preds zeroed
    assert np.isneginf(mx[6]) and idx[6] == 0                                    # -inf only
    assert np.isnan(mx[7]) and np.isnan(s[7]).sum() == 2 and idx[7] == np.flatnonzero(np.isnan(s[7]))[0] and np.nanmax(s[7]) == 3.0
    assert FIX["peaks1/scores"].shape == (3, 5, 5, 7) and FIX["peaks3/scores"].shape == (1, 3, 64, 64)
    assert os.path.getsize(os.path.join(GOLDEN, "confidence_cases.npz")) < 200 * 1024


@pytest.mark.parametrize("name", ["gate", "masked"])
def test_oracle_selection_is_the_fixture_s(name):
    extra = dict(present=FIX["masked/present"], joint_mask=FIX["masked/joint_mask"]) if name == "masked" else {}
    got = co.select(FIX["gate/conf"], 0.5, 0.05, carry=True, **extra)
    for k in KEYS:
        assert same_bits(got[k], FIX[f"{name}/{k}"]), (name, k)
    assert (got["selected"] >= 2).all() and np.array_equal(got["selected"], (got["mask"] == 0).sum(1))
    if name == "masked":
        out = (FIX["masked/present"][:, :, None] == 0) | (FIX["masked/joint_mask"] != 0)
        assert (got["mask"][out] == 1).all()


def test_the_fixture_separates_carry_and_the_fp32_comparison():
    conf = FIX["gate/conf"]
    carry, free = co.select(conf, carry=True), co.select(conf, carry=False)
    assert len(set(carry["level"].reshape(-1).tolist())) >= 4 and carry["level"].min() <= 0
    differs = (carry["mask"] != free["mask"]).any(axis=1)
    own = (conf > np.float32(0.5)).sum(axis=1) >= 2
    assert (differs & own & (carry["level"] < 0.5) & (carry["lowered"] == 0)).any()      # decided lower only because of the carry
    assert (free["level"][own] == 0.5).all()
    # a comparison in double selects other views somewhere: confidences equal to float32(level) are in the fixture
    wrong = np.zeros_like(carry["mask"])
    for b in range(conf.shape[0]):
        t = 0.5
        for j in range(conf.shape[2]):
            while True:
                sel = conf[b, :, j].astype(np.float64) > t
                if t <= 0 or sel.sum() > 1:
                    break
                t -= 0.05
            wrong[b, :, j] = ~sel
    assert (wrong != carry["mask"]).any()


def test_the_twelve_levels_from_one_half():
    lv = co.levels(0.5, 0.05)
    assert len(lv) == 12 and lv[0] == 0.5 and lv[1] == 0.45
    assert lv[9] == 0.05000000000000007 and 0 < lv[10] < 1e-16 and lv[11] == -0.04999999999999993
    assert not (np.array([0.4], dtype=np.float32) > 0.4)[0] and float(np.float32(0.4)) > 0.4      # fp32 against double
    assert FIX["gate/level"].min() == np.float32(lv[11]) and FIX["gate/lowered"].max() == 8


# ---------------------------------------------------------------- header, library, binding
def test_the_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    lib = _lib.load()
    for sym, struct, cls in (("hmv_op_heatmap_peaks", "hmv_peaks_args", _lib.HmvPeaksArgs),
                             ("hmv_op_confidence_select", "hmv_confidence_select_args", _lib.HmvConfidenceSelectArgs)):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header)
        assert hasattr(lib, sym) and sym in _lib.SYMBOLS and len(getattr(lib, sym).argtypes) == 3
        fields = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        assert re.findall(r"(\w+)\s*(?=[,;])", fields) == [f[0] for f in cls._fields_]
        assert cls._fields_[0][0] == "struct_size"
    assert ctypes.sizeof(_lib.HmvPeaksArgs) == 24 + 4 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.HmvConfidenceSelectArgs) == 24 + 16 + 7 * ctypes.sizeof(ctypes.c_void_p)
    from handmvnet_amd import build
    assert "confidence.hip" in build.SOURCES
    import handmvnet_amd
    for name in ("heatmap_peaks", "heatmaps_to_coordinates", "confidence_mask", "triangulate_dlt"):
        assert callable(getattr(handmvnet_amd, name))


def _peaks(**over):
    a = _lib.HmvPeaksArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvPeaksArgs)
    a.N, a.J, a.h, a.w = 2, 21, 32, 32
    a.heatmap, a.maxval, a.index, a.preds = 0x1000, 0x2000, 0x3000, 0x4000
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _select(**over):
    a = _lib.HmvConfidenceSelectArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvConfidenceSelectArgs)
    a.B, a.V, a.J, a.carry, a.threshold, a.step = 2, 5, 21, 1, 0.5, 0.05
    a.conf, a.present, a.joint_mask, a.mask_out, a.level, a.lowered, a.selected = (0x1000 * i for i in range(1, 8))
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over, text", [
    (dict(struct_size=0), b"struct_size"), (dict(struct_size=ctypes.sizeof(_lib.HmvPeaksArgs) + 8), b"struct_size"),
    (dict(heatmap=None), b"heatmap is NULL"), (dict(maxval=None, index=None, preds=None), b"all NULL"),
    (dict(N=0), b"N must"), (dict(N=-1), b"N must"), (dict(J=0), b"J must"), (dict(h=0), b"h must"), (dict(w=0), b"w must"), (dict(w=-4), b"w must"),
    (dict(N=1 << 20, J=17), b"N * J"), (dict(h=1024, w=1025), b"h * w"), (dict(h=1 << 16, w=1 << 16), b"h * w"),
])
def test_peaks_refuses_bad_arguments_without_a_device(over, text):
    lib = _lib.load()
    rc = lib.hmv_op_heatmap_peaks(0, ctypes.byref(_peaks(**over)), None)
    msg = lib.hmv_last_error(None)
    assert rc == _lib.HMV_ERR_ARG and msg and b"hmv_op_heatmap_peaks" in msg and text in msg, (over, rc, msg)


@pytest.mark.parametrize("over, text", [
    (dict(struct_size=0), b"struct_size"), (dict(struct_size=ctypes.sizeof(_lib.HmvConfidenceSelectArgs) - 8), b"struct_size"),
    (dict(conf=None), b"conf is NULL"), (dict(mask_out=None), b"mask_out is NULL"),
    (dict(B=0), b"B must"), (dict(B=-2), b"B must"), (dict(V=0), b"V must"), (dict(V=17), b"V must"), (dict(J=0), b"J must"), (dict(J=65), b"J must"),
    (dict(carry=2), b"carry"), (dict(carry=-1), b"carry"),
    (dict(threshold=float("nan")), b"threshold must be finite"), (dict(threshold=float("inf")), b"threshold must be finite"),
    (dict(threshold=float("-inf")), b"threshold must be finite"),
    (dict(step=float("nan")), b"step"), (dict(step=float("inf")), b"step"), (dict(step=0.0), b"step"), (dict(step=-0.05), b"step"),
    (dict(threshold=1.0, step=0.0009), b"threshold / step"), (dict(threshold=1e300, step=1e-300), b"threshold / step"),
])
def test_select_refuses_bad_arguments_without_a_device(over, text):
    lib = _lib.load()
    rc = lib.hmv_op_confidence_select(0, ctypes.byref(_select(**over)), None)
    msg = lib.hmv_last_error(None)
    assert rc == _lib.HMV_ERR_ARG and msg and b"hmv_op_confidence_select" in msg and text in msg, (over, rc, msg)


def test_both_refuse_null_args():
    lib = _lib.load()
    for f in (lib.hmv_op_heatmap_peaks, lib.hmv_op_confidence_select):
        assert f(0, None, None) == _lib.HMV_ERR_ARG
        assert b"args is NULL" in lib.hmv_last_error(None)


def test_python_refusals_come_before_the_library():
    hm, conf = torch.zeros(2, 4, 21, 8, 8), torch.zeros(2, 4, 21)
    for f, arg in ((heatmap_peaks, hm), (heatmaps_to_coordinates, hm[0]), (confidence_mask, conf)):
        with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
            f(arg)
    with pytest.raises(ValueError, match=r"\[\.\.\., J, h, w\]"):
        heatmap_peaks(torch.zeros(8, 8))
    with pytest.raises(ValueError, match="at least one map"):
        heatmap_peaks(torch.zeros(0, 21, 8, 8))
    with pytest.raises(ValueError, match="2\\^20"):
        heatmap_peaks(torch.zeros(1, 1, 1, (1 << 20) + 1))
    with pytest.raises(ValueError, match="4-dim"):
        heatmaps_to_coordinates(hm)
    # no quiet conversion: the maps and the confidences are fp32 or refused
    with pytest.raises(ValueError, match="heatmap must be float32"):
        heatmap_peaks(hm.half())
    with pytest.raises(ValueError, match="heatmap must be float32"):
        heatmap_peaks(hm.double())
    with pytest.raises(ValueError, match="conf must be float32"):
        confidence_mask(conf.double())
    with pytest.raises(ValueError, match="confidences must be float32"):
        triangulate(torch.zeros(2, 4, 21, 2), torch.ones(2, 4, 4), torch.eye(4).repeat(2, 4, 1, 1), confidences=conf.half())
    with pytest.raises(ValueError, match=r"\[B, V, J\]"):
        confidence_mask(conf[0])
    with pytest.raises(ValueError, match="1 <= V"):
        confidence_mask(torch.zeros(2, 17, 21))
    with pytest.raises(ValueError, match="1 <= J"):
        confidence_mask(torch.zeros(2, 4, 65))
    for kw, text in ((dict(threshold=float("nan")), "finite"), (dict(step=float("inf")), "finite"), (dict(step=0), "step must be > 0"),
                     (dict(step=-1), "step must be > 0"), (dict(threshold=2.0, step=0.001), "levels"), (dict(threshold="high"), "numbers"),
                     (dict(present=torch.ones(2, 5)), "present must be"), (dict(joint_mask=torch.ones(2, 4)), "joint_mask must be")):
        with pytest.raises(ValueError, match=text):
            confidence_mask(conf, **kw)
    # triangulate(confidences=...) and the drop-in
    p, k, e = torch.zeros(2, 4, 21, 2), torch.ones(2, 4, 4), torch.eye(4).repeat(2, 4, 1, 1)
    with pytest.raises(ValueError, match="confidences must be"):
        triangulate(p, k, e, confidences=torch.zeros(2, 4, 20))
    with pytest.raises(ValueError, match="step must be > 0"):
        triangulate(p, k, e, confidences=conf, confidence_step=0.0)
    with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
        triangulate(p, k, e, confidences=conf)
    K = torch.zeros(4, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 600.0
    K[:, 2, 2] = 1.0
    skew = K.clone()
    skew[1, 0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        triangulate_dlt(p[0], conf[0], skew, e[0])
    with pytest.raises(ValueError, match=r"confis must be a \[N, J\]"):
        triangulate_dlt(p[0], conf[0, :, :20], K, e[0])
    with pytest.raises(ValueError, match=r"pts must be a \[N, J, 2\]"):
        triangulate_dlt(p, conf[0], K, e[0])
    with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
        triangulate_dlt(p[0], conf[0], K, e[0])
    assert "Deliberately different" in triangulate_dlt.__doc__ and "carry=True" in triangulate_dlt.__doc__


def test_forward_absolute_refuses_a_bad_confidence_before_the_forward():
    from handmvnet_amd import HandMvNet
    from helpers import load_case
    _, (tp, mp, dp), _, _, _ = load_case("tiny_r18")
    m = HandMvNet(tp, mp, dp)
    assert m.absolute_confidence is None
    x = torch.zeros(1, m.num_views, 3, 64, 64)
    cp = {"intrinsic": torch.ones(1, m.num_views, 4), "extrinsic": torch.eye(4).repeat(1, m.num_views, 1, 1)}
    for bad, text in (((0.5, 0.05), "threshold, step, carry"), (float("nan"), "finite"), ((0.5, 0.0, True), "step must be > 0")):
        with pytest.raises(ValueError, match=text):
            m.forward_absolute(x, torch.zeros(1, m.num_views, 4), cp, confidence=bad)
