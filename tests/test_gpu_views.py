"""Ragged view sets on the GPU: HandMvNet.forward_views / hmv_forward_views -- one batch whose samples have different cameras.

A sample's result is defined by the model built with num_views = its number of present views, run on those views in camera order
from the same weights: checked against the real reference's fixture (golden/views_cases.npz), the f64 oracle and, bit for bit, this
engine's own unchanged uniform path."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from guards import Guards
from helpers import check_against_fixture, rel_l2
from views_cases import VIEWS_CASES
from views_helpers import OUT_KEYS, load_views_case, oracle_per_sample, per_sample, sample_inputs

pytestmark = pytest.mark.gpu

TOL_CAM, TOL_STAGE = 1e-3, 2e-4          # test_gpu_parity.py's bars for its tiny r18 / r50_lq cases
MODES = ["f32", "f32x3", "f16"]
DEV = torch.device("cuda:0")


def _build(params, sd, mode):
    from handmvnet_amd import HandMvNet
    m = HandMvNet(*params)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    if mode == "f16":
        m.half()
    elif mode == "f32x3":
        m.float32x3()
    return m


@functools.lru_cache(maxsize=None)
def _model(name, mode):
    case = load_views_case(name)
    return _build(case["params"], case["sd"], mode)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return tuple(torch.from_numpy(a).to(DEV) for a in load_views_case(name)["inputs"])


def _np(out):
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in OUT_KEYS}


def _views(m, x, bbox, intr, mask):
    return _np(m.forward_views(x, mask, bbox, {"intrinsic": intr}))


@functools.lru_cache(maxsize=None)
def _ragged(name, mode):
    """The case's batch through forward_views (read-only arrays, shared by the tests below)."""
    out = _views(_model(name, mode), *_inputs(name), load_views_case(name)["mask"])
    for a in out.values():
        a.setflags(write=False)
    return out


def _same(a, b, what):
    for k in OUT_KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k] - b[k]).max()))


@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_forward_views_matches_reference_and_oracle(name):
    """f32: every sample against the reference's fixture and the f64 oracle, both built with num_views = its view count; the rows of
    absent views are exactly zero."""
    case, got = load_views_case(name), _ragged(name, "f32")
    cfg, B, V = case["cfg"], case["spec"]["B"], case["spec"]["V"]
    px = 0.05 * cfg.image_size / cfg.heatmap_size
    assert got["joints_cam"].shape == (B, 21, 3) and got["joints_crop_img"].shape == (B, V, 21, 2)
    assert got["heatmap"].shape[:3] == (B, V, 21)
    for b, (s, ref) in enumerate(zip(case["samples"], oracle_per_sample(name))):
        mine = per_sample(got, case, b)
        rep = check_against_fixture(mine, s["fx"], tol_cam=TOL_CAM, tol_coord_px=px, tol_stage=TOL_STAGE)
        orc = {k: rel_l2(mine[k], ref[k]) for k in ("joints_cam", "heatmap")}
        orc["crop_px"] = float(np.abs(mine["joints_crop_img"] - ref["joints_crop_img"]).max())
        print(name, b, s["views"], "fixture", rep, "oracle", orc)
        assert orc["joints_cam"] <= TOL_CAM and orc["heatmap"] <= TOL_STAGE and orc["crop_px"] < px, (b, orc)
    absent = ~case["mask"]
    assert absent.any()
    assert not got["joints_crop_img"][absent].any() and not got["heatmap"][absent].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_forward_views_equals_the_uniform_path_per_sample(name, mode):
    """Per sample, a second model object built with num_views = its view count, in the same mode, run through the UNCHANGED forward()
    on that sample alone: the same bits.  (The engine's rule: arithmetic never depends on a size, and the split of a sample's key
    range depends on its own token count alone.)"""
    case, got = load_views_case(name), _ragged(name, mode)
    for b, s in enumerate(case["samples"]):
        m = _build(s["params"], case["sd"], mode)
        x, bbox, intr = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in sample_inputs(case, b))
        ref = _np(m(x, bbox, {"intrinsic": intr}))
        _same(per_sample(got, case, b), ref, (name, mode, b, s["views"]))
        del m


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_full_mask_equals_forward(name, mode):
    m, (x, bbox, intr) = _model(name, mode), _inputs(name)
    a = _views(m, x, bbox, intr, np.ones(x.shape[:2], dtype=bool))
    _same(a, _np(m(x, bbox, {"intrinsic": intr})), (name, mode))


@pytest.mark.parametrize("mode", MODES)
def test_result_does_not_depend_on_the_batch_composition(mode):
    """views_r18_v7 as it is, with its samples in reversed order, and every sample alone: bit-identical per sample."""
    name = "views_r18_v7"
    case, got, m = load_views_case(name), _ragged(name, mode), _model(name, mode)
    x, bbox, intr = _inputs(name)
    mask = case["mask"]
    rev = _views(m, x.flip(0), bbox.flip(0), intr.flip(0), mask[::-1].copy())
    _same({k: v[::-1] for k, v in rev.items()}, got, (mode, "reversed"))
    # (the five calls are enqueued back to back, each with another row table, and read after one synchronisation: a call must not
    # disturb the table of the one in front of it)
    alone = [m.forward_views(x[b:b + 1], mask[b:b + 1], bbox[b:b + 1], {"intrinsic": intr[b:b + 1]}) for b in range(case["spec"]["B"])]
    for b, one in enumerate(alone):
        _same(_np(one), {k: v[b:b + 1] for k, v in got.items()}, (mode, "alone", b))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_poisoned_workspace(name, mode):
    """A ragged call after the workspace was filled with NaN patterns: finite, and the bits of the call before -- no row or pad
    column that the ragged kernels read without having written it."""
    got, m = _ragged(name, mode), _model(name, mode)
    m.poison_workspace(0xFF)
    again = _views(m, *_inputs(name), load_views_case(name)["mask"])
    for k in OUT_KEYS:
        assert np.isfinite(again[k]).all(), (name, mode, k)
    _same(again, got, (name, mode))


def test_raw_abi_refuses_bad_view_counts_before_any_launch():
    from handmvnet_amd import _lib
    lib = _lib.load()
    name = "views_r18_v7"
    m, (x, bbox, intr) = _model(name, "f32"), _inputs(name)
    good = _np(m(x, bbox, {"intrinsic": intr}))
    h = m._engine(64, 64, 0)
    B, V = x.shape[:2]
    crop = torch.full((B * V, 21, 2), float("nan"), device=DEV)
    cam = torch.full((B, 21, 3), float("nan"), device=DEV)
    ptrs = (x.data_ptr(), bbox.data_ptr(), intr.data_ptr(), crop.data_ptr(), cam.data_ptr(), None, None)
    arr = lambda *c: (ctypes.c_int32 * len(c))(*c)
    for what, (batch, counts) in {"a count of 0": (B, arr(7, 0, 2, 3, 5)), "a count above num_views": (B, arr(7, 1, V + 1, 3, 5)),
                                  "B = 0": (0, arr(7, 1, 2, 3, 5)), "a null table": (B, None)}.items():
        rc = lib.hmv_forward_views(h, batch, counts, *ptrs)
        msg = lib.hmv_last_error(h)
        assert rc != 0 and msg and b"hmv_forward_views" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(crop).all() and torch.isnan(cam).all()      # nothing was launched
    _same(_np(m(x, bbox, {"intrinsic": intr})), good, "hmv_forward after the refused calls")
    # ... and stages are not captured for a ragged call
    m.capture_stages(True)
    try:
        m.forward_views(x, load_views_case(name)["mask"], bbox, {"intrinsic": intr})
        with pytest.raises(_lib.HandMvError, match="ragged"):
            m.read_stage("tokens")
        m(x, bbox, {"intrinsic": intr})
        assert m.read_stage("tokens").shape == (B, V * 21, m.feat_dim)
    finally:
        m.capture_stages(False)


SEG = [0, 147, 168, 210, 273, 294]      # token counts 147, 21, 42, 63, 21: the chunk splits of views_r18_v7 and two one-view samples


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("kind", ["f32", "x3", "lq"])
def test_attention_views_kernels_vs_torch(kind, cross):
    """op-level: the ragged attention kernels against torch fp64 softmax attention per sample, at the bar of
    test_attention_kernel_vs_torch / test_lq_attention_kernel_vs_torch for the same kernels (4e-6 of max(|ref|, 1)), sharp rows
    included.  The cross block of the 128-wide heads has two samples WITHOUT keys: their rows are exact zeros."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    D = 256 if kind == "lq" else 128
    B, rows = len(SEG) - 1, SEG[-1]
    g = torch.Generator().manual_seed(100 + 10 * cross + len(kind))
    seg = (ctypes.c_int32 * len(SEG))(*SEG)
    probe = None
    if kind == "lq" and cross:
        probe = torch.randn(21, 8, D, generator=g) * 3.0
        mat = torch.randn(rows, 2, 8, D, generator=g)
        kcol, vcol = 0, 1
    else:
        mat = torch.randn(rows, 3, 8, D, generator=g)
        mat[:, 0] *= 3.0
        kcol, vcol = 1, 2
    gd = Guards(DEV)                        # 0xFF bands around the rows, the probe and the output (which starts as NaN)
    md = gd.inp(mat.reshape(rows, -1))
    pd = gd.inp(probe.reshape(21, 8 * D)) if probe is not None else None
    out_rows = B * 21 if cross else rows
    out = gd.out((out_rows, 8 * D))
    rc = lib.hmv_op_attention_views(0, {"f32": 0, "x3": 1, "lq": 2}[kind], md.data_ptr(), pd.data_ptr() if pd is not None else None, B, seg,
                                    cross, out.data_ptr(), None)
    assert rc == 0, lib.hmv_last_error(None)
    torch.cuda.synchronize()
    gd.check()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    worst = 0.0
    for b in range(B):
        r0, r1 = SEG[b], SEG[b + 1]
        koff = 21 if (cross and kind != "lq") else 0
        q = (probe if probe is not None else mat[r0:(r0 + 21 if cross else r1), 0]).double().permute(1, 0, 2)     # [8, Tq, D]
        k, v = mat[r0 + koff:r1, kcol].double().permute(1, 0, 2), mat[r0 + koff:r1, vcol].double().permute(1, 0, 2)
        mine = got[b * 21:(b + 1) * 21] if cross else got[r0:r1]
        if k.shape[1] == 0:
            assert not mine.any(), (kind, b)
            continue
        ref = (torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1) @ v).permute(1, 0, 2).reshape(-1, 8 * D)
        worst = max(worst, (mine - ref).abs().max().item() / max(ref.abs().max().item(), 1.0))
    print(kind, cross, worst)
    assert worst < 4e-6, worst
