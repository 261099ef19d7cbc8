"""Camera-subset sweeps on the GPU: HandMvNet.forward_subsets / hmv_forward_subsets / evaluate_subsets -- one backbone pass, the
fusion tail per subset.

The rule that defines every number: subset s's outputs and epoch values are what forward_views / evaluate give on the same batches
with view_mask equal to subset s on every sample.  So the bars are equal bits and equal values against those entries (which
tests/test_gpu_views.py and test_gpu_views_eval.py tie to the reference), plus, directly, the reference's fixture on the diagonal of
the sweep at test_forward_views_matches_reference_and_oracle's tolerances.

The subsets are the cases' own `views` lists (views_r18_v7: 7, 1, 2, 3 and 5 cameras -- a one-camera subset without keys in the cross
block, the partial 32-key chunk, two chunks on one wave, idle waves, subsets that are no camera prefixes) and one duplicate."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import loss_oracle as lo
from helpers import check_against_fixture, rel_l2
from views_cases import VIEWS_CASES
from views_helpers import OUT_KEYS, load_views_case, oracle_per_sample, per_sample

pytestmark = pytest.mark.gpu

TOL_CAM, TOL_STAGE = 1e-3, 2e-4          # test_gpu_views.py's bars (test_gpu_parity.py's for its tiny r18 / r50_lq cases)
MODES = ["f32", "f32x3", "f16"]
DEV = torch.device("cuda:0")
NAME = "views_r18_v7"


def _subsets(name):
    views = [list(v) for v in VIEWS_CASES[name]["views"]]
    return views + [list(views[-1])]      # ... and one duplicate of an earlier subset


def _build(name, mode, tp_over=None):
    from handmvnet_amd import HandMvNet
    case = load_views_case(name)
    tp, mp, dp = case["params"]
    m = HandMvNet(dict(tp, **(tp_over or {})), mp, dp)
    m.load_state_dict(case["sd"], strict=True)
    m.to("cuda").eval()
    if mode == "f16":
        m.half()
    elif mode == "f32x3":
        m.float32x3()
    return m


@functools.lru_cache(maxsize=None)
def _model(name, mode):
    return _build(name, mode)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return tuple(torch.from_numpy(a).to(DEV) for a in load_views_case(name)["inputs"])


def _np(out):
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in OUT_KEYS}


def _sweep_on(m, name, subsets):
    x, bbox, intr = _inputs(name)
    return _np(m.forward_subsets(x, subsets, bbox, {"intrinsic": intr}))


@functools.lru_cache(maxsize=None)
def _sweep(name, mode):
    """The case's sweep over its own subsets (read-only arrays, shared by the tests below)."""
    out = _sweep_on(_model(name, mode), name, _subsets(name))
    for a in out.values():
        a.setflags(write=False)
    return out


def _mask_of(subset, B, V):
    m = np.zeros((B, V), dtype=bool)
    m[:, subset] = True
    return m


# ---------------------------------------------------------------- 1. bits per subset
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_every_subset_has_the_bits_of_forward_views(name, mode):
    m, (x, bbox, intr), got = _model(name, mode), _inputs(name), _sweep(name, mode)
    B, V = x.shape[:2]
    subsets = _subsets(name)
    assert got["joints_cam"].shape == (len(subsets), B, 21, 3)
    for s, sub in enumerate(subsets):
        ref = _np(m.forward_views(x, _mask_of(sub, B, V), bbox, {"intrinsic": intr}))
        assert np.array_equal(got["joints_cam"][s], ref["joints_cam"]), (name, mode, s, sub, float(np.abs(got["joints_cam"][s] - ref["joints_cam"]).max()))
    full = _np(m(x, bbox, {"intrinsic": intr}))
    for k in ("joints_crop_img", "heatmap"):
        assert got[k].shape == full[k].shape and np.array_equal(got[k], full[k]), (name, mode, k)
    m.check_range()      # the sweep's pair conversions report into the handle's range word like any forward's; nothing clamps here


# ---------------------------------------------------------------- 2. the reference, directly: the diagonal of the sweep
@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_the_diagonal_meets_the_reference_fixture_and_the_oracle(name):
    """Sample b under subset views[b] is the ragged case's sample b: the reference's fixture and the f64 oracle, both built with
    num_views = its view count, at test_forward_views_matches_reference_and_oracle's tolerances."""
    case, got = load_views_case(name), _sweep(name, "f32")
    cfg = case["cfg"]
    px = 0.05 * cfg.image_size / cfg.heatmap_size
    for b, (s, ref) in enumerate(zip(case["samples"], oracle_per_sample(name))):
        assert _subsets(name)[b] == s["views"]
        mine = per_sample({"joints_cam": got["joints_cam"][b], "joints_crop_img": got["joints_crop_img"], "heatmap": got["heatmap"]}, case, b)
        rep = check_against_fixture(mine, s["fx"], tol_cam=TOL_CAM, tol_coord_px=px, tol_stage=TOL_STAGE)
        orc = {k: rel_l2(mine[k], ref[k]) for k in ("joints_cam", "heatmap")}
        orc["crop_px"] = float(np.abs(mine["joints_crop_img"] - ref["joints_crop_img"]).max())
        print(name, b, s["views"], "fixture", rep, "oracle", orc)
        assert orc["joints_cam"] <= TOL_CAM and orc["heatmap"] <= TOL_STAGE and orc["crop_px"] < px, (b, orc)


# ---------------------------------------------------------------- 3. chunking and order
@pytest.mark.parametrize("mode", MODES)
def test_bits_do_not_depend_on_the_chunks_or_the_order(mode):
    """A fusion pass takes max(B, reserved batch) virtual samples: a fresh handle (reservation B: one subset per pass), then the same
    handle reserved for 3 B (three subsets per pass) and for 3 B + 2 (passes that cut through a subset): the same bits.  Permuted
    subsets: permuted outputs, nothing else.  The duplicate equals its original."""
    subsets, want = _subsets(NAME), _sweep(NAME, mode)
    B = VIEWS_CASES[NAME]["B"]
    m = _build(NAME, mode)
    for reserve in (None, 3 * B, 3 * B + 2):
        if reserve:
            m.reserve(reserve, 64, 64)
        got = _sweep_on(m, NAME, subsets)
        for k in OUT_KEYS:
            assert np.array_equal(got[k], want[k]), (mode, reserve, k)
    perm = [3, 5, 0, 2, 4, 1]
    got = _sweep_on(m, NAME, [subsets[i] for i in perm])
    assert np.array_equal(got["joints_cam"], want["joints_cam"][perm]), mode
    for k in ("joints_crop_img", "heatmap"):
        assert np.array_equal(got[k], want[k]), (mode, k)
    assert np.array_equal(want["joints_cam"][-1], want["joints_cam"][len(subsets) - 2])
    del m


# ---------------------------------------------------------------- 4. poisoned workspace
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_poisoned_workspace(name, mode):
    """A sweep after the workspace was filled with NaN patterns: finite, and the bits of the sweep before -- no pad column and no
    retained or packed row that is read without having been written."""
    want, m = _sweep(name, mode), _model(name, mode)
    m.poison_workspace(0xFF)
    again = _sweep_on(m, name, _subsets(name))
    for k in OUT_KEYS:
        assert np.isfinite(again[k]).all(), (name, mode, k)
        assert np.array_equal(again[k], want[k]), (name, mode, k)


# ---------------------------------------------------------------- 5. launch arithmetic
def test_the_backbone_runs_once():
    """Reservation B puts one subset into a pass, so the launch count is (per-frame stage) + S x (one tail): subsets of one size,
    n(5) - n(1) == 4 (n(2) - n(1)), and a tail is less than half of a forward's launches."""
    from handmvnet_amd.subsets import k_of_n
    m, (x, bbox, intr) = _build(NAME, "f32"), _inputs(NAME)
    subsets = k_of_n(7, 3)[3:8]
    n = {}
    for S in (1, 2, 5):
        m.forward_subsets(x, subsets[:S], bbox, {"intrinsic": intr})
        n[S] = m.launch_count()
    m(x, bbox, {"intrinsic": intr})
    forward = m.launch_count()
    torch.cuda.synchronize()
    tail = n[2] - n[1]
    print("launches", n, "forward", forward, "tail", tail)
    assert tail > 0 and n[5] - n[1] == 4 * tail
    assert 2 * tail < forward
    del m


# ---------------------------------------------------------------- 6. ABI refusals
def test_raw_abi_refuses_before_any_launch():
    from handmvnet_amd import _lib
    lib = _lib.load()
    m, (x, bbox, intr) = _model(NAME, "f32"), _inputs(NAME)
    want = _sweep(NAME, "f32")
    B, V = x.shape[:2]
    h = m._engine(64, 64, 0)
    m.forward_subsets(x, _subsets(NAME), bbox, {"intrinsic": intr})
    launches = lib.hmv_launch_count(h)
    crop = torch.full((B, V, 21, 2), float("nan"), device=DEV)
    cam = torch.full((2, B, 21, 3), float("nan"), device=DEV)
    good = np.ascontiguousarray(np.array([[1] * V, [0, 1] + [0] * (V - 2)], dtype=np.uint8))
    empty = good.copy()
    empty[1] = 0

    def call(batch, S, table):
        ptr = table.ctypes.data_as(ctypes.c_void_p) if table is not None else None
        return lib.hmv_forward_subsets(h, batch, S, ptr, x.data_ptr(), bbox.data_ptr(), intr.data_ptr(), crop.data_ptr(), cam.data_ptr(), None, None)
    for what, args in {"n_subsets = 0": (B, 0, good), "a subset without a camera": (B, 2, empty), "a null table": (B, 2, None),
                       "batch = 0": (0, 2, good)}.items():
        rc = call(*args)
        msg = lib.hmv_last_error(h)
        assert rc != 0 and msg and b"hmv_forward_subsets" in msg, (what, rc, msg)
        assert lib.hmv_launch_count(h) == launches, what
    torch.cuda.synchronize()
    assert torch.isnan(crop).all() and torch.isnan(cam).all()      # nothing was launched
    from handmvnet_amd.subsets import as_subset_table
    with pytest.raises(ValueError, match="no camera"):
        m.forward_subsets(x, [[0, 1], []], bbox, {"intrinsic": intr})
    assert call(B, 2, good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cam[0].cpu().numpy(), want["joints_cam"][0])      # (subset 0 of the case is the full rig)
    assert as_subset_table(good, V).tobytes() == good.tobytes()
    # no stages after a sweep, as after a ragged call
    m.capture_stages(True)
    try:
        m.forward_subsets(x, _subsets(NAME), bbox, {"intrinsic": intr})
        with pytest.raises(_lib.HandMvError, match="ragged"):
            m.read_stage("tokens")
    finally:
        m.capture_stages(False)


# ---------------------------------------------------------------- 7. epoch numbers
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}
ROOT_IDX = 3


@functools.lru_cache(maxsize=None)
def _labelled(mode):
    """views_r18_v7 with loss weights, and synthetic labels around its own full-view forward (host arrays, never written)."""
    case = load_views_case(NAME)
    model = _build(NAME, mode, {"loss_weights": WEIGHTS, "mask_invisible_joints": True})
    x, bbox, intr = case["inputs"]
    B, V = x.shape[:2]
    rig = lo.loss_case("vii_many")
    assert rig["V"] >= V and rig["B"] >= B
    own = _np(model(*(torch.from_numpy(a).to(DEV) for a in (x, bbox)), {"intrinsic": torch.from_numpy(intr).to(DEV)}))
    S, hs = model.data_params["image_size"], own["heatmap"].shape[-1]
    rng = np.random.default_rng(19)
    gt_crop = np.clip(own["joints_crop_img"] + rng.standard_normal(own["joints_crop_img"].shape) * 2, -5, S + 5).astype(np.float32)
    d = dict(rgb=x, bboxes=bbox, intr=intr, extr=np.ascontiguousarray(rig["extr"][:B, :V]), gt_crop=gt_crop,
             root_mm=(rig["root_joint"][:B] * 1000).astype(np.float32),
             gt_cam_mm=((own["joints_cam"] + rng.standard_normal(own["joints_cam"].shape) * 0.006) * 1000).astype(np.float32),
             jmask=rng.random((B, V, 21)) < 0.2, heat=lo.target_heatmaps(gt_crop, S, hs, hs).astype(np.float32))
    return model, d


def _batch(d, sl):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    data = {"rgb": dev(d["rgb"][sl]), "bboxes": dev(d["bboxes"][sl]), "joints_cam": dev(d["gt_cam_mm"][sl]),
            "root_joint": dev(d["root_mm"][sl]), "joints_crop_img": dev(d["gt_crop"][sl]), "joints_img_mask": dev(d["jmask"][sl]),
            "root_idx": torch.tensor([ROOT_IDX]), "heatmap": dev(d["heat"][sl])}
    return {"data": data, "cam_params": {"intrinsic": dev(d["intr"][sl]), "extrinsic": dev(d["extr"][sl])}}


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_epoch_numbers_equal_evaluate_per_subset(mode):
    """Two steps of different batch size (5 and 3 samples): every value of evaluate_subsets()["per_subset"][s] equals evaluate() on
    copies of the same batches carrying mask s -- the same launches on the same bits, the same fp64 order: exact equality."""
    from handmvnet_amd.subsets import SubsetSweepEvaluator
    model, d = _labelled(mode)
    V = d["rgb"].shape[1]
    subsets = _subsets(NAME)
    batches = [_batch(d, slice(0, 5)), _batch(d, slice(2, 5))]
    got = model.evaluate_subsets(copy.deepcopy(batches), subsets)
    assert got["subsets"] == subsets and len(got["per_subset"]) == len(subsets)
    for s, sub in enumerate(subsets):
        mine = copy.deepcopy(batches)
        for b in mine:
            b["view_mask"] = torch.from_numpy(_mask_of(sub, b["data"]["rgb"].shape[0], V))
        want = model.evaluate(mine)
        assert want["samples"] == 8 and want["steps"] == 2 and want["test/loss"] is not None
        assert set(got["per_subset"][s]) == set(want)
        for k, v in want.items():
            print(mode, s, sub, k, got["per_subset"][s][k], v)
            assert got["per_subset"][s][k] == v, (mode, s, k)
    counts = sorted({len(s) for s in subsets})
    assert sorted(got["by_count"]) == counts
    for k in counts:
        rows = [r for r, sub in zip(got["per_subset"], subsets) if len(sub) == k]
        assert got["by_count"][k]["subsets"] == len(rows)
        for key in ("test_mpjpe", "test_pa_mpjpe", "test_mpjpe2d", "test_auc_j", "test/loss", "test/heatmap_loss"):
            assert got["by_count"][k][key] == pytest.approx(np.mean([r[key] for r in rows]), rel=1e-12), (k, key)
    # a second epoch after reset() repeats the first
    ev = SubsetSweepEvaluator(model, subsets, "test")
    for b in copy.deepcopy(batches):
        ev.step(b)
    first = ev.compute()
    assert first == got
    ev.reset()
    for b in copy.deepcopy(batches):
        ev.step(b)
    assert ev.compute() == first
