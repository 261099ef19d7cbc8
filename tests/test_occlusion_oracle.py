"""Occlusion sweeps without a GPU: the numpy oracle of the occluder against the reference fixture (the real OcclusionAugmentation with
scripted randomness, tests/golden/make_occlusion_fixture.py), cell_rects against the reference's patch grid, grid_variants' argument
errors, the two new entries in the header, the binding and the library, and the evaluator's sensitivity arithmetic."""
import os
import re
import types

import numpy as np
import pytest
import torch

import occlusion_oracle as oo
from handmvnet_amd import _lib
from handmvnet_amd.occlusion import OcclusionSweepEvaluator, cell_rects, grid_variants, sensitivity_maps
from oracle import frames_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "occlusion_cases.npz"))
NAMES = sorted({k.split(".")[0] for k in FIX.files})


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_the_reference_fixture(name):
    """5e-6 in normalised units: the bar of the plain filter's oracle (tests/test_frames_oracle.py)."""
    frames, boxes, rects, size = FIX[f"{name}.frames"], FIX[f"{name}.boxes"], FIX[f"{name}.rects"], int(FIX[f"{name}.size"])
    for (p, r, c), rect in zip(FIX[f"{name}.patches"], rects):
        assert oo.patch_rect(int(p), int(r), int(c)) == rect.tolist()
    got = oo.prepare_batch_occluded(frames, boxes, rects, size)
    assert got.shape == FIX[f"{name}.out"].shape
    assert np.abs(got - FIX[f"{name}.out"]).max() < 5e-6
    # the occluder changes the result (the fixture would pin nothing otherwise) ...
    assert np.abs(got - fo.prepare_batch(frames, boxes, size)).max() > 1e-3
    # ... and zeroing the frame pixels instead gives the identical window, hence the identical view
    zeroed = oo.zero_batch(frames, boxes, rects)
    for f, z, b, r in zip(frames, zeroed, boxes, rects):
        assert np.array_equal(fo.crop_and_pad(z, b), oo.occluded_window(f, b, r))
    assert np.array_equal(fo.prepare_batch(zeroed, boxes, size), got)


def test_fixture_covers_the_cases_it_is_for():
    p = np.concatenate([FIX[f"{n}.patches"][:, 0] for n in NAMES])
    assert 8 in p and 64 in p
    b, (ps, r, c) = FIX["odd_scale.boxes"][1], FIX["odd_scale.patches"][1]
    assert (b[3] - b[1]) % ps != 0 and r == (b[3] - b[1]) // ps - 1 and c == (b[2] - b[0]) // ps - 1   # the last valid row / column
    b = FIX["two_sides.boxes"][0]
    assert b[0] < 0 and b[1] < 0 and FIX["two_sides.rects"][0][2] + b[0] > 0        # the patch partly over padding
    b = FIX["non_square.boxes"][0]
    assert b[3] - b[1] < b[2] - b[0]
    b = FIX["upsample.boxes"][0]
    assert b[2] - b[0] < int(FIX["upsample.size"])


def test_oracle_clips_and_ignores_empty_rectangles():
    rng = np.random.default_rng(3)
    frame = rng.integers(1, 256, (40, 50, 3), dtype=np.uint8)
    box = [-5, 10, 35, 45]   # 40 x 35, leaves the frame left and below
    clean = fo.prepare_view(frame, box, 16)
    for rect in ([7, 7, 7, 30], [9, 12, 3, 20], [40, 0, 90, 35], [-9, -9, 0, 50], [2 ** 31 - 1, 0, -2 ** 31, 5]):
        assert np.array_equal(oo.prepare_view_occluded(frame, box, rect, 16), clean)
    black = np.broadcast_to(((0 - fo.MEAN) / fo.STD)[:, None, None], (3, 16, 16))
    for rect in ([0, 0, 40, 35], [-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1]):
        assert np.allclose(oo.prepare_view_occluded(frame, box, rect, 16), black, atol=1e-6)
    assert np.array_equal(oo.prepare_view_occluded(frame, box, [-100, 5, 12, 1000], 16), oo.prepare_view_occluded(frame, box, [0, 5, 12, 35], 16))


@pytest.mark.parametrize("grid", [1, 3, 4])
def test_cell_rects_are_patches_the_reference_can_draw(grid):
    """Every cell of the grid on square and non-square windows, one of them smaller than the grid: p = min(cw, ch) // grid, the cell is
    the reference's patch (p, row, col) and lies inside the reference's own patch grid (row < ch // p, col < cw // p)."""
    boxes = torch.tensor([[[10, 20, 90, 100], [-20, -30, 50, 43]], [[5, 7, 105, 57], [17, 3, 44, 92]], [[4, 4, 6, 7], [3, 3, 3, 9]]],
                         dtype=torch.int32)   # 80x80, 70x73 | 100x50, 27x89 | 2x3 (smaller than grids 3 and 4), empty
    for row in range(grid):
        for col in range(grid):
            got = cell_rects(boxes, grid, row, col)
            assert got.dtype == torch.int32 and tuple(got.shape) == (3, 2, 4) and got.device == boxes.device
            for b, g in zip(boxes.reshape(-1, 4).tolist(), got.reshape(-1, 4).tolist()):
                cw, ch = b[2] - b[0], b[3] - b[1]
                p = max(min(cw, ch), 0) // grid
                assert g == oo.patch_rect(p, row, col)
                if p == 0:
                    assert oo.clip_rect(g, max(cw, 0), max(ch, 0)) is None   # an empty rectangle: the clean result
                else:
                    assert row < ch // p and col < cw // p and g[2] <= cw and g[3] <= ch
    assert cell_rects(boxes.long(), grid, 0, 0).dtype == torch.int32
    for bad in ((grid, 0), (0, grid), (-1, 0)):
        with pytest.raises(ValueError):
            cell_rects(boxes, grid, *bad)
    with pytest.raises(ValueError):
        cell_rects(boxes, 0, 0, 0)
    with pytest.raises(ValueError):
        cell_rects(boxes.float(), grid, 0, 0)


def test_grid_variants_order_and_argument_errors():
    assert grid_variants(2, 2) == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
    assert grid_variants(4, 1, cameras=[3, 1]) == [(3, 0, 0), (1, 0, 0)]
    assert grid_variants(3, 2, cameras=np.array([2])) == [(2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1)]
    assert len(grid_variants(8, 4)) == 128
    for kwargs, word in ((dict(V=0, grid=2), "V"), (dict(V=3, grid=0), "grid"), (dict(V=3, grid=2, cameras=[]), "at least one camera"),
                         (dict(V=3, grid=2, cameras=[0, 3]), "cameras[1]: camera 3 is outside [0, 3)"),
                         (dict(V=3, grid=2, cameras=[-1]), "cameras[0]: camera -1 is outside"),
                         (dict(V=3, grid=2, cameras=[1, 2, 1]), "cameras[2]: camera 1 is named twice"),
                         (dict(V=3, grid=2, cameras=[0.5]), "cameras[0]: camera indices must be integers"),
                         (dict(V=3, grid=2, cameras=[True]), "cameras[0]: camera indices must be integers")):
        with pytest.raises(ValueError) as e:
            grid_variants(**kwargs)
        assert word in str(e.value), (kwargs, str(e.value))


def test_the_two_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    lib = _lib.load()
    for sym in ("hmv_op_prepare_frames_occluded", "hmv_forward_frames_occlusions"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in _lib.SYMBOLS
        assert hasattr(lib, sym)
        assert getattr(lib, sym).argtypes is not None
    # the op-level entry refuses null operands before any HIP call
    assert lib.hmv_op_prepare_frames_occluded(0, None, 1, 8, 8, None, None, None, None, 8, 8, None, None) == _lib.HMV_ERR_ARG
    assert lib.hmv_forward_frames_occlusions(None, 1, None, 8, 8, None, None, None, None, None, 1, None, None, None, None, None, None, None,
                                             None) == _lib.HMV_ERR_ARG


def _state(samples, steps, mpjpe_sum, pa_sum, sum2d, loss=None):
    s = np.zeros(15 + 20)
    s[0], s[1], s[2], s[3], s[4] = samples, steps, samples, mpjpe_sum, pa_sum
    s[5], s[6] = samples, sum2d
    s[14] = samples   # every pose inside the first threshold
    if loss is not None:
        s[7] = samples
        s[8:14] = np.asarray(loss) * samples
    return s


def test_sensitivity_is_variant_minus_clean_per_cell():
    model = types.SimpleNamespace(num_views=3, auc_thresh=(0.0, 0.02))
    ev = OcclusionSweepEvaluator(model, grid=2, cameras=[2, 0], mode="test")
    assert ev.variants == [(2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1)]
    assert ev.occ_view.tolist() == [2, 2, 2, 2, 0, 0, 0, 0] and ev.occ_view.dtype == np.int32
    host = np.stack([_state(8, 2, 8 * 0.010, 8 * 0.005, 8 * 3.0, loss=[1, 2, 3, 4, 5, 6])] +
                    [_state(8, 2, 8 * (0.010 + 0.001 * (o + 1)), 8 * 0.005, 8 * (3.0 + o), loss=[1, 2, 3, 4, 5, 6 + o]) for o in range(8)])
    res = ev.finish(host)
    assert set(res) == {"variants", "clean", "per_variant", "sensitivity"}
    assert res["variants"] == ev.variants and len(res["per_variant"]) == 8
    assert res["clean"]["test_mpjpe"] == pytest.approx(10.0) and res["clean"]["samples"] == 8
    sens = res["sensitivity"]
    assert "test_pck_j" not in sens and "thresholds" not in sens and "samples" not in sens and "steps" not in sens
    for key in ("test_mpjpe", "test_pa_mpjpe", "test_mpjpe2d", "test_auc_j", "test/loss", "test/heatmap_loss"):
        m = sens[key]
        assert m.shape == (3, 2, 2) and np.isnan(m[1]).all() and not np.isnan(m[[0, 2]]).any()
        for o, (c, r, k) in enumerate(ev.variants):
            assert m[c, r, k] == res["per_variant"][o][key] - res["clean"][key]
    assert sens["test_mpjpe"][2, 0, 1] == pytest.approx(2.0) and sens["test_mpjpe"][0, 1, 1] == pytest.approx(8.0)
    assert sens["test_mpjpe2d"][0, 0, 0] == pytest.approx(4.0) and not sens["test_pa_mpjpe"][[0, 2]].any()
    assert sens["test/loss"][0, 1, 0] == pytest.approx(6.0)
    # a key that is None (no step carried a loss) stays NaN everywhere
    none = ev.finish(np.stack([_state(4, 1, 0.04, 0.02, 4.0)] * 9))
    assert np.isnan(none["sensitivity"]["test/loss"]).all() and not none["sensitivity"]["test_mpjpe"][[0, 2]].any()
    assert np.array_equal(sensitivity_maps(res["clean"], res["per_variant"], ev.variants, 3, 2)["test_mpjpe"], sens["test_mpjpe"], equal_nan=True)
    with pytest.raises(ValueError):
        ev.finish(np.zeros((9, 35)))   # an empty epoch
    with pytest.raises(ValueError):
        sensitivity_maps(res["clean"], res["per_variant"][:3], ev.variants, 3, 2)
