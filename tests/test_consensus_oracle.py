"""tests/consensus_oracle.py (numpy float64, the operation order of hmv_op_pose_consensus) against the reference and against closed
forms.

The alignment is checked against tests/golden/consensus_cases.npz, written by golden/make_consensus_fixture.py from the real
reference: transform_joints_between_cameras (utils/camera.py:4-22) on float64 inputs, T(x) - T(0).  The oracle and the reference differ
only in how the 4x4 is inverted; the generator stored the largest deviation it measured, and the bar is 100 times that value (room for
another inversion routine), itself asserted to be at most 1e-9 m -- below fp32 resolution at the 0.1 m scale of the poses.

Mean, median, spread and deviation are pinned to closed forms."""
import os

import numpy as np
import pytest

import consensus_oracle as co
from helpers import GOLDEN


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "consensus_cases.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def test_alignment_matches_the_reference_fixture(fx):
    S, B = fx["poses"].shape[:2]
    assert (S, B, fx["extrinsic"].shape[1]) == (5, 3, 8)
    bar = 100.0 * float(fx["oracle_deviation"])
    assert 0 < bar <= 1e-9
    got = co.align(fx["poses"], fx["ref_cam"], fx["extrinsic"], int(fx["target"]))
    err = float(np.abs(got - fx["aligned"]).max())
    print("alignment: max |oracle - reference| =", err, "bar", bar)
    assert err <= bar
    # a rigid rig: the rotation keeps every length
    assert np.allclose(np.linalg.norm(got, axis=-1), np.linalg.norm(fx["poses"].astype(np.float64), axis=-1), rtol=0, atol=1e-6)
    assert np.abs(fx["extrinsic"][..., :3, 3]).max() > 1.0 and np.abs(fx["poses"]).max() < 1.0


def test_the_inverse_rows_invert(fx):
    E = fx["extrinsic"].astype(np.float64)
    T = co.inverse_rows(E)
    assert T.shape == E.shape[:-2] + (3, 4)
    assert np.abs(T @ E - np.eye(4)[:3]).max() < 1e-12
    singular = np.zeros((4, 4))
    assert not np.isfinite(co.inverse_rows(singular)).any()


def test_the_target_camera_s_own_estimate_is_unchanged(fx):
    """ref_cam == target: M is inverse(E) E, the identity up to the rounding of the inverse."""
    got = co.align(fx["poses"][:1], [4], fx["extrinsic"], 4)
    assert np.abs(got[0] - fx["poses"][0]).max() < 1e-15


def test_identical_poses_have_no_spread():
    rng = np.random.default_rng(1)
    one = rng.standard_normal((1, 2, 21, 3)) * 0.1
    x = np.repeat(one, 4, axis=0)
    y, spread, dev = co.reduce(x, "mean")       # 4 x / 4: exact
    assert np.array_equal(y, one[0])
    assert np.array_equal(spread, np.zeros((2, 21))) and np.array_equal(dev, np.zeros((4, 2)))
    # the median's steps divide by the 1e-12 floor and back: (4 x / 1e-12) / (4 / 1e-12) is x to a few roundings (|x| < 1: 1e-15)
    y, spread, dev = co.reduce(x, "median")
    assert np.abs(y - one[0]).max() < 1e-15 and spread.max() < 1e-15 and dev.max() < 1e-15


def test_one_estimate_is_returned_as_it_is():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1, 3, 21, 3)) * 0.1
    y, spread, dev = co.reduce(x, "mean")
    assert np.array_equal(y, x[0]) and not spread.any() and not dev.any()
    y, spread, dev = co.reduce(x, "median")      # (x / 1e-12) / (1 / 1e-12): x to a few roundings
    assert np.abs(y - x[0]).max() < 1e-15 and spread.max() < 1e-15 and dev.max() < 1e-15
    y, spread, dev = co.reduce(x, "median", iterations=0)
    assert np.array_equal(y, x[0]) and not spread.any() and not dev.any()


def test_two_estimates_keep_the_median_at_the_mean():
    """Both points are equally far from their midpoint, so every Weiszfeld step returns it (up to rounding)."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 2, 21, 3)) * 0.1
    mean, spread, dev = co.reduce(x, "mean")
    median, spread_m, dev_m = co.reduce(x, "median", iterations=16)
    assert np.array_equal(mean, (x[0] + x[1]) / 2.0)
    assert np.abs(median - mean).max() < 1e-15
    half = np.linalg.norm(x[0] - x[1], axis=-1) / 2.0
    assert np.allclose(spread, half, rtol=1e-14, atol=0) and np.allclose(dev, np.broadcast_to(half.mean(-1), (2, 2)), rtol=1e-14, atol=0)
    assert np.allclose(spread_m, spread, rtol=1e-12, atol=0) and np.allclose(dev_m, dev, rtol=1e-12, atol=0)


def test_one_weiszfeld_step_on_three_points_by_hand():
    """Joint 0 of one sample: x = (0,0,0), (3,0,0), (0,4,0).  Mean (1, 4/3, 0); distances 5/3, sqrt(52)/3, sqrt(73)/3; one step gives
    (sum x_s / d_s) / (sum 1 / d_s)."""
    x = np.zeros((3, 1, 21, 3))
    x[1, 0, :, 0] = 3.0
    x[2, 0, :, 1] = 4.0
    mean, spread, dev = co.reduce(x, "mean")
    assert np.allclose(mean[0, 0], [1.0, 4.0 / 3.0, 0.0], rtol=1e-15)
    d = np.array([5.0, np.sqrt(52.0), np.sqrt(73.0)]) / 3.0
    assert np.allclose(spread[0, 0], np.sqrt((d ** 2).sum() / 3.0), rtol=1e-15)
    assert np.allclose(dev[:, 0], d, rtol=1e-15)
    y1, _, _ = co.reduce(x, "median", iterations=1)
    w = 1.0 / d
    want = np.array([3.0 * w[1], 4.0 * w[2], 0.0]) / w.sum()
    assert np.allclose(y1[0, 0], want, rtol=1e-15)
    y0, _, _ = co.reduce(x, "median", iterations=0)
    assert np.array_equal(y0, mean)
    # many steps approach the Fermat point of the right triangle, which is nearer the right angle than the mean is
    y64, _, _ = co.reduce(x, "median", iterations=64)
    assert np.linalg.norm(y64[0, 0]) < np.linalg.norm(mean[0, 0])
    total = lambda p: sum(np.linalg.norm(x[s, 0, 0] - p) for s in range(3))      # noqa: E731
    assert total(y64[0, 0]) < total(y1[0, 0]) < total(mean[0, 0])


def test_a_point_on_the_current_estimate_takes_the_floor():
    """d_s = 0 is replaced by 1e-12: the step stays finite and lands on that point."""
    x = np.zeros((3, 1, 21, 3))
    x[0, 0, :, 0], x[2, 0, :, 0] = -1.0, 1.0          # the mean IS x[1]
    y, spread, dev = co.reduce(x, "median", iterations=3)
    assert np.isfinite(y).all() and np.abs(y).max() < 1e-11


def test_an_out_of_range_reference_camera_gives_nan(fx):
    got = co.pose_consensus(fx["poses"], [3, 0, 8, 5, -1], fx["extrinsic"], 2)
    assert np.isnan(got["aligned"][2]).all() and np.isnan(got["aligned"][4]).all() and np.isfinite(got["aligned"][[0, 1, 3]]).all()
    assert np.isnan(got["deviation"][[2, 4]]).all() and np.isnan(got["consensus"]).all() and np.isnan(got["spread"]).all()
