"""The evaluation breakdown without a GPU: the numpy oracle (tests/breakdown_oracle.py) against the fixture written by the real
reference functions (tests/golden/make_breakdown_fixture.py), its identities with the pooled oracle (tests/epoch_oracle.py), the host
side (finish_breakdown, merge_breakdown_states, worst) and the new C-ABI symbols with the argument checks that run before any HIP call.

Tolerances: counts and PCK values exact; distances within 2e-5 relative of the reference's fp32 run, the project's fp64-against-fp32
bar (tests/test_gpu_metrics.py); fp64 sums of the same few thousand non-negative terms in another order within 1e-12 relative."""
import ctypes
import os

import numpy as np
import pytest

import breakdown_oracle as bo
import epoch_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "breakdown_cases.npz"))
SRC = np.load(os.path.join(ROOT, "tests", "golden", "metrics_cases.npz"))
CASES = ("noise_5mm", "similarity", "mirrored", "single_pose_7steps", "many_poses")
NEW_SYMBOLS = ["hmv_eval_breakdown_doubles", "hmv_eval_record_floats", "hmv_eval_breakdown_add"]


def _case(name):
    n = int(FIX[f"{name}.poses"])
    lo, hi, steps = SRC[f"{name}.range"]
    return SRC[f"{name}.pred"][:n], SRC[f"{name}.gt"][:n], float(lo), float(hi), int(steps)


def _flat2d(B, V=1):
    z = np.zeros((B, V, 21, 2), np.float32)
    return z, z


def _invented_2d(rng, B, V):
    g2 = (rng.random((B, V, 21, 2)) * 128).astype(np.float32)
    return g2 + rng.standard_normal(g2.shape).astype(np.float32) * 2, g2, rng.random((B, V, 21)) < 0.2


# ---------------------------------------------------------------- the oracle against the reference
def test_fixture_is_what_the_issue_lists():
    assert [int(FIX[f"{n}.poses"]) for n in CASES] == [16, 8, 8, 1, 64]
    assert FIX["many_poses.pck"].shape == (21, 20) and FIX["single_pose_7steps.pck"].shape == (21, 7)
    assert FIX["crop2d.pred"].shape == (4, 3, 21, 2) and 0.1 < FIX["crop2d.mask"].mean() < 0.3
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "breakdown_cases.npz")) < 64 * 1024


@pytest.mark.parametrize("name", CASES)
def test_oracle_per_joint_equals_reference_fixture(name):
    p, g, lo, hi, steps = _case(name)
    B = p.shape[0]
    state = bo.accumulate(bo.new_state(1, steps), p, g, *_flat2d(B), thr_min=lo, thr_max=hi, steps=steps)
    s = bo.slices(state, 1, steps)
    assert state[:4].tolist() == [B, 1, 1, steps]
    assert np.abs(s["J3"] / B - FIX[f"{name}.mpjpe"]).max() <= 2e-5 * FIX[f"{name}.mpjpe"].min()
    rel_pa = np.abs(s["JPA"] / B - FIX[f"{name}.pa_mpjpe"]) / FIX[f"{name}.pa_mpjpe"]
    print(name, "pa rel", rel_pa.max())
    assert rel_pa.max() <= 2e-5
    counts = np.cumsum(s["H"][:, :steps], axis=1)
    assert np.array_equal(counts, np.round(FIX[f"{name}.pck"] * B))                      # the counts
    assert np.array_equal(counts.astype(np.float32) / np.float32(B), FIX[f"{name}.pck"].astype(np.float32))
    assert (s["H"].sum(1) == B).all() and np.all(s["H"] == np.round(s["H"]))


def test_oracle_per_camera_equals_reference_fixture():
    p2, g2, mask = FIX["crop2d.pred"], FIX["crop2d.gt"], FIX["crop2d.mask"]
    rng = np.random.default_rng(3)
    g = (rng.standard_normal((4, 21, 3)) * 0.04).astype(np.float32)
    state = bo.accumulate(bo.new_state(3), g + np.float32(0.001), g, p2, g2, mask)
    s = bo.slices(state, 3)
    assert s["CN"].tolist() == [4, 4, 4] and np.array_equal(s["CV"], (~mask).sum(0))
    assert np.allclose(s["C2"] / 4, FIX["crop2d.per_camera_joint"], rtol=2e-5, atol=0)
    assert np.allclose(s["C2"].sum(1) / (4 * 21), FIX["crop2d.per_camera"], rtol=2e-5, atol=0)
    assert s["C2"].sum() / (4 * 3 * 21) == pytest.approx(float(FIX["crop2d.pooled"]), rel=2e-5)
    assert (s["C2"][mask.all(0)] == 0).all()                                            # a joint masked in every sample adds 0
    rows = bo.record_rows(g + np.float32(0.001), g, p2, g2, mask)
    assert np.allclose(rows[:, 4:].mean(0), FIX["crop2d.per_camera"], rtol=2e-5, atol=0) and (rows[:, 3] == 3).all()
    assert np.allclose(rows[:, 2], rows[:, 4:].mean(1), rtol=1e-12, atol=0)


# ---------------------------------------------------------------- identities with the pooled oracle
def test_breakdown_sums_to_the_pooled_state():
    rng = np.random.default_rng(5)
    pooled, state, V = eo.new_state(20), bo.new_state(3), 3
    for name in ("noise_5mm", "similarity", "mirrored", "many_poses"):
        p, g, lo, hi, steps = _case(name)
        p2, g2, mask = _invented_2d(rng, p.shape[0], V)
        eo.accumulate(pooled, p, g, p2, g2, mask, None, lo, hi, steps)
        bo.accumulate(state, p, g, p2, g2, mask, None, lo, hi, steps)
    s = bo.slices(state, V)
    assert np.array_equal(s["H"].sum(0), pooled[14:])                                     # exactly
    assert state[0] == pooled[0] == 96 and state[1] == pooled[1] == 4
    for mine, theirs in ((s["J3"].sum(), pooled[3]), (s["JPA"].sum(), pooled[4]), (s["C2"].sum(), pooled[6])):
        assert mine == pytest.approx(theirs, rel=1e-12)
    assert (s["CN"] == 96).all() and s["CV"].sum() < 96 * V * 21


def test_ragged_oracle_never_reads_an_absent_slot():
    rng = np.random.default_rng(6)
    p, g, lo, hi, steps = _case("mirrored")
    p2, g2, mask = _invented_2d(rng, 8, 3)
    present = rng.random((8, 3)) < 0.6
    present[:, 0] |= ~present.any(1)
    poisoned = p2.copy()
    poisoned[~present] = np.nan
    state = bo.accumulate(bo.new_state(3), p, g, poisoned, g2, mask, present)
    s = bo.slices(state, 3)
    assert np.isfinite(state).all() and s["CN"].tolist() == present.sum(0).tolist()
    full = bo.slices(bo.accumulate(bo.new_state(3), p, g, p2, g2, mask), 3)
    assert np.array_equal(full["J3"], s["J3"]) and (s["C2"] <= full["C2"] + 1e-9).all()
    rows = bo.record_rows(p, g, poisoned, g2, mask, present)
    assert np.array_equal(np.isnan(rows[:, 4:]), ~present) and np.isfinite(rows[:, :4]).all()
    assert np.isnan(bo.record_rows(p[:1], g[:1], p2[:1], g2[:1], None, np.zeros((1, 3), bool))[0, 2])


# ---------------------------------------------------------------- the host side of compute()
def _hand_state(V=2, steps=3, samples=4):
    st = bo.new_state(V, steps)
    st[:4] = [samples, 2, V, steps]
    s = bo.slices(st, V, steps)
    s["J3"][:] = np.arange(21) * 0.004
    s["JPA"][:] = np.arange(21) * 0.002
    s["H"][:, 0], s["H"][:, 2], s["H"][:, 3] = 1, 2, 1                                  # of 4 rows per joint: 1, 1, 3 within; 1 beyond
    s["CN"][:] = [4, 3]
    s["C2"][0], s["C2"][1] = 8.0, 6.0
    s["CV"][0], s["CV"][1] = 4, 3
    s["CV"][1, 5] = 0
    s["C2"][1, 5] = 0.0
    return st


def test_finish_breakdown_on_hand_made_states():
    from handmvnet_amd.evaluation import finish_breakdown
    out = finish_breakdown(_hand_state(), 0.0, 0.02, 3, "val")
    assert set(out) == {"val_mpjpe_per_joint", "val_pa_mpjpe_per_joint", "val_pck_per_joint", "val_auc_per_joint", "val_mpjpe2d_per_camera",
                        "val_mpjpe2d_per_camera_joint", "val_mpjpe2d_visible_per_camera", "val_mpjpe2d_visible_per_camera_joint",
                        "camera_samples", "visible_joints"}
    assert out["val_mpjpe_per_joint"] == pytest.approx((np.arange(21) * 0.004 / 4 * 1000).tolist(), rel=1e-15)
    assert out["val_pa_mpjpe_per_joint"] == pytest.approx((np.arange(21) * 0.002 / 4 * 1000).tolist(), rel=1e-15)
    assert out["val_pck_per_joint"] == [[0.25, 0.25, 0.75]] * 21
    thr = eo.mo.linspace_f32(0.0, 0.02, 3)
    auc = np.float32(0) + (thr[1] - thr[0]) * np.float32(0.5) * np.float32(0.5) + (thr[2] - thr[1]) * np.float32(1.0) * np.float32(0.5)
    assert out["val_auc_per_joint"] == pytest.approx([float(auc)] * 21, rel=1e-6)
    assert out["camera_samples"] == [4, 3] and out["visible_joints"][1][5] == 0 and out["visible_joints"][0] == [4] * 21
    assert out["val_mpjpe2d_per_camera"] == [2.0, pytest.approx(6.0 * 20 / (3 * 21))]
    assert out["val_mpjpe2d_per_camera_joint"][0] == [2.0] * 21 and out["val_mpjpe2d_per_camera_joint"][1][5] == 0.0
    assert out["val_mpjpe2d_visible_per_camera_joint"][1][5] is None and out["val_mpjpe2d_visible_per_camera_joint"][1][4] == 2.0
    assert out["val_mpjpe2d_visible_per_camera"] == [2.0, 2.0]
    # a camera no sample had: every quotient over it is None
    st = _hand_state()
    s = bo.slices(st, 2, 3)
    s["CN"][1], s["C2"][1], s["CV"][1] = 0, 0, 0
    gone = finish_breakdown(st, 0.0, 0.02, 3, "val")
    assert gone["val_mpjpe2d_per_camera"][1] is None and gone["val_mpjpe2d_visible_per_camera"][1] is None
    assert gone["val_mpjpe2d_per_camera_joint"][1] == [None] * 21 and gone["camera_samples"] == [4, 0]
    with pytest.raises(ValueError, match="empty epoch"):
        finish_breakdown(bo.new_state(2, 3), 0.0, 0.02, 3, "val")
    with pytest.raises(ValueError, match="not a breakdown state"):
        finish_breakdown(_hand_state()[:-1], 0.0, 0.02, 3, "val")
    with pytest.raises(ValueError, match="not a breakdown state"):
        finish_breakdown(np.zeros(4 + 42 + 21 * 4), 0.0, 0.02, 3, "val")                 # V = 0
    wrong = _hand_state()
    wrong[2] = 4                                                                         # e.g. two states added header and all
    with pytest.raises(ValueError, match="V = 4"):
        finish_breakdown(wrong, 0.0, 0.02, 3, "val")


def test_the_sum_of_two_states_finishes_to_the_unions_numbers():
    from handmvnet_amd.evaluation import finish_breakdown, merge_breakdown_states
    rng = np.random.default_rng(8)
    a, b, both = bo.new_state(2), bo.new_state(2), bo.new_state(2)
    for name, into in (("noise_5mm", a), ("similarity", b), ("mirrored", b)):
        p, g, lo, hi, steps = _case(name)
        p2, g2, mask = _invented_2d(rng, p.shape[0], 2)
        present = np.ones((p.shape[0], 2), bool)
        present[::3, 1] = False
        for st in (into, both):
            bo.accumulate(st, p, g, p2, g2, mask, present, lo, hi, steps)
    merged = merge_breakdown_states(a, b, bo.new_state(2))                              # an idle rank's zero state joins
    assert merged[:4].tolist() == [32, 3, 2, 20]
    got, want = finish_breakdown(merged, 0.0, 0.02, 20, "test"), finish_breakdown(both, 0.0, 0.02, 20, "test")
    assert got["test_pck_per_joint"] == want["test_pck_per_joint"] and got["camera_samples"] == want["camera_samples"] == [32, 20]
    assert got["visible_joints"] == want["visible_joints"]
    for key in ("test_mpjpe_per_joint", "test_pa_mpjpe_per_joint", "test_auc_per_joint", "test_mpjpe2d_per_camera",
                "test_mpjpe2d_visible_per_camera"):
        assert got[key] == pytest.approx(want[key], rel=1e-12), key
    assert np.allclose(got["test_mpjpe2d_per_camera_joint"], want["test_mpjpe2d_per_camera_joint"], rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="cannot be added"):
        merge_breakdown_states(a, bo.accumulate(bo.new_state(2, 7), *_case("single_pose_7steps")[:2], *_flat2d(1, 2), steps=7))
    with pytest.raises(ValueError, match="cannot be added"):
        merge_breakdown_states(a, bo.accumulate(bo.new_state(3), *_case("mirrored")[:2], *_flat2d(8, 3)))


def test_worst_picks_the_largest_in_feed_order():
    from handmvnet_amd.evaluation import worst
    rec = {"mpjpe": np.array([3.0, 9.0, np.nan, 9.0, 1.0]), "mpjpe2d_per_camera": np.zeros((5, 2))}
    assert worst(rec, k=3) == [1, 3, 0] and worst(rec, "mpjpe", 10) == [1, 3, 0, 4, 2] and worst(rec, k=0) == []
    with pytest.raises(ValueError):
        worst(rec, "mpjpe2d_per_camera")


def test_evaluator_refusals_without_a_device():
    from handmvnet_amd.evaluation import EpochEvaluator

    class Labels:
        auc_thresh = [0.0, 0.02]

    with pytest.raises(ValueError, match="records"):
        EpochEvaluator(Labels(), "test", records=-1)
    with pytest.raises(ValueError, match="records=0"):
        EpochEvaluator(Labels(), "test", breakdown=True).records()
    with pytest.raises(ValueError, match="empty epoch"):
        EpochEvaluator(Labels(), "test", breakdown=True).compute()
    ev = EpochEvaluator(Labels(), "test", breakdown=True, records=4)
    ev.views, ev.record_rows = 2, 3
    with pytest.raises(ValueError, match="2 views, the step has 3"):
        ev._check_detail(1, 3)
    with pytest.raises(ValueError, match="record rows"):
        ev._check_detail(2, 2)
    ev._check_detail(1, 2)


# ---------------------------------------------------------------- the C ABI, host side only
def test_new_symbols_sizes_and_struct():
    import re
    from handmvnet_amd import _lib
    from handmvnet_amd.evaluation import breakdown_doubles
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    declared = set(re.findall(r"\b(hmv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert "eval_breakdown.hip" in __import__("handmvnet_amd.build", fromlist=["SOURCES"]).SOURCES
    assert ctypes.sizeof(_lib.HmvEvalBreakdownArgs) == 112
    for V, steps in ((1, 1), (2, 7), (8, 20), (3, 256)):
        want = 4 + 42 + 21 * (steps + 1) + 43 * V
        assert lib.hmv_eval_breakdown_doubles(V, steps) == want == breakdown_doubles(V, steps) == bo.doubles(V, steps)
    assert lib.hmv_eval_breakdown_doubles(8, 20) == 831
    assert [lib.hmv_eval_breakdown_doubles(*a) for a in ((0, 20), (-1, 20), (8, 0), (8, 257), (8, -3))] == [0] * 5
    assert [lib.hmv_eval_record_floats(v) for v in (1, 8, 13, 0, -2)] == [5, 12, 17, 0, 0]


def _args(B=2, V=3, steps=20, records=False):
    """An argument block that passes every check up to the device selection: the pointers are never dereferenced on the host."""
    from handmvnet_amd import _lib
    a = _lib.HmvEvalBreakdownArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvEvalBreakdownArgs)
    a.B, a.V, a.steps, a.thr_min, a.thr_max = B, V, steps, 0.0, 0.02
    a.pred_joints_cam = a.gt_joints_cam = a.pred_joints_2d = a.gt_joints_2d = a.state = 4096
    a.state_doubles = bo.doubles(V, steps)
    if records:
        a.records, a.record_capacity, a.record_base = 4096, 10, 8
    return a


@pytest.mark.parametrize("records, damage, word", [
    (False, lambda a: setattr(a, "struct_size", 104), "struct_size"), (False, lambda a: setattr(a, "B", 0), "B must"),
    (False, lambda a: setattr(a, "V", 0), "V must"), (False, lambda a: (setattr(a, "B", 1 << 13), setattr(a, "V", 1 << 12)), "B * V"),
    (False, lambda a: setattr(a, "steps", 0), "steps must"), (False, lambda a: setattr(a, "steps", 257), "steps must"),
    (False, lambda a: setattr(a, "thr_max", -1.0), "thr_max"), (False, lambda a: setattr(a, "thr_max", float("nan")), "thr_max"),
    (False, lambda a: setattr(a, "pred_joints_cam", None), "pred_joints_cam"), (False, lambda a: setattr(a, "gt_joints_cam", None), "gt_joints_cam"),
    (False, lambda a: setattr(a, "pred_joints_2d", None), "pred_joints_2d"), (False, lambda a: setattr(a, "gt_joints_2d", None), "gt_joints_2d"),
    (False, lambda a: setattr(a, "state", None), "state is NULL"), (False, lambda a: setattr(a, "state", 4100), "8-byte"),
    (False, lambda a: setattr(a, "state_doubles", bo.doubles(3) - 1), "state_doubles"),
    (False, lambda a: setattr(a, "state_doubles", 35), "state_doubles"),               # the pooled state's size is not enough
    (True, lambda a: setattr(a, "records", 4098), "records is not 4-byte"), (True, lambda a: setattr(a, "record_capacity", 0), "record_capacity must"),
    (True, lambda a: setattr(a, "record_base", -1), "record_base must"), (True, lambda a: setattr(a, "record_base", 9), "exceeds record_capacity"),
    (True, lambda a: setattr(a, "record_capacity", 1), "exceeds record_capacity"),
])
def test_breakdown_add_rejects_bad_arguments_before_touching_the_device(records, damage, word):
    from handmvnet_amd import _lib
    lib = _lib.load()
    a = _args(records=records)
    damage(a)
    assert lib.hmv_eval_breakdown_add(0, ctypes.byref(a), None) == _lib.HMV_ERR_ARG
    msg = lib.hmv_last_error(None).decode()
    assert msg.startswith("hmv_eval_breakdown_add: ") and word in msg, msg
    assert lib.hmv_eval_breakdown_add(0, None, None) == _lib.HMV_ERR_ARG and "args is NULL" in lib.hmv_last_error(None).decode()
