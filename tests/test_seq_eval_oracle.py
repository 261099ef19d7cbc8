"""Sequence evaluation without a GPU: the numpy oracle (tests/seq_eval_oracle.py) against the fixture written by the real reference
functions (tests/golden/make_seq_eval_fixture.py), the new C-ABI symbols with the argument checks that run before any HIP call, and
the Python refusals that need no device.

Tolerances: the mapping is compared bit for bit (the same fp32 operations in the same order); MKA and the streamed accumulation to
1e-12 relative, the project's figure for fp64 sums of the same terms in another order (tests/test_gpu_eval_epoch.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import seq_eval_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "seq_eval_cases.npz"))
MAP_NAMES = sorted({k.split(".")[0] for k in FIX.files if k.startswith("map_")})
HAND_NAMES = [n for n in MAP_NAMES if f"{n}.hand_outside" in FIX.files]
MKA_NAMES = sorted({k.split(".")[0] for k in FIX.files if k.startswith("mka_")})
NEW_SYMBOLS = ["hmv_op_labels_to_windows", "hmv_op_mka", "hmv_seq_eval_sums_doubles", "hmv_seq_eval_history_floats", "hmv_seq_eval_add"]
REL = 1e-12


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def case(name):
    return FIX[f"{name}.joints"], FIX[f"{name}.boxes"], int(FIX[f"{name}.size"]), FIX[f"{name}.mask"]


# ---------------------------------------------------------------- the mapping
def test_fixture_holds_the_cases_the_rule_needs():
    assert len(HAND_NAMES) == 6 and len(MAP_NAMES) == 9
    assert {int(FIX[f"{n}.size"]) for n in MAP_NAMES} == {64, 192, 256, 320}
    rnd = [n for n in MAP_NAMES if n.startswith("map_random")]
    assert [FIX[f"{n}.boxes"].shape[0] for n in rnd] == [65, 65, 65]
    boxes = np.concatenate([FIX[f"{n}.boxes"] for n in MAP_NAMES])
    assert (boxes[:, 0] < 0).any() and (boxes[:, 2] - boxes[:, 0] == 1).any() and (boxes[:, 2] - boxes[:, 0] != boxes[:, 3] - boxes[:, 1]).any()
    outside = np.concatenate([FIX[f"{n}.outside"] for n in MAP_NAMES])
    visible = np.concatenate([FIX[f"{n}.visible"] for n in MAP_NAMES])
    assert (outside > 0).any() and (outside == 0).any() and (visible == 0).any()
    assert all(np.isfinite(FIX[f"{n}.out"]).all() for n in MAP_NAMES)
    # joints exactly on 0 count as inside, exactly on S as outside
    e = FIX["map_edges_64.out"][0]
    assert e[0].tolist() == [0, 0] and e[1, 0] == 64 and e[2, 1] == 64 and e[4].tolist() == [63.5, 63.5]
    assert FIX["map_edges_64.hand_outside"].tolist() == [3]


@pytest.mark.parametrize("name", MAP_NAMES)
def test_oracle_mapping_equals_reference_fixture(name):
    joints, boxes, size, mask = case(name)
    crop, mask_out, info = so.labels_to_windows(joints, boxes, size, mask)
    assert crop.dtype == np.float32 and (bits(crop) == bits(FIX[f"{name}.out"])).all()
    assert (info[:, 0] == 0).all()
    assert (info[:, 1] == FIX[f"{name}.outside"]).all() and (info[:, 2] == FIX[f"{name}.visible"]).all()
    assert mask_out.dtype == np.uint8 and (mask_out == (mask != 0)).all()
    if name in HAND_NAMES:
        assert info[:, 1].tolist() == FIX[f"{name}.hand_outside"].tolist() and info[:, 2].tolist() == FIX[f"{name}.hand_visible"].tolist()
    # without a mask every joint is visible, and the mapped joints are the same
    crop2, mask2, info2 = so.labels_to_windows(joints, boxes, size)
    assert (bits(crop2) == bits(crop)).all() and not mask2.any() and (info2[:, 2] == 21).all() and (info2[:, 1] >= info[:, 1]).all()


def test_the_fixture_tells_the_two_operation_orders_apart():
    for size in (192, 320):
        differ = 0
        for name in MAP_NAMES:
            joints, boxes, s, _ = case(name)
            if s == size:
                differ += int((bits(so.map_to_windows_divide(joints, boxes, s)) != bits(FIX[f"{name}.out"])).sum())
        assert differ > 0, size


def test_oracle_empty_windows_and_absent_slots():
    joints, boxes, size, mask = (a[:8].copy() if isinstance(a, np.ndarray) else a for a in case("map_random_256"))
    boxes[1] = [50, 60, 50, 90]                     # zero width
    boxes[2] = [80, 70, 60, 50]                     # negative extents
    boxes[5] = [7, 9, 30, 9]                        # zero height
    present = np.array([1, 1, 0, 1, 0, 1, 1, 1], np.uint8)
    crop, mask_out, info = so.labels_to_windows(joints, boxes, size, mask, present)
    assert info[:, 0].tolist() == [0, 2, 1, 0, 1, 2, 0, 0]          # absent wins over empty
    for n in (1, 2, 4, 5):
        assert not crop[n].any() and mask_out[n].all() and info[n, 1:].tolist() == [0, 0]
    ref = so.labels_to_windows(*case("map_random_256"))
    for n in (0, 3, 6, 7):
        assert (bits(crop[n]) == bits(ref[0][n])).all() and (mask_out[n] == ref[1][n]).all() and (info[n] == ref[2][n]).all()
    assert np.isfinite(crop).all()
    # a non-finite label of a mapped slot counts as outside
    was_out = int(mask[0, 2] == 0 and not ((crop[0, 2] >= 0) & (crop[0, 2] < size)).all())
    joints[0, 2, 0] = np.nan
    mask[0, 2] = 0
    again = so.labels_to_windows(joints, boxes, size, mask, present)
    assert np.isnan(again[0][0, 2, 0]) and again[2][0, 1] == info[0, 1] - was_out + 1


# ---------------------------------------------------------------- MKA and the streamed accumulation
@pytest.mark.parametrize("name", MKA_NAMES)
def test_oracle_mka_matches_reference_float64(name):
    preds, want = FIX[f"{name}.preds"], FIX[f"{name}.ref64"]
    got = so.mka(preds)
    assert got.shape == want.shape
    if preds.shape[1] < 3:
        assert np.isnan(got).all() and np.isnan(want).all()           # T = 2: the mean of an empty tensor
    else:
        assert np.abs(got - want).max() <= REL * np.abs(want).max()
        assert float(FIX[f"{name}.rel"]) < 1e-6                       # the reference's own fp32 run, for information


def _stream(preds, labels=None, restart_at=None, restart_lane=None):
    B, T = preds.shape[:2]
    sums, hist = so.empty_state(B)
    for t in range(T):
        restart = None
        if restart_at is not None and t == restart_at:
            restart = np.zeros(B, np.uint8)
            restart[restart_lane] = 1
        so.accumulate(sums, hist, preds[:, t], None if labels is None else labels[:, t], restart=restart)
    return sums, hist


def test_oracle_accumulate_equals_mka():
    preds = FIX["mka_3x7.preds"]
    labels = preds[::-1].copy()
    sums, hist = _stream(preds, labels)
    B, T = preds.shape[:2]
    assert (sums[:, 0] == T).all() and (sums[:, 1] == T).all() and (sums[:, 2] == (T - 2) * 21).all() and not sums[:, 5:].any()
    want, want_gt = so.mka(preds), so.mka(labels)
    assert np.abs(sums[:, 3] / sums[:, 2] - want).max() <= REL * np.abs(want).max()
    assert np.abs(sums[:, 4] / sums[:, 2] - want_gt).max() <= REL * np.abs(want_gt).max()
    assert (bits(hist[:, 0, 1].reshape(B, 21, 3)) == bits(preds[:, -1])).all() and (bits(hist[:, 1, 0].reshape(B, 21, 3)) == bits(labels[:, -2])).all()
    # without labels [4] and the label history stay untouched
    sums2, hist2 = _stream(preds)
    assert not sums2[:, 4].any() and not hist2[:, 1].any() and (sums2[:, 3] == sums[:, 3]).all()
    # fewer than three steps: no rows, a NaN quotient like the reference's
    short, _ = _stream(FIX["mka_1x2.preds"])
    assert short[0, 2] == 0 and short[0, 3] == 0 and short[0, :2].tolist() == [2, 2]


def test_oracle_accumulate_with_a_restart_pools_the_two_segments():
    preds = FIX["mka_3x7.preds"]
    T = preds.shape[1]
    sums, _ = _stream(preds, restart_at=3, restart_lane=1)
    whole = so.mka(preds)
    assert np.abs(sums[[0, 2], 3] / sums[[0, 2], 2] - whole[[0, 2]]).max() <= REL * whole.max()      # the other lanes do not notice
    a, b = preds[1:2, :3], preds[1:2, 3:]                                                           # segments of 3 and 4 steps
    rows = np.array([1 * 21, 2 * 21])
    pooled = (so.mka(a)[0] * rows[0] + so.mka(b)[0] * rows[1]) / rows.sum()
    assert sums[1, 2] == rows.sum() and sums[1, 0] == T - 3 and sums[1, 1] == T
    assert abs(sums[1, 3] / sums[1, 2] - pooled) <= REL * pooled
    assert abs(sums[1, 3] / sums[1, 2] - whole[1]) > 1e-6 * whole[1]                                  # and that is another number


def test_oracle_accumulate_counts():
    sums, hist = so.empty_state(2)
    pred = FIX["mka_2x3.preds"]
    status = np.array([[0, 2, 1], [0, 0, 5]])
    info = np.array([[[0, 3, 20], [2, 0, 0], [1, 0, 0]], [[0, 0, 21], [0, 1, 7], [2, 0, 0]]])
    for t in range(3):
        so.accumulate(sums, hist, pred[:, t], track_status=status, slot_info=info)
    assert sums[0, 5:11].tolist() == [3, 3, 3, 3, 60, 9] and sums[1, 5:11].tolist() == [6, 0, 0, 3, 84, 3] and not sums[:, 11].any()


# ---------------------------------------------------------------- reduce over ranks (gloo on the CPU) and the host side of compute()
def _rank_state(rank):
    """One rank's streamed sums: two lanes each, other inputs per rank; rank 1 has a step without labels."""
    preds = FIX["mka_3x7.preds"][[rank, 2]]
    labels = preds[::-1].copy()
    rng = np.random.default_rng(40 + rank)
    sums, hist = so.empty_state(2)
    unlabelled = 0
    for t in range(preds.shape[1]):
        status = rng.integers(0, 3, (2, 3))
        info = np.stack([rng.integers(0, 3, (2, 3)), rng.integers(0, 5, (2, 3)), rng.integers(5, 22, (2, 3))], -1)
        gt = None if (rank == 1 and t == 4) else labels[:, t]
        unlabelled += 2 * (gt is None)
        so.accumulate(sums, hist, preds[:, t], gt, status, info if gt is not None else None)
    return sums, unlabelled


def _reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from handmvnet_amd.sequence_eval import finish_sequence, pool_sums, reduce_pooled
        sums, unlabelled = _rank_state(rank)
        pooled = reduce_pooled(pool_sums(torch.from_numpy(sums.reshape(-1)), unlabelled))
        q.put((rank, pooled.numpy().copy(), finish_sequence(sums, pooled.numpy(), True, "test")))
    finally:
        dist.destroy_process_group()


def test_two_rank_reduce_pools_the_lanes_of_both_ranks():
    import socket

    import torch.multiprocessing as mp
    from handmvnet_amd.sequence_eval import finish_sequence, pool_sums
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (pooled, numbers)) for r, pooled, numbers in (q.get(timeout=120) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (s0, u0), (s1, u1) = _rank_state(0), _rank_state(1)
    both = np.concatenate([s0, s1])
    want = np.concatenate([both[:, 1:11].sum(0), [u0 + u1]])
    assert u0 == 0 and u1 == 2
    for r, s in ((0, s0), (1, s1)):
        pooled, numbers = got[r]
        counts = [0, 1, 4, 5, 6, 7, 8, 9, 10]                                 # pooled[k] is sums[k + 1]; [10] the unlabelled lane-steps
        assert pooled[counts].tolist() == want[counts].tolist()
        assert pooled[[2, 3]].tolist() == pytest.approx(want[[2, 3]].tolist(), rel=REL)
        assert numbers["test_mka"] == pytest.approx(1000 * both[:, 3].sum() / both[:, 2].sum(), rel=REL)
        assert numbers["test_mka_gt"] is None                                 # rank 1 had an unlabelled step: both ranks agree
        assert numbers["test_mka_per_sequence"] == (1000 * s[:, 3] / s[:, 2]).tolist()      # local to the rank
        slots = both[:, 5:8].sum()
        assert [numbers["window_moved"], numbers["window_absent"], numbers["window_kept"]] == (both[:, 5:8].sum(0) / slots).tolist()
        assert numbers["empty_windows"] == int(both[:, 8].sum()) and numbers["labels_outside_window"] == both[:, 10].sum() / both[:, 9].sum()
    # one rank alone, every step labelled: the labels' jitter is reported; without any labelled step it and the outside fraction are None
    alone = finish_sequence(s0, pool_sums(torch.from_numpy(s0), 0).numpy(), True, "val")
    assert alone["val_mka_gt"] == pytest.approx(1000 * s0[:, 4].sum() / s0[:, 2].sum(), rel=REL) and set(alone) == {
        "val_mka", "val_mka_gt", "val_mka_per_sequence", "window_moved", "window_absent", "window_kept", "empty_windows", "labels_outside_window"}
    live = finish_sequence(s0, pool_sums(torch.from_numpy(s0), 14).numpy(), False, "val")
    assert live["val_mka_gt"] is None and live["labels_outside_window"] is None and live["val_mka"] == alone["val_mka"]
    with pytest.raises(ValueError, match="empty"):
        finish_sequence(np.zeros((2, 12)), np.zeros(11), False, "val")
    with pytest.raises(ValueError):
        finish_sequence(s0, np.zeros(10), True, "val")


# ---------------------------------------------------------------- the C ABI, host side only
def test_new_symbols_are_declared_and_exported():
    from handmvnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    declared = set(re.findall(r"\b(hmv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/handmv.h"
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), f"{sym} is not exported / bound"
    import handmvnet_amd
    for name in ("SequenceEvaluator", "labels_to_windows"):
        assert callable(getattr(handmvnet_amd, name))
    from handmvnet_amd.metrics import PoseMetrics
    assert callable(PoseMetrics.mka)
    assert "seq_eval.hip" in __import__("handmvnet_amd.build", fromlist=["SOURCES"]).SOURCES
    assert ctypes.sizeof(_lib.HmvSeqEvalArgs) == 88
    assert lib.hmv_seq_eval_sums_doubles(3) == 36 and lib.hmv_seq_eval_history_floats(3) == 3 * 2 * 2 * 63
    assert lib.hmv_seq_eval_sums_doubles(0) == 0 and lib.hmv_seq_eval_history_floats(-1) == 0


def test_the_small_entries_refuse_bad_arguments_before_any_hip_call():
    from handmvnet_amd import _lib
    lib = _lib.load()
    p = 4096   # never dereferenced
    for args, word in (((0, 0, p, p, None, None, 64, p, None, None, None), "n_slots"), ((0, -2, p, p, None, None, 64, p, p, p, None), "n_slots"),
                       ((0, 4, p, p, None, None, 0, p, None, None, None), "image_size"),
                       ((0, 4, None, p, None, None, 64, p, None, None, None), "joints_img"),
                       ((0, 4, p, None, None, None, 64, p, None, None, None), "crop_boxes"),
                       ((0, 4, p, p, None, None, 64, None, p, p, None), "joints_crop")):
        assert lib.hmv_op_labels_to_windows(*args) == 1               # the header's argument-error code
        msg = lib.hmv_last_error(None).decode()
        assert msg.startswith("hmv_op_labels_to_windows: ") and word in msg, msg
    for args, word in (((0, p, 0, 5, 21, 3, p, None), "B must"), ((0, p, 2, -1, 21, 3, p, None), "T must"), ((0, p, 2, 5, 0, 3, p, None), "n_pts"),
                       ((0, p, 2, 5, 21, 0, p, None), "dim"), ((0, p, 2, 5, 21, 5, p, None), "dim"), ((0, None, 2, 5, 21, 3, p, None), "preds"),
                       ((0, p, 2, 5, 21, 3, None, None), "out")):
        assert lib.hmv_op_mka(*args) == 1
        msg = lib.hmv_last_error(None).decode()
        assert msg.startswith("hmv_op_mka: ") and word in msg, msg


def _seq_args(B=2, V=3):
    """An argument block that passes every check up to the device selection: the pointers are never dereferenced on the host."""
    from handmvnet_amd import _lib
    a = _lib.HmvSeqEvalArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvSeqEvalArgs)
    a.B, a.V = B, V
    a.pred_joints_cam, a.sums, a.history = 4096, 4096, 4096
    a.sums_doubles, a.history_floats = 12 * B, 252 * B
    return a


@pytest.mark.parametrize("damage, word", [
    (lambda a: setattr(a, "struct_size", 80), "struct_size"), (lambda a: setattr(a, "B", 0), "B must"),
    (lambda a: setattr(a, "V", 0), "V must"), (lambda a: (setattr(a, "B", 1 << 13), setattr(a, "V", 1 << 12)), "B * V"),
    (lambda a: setattr(a, "pred_joints_cam", None), "pred_joints_cam"), (lambda a: setattr(a, "sums", None), "sums"),
    (lambda a: setattr(a, "sums", 4100), "sums"), (lambda a: setattr(a, "history", None), "history"),
    (lambda a: setattr(a, "sums_doubles", 23), "sums_doubles"), (lambda a: setattr(a, "history_floats", 503), "history_floats"),
])
def test_seq_eval_add_rejects_bad_arguments_before_touching_the_device(damage, word):
    from handmvnet_amd import _lib
    lib = _lib.load()
    a = _seq_args()
    damage(a)
    assert lib.hmv_seq_eval_add(0, ctypes.byref(a), None) == 1
    msg = lib.hmv_last_error(None).decode()
    assert msg.startswith("hmv_seq_eval_add: ") and word in msg, msg
    assert lib.hmv_seq_eval_add(0, None, None) == 1 and "args" in lib.hmv_last_error(None).decode()


# ---------------------------------------------------------------- Python refusals that need no device
def test_labels_to_windows_refusals_without_a_device():
    from handmvnet_amd import _lib
    from handmvnet_amd.sequence_eval import labels_to_windows
    j, b = torch.zeros(2, 3, 21, 2), torch.zeros(2, 3, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        labels_to_windows(torch.zeros(2, 3, 20, 2), b, 64)               # not 21 joints
    with pytest.raises(ValueError):
        labels_to_windows(j.long(), b, 64)                               # labels are floating point
    with pytest.raises(ValueError):
        labels_to_windows(j, b[:, :2], 64)                               # one window per row of joints
    with pytest.raises(ValueError):
        labels_to_windows(j, b.float(), 64)                              # windows are integers
    with pytest.raises(ValueError):
        labels_to_windows(j, b, 64, joints_img_mask=torch.zeros(2, 3, 20))
    with pytest.raises(ValueError):
        labels_to_windows(j, b, 64, present=torch.ones(2, 2))
    with pytest.raises(ValueError):
        labels_to_windows(j, b, 0)
    with pytest.raises(_lib.HandMvError, match="MI355X only"):
        labels_to_windows(j, b, 64)                                      # CPU tensors: no fallback


def test_mka_refusals_without_a_device():
    from handmvnet_amd import _lib
    from handmvnet_amd.metrics import PoseMetrics
    with pytest.raises(ValueError):
        PoseMetrics.mka(torch.zeros(7, 21, 3))                           # no batch axis
    with pytest.raises(ValueError):
        PoseMetrics.mka(torch.zeros(2, 7, 21, 5))                        # dim outside 1 .. 4
    with pytest.raises(ValueError):
        PoseMetrics.mka(torch.zeros(0, 7, 21, 3))
    with pytest.raises(_lib.HandMvError, match="MI355X only"):
        PoseMetrics.mka(torch.zeros(2, 7, 21, 3))
    with pytest.raises(NotImplementedError):
        PoseMetrics.pck(torch.zeros(1, 21, 3), torch.zeros(1, 21, 3), 0.01, reference_len=1.0)      # the refusals stay
