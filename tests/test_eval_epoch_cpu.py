"""The evaluation epoch without a GPU: the host-side finishing of a state vector against the reference's formulas, the argument
checks hmv_eval_add makes before any HIP call, the one all-reduce that combines ranks (two gloo processes), an empty epoch."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import epoch_oracle as eo
from cases import CASES, case_params
from handmvnet_amd import _lib
from handmvnet_amd.evaluation import EpochEvaluator, finish_state, reduce_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle import metrics_oracle as mo  # noqa: E402

FIX = np.load(os.path.join(ROOT, "tests", "golden", "metrics_cases.npz"))


def test_finish_state_matches_the_reference_formulas_on_the_pooled_split():
    """Three steps of 16, 8 and 8 poses accumulated by the oracle; finished by the product code; compared with the reference's
    formulas on the 32 concatenated poses.  Means are fp64 on both sides (1e-12), the curve is integer counts (equal)."""
    names = ("noise_5mm", "similarity", "mirrored")
    rng = np.random.default_rng(11)
    state = eo.new_state(20)
    for n in names:
        p, g = FIX[f"{n}.pred"], FIX[f"{n}.gt"]
        g2 = (rng.random((p.shape[0], 2, 21, 2)) * 128).astype(np.float32)
        eo.accumulate(state, p, g, g2 + rng.standard_normal(g2.shape).astype(np.float32), g2)
    pred, gt = np.concatenate([FIX[f"{n}.pred"] for n in names]), np.concatenate([FIX[f"{n}.gt"] for n in names])
    assert pred.shape == (32, 21, 3)
    got = finish_state(state, 0.0, 0.02, 20, "test")
    assert got["test_mpjpe"] == pytest.approx(mo.mpjpe(pred, gt) * 1000, rel=1e-12)
    assert got["test_pa_mpjpe"] == pytest.approx(mo.pa_mpjpe(pred, gt) * 1000, rel=1e-12)
    auc, norm_auc, vals, thr = mo.pck_auc(pred, gt, 0.0, 0.02, 20)
    assert got["test_pck_j"] == vals and got["thresholds"] == thr
    assert got["test_auc_j"] == pytest.approx(auc, rel=1e-6) and got["test_norm_auc_j"] == pytest.approx(norm_auc, rel=1e-6)
    assert got["samples"] == 32 and got["steps"] == 3
    assert got["test/loss"] is None and got["test/heatmap_loss"] is None and got["test/root_3d_loss"] is None
    # loss slots: sum(B * term) / sum(B) over the steps that carried one
    state[7] = 3.0
    state[8:14] = 3.0 * np.arange(1, 7)
    got = finish_state(state, 0.0, 0.02, 20, "val")
    assert [got[f"val/{t}"] for t in ("heatmap_loss", "joints_2d_loss", "joints_3d_loss", "g2d_loss", "p2d_loss", "loss")] == \
        [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert got["val/root_3d_loss"] == 0.0 and "val_mpjpe" in got


def test_weighted_mean_over_uneven_batches_is_the_pooled_value():
    """1100 poses in batches of 1, 2, 5 and 1092: sum(B x step value) / sum(B) is the value on the pooled split (fp64, 1e-12)."""
    pred, gt = FIX["many_poses.pred"], FIX["many_poses.gt"]
    state, at = eo.new_state(20), 0
    z2 = np.zeros((1100, 1, 21, 2), np.float32)
    for n in (1, 2, 5, 1092):
        eo.accumulate(state, pred[at:at + n], gt[at:at + n], z2[at:at + n] + 1, z2[at:at + n])
        at += n
    got = finish_state(state, 0.0, 0.02, 20, "test")
    assert got["test_mpjpe"] == pytest.approx(mo.mpjpe(pred, gt) * 1000, rel=1e-12)
    assert got["test_pa_mpjpe"] == pytest.approx(mo.pa_mpjpe(pred, gt) * 1000, rel=1e-12)
    assert got["test_mpjpe2d"] == pytest.approx(np.sqrt(2.0), rel=1e-12)
    assert got["test_pck_j"] == mo.pck_auc(pred, gt, 0.0, 0.02, 20)[2] and got["samples"] == 1100 and got["steps"] == 4


def test_state_size_entry():
    lib = _lib.load()
    assert lib.hmv_eval_state_doubles(20) == 35
    assert lib.hmv_eval_state_doubles(0) == 0
    assert lib.hmv_eval_state_doubles(257) == 0
    assert lib.hmv_eval_state_doubles(256) == 15 + 256 and lib.hmv_eval_state_doubles(1) == 16


def _args(**over):
    """A hmv_eval_args that passes every check (the pointers are never dereferenced on the host), with `over` applied."""
    a = _lib.HmvEvalArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvEvalArgs)
    a.B, a.V, a.steps, a.thr_min, a.thr_max = 2, 4, 20, 0.0, 0.02
    a.pred_joints_cam = a.gt_joints_cam = a.pred_joints_2d = a.gt_joints_2d = a.state = 4096
    a.state_doubles = 35
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("field, value, word", [
    ("struct_size", ctypes.sizeof(_lib.HmvEvalArgs) - 8, "struct_size"), ("pred_joints_cam", None, "pred_joints_cam is NULL"),
    ("gt_joints_cam", None, "gt_joints_cam is NULL"), ("pred_joints_2d", None, "pred_joints_2d is NULL"),
    ("gt_joints_2d", None, "gt_joints_2d is NULL"), ("state", None, "state is NULL"), ("state", 4100, "8-byte aligned"),
    ("B", 0, "B must"), ("B", -3, "B must"), ("V", 0, "V must"), ("steps", 0, "steps must"), ("steps", 257, "steps must"),
    ("state_doubles", 34, "state_doubles"), ("thr_max", -0.01, "thr_max"), ("thr_max", float("nan"), "thr_max")])
def test_argument_checks_come_before_any_hip_call(field, value, word):
    """No GPU here: reaching hipSetDevice would give the HIP error code, not the argument one."""
    lib = _lib.load()
    assert lib.hmv_eval_add(0, ctypes.byref(_args(**{field: value})), None) == 1          # HMV_ERR_ARG
    msg = lib.hmv_last_error(None).decode()
    assert msg.startswith("hmv_eval_add: ") and word in msg, msg


def test_null_args_struct():
    lib = _lib.load()
    assert lib.hmv_eval_add(0, None, None) == 1
    assert b"args is NULL" in lib.hmv_last_error(None)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reduce_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        calls = {"n": 0}
        real = dist.all_reduce

        def counted(*a, **k):
            calls["n"] += 1
            return real(*a, **k)
        dist.all_reduce = counted
        for forbidden in ("all_gather", "all_gather_into_tensor", "broadcast", "all_to_all", "reduce"):
            setattr(dist, forbidden, lambda *a, _n=forbidden, **k: (_ for _ in ()).throw(AssertionError(f"unexpected collective {_n}")))
        state = torch.arange(35, dtype=torch.float64) * (rank + 1) + 0.25 * rank
        out = reduce_state(state, None)
        assert out is state and calls["n"] == 1, calls
        q.put((rank, state.numpy().copy()))
    finally:
        dist.destroy_process_group()


def test_reduce_state_is_one_all_reduce_under_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    want = np.arange(35, dtype=np.float64) * 3 + 0.25
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)


def test_an_empty_epoch_raises():
    from handmvnet_amd import HandMvNet
    ev = EpochEvaluator(HandMvNet(*case_params(CASES["tiny_r50"])), "test")
    assert ev.state_doubles == 35 and (ev.thr_min, ev.thr_max) == (0.0, 0.05)      # ho3d: 0 .. 50 mm
    with pytest.raises(ValueError, match="empty epoch"):
        ev.compute()
    with pytest.raises(ValueError, match="empty epoch"):
        finish_state(np.zeros(35), 0.0, 0.02, 20, "test")
    with pytest.raises(ValueError, match="35 elements"):
        finish_state(np.zeros(34), 0.0, 0.02, 20, "test")
