"""Evaluating a followed sequence on the device (include/handmv.h "sequence evaluation"; csrc/seq_eval.hip;
handmvnet_amd/sequence_eval.py):
  (1) hmv_op_labels_to_windows against the fixture of the real reference function, bit for bit, with the optional arguments present
      and absent, the status paths against the oracle, the raw entry's refusals;
  (2) PoseMetrics.mka against the float64 fixture;   (3) hmv_seq_eval_add streamed against the oracle;
  (4) SequenceEvaluator == the loop a caller writes today (tracker.step -> host -> tests/seq_eval_oracle.py -> upload ->
      EpochEvaluator.add), uniform and ragged;   (5) the same from replayed hipGraphs;   (6) the tracker is untouched by an evaluator.

Tolerances, none from what the kernels return: the mapping, masks, counts and every state of (4)-(6) are compared with == (the same
fp32 operations, the same kernels on the same bits).  MKA and the float sums of (3): 1e-12 relative, the project's figure for fp64
sums of the same terms in another order (tests/test_gpu_eval_epoch.py); hmv_op_mka's fp32 output adds one rounding, 2^-24 = 6e-8."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import loss_oracle as lo
import seq_eval_oracle as so
from helpers import load_case
from handmvnet_amd.synth import synth_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "seq_eval_cases.npz"))
MAP_NAMES = sorted({k.split(".")[0] for k in FIX.files if k.startswith("map_")})
ROWS_PER_WORKGROUP = 4
DEV = "cuda:0"
REL = 1e-12
F32 = 6e-8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_map(n, joints, boxes, present, hidden, size, crop, mask, info):
    from handmvnet_amd import _lib
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    return _lib.load().hmv_op_labels_to_windows(0, n, p(joints), p(boxes), p(present), p(hidden), size, p(crop), p(mask), p(info), _stream())


# ---------------------------------------------------------------- 1. the mapping
@pytest.mark.parametrize("name", MAP_NAMES)
def test_mapping_matches_reference_fixture(name):
    from handmvnet_amd.sequence_eval import labels_to_windows
    size, total = int(FIX[f"{name}.size"]), FIX[f"{name}.boxes"].shape[0]
    for n in sorted({1, 3, ROWS_PER_WORKGROUP + 1, total}):
        if n > total:
            continue
        j, b, m = _dev(FIX[f"{name}.joints"][:n]), _dev(FIX[f"{name}.boxes"][:n]), _dev(FIX[f"{name}.mask"][:n])
        crop, mask, info = labels_to_windows(j, b, size, m)
        assert crop.dtype == torch.float32 and mask.dtype == torch.uint8 and info.dtype == torch.int32
        assert (bits(crop) == bits(FIX[f"{name}.out"][:n])).all(), (name, n)
        assert (mask.cpu().numpy() == (FIX[f"{name}.mask"][:n] != 0)).all()
        got = info.cpu().numpy()
        assert (got[:, 0] == 0).all() and (got[:, 1] == FIX[f"{name}.outside"][:n]).all() and (got[:, 2] == FIX[f"{name}.visible"][:n]).all()
        # `present` given (every slot present, as a bool tensor) and the mask as bool: the same call
        again = labels_to_windows(j, b.long(), size, m.bool(), torch.ones(n, dtype=torch.bool, device=DEV))
        assert all(torch.equal(x, y) for x, y in zip(again, (crop, mask, info)))
        # no joint mask: every joint of a mapped slot is visible
        crop2, mask2, info2 = labels_to_windows(j, b, size)
        assert (bits(crop2) == bits(crop)).all() and not mask2.any() and (info2[:, 2] == 21).all()
        # every optional argument NULL through the raw entry
        out = torch.full((n, 21, 2), 7.5, device=DEV)
        assert _raw_map(n, j, b, None, None, size, out, None, None) == 0
        assert (bits(out) == bits(crop)).all()


def test_mapping_leading_shapes():
    from handmvnet_amd.sequence_eval import labels_to_windows
    name = "map_random_320"
    j, b = _dev(FIX[f"{name}.joints"][:6].reshape(2, 3, 21, 2)), _dev(FIX[f"{name}.boxes"][:6].reshape(2, 3, 4))
    crop, mask, info = labels_to_windows(j, b, 320, _dev(FIX[f"{name}.mask"][:6].reshape(2, 3, 21)))
    assert tuple(crop.shape) == (2, 3, 21, 2) and tuple(mask.shape) == (2, 3, 21) and tuple(info.shape) == (2, 3, 3)
    assert (bits(crop).reshape(6, 21, 2) == bits(FIX[f"{name}.out"][:6])).all()


def test_mapping_status_paths():
    from handmvnet_amd.sequence_eval import labels_to_windows
    name = "map_random_256"
    j, b, m = FIX[f"{name}.joints"][:11].copy(), FIX[f"{name}.boxes"][:11].copy(), FIX[f"{name}.mask"][:11].copy()
    b[1] = [50, 60, 50, 90]                                 # zero width
    b[4] = [80, 70, 60, 50]                                 # negative extents, across a workgroup boundary
    b[9] = [7, 9, 30, 9]                                    # zero height
    j[6, 2, 0], m[6, 2] = np.nan, 0                         # a non-finite visible label: outside
    j[7, 5, 1], m[7, 5] = np.inf, 1                         # a non-finite masked one: not counted
    present = np.ones(11, np.uint8)
    present[[0, 4, 5, 10]] = 0                              # scattered, at both ends; slot 4 is absent AND empty: absent wins
    crop, mask, info = labels_to_windows(_dev(j), _dev(b), 256, _dev(m), _dev(present))
    want = so.labels_to_windows(j, b, 256, m, present)
    assert info.cpu().numpy()[:, 0].tolist() == [1, 2, 0, 0, 1, 1, 0, 0, 0, 2, 1] == want[2][:, 0].tolist()
    got, nan = crop.cpu().numpy(), np.isnan(want[0])
    assert nan.sum() == 1 and (np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want[0].view(np.uint32)[~nan]).all()
    assert (mask.cpu().numpy() == want[1]).all() and (info.cpu().numpy() == want[2]).all()
    for n in (0, 1, 4, 5, 9, 10):
        assert not crop[n].any() and mask[n].all() and info[n, 1:].tolist() == [0, 0]
    for n in (2, 3, 8):                                     # the neighbours are unaffected
        assert (bits(crop[n]) == bits(FIX[f"{name}.out"][n])).all()
    assert torch.isnan(crop[6, 2, 0]) and int(info[6, 1]) >= 1


def test_mapping_refusals_leave_outputs_alone():
    from handmvnet_amd import _lib
    name = "map_edges_64"
    j, b = _dev(FIX[f"{name}.joints"]), _dev(FIX[f"{name}.boxes"])
    canary = [torch.full((21, 2), 7.5, device=DEV), torch.full((21,), 0x5A, dtype=torch.uint8, device=DEV),
              torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)]
    keep = [c.clone() for c in canary]
    for args, word in (((0, j, b, None, None, 64) + tuple(canary), b"n_slots"), ((-3, j, b, None, None, 64) + tuple(canary), b"n_slots"),
                       ((1, j, b, None, None, 0) + tuple(canary), b"image_size"), ((1, None, b, None, None, 64) + tuple(canary), b"joints_img"),
                       ((1, j, None, None, None, 64) + tuple(canary), b"crop_boxes"),
                       ((1, j, b, None, None, 64, None) + tuple(canary[1:]), b"joints_crop")):
        assert _raw_map(*args) == 1                         # the header's argument-error code
        assert word in _lib.load().hmv_last_error(None)
    torch.cuda.synchronize()
    for c, k in zip(canary, keep):
        assert torch.equal(c, k)


# ---------------------------------------------------------------- 2. MKA
def test_mka_matches_reference_float64():
    from handmvnet_amd.metrics import PoseMetrics
    for name in ("mka_3x7", "mka_2x3"):
        preds, want = _dev(FIX[f"{name}.preds"]), FIX[f"{name}.ref64"]
        got = PoseMetrics.mka(preds)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_cuda
        err = np.abs(got.cpu().numpy().astype(np.float64) - want) / np.abs(want)
        print(f"{name}: dev {got.cpu().numpy()!r} reference float64 {want!r} rel {err.max():.3e}")
        assert err.max() <= REL + F32
        assert torch.equal(PoseMetrics.mka(preds), got)     # two calls, the same bits
    short = PoseMetrics.mka(_dev(FIX["mka_1x2.preds"]))
    assert tuple(short.shape) == (1,) and torch.isnan(short).all() and np.isnan(FIX["mka_1x2.ref64"]).all()
    # more rows than the workgroup has threads, other point counts and dims: against the oracle
    rng = np.random.default_rng(3)
    for shape in ((2, 20, 21, 3), (3, 9, 5, 2), (1, 300, 1, 1), (2, 4, 7, 4)):
        p = np.cumsum(rng.standard_normal(shape) * 2e-3, axis=1).astype(np.float32)
        want = so.mka(p)
        got = PoseMetrics.mka(_dev(p)).cpu().numpy().astype(np.float64)
        assert (np.abs(got - want) <= (REL + F32) * np.abs(want)).all(), shape
    # a non-contiguous view of another dtype goes through the same entry
    p = _dev(FIX["mka_3x7.preds"])
    assert torch.equal(PoseMetrics.mka(p.double().transpose(0, 1).contiguous().transpose(0, 1)), PoseMetrics.mka(p))


# ---------------------------------------------------------------- 3. the streamed accumulation
def _raw_add(B, V, pred, gt, status, info, restart, sums, history):
    from handmvnet_amd import _lib
    a = _lib.HmvSeqEvalArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvSeqEvalArgs)
    a.B, a.V = B, V
    for k, t in (("pred_joints_cam", pred), ("gt_joints_cam", gt), ("track_status", status), ("slot_info", info), ("restart", restart),
                 ("sums", sums), ("history", history)):
        setattr(a, k, None if t is None else t.data_ptr())
    a.sums_doubles, a.history_floats = sums.numel(), history.numel()
    return _lib.load().hmv_seq_eval_add(0, ctypes.byref(a), _stream())


def _check_sums(got, want):
    got = np.asarray(got, np.float64).reshape(want.shape)
    counts = [0, 1, 2, 5, 6, 7, 8, 9, 10, 11]
    assert (got[:, counts] == want[:, counts]).all(), (got[:, counts], want[:, counts])
    for k in (3, 4):
        assert (np.abs(got[:, k] - want[:, k]) <= REL * np.abs(want[:, k])).all(), (k, got[:, k], want[:, k])


def test_streamed_accumulation_matches_the_oracle():
    T, B, V = 7, 2, 3
    all_preds = FIX["mka_3x7.preds"]
    preds, labels = all_preds[:2], all_preds[[2, 0]]
    rng = np.random.default_rng(4)
    status = rng.integers(0, 3, (T, B, V)).astype(np.int32)
    info = np.stack([rng.integers(0, 3, (T, B, V)), rng.integers(0, 5, (T, B, V)), rng.integers(5, 22, (T, B, V))], -1).astype(np.int32)
    restart = np.array([0, 1], np.uint8)

    def run(lanes, with_gt=True):
        n = len(lanes)
        sums, hist = torch.zeros(12 * n, device=DEV, dtype=torch.float64), torch.zeros(252 * n, device=DEV)
        for t in range(T):
            rc = _raw_add(n, V, _dev(preds[lanes, t]), _dev(labels[lanes, t]) if with_gt else None, _dev(status[t][lanes]),
                          _dev(info[t][lanes]), _dev(restart[lanes]) if t == 3 else None, sums, hist)
            assert rc == 0
        return sums.cpu().numpy().reshape(n, 12), hist.cpu().numpy().reshape(n, 2, 2, 63)

    got, ghist = run([0, 1])
    want, whist = so.empty_state(B)
    for t in range(T):
        so.accumulate(want, whist, preds[:, t], labels[:, t], status[t], info[t], restart if t == 3 else None)
    print("sums dev", got.tolist(), "oracle", want.tolist())
    _check_sums(got, want)
    assert got[:, 0].tolist() == [7, 4] and got[:, 2].tolist() == [5 * 21, 3 * 21]
    assert (ghist.view(np.uint32) == whist.view(np.uint32)).all()
    # the jitter of the uninterrupted lane is hmv_op_mka's number
    assert abs(got[0, 3] / got[0, 2] - so.mka(preds)[0]) <= REL * so.mka(preds)[0]
    # lane 0 of the two-lane run has the bits of a one-lane run
    one, ohist = run([0])
    assert one.tobytes() == got[:1].tobytes() and ohist.tobytes() == ghist[:1].tobytes()
    # without labels [4] and the label history stay zero, the rest is the same
    nogt, nhist = run([0, 1], with_gt=False)
    assert not nogt[:, 4].any() and not nhist[:, 1].any()
    assert np.delete(nogt, 4, axis=1).tobytes() == np.delete(got, 4, axis=1).tobytes() and nhist[:, 0].tobytes() == ghist[:, 0].tobytes()
    # status and slot info are optional as well
    sums, hist = torch.zeros(24, device=DEV, dtype=torch.float64), torch.zeros(504, device=DEV)
    assert _raw_add(2, V, _dev(preds[:, 0]), None, None, None, None, sums, hist) == 0
    assert sums.cpu().numpy().reshape(2, 12).tolist() == [[1, 1] + [0] * 10] * 2


# ---------------------------------------------------------------- 4 - 6. sequences
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}
ROOT_IDX = 1


def _new_model():
    from handmvnet_amd import HandMvNet
    cfg, (tp, mp, dp), sd, _, _ = load_case("tiny_r18")
    m = HandMvNet(dict(tp, loss_weights=WEIGHTS, mask_invisible_joints=True), mp, dp)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    m.heatmap_targets = "joints"
    return m, cfg


_model = functools.lru_cache(maxsize=None)(_new_model)      # shared by the tests that leave its settings alone


FH, FW = 96, 128


def _sequence(cfg, B, T, seed):
    """Seeded smooth frames [T, B, V, 96, 128, 3], first windows [B, V, 4] and intrinsics [B, V, 4] (the recipe of tests/test_gpu_track.py)."""
    rng = np.random.default_rng(seed)
    V = cfg.num_views
    yy, xx = np.mgrid[0:FH, 0:FW].astype(np.float32)
    frames = np.empty((T, B, V, FH, FW, 3), np.uint8)
    for t in range(T):
        for b in range(B):
            for v in range(V):
                ph = rng.uniform(0, 6.28, 3)
                img = np.stack([127 + 80 * np.sin(xx / (9 + 2 * c) + ph[c] + 0.3 * t) * np.cos(yy / (7 + c) + 0.2 * t) for c in range(3)], -1)
                frames[t, b, v] = np.clip(img + rng.standard_normal(img.shape) * 6, 0, 255).astype(np.uint8)
    x1, y1 = rng.integers(5, 50, (B, V)), rng.integers(2, 25, (B, V))
    side = rng.integers(48, 72, (B, V))
    boxes0 = np.stack([x1, y1, x1 + side, y1 + side], -1).astype(np.int32)
    return frames, boxes0, synth_inputs(cfg, B, 12, cfg.image_size)[2]


@functools.lru_cache(maxsize=None)
def _labelled_sequence(B, T, seed):
    """Frames, first windows and intrinsics of tests/test_gpu_track.py plus seeded labels: frame-space joints around the first
    windows (some leave the windows as they move), camera-space joints that drift in millimetres, a joint mask, a rig."""
    _, cfg = _model()
    frames, boxes0, intr = _sequence(cfg, B, T, seed=seed)
    V = cfg.num_views
    rng = np.random.default_rng(seed + 100)
    f = rng.uniform(-0.1, 1.1, (T, B, V, 21, 2))
    side = (boxes0[..., 2:] - boxes0[..., :2])[None, :, :, None, :]
    joints_img = (boxes0[None, :, :, None, :2] + f * side + np.arange(T)[:, None, None, None, None] * 1.5).astype(np.float32)
    cam_mm = (rng.standard_normal((1, B, 21, 3)) * 40 + np.cumsum(rng.standard_normal((T, B, 21, 3)) * 2, axis=0)).astype(np.float32)
    rig = lo.loss_case("vii_many")
    labels = dict(joints_img=joints_img, cam_mm=cam_mm, jmask=rng.random((T, B, V, 21)) < 0.2,
                  root_mm=(rig["root_joint"][:B] * 1000).astype(np.float32), extr=np.ascontiguousarray(rig["extr"][:B, :V]))
    return frames, boxes0, intr, labels


def _cam(intr, labels):
    return {"intrinsic": _dev(intr), "extrinsic": _dev(labels["extr"])}


def _labels_at(labels, t):
    return {"joints_img": _dev(labels["joints_img"][t]), "joints_cam": _dev(labels["cam_mm"][t]), "root_joint": _dev(labels["root_mm"]),
            "root_idx": torch.tensor([ROOT_IDX]), "joints_img_mask": _dev(labels["jmask"][t])}


def _host_loop(m, cfg, frames, boxes0, intr, labels, mask=None):
    """What a caller writes today from the public pieces: tracker.step, the windows to the host, the labels mapped in numpy, upload,
    EpochEvaluator.add.  The sequence sums come from the oracle."""
    from handmvnet_amd import SequenceTracker
    from handmvnet_amd.evaluation import EpochEvaluator
    cam = _cam(intr, labels)
    tr = SequenceTracker(m, torch.from_numpy(boxes0), cam, margin=4)
    ev = EpochEvaluator(m, "test")
    B, V = boxes0.shape[:2]
    present = None if mask is None else np.asarray(mask, np.uint8).reshape(-1)
    sums, hist = so.empty_state(B)
    for t, f in enumerate(frames):
        out = tr.step(_dev(f), view_mask=mask)
        used = out["crop_boxes_used"].cpu().numpy()
        crop, hidden, info = so.labels_to_windows(labels["joints_img"][t].reshape(-1, 21, 2), used.reshape(-1, 4), cfg.image_size,
                                                  labels["jmask"][t].reshape(-1, 21), present)
        gt_m = _dev(labels["cam_mm"][t]) / 1000
        inputs = {"joints_crop_img": _dev(crop.reshape(B, V, 21, 2)), "joints_cam": gt_m, "root_joint": _dev(labels["root_mm"]) / 1000,
                  "root_idx": torch.tensor([ROOT_IDX]), "joints_img_mask": _dev(hidden.reshape(B, V, 21)), "bboxes": _dev(used.astype(np.float32))}
        if mask is None:
            ev.add(out, inputs, cam)
        else:
            ev.add(out, inputs, cam, view_mask=mask)
        so.accumulate(sums, hist, out["joints_cam"].cpu().numpy(), gt_m.cpu().numpy(), out["status"].cpu().numpy(), info.reshape(B, V, 3))
    return ev, sums


def _evaluator_loop(m, frames, boxes0, intr, labels, mask=None, labelled=True):
    from handmvnet_amd import SequenceEvaluator, SequenceTracker
    cam = _cam(intr, labels)
    tr = SequenceTracker(m, torch.from_numpy(boxes0), cam, margin=4)
    ev = SequenceEvaluator(tr, cam)
    steps = []
    for t, f in enumerate(frames):
        out = ev.step(_dev(f), _labels_at(labels, t) if labelled else None, view_mask=mask)
        steps.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    return ev, steps


def _check_numbers(numbers, epoch_numbers, sums):
    p = sums.sum(0)
    for k, v in epoch_numbers.items():
        assert numbers[k] == v, k
    assert numbers["test_mka"] == pytest.approx(1000 * p[3] / p[2], rel=REL)
    assert numbers["test_mka_gt"] == pytest.approx(1000 * p[4] / p[2], rel=REL)
    assert numbers["test_mka_per_sequence"] == pytest.approx((1000 * sums[:, 3] / sums[:, 2]).tolist(), rel=REL)
    slots = p[5] + p[6] + p[7]
    assert [numbers["window_moved"], numbers["window_absent"], numbers["window_kept"]] == [p[5] / slots, p[6] / slots, p[7] / slots]
    assert numbers["empty_windows"] == int(p[8]) and numbers["labels_outside_window"] == p[10] / p[9]
    assert "sequence_steps" not in numbers


@pytest.mark.parametrize("B,T,mask", [(2, 5, None), (2, 3, [[1, 1], [1, 0]])])
def test_closed_loop_equals_host_loop(B, T, mask):
    m, cfg = _model()
    frames, boxes0, intr, labels = _labelled_sequence(B, T, 5 if mask is None else 7)
    host, want = _host_loop(m, cfg, frames, boxes0, intr, labels, mask)
    ev, _ = _evaluator_loop(m, frames, boxes0, intr, labels, mask)
    assert ev.state.cpu().numpy().tobytes() == host.state.cpu().numpy().tobytes()          # same label bits, same kernels
    got = ev.sums.cpu().numpy().reshape(B, 12)
    print("sums dev", got.tolist(), "oracle", want.tolist())
    _check_sums(got, want)
    assert want[:, 1].tolist() == [T] * B and want[:, 2].tolist() == [(T - 2) * 21] * B
    assert 0 < want[:, 10].sum() < want[:, 9].sum()                                         # some labels are outside, most are not
    numbers = ev.compute()
    _check_numbers(numbers, host.compute(), got)
    assert numbers["test/heatmap_loss"] > 0 and numbers["test/g2d_loss"] > 0 and numbers["samples"] == B * T
    if mask is not None:
        assert numbers["window_absent"] == 0.25 and got[1, 9] < got[0, 9]                   # the absent view has no visible labels
    # the labels were not modified
    assert np.array_equal(_labels_at(labels, 0)["joints_cam"].cpu().numpy(), labels["cam_mm"][0])


def test_steps_without_labels_and_a_restart():
    from handmvnet_amd import SequenceEvaluator, SequenceTracker
    m, cfg = _model()
    frames, boxes0, intr, labels = _labelled_sequence(2, 5, 5)
    ev, steps = _evaluator_loop(m, frames, boxes0, intr, labels, labelled=False)
    assert ev.state is None
    numbers = ev.compute()                                                                  # does not raise
    assert "test_mpjpe" not in numbers and numbers["test_mka_gt"] is None and numbers["labels_outside_window"] is None
    pred = np.stack([s["joints_cam"] for s in steps], axis=1)                               # [B, T, 21, 3]
    want = so.mka(pred) * 1000
    assert numbers["test_mka_per_sequence"] == pytest.approx(want.tolist(), rel=REL) and numbers["test_mka"] == pytest.approx(want.mean(), rel=REL)
    assert numbers["window_moved"] + numbers["window_kept"] == 1.0 and numbers["window_absent"] == 0.0
    # lane 1 starts anew after three steps: two segments pooled there, lane 0 does not notice
    cam = _cam(intr, labels)
    ev2 = SequenceEvaluator(SequenceTracker(m, torch.from_numpy(boxes0), cam, margin=4), cam)
    with pytest.raises(ValueError):
        ev2.restart(torch.from_numpy(boxes0), lanes=[2])
    with pytest.raises(ValueError):
        ev2.compute()                                                                       # empty
    for t, f in enumerate(frames):
        if t == 3:
            ev2.restart(ev2.tracker.crop_boxes.clone(), lanes=[1])                          # the windows stay where they are
        ev2.step(_dev(f))
    s2 = ev2.sums.cpu().numpy().reshape(2, 12)
    assert s2[:, 0].tolist() == [5, 2] and s2[:, 2].tolist() == [63, 21] and s2[0].tobytes() == ev.sums.cpu().numpy().reshape(2, 12)[0].tobytes()
    assert s2[1, 3] == pytest.approx(so.mka(pred[1:2, :3])[0] * 21, rel=REL)
    with pytest.raises(ValueError):
        ev2.step(_dev(frames[0]), {"joints_img": torch.zeros(2, 2, 21, 2)})                 # labels without joints_cam
    with pytest.raises(ValueError):
        ev2.step(_dev(frames[0]), {"joints_img": torch.zeros(2, 2, 20, 2), "joints_cam": torch.zeros(2, 21, 3)})
    assert ev2.sums.cpu().numpy().reshape(2, 12)[:, 1].tolist() == [5, 5]                   # refused before anything was launched


def test_reduce_over_a_one_rank_group(tmp_path):
    """reduce() through a real process group of one rank: the numbers stay what they were, and a later step drops the reduced sums."""
    import torch.distributed as dist
    m, cfg = _model()
    frames, boxes0, intr, labels = _labelled_sequence(2, 5, 5)
    ev, _ = _evaluator_loop(m, frames[:4], boxes0, intr, labels)
    before = ev.compute()
    assert before["test_mka_gt"] is not None
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        ev.reduce()
        assert ev._reduced is not None and ev.compute() == before
        ev.step(_dev(frames[4]))                                                            # without labels
        assert ev._reduced is None
        after = ev.compute()
        ev.reduce()
        assert ev.compute() == after
    finally:
        dist.destroy_process_group()
    assert after["test_mka_gt"] is None and after["samples"] == before["samples"] and after["test_mka"] != before["test_mka"]
    assert after["window_moved"] + after["window_kept"] == 1.0


def test_g2d_needs_the_extrinsics():
    from handmvnet_amd import SequenceEvaluator, SequenceTracker
    m, cfg = _model()
    _, boxes0, intr, _ = _labelled_sequence(2, 5, 5)
    tr = SequenceTracker(m, torch.from_numpy(boxes0), {"intrinsic": _dev(intr)})
    with pytest.raises(TypeError, match="extrinsic"):
        SequenceEvaluator(tr, {"intrinsic": _dev(intr)})
    with pytest.raises(TypeError, match="extrinsic"):
        SequenceEvaluator(tr)


def test_graph_replay_of_an_evaluated_sequence():
    T = 5
    m, cfg = _new_model()                                   # its own engine: the graph count below is this test's
    frames, boxes0, intr, labels = _labelled_sequence(2, T, 6)
    m.set_graphs(False)
    eager, esteps = _evaluator_loop(m, frames, boxes0, intr, labels)
    try:
        m.set_graphs(True)
        ev, steps = _evaluator_loop(m, frames, boxes0, intr, labels)
        cached, replays = m.graph_stats()
    finally:
        m.set_graphs(False)
    assert ev.state.cpu().numpy().tobytes() == eager.state.cpu().numpy().tobytes()
    assert ev.sums.cpu().numpy().tobytes() == eager.sums.cpu().numpy().tobytes()
    assert ev.history.cpu().numpy().tobytes() == eager.history.cpu().numpy().tobytes()
    for t in range(T):
        for k in esteps[t]:
            assert (esteps[t][k].view(np.uint8) == steps[t][k].view(np.uint8)).all(), (t, k)
    assert cached == 1 and replays >= T - 2
    assert ev.compute() == eager.compute()


def test_the_tracker_is_untouched_by_an_evaluator():
    from handmvnet_amd import SequenceTracker
    m, cfg = _model()
    frames, boxes0, intr, labels = _labelled_sequence(2, 5, 5)
    tr = SequenceTracker(m, torch.from_numpy(boxes0), _cam(intr, labels), margin=4)
    alone = []
    for f in frames:
        out = tr.step(_dev(f))
        alone.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    _, steps = _evaluator_loop(m, frames, boxes0, intr, labels)
    for t in range(len(frames)):
        assert set(alone[t]) == set(steps[t])
        for k in alone[t]:
            assert (alone[t][k].view(np.uint8) == steps[t][k].view(np.uint8)).all(), (t, k)
