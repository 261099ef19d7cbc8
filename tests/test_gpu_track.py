"""Window following on the device (include/handmv.h "sequences"; csrc/track.hip; handmvnet_amd/tracking.py):
  (1) hmv_op_next_crop_boxes against the fixture of the real reference functions, exactly, at slot counts that cross the kernel's
      partition (4 rows per workgroup), also with outputs aliasing inputs;   (2) the status paths;   (3) the raw entry's refusals;
  (4) SequenceTracker.step == the host loop (forward_frames -> host -> tests/track_oracle.py -> forward_frames), bit for bit;
  (5) the same sequence from replayed hipGraphs;   (6) a ragged sequence;   (7) forward_frames is untouched by a tracker.
Everything is compared with == : the windows are integers and the forward is deterministic in every arithmetic mode."""
import ctypes
import os

import numpy as np
import pytest
import torch

import track_oracle as to
from helpers import load_case
from handmvnet_amd.synth import synth_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "track_cases.npz"))
NAMES = sorted({k.split(".")[0] for k in FIX.files})
ROWS_PER_WORKGROUP = 4
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _raw(n, jc, boxes_in, present, size, margin, square, boxes_out, bbox_out, img, status):
    from handmvnet_amd import _lib
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    return _lib.load().hmv_op_next_crop_boxes(0, n, p(jc), p(boxes_in), p(present), size, margin, int(square), p(boxes_out), p(bbox_out),
                                              p(img), p(status), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name", NAMES)
def test_op_matches_reference_fixture(name):
    from handmvnet_amd.tracking import joints_to_frame, next_crop_boxes
    size, margin, square = int(FIX[f"{name}.size"]), int(FIX[f"{name}.margin"]), bool(FIX[f"{name}.square"])
    total = FIX[f"{name}.boxes"].shape[0]
    for n in sorted({1, 3, ROWS_PER_WORKGROUP + 1, 65, total}):
        if n > total:
            continue
        j, b = _dev(FIX[f"{name}.joints"][:n]), _dev(FIX[f"{name}.boxes"][:n])
        want_box, want_img = FIX[f"{name}.out"][:n], FIX[f"{name}.joints_img"][:n]
        boxes, bbox, img, status = next_crop_boxes(j, b, size, margin, square)
        assert boxes.dtype == torch.int32 and status.dtype == torch.int32
        assert (boxes.cpu().numpy() == want_box).all(), (name, n)
        assert (status.cpu().numpy() == 0).all()
        assert (bits(img) == bits(want_img)).all(), (name, n)
        assert (bits(bbox) == bits(want_box.astype(np.float32))).all()
        assert (bits(joints_to_frame(j, b, size)) == bits(want_img)).all()
        # outputs aliasing inputs: the windows in place, bbox into the fp32 copy of them
        b2, bb2, img2, st2 = b.clone(), b.float(), torch.empty_like(j), torch.full((n,), -1, dtype=torch.int32, device=DEV)
        assert _raw(n, j, b2, None, size, margin, square, b2, bb2, img2, st2) == 0
        assert torch.equal(b2, boxes) and torch.equal(bb2, bbox) and torch.equal(st2, status) and (bits(img2) == bits(img)).all()


def test_op_leading_shapes_and_optional_outputs():
    from handmvnet_amd.tracking import next_crop_boxes
    name = "random_256_m20"
    j, b = _dev(FIX[f"{name}.joints"][:6].reshape(2, 3, 21, 2)), _dev(FIX[f"{name}.boxes"][:6].reshape(2, 3, 4))
    boxes, bbox, img, status = next_crop_boxes(j, b.long(), 256, 20, True)
    assert tuple(boxes.shape) == (2, 3, 4) and tuple(img.shape) == (2, 3, 21, 2) and tuple(status.shape) == (2, 3)
    assert (boxes.cpu().numpy().reshape(6, 4) == FIX[f"{name}.out"][:6]).all()
    out = torch.zeros(6, 4, dtype=torch.int32, device=DEV)
    assert _raw(6, j, b.reshape(6, 4).contiguous(), None, 256, 20, True, out, None, None, None) == 0     # every optional output absent
    assert (out.cpu().numpy() == FIX[f"{name}.out"][:6]).all()


def test_status_paths():
    from handmvnet_amd.tracking import next_crop_boxes
    name = "random_64_m0"
    j, b = FIX[f"{name}.joints"][:11].copy(), FIX[f"{name}.boxes"][:11].copy()
    present = np.ones(11, np.uint8)
    present[[0, 4, 5, 10]] = 0                              # scattered, across a workgroup boundary and at both ends
    boxes, bbox, img, status = next_crop_boxes(_dev(j), _dev(b), 64, 0, True, present=_dev(present))
    want = to.next_crop_boxes(j, b, 64, 0, True, present)
    assert status.cpu().numpy().tolist() == [1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1]
    assert (boxes.cpu().numpy()[present == 0] == b[present == 0]).all() and (img.cpu().numpy()[present == 0] == 0).all()
    assert (bits(bbox)[present == 0] == bits(b.astype(np.float32))[present == 0]).all()
    assert (boxes.cpu().numpy() == want[0]).all() and (bits(img) == bits(want[2])).all() and (status.cpu().numpy() == want[3]).all()
    assert (boxes.cpu().numpy()[present == 1] == FIX[f"{name}.out"][:11][present == 1]).all()   # the neighbours are unaffected
    # ordinary data the reference would raise on: a NaN joint, an absurd joint, a window beyond 65536 px
    j2, b2 = FIX[f"{name}.joints"][:7].copy(), FIX[f"{name}.boxes"][:7].copy()
    j2[1, 4, 0] = np.nan
    j2[3, 7, 1] = 1e12
    j2[5, 0, 0], b2[5] = 40000.0 * 64, [0, 0, 2, 2]
    boxes, bbox, img, status = next_crop_boxes(_dev(j2), _dev(b2), 64, 0, True)
    want = to.next_crop_boxes(j2, b2, 64, 0, True)
    assert status.cpu().numpy().tolist() == [0, 2, 0, 2, 0, 2, 0] == want[3].tolist()
    assert (boxes.cpu().numpy()[[1, 3, 5]] == b2[[1, 3, 5]]).all()
    assert (boxes.cpu().numpy() == want[0]).all() and (bits(bbox) == bits(want[1])).all() and (bits(img) == bits(want[2])).all()
    assert (boxes.cpu().numpy()[[0, 2, 4, 6]] == FIX[f"{name}.out"][[0, 2, 4, 6]]).all()


def test_raw_entry_refusals_leave_outputs_alone():
    from handmvnet_amd import _lib
    j, b = _dev(FIX["h_eq_w.joints"]), _dev(FIX["h_eq_w.boxes"])
    canary = [torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV), torch.full((4,), 7.5, device=DEV),
              torch.full((21, 2), 7.5, device=DEV), torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)]
    keep = [c.clone() for c in canary]
    for args, word in (((0, j, b, None, 64, 0, True) + tuple(canary), b"n_slots"), ((-3, j, b, None, 64, 0, True) + tuple(canary), b"n_slots"),
                       ((1, j, b, None, 0, 0, True) + tuple(canary), b"image_size"), ((1, j, b, None, 64, -1, True) + tuple(canary), b"margin"),
                       ((1, None, b, None, 64, 0, True) + tuple(canary), b"required"), ((1, j, None, None, 64, 0, True) + tuple(canary), b"required"),
                       ((1, j, b, None, 64, 0, True, None) + tuple(canary[1:]), b"required")):
        assert _raw(*args) == 1                             # HMV_ERR_ARG
        assert word in _lib.load().hmv_last_error(None)
    torch.cuda.synchronize()
    for c, k in zip(canary, keep):
        assert torch.equal(c, k)


# ------------------------------------------------------------------ sequences
FH, FW = 96, 128


def _model(mode="f32"):
    from handmvnet_amd import HandMvNet
    cfg, (tp, mp, dp), sd, _, _ = load_case("tiny_r18")
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    if mode == "f16":
        m.half()
    elif mode == "f32x3":
        m.float32x3()
    return m, cfg


def _sequence(cfg, B, T, seed=5):
    """Seeded smooth frames [T, B, V, 96, 128, 3], first windows [B, V, 4] and intrinsics [B, V, 4]."""
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
    intr = synth_inputs(cfg, B, 12, cfg.image_size)[2]
    return frames, boxes0, intr


def _host_loop(m, cfg, frames, boxes0, intr, margin, square, mask=None):
    """What a caller had to do before: per step a forward, the joints to the host, the windows in numpy, upload."""
    boxes, cam, steps = boxes0.copy(), {"intrinsic": _dev(intr)}, []
    B, V = boxes.shape[:2]
    present = None if mask is None else np.asarray(mask, np.uint8).reshape(-1)
    for f in frames:
        out = m.forward_frames(_dev(f), _dev(boxes), cam, view_mask=mask)
        jc = out["joints_crop_img"].cpu().numpy()
        nb, _, img, st = to.next_crop_boxes(jc.reshape(-1, 21, 2), boxes.reshape(-1, 4), cfg.image_size, margin, square, present)
        steps.append({"used": boxes.copy(), "next": nb.reshape(B, V, 4), "joints_img": img.reshape(B, V, 21, 2), "status": st.reshape(B, V),
                      **{k: out[k].cpu().numpy() for k in ("joints_crop_img", "joints_cam", "heatmap")}})
        boxes = nb.reshape(B, V, 4)
    return steps


def _tracker_loop(m, frames, boxes0, intr, margin, square, mask=None):
    from handmvnet_amd import SequenceTracker
    tr = SequenceTracker(m, torch.from_numpy(boxes0), {"intrinsic": _dev(intr)}, margin=margin, square=square)
    ptrs, steps = None, []
    for f in frames:
        out = tr.step(_dev(f), view_mask=mask)
        now = {k: v.data_ptr() for k, v in out.items()}
        assert ptrs is None or now == ptrs                  # the tracker's own buffers, the same at every step
        ptrs = now
        steps.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    assert out["crop_boxes"].data_ptr() == tr.crop_boxes.data_ptr()
    return tr, steps


def _same(got, want, what):
    for t, (g, w) in enumerate(zip(got, want)):
        assert (g["crop_boxes_used"] == w["used"]).all(), (what, t)
        for k in ("joints_crop_img", "joints_cam", "heatmap", "joints_img"):
            assert g[k].shape == w[k].shape and (bits(g[k]) == bits(w[k])).all(), (what, t, k)
        assert (g["status"] == w["status"]).all(), (what, t)
        assert (g["crop_boxes"] == w["next"]).all(), (what, t)


@pytest.mark.parametrize("mode,B", [("f32", 1), ("f32", 2), ("f16", 1), ("f32x3", 1)])
def test_closed_loop_equals_host_loop(mode, B):
    m, cfg = _model(mode)
    frames, boxes0, intr = _sequence(cfg, B, 4)
    want = _host_loop(m, cfg, frames, boxes0, intr, 4, True)
    tr, got = _tracker_loop(m, frames, boxes0, intr, 4, True)
    _same(got, want, (mode, B))
    assert any((s["next"] != s["used"]).any() for s in want)          # the windows do move
    # reset() puts new first windows into the same buffers: the sequence runs again to the same bits
    tr.reset(torch.from_numpy(boxes0))
    out = tr.step(_dev(frames[0]))
    assert (out["crop_boxes"].cpu().numpy() == want[0]["next"]).all() and (bits(out["joints_cam"]) == bits(want[0]["joints_cam"])).all()
    with pytest.raises(ValueError):
        tr.step(_dev(frames[0][:, :, :64]))                               # another frame size
    with pytest.raises(ValueError):
        tr.step(_dev(np.concatenate([frames[0], frames[0]])))             # another batch


def test_graph_replay_of_a_sequence():
    T = 5
    m, cfg = _model()
    frames, boxes0, intr = _sequence(cfg, 2, T, seed=6)
    m.set_graphs(False)
    _, eager = _tracker_loop(m, frames, boxes0, intr, 4, True)
    m.set_graphs(True)
    tr, got = _tracker_loop(m, frames, boxes0, intr, 4, True)
    cached, replays = m.graph_stats()
    m.set_graphs(False)
    for t in range(T):
        for k in eager[t]:
            assert (eager[t][k].view(np.uint8) == got[t][k].view(np.uint8)).all(), (t, k)
    assert cached == 1 and replays >= T - 2
    assert (tr.crop_boxes.cpu().numpy() == eager[-1]["crop_boxes"]).all()


def test_ragged_sequence():
    m, cfg = _model()
    mask = [[1, 1], [1, 0]]
    frames, boxes0, intr = _sequence(cfg, 2, 3, seed=7)
    want = _host_loop(m, cfg, frames, boxes0, intr, 4, True, mask=mask)
    tr, got = _tracker_loop(m, frames, boxes0, intr, 4, True, mask=mask)
    _same(got, want, "ragged")
    for g in got:
        assert g["status"][1, 1] == 1 and (g["crop_boxes"][1, 1] == boxes0[1, 1]).all() and (g["joints_img"][1, 1] == 0).all()
        assert (g["status"][[0, 0, 1], [0, 1, 0]] != 1).all()
    # the view returns: a uniform step on the tracker's buffers moves its window from where it stayed
    out = tr.step(_dev(frames[0]))
    assert (out["crop_boxes_used"][1, 1].cpu().numpy() == boxes0[1, 1]).all() and int(out["status"][1, 1]) != 1


def test_forward_frames_is_untouched_by_a_tracker():
    m, cfg = _model()
    frames, boxes0, intr = _sequence(cfg, 1, 3, seed=8)
    cam = {"intrinsic": _dev(intr)}
    before = {k: v.clone() for k, v in m.forward_frames(_dev(frames[0]), _dev(boxes0), cam).items()}
    _tracker_loop(m, frames, boxes0, intr, 0, True)
    after = m.forward_frames(_dev(frames[0]), _dev(boxes0), cam)
    torch.cuda.synchronize()
    for k in before:
        assert torch.equal(before[k], after[k]), k
