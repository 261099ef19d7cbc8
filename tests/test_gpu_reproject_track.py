"""Windows from the reprojected pose on the device (include/handmv.h: hmv_op_reproject_crop_boxes; csrc/track.hip;
handmvnet_amd/tracking.py):
  (1) the raw entry against the fixture of the real reference functions on guarded buffers -- windows, bbox, status and source exactly,
      joints_reproj equal-or-adjacent fp32, gap equal-or-adjacent against the oracle on the device's own joints_reproj;
  (2) every slot of a 1-, 5- and 9-slot call against a call that holds it alone, bit for bit;   (3) the optional operands absent;
  (4) joints_reproj == hmv_project_joints, bit for bit;   (5) an exact rig with a fooled and an absent camera;
  (6) SequenceTracker(windows="reprojected") == the host loop from the public pieces, bit for bit, on a rig where the windows must
      follow the reprojection;   (7) a rig whose cameras look away: the own-joints windows;   (8) graphs;   (9) a ragged sequence;
  (10) a tracker without the new arguments;   (11) a SequenceEvaluator over a reprojecting tracker."""
import ctypes
import os

import numpy as np
import pytest
import torch

import reproject_oracle as ro
from guards import Guards
from helpers import load_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "reproject_cases.npz"))
NAMES = sorted({k.split(".")[0] for k in FIX.files})
DEV = "cuda:0"


def case(name):
    return {k.split(".", 1)[1]: FIX[k] for k in FIX.files if k.startswith(name + ".")}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return bool((bits(a) == bits(b)).all())


def raw(p3, intr, ext, boxes, status, *, point_status=None, frame_cam=None, joints_img=None, margin=0, square=True, require_all=False,
        with_bbox=True, with_reproj=True, with_gap=True):
    """One raw hmv_op_reproject_crop_boxes call from numpy arrays on guarded device buffers -> numpy dict; the bands and the inputs
    are checked.  The in/out operands start as the given windows and status."""
    from handmvnet_amd import _lib
    g = Guards(DEV)
    B, V = status.shape
    a = _lib.HmvReprojectBoxesArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvReprojectBoxesArgs)
    a.B, a.V, a.margin, a.square, a.require_all = B, V, int(margin), int(square), int(require_all)
    keep = {}
    for name, arr, dt in (("points3d", p3, np.float32), ("intrinsic", intr, np.float32), ("extrinsic", ext, np.float32),
                          ("point_status", point_status, np.int32), ("frame_cam", frame_cam, np.int32), ("joints_img", joints_img, np.float32)):
        if arr is not None:
            keep[name] = g.inp(torch.from_numpy(np.ascontiguousarray(arr, dt)))
            setattr(a, name, keep[name].data_ptr())
    out = {"crop_boxes": g.out((B, V, 4), torch.int32), "status": g.out((B, V), torch.int32), "source": g.out((B, V), torch.int32)}
    out["crop_boxes"].copy_(_dev(boxes.astype(np.int32)))
    out["status"].copy_(_dev(status.astype(np.int32)))
    if with_bbox:
        out["bbox"] = g.out((B, V, 4))
        out["bbox"].copy_(_dev(boxes.astype(np.float32)))
    if with_reproj:
        out["joints_reproj"] = g.out((B, V, 21, 2))
    if with_gap:
        out["gap"] = g.out((B, V))
    for name, t in out.items():
        setattr(a, name, t.data_ptr())
    _lib.check(_lib.load().hmv_op_reproject_crop_boxes(0, ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    g.check()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def raw_case(c, **over):
    kw = dict(point_status=c["point_status"], frame_cam=c["frame_cam"], joints_img=c["joints_img"], margin=int(c["margin"]),
              square=bool(c["square"]))
    kw.update(over)
    return raw(c["points3d"], c["intr"], c["ext"], c["boxes_in"], c["status_in"], **kw)


# ------------------------------------------------------------------ the op
@pytest.mark.parametrize("require_all", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_op_matches_reference_fixture(name, require_all):
    c = case(name)
    tag = "_all" if require_all else ""
    got = raw_case(c, require_all=require_all)
    assert np.array_equal(got["crop_boxes"], c["boxes" + tag]), name
    assert np.array_equal(got["status"], c["status" + tag]) and np.array_equal(got["source"], c["source" + tag])
    moved = got["source"] == 1
    assert same_bits(got["bbox"][moved], c["boxes" + tag].astype(np.float32)[moved])
    # a slot that is not reprojected keeps every byte of its window, its fp32 copy and its status
    assert np.array_equal(got["crop_boxes"][~moved], c["boxes_in"][~moved]) and np.array_equal(got["status"][~moved], c["status_in"][~moved])
    assert same_bits(got["bbox"][~moved], c["boxes_in"].astype(np.float32)[~moved])
    want = c["joints_2d"].copy()
    want[~c["ok" + tag]] = np.nan
    near = ro.adjacent(got["joints_reproj"], want)
    print(f"{name}{tag}: joints_reproj differs from the reference's fp32 in {int((bits(got['joints_reproj']) != bits(want)).sum())} of {want.size} values")
    assert near.all(), (name, np.argwhere(~near)[:4])
    gap = ro.gap_of(c["joints_img"], got["joints_reproj"], c["status_in"], c["ok" + tag])
    assert ro.adjacent(got["gap"], gap).all(), (name, got["gap"], gap)
    # python op: new tensors, the inputs untouched
    from handmvnet_amd import reproject_crop_boxes
    b_in, s_in = _dev(c["boxes_in"]), _dev(c["status_in"])
    res = reproject_crop_boxes(_dev(c["points3d"]), _dev(c["intr"]), _dev(c["ext"]), b_in, s_in, point_status=_dev(c["point_status"]),
                               frame_cam=c["frame_cam"], joints_img=_dev(c["joints_img"]), margin=int(c["margin"]),
                               square=bool(c["square"]), require_all=require_all)
    for k, t in zip(("crop_boxes", "bbox", "status", "source", "joints_reproj", "gap"), res):
        assert t.cpu().numpy().tobytes() == got[k].tobytes(), (name, k)
    assert np.array_equal(b_in.cpu().numpy(), c["boxes_in"]) and np.array_equal(s_in.cpu().numpy(), c["status_in"])


def _alone(p3, intr, ext, boxes, status, ps, fc, ji, b, v, **kw):
    """Slot (b, v) in a call that holds it alone: one sample, and the one view -- behind its frame camera where that is another."""
    views = [v] if fc[b] == v else [int(fc[b]), v]
    sel = np.ix_([b], views)
    got = raw(p3[[b]], intr[sel], ext[sel], boxes[sel], status[sel], point_status=ps[[b]], frame_cam=np.zeros(1, np.int32),
              joints_img=ji[sel], **kw)
    return {k: a[0, -1] for k, a in got.items()}


@pytest.mark.parametrize("slots", [1, 5, 9])
def test_every_slot_has_the_bits_of_a_call_that_holds_it_alone(slots):
    """B * V = 1, 5 and 9 slots (no multiple of the four slots of a workgroup), cut from the fixture's rigs: any matrices are a rig."""
    c, d = case("plain_v4_m4"), case("frame_cam")
    keys = ("intr", "ext", "boxes_in", "status_in", "joints_img")
    if slots == 1:
        arrs = [c[k][:1, :1] for k in keys]
        p3, ps, fc = c["points3d"][:1], c["point_status"][:1], np.zeros(1, np.int32)
    elif slots == 5:      # one sample with five cameras: the four of sample 0 and one of sample 1
        arrs = [np.concatenate([c[k][:1], c[k][1:2, :1]], axis=1) for k in keys]
        p3, ps, fc = c["points3d"][:1], c["point_status"][:1], np.zeros(1, np.int32)
    else:                 # three samples of three cameras, each with its own frame camera, an absent and a kept view among them
        arrs = [d[k][:, [0, 2, 3]].copy() for k in keys]
        p3, ps, fc = d["points3d"], d["point_status"], np.array([1, 0, 2], np.int32)
        assert d["frame_cam"].tolist() == [2, 0, 3]
        arrs[3][0, 1], arrs[3][1, 2] = 1, 2
    intr, ext, boxes, status, ji = arrs
    kw = dict(margin=4, square=True)
    full = raw(p3, intr, ext, boxes, status, point_status=ps, frame_cam=fc, joints_img=ji, **kw)
    assert full["source"].size == slots and full["source"].sum() >= slots - 1
    for b, v in np.ndindex(*status.shape):
        one = _alone(p3, intr, ext, boxes, status, ps, fc, ji, b, v, **kw)
        for k in full:
            assert full[k][b, v].tobytes() == one[k].tobytes(), (slots, b, v, k)


def test_optional_operands_absent():
    c = case("plain_v4_m4")
    full = raw_case(c, frame_cam=None, point_status=None)
    bare = raw_case(c, frame_cam=None, point_status=None, joints_img=None, with_bbox=False, with_reproj=False, with_gap=False)
    assert set(bare) == {"crop_boxes", "status", "source"}
    for k in bare:
        assert np.array_equal(bare[k], full[k]), k
    assert np.array_equal(full["crop_boxes"], c["boxes"]) and not np.isnan(full["gap"]).any()
    nogap = raw_case(c, joints_img=None)
    assert np.isnan(nogap["gap"]).all() and same_bits(nogap["joints_reproj"], raw_case(c)["joints_reproj"])


def test_joints_reproj_has_the_bits_of_hmv_project_joints():
    from handmvnet_amd.camera import get_2d_joints_from_3d_joints
    for name in ("plain_v3", "plain_v4_m4", "square_off", "behind", "huge_window"):
        c = case(name)
        assert not c["frame_cam"].any()
        got = raw_case(c)["joints_reproj"]
        want = get_2d_joints_from_3d_joints(_dev(c["points3d"]), 0, _dev(c["intr"]), _dev(c["ext"]))
        assert same_bits(got, want), name
    c = case("one_sample")      # another frame camera is another root_idx
    want = get_2d_joints_from_3d_joints(_dev(c["points3d"]), int(c["frame_cam"][0]), _dev(c["intr"]), _dev(c["ext"]))
    assert same_bits(raw_case(c)["joints_reproj"], want)


def test_geometry_a_fooled_and_an_absent_camera_get_the_hand_back():
    """An exact rig with four cameras.  The 2D joints are the true projections, but view 2's are displaced by 200 px and view 3 is
    absent; RANSAC runs over candidates of two cameras.  After triangulate and the new op every view's window (margin 4, which covers
    the truncation of the maximum toward zero) contains every true projection; the own-joints window of view 2 does not."""
    from handmvnet_amd import next_crop_boxes, reproject_crop_boxes, triangulate
    c = case("plain_v4_m4")
    p3, intr, ext = c["points3d"][:1], c["intr"][:1], c["ext"][:1]
    u, v, z = ro.project(p3, intr, ext)
    true = np.stack([u, v], axis=-1).astype(np.float32)                     # [1, 4, 21, 2]
    assert (z > 0).all()
    pts = true.copy()
    pts[0, 2, :, 0] += 200.0
    present = np.array([[1, 1, 1, 0]], np.uint8)
    pts[0, 3] = 0.0
    boxes0 = np.tile(np.array([0, 0, 64, 64], np.int32), (1, 4, 1))
    # the own-joints rule, with the frame as the window (scale 1): every camera follows what it saw itself
    own, _, _, st = next_crop_boxes(_dev(pts), _dev(boxes0), 64, 4, True, present=_dev(present))
    tri, tst = triangulate(_dev(pts), _dev(intr), _dev(ext), present=_dev(present), subsets=[[0, 1], [0, 2], [1, 2], [0, 3], [1, 3], [2, 3]],
                           threshold=5.0, refit=True, frame_cam=0)
    assert not tst.cpu().numpy().any()
    boxes, _, st2, source, reproj, gap = reproject_crop_boxes(tri, _dev(intr), _dev(ext), own, st, point_status=tst, frame_cam=0,
                                                              joints_img=_dev(pts), margin=4, square=True, require_all=True)

    def contains(box, p):
        return bool((p[:, 0] >= box[0]).all() and (p[:, 0] <= box[2]).all() and (p[:, 1] >= box[1]).all() and (p[:, 1] <= box[3]).all())
    boxes, own = boxes.cpu().numpy(), own.cpu().numpy()
    assert source.cpu().numpy().tolist() == [[1, 1, 1, 1]] and st2.cpu().numpy().tolist() == [[0, 0, 0, 1]]
    for cam in range(4):
        assert contains(boxes[0, cam], true[0, cam]), cam
    assert not contains(own[0, 2], true[0, 2]) and (own[0, 3] == boxes0[0, 3]).all()
    assert np.abs(reproj.cpu().numpy() - true).max() < 0.05                 # the triangulation of exact fp32 pixels
    gap = gap.cpu().numpy()
    assert gap[0, 0] < 0.05 and gap[0, 1] < 0.05 and abs(gap[0, 2] - 200) < 0.05 and np.isnan(gap[0, 3])


# ------------------------------------------------------------------ sequences
FH, FW = 96, 128
FOLLOW_X = {2: [(72, 120), (6, 54)], 3: [(88, 124), (46, 82), (4, 40)]}
BASELINE = 1000.0      # between neighbouring cameras, in the pose's unit: see _rig


def _model(case_name="tiny_r18", mode="f32"):
    from handmvnet_amd import HandMvNet
    cfg, (tp, mp, dp), sd, _, _ = load_case(case_name)
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    if mode == "f16":
        m.half()
    return m, cfg


def _frames(V, B, T, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:FH, 0:FW].astype(np.float32)
    frames = np.empty((T, B, V, FH, FW, 3), np.uint8)
    for t, b, v in np.ndindex(T, B, V):
        ph = rng.uniform(0, 6.28, 3)
        img = np.stack([127 + 80 * np.sin(xx / (9 + 2 * c) + ph[c] + 0.3 * t) * np.cos(yy / (7 + c) + 0.2 * t) for c in range(3)], -1)
        frames[t, b, v] = np.clip(img + rng.standard_normal(img.shape) * 6, 0, 255).astype(np.uint8)
    return frames


def _rig(B, V, kind):
    """Intrinsics [B, V, 4], camera-to-world extrinsics [B, V, 4, 4] (metres) and first windows [B, V, 4].
    "follow": near-parallel cameras BASELINE apart along x, each later view's first window strictly to the left of the earlier one's.
       A joint anywhere in its window then has a positive disparity d between any two views, whatever the synthetic weights make of the
       frames, and is triangulated at the depth fx * BASELINE / d in front of every camera.  The synthetic weights' joints_cam spans
       several units (up to 7.7 on the golden input of tiny_r18) where a trained model's spans a hand: the baseline is chosen far above
       that, so the whole fused pose lies in front of every camera and projects into a window a few pixels wide -- far narrower than the
       disparity that separates the windows of two views, which therefore stay strictly apart at the next step, and so on.
    "away": two cameras BASELINE apart that look away from each other along the baseline, the first windows on the sides of the
       principal points (which lie beside the frame) where the two rays meet BETWEEN the cameras: hundreds of units behind both, so
       no view can be reprojected at any step."""
    intr = np.tile(np.array([500, 500, 64, 48], np.float32), (B, V, 1))
    ext = np.tile(np.eye(4, dtype=np.float32), (B, V, 1, 1))
    if kind == "follow":
        for v in range(V):
            a = 0.01 * v
            ext[:, v, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
            ext[:, v, 0, 3] = BASELINE * v
        xs = FOLLOW_X[V]
    else:
        assert V == 2
        ext[:, 0, :3, :3] = np.stack([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], axis=1)       # columns: the camera's x, y, z axes in the world
        ext[:, 1, :3, :3] = np.stack([[0, 0, -1], [0, 1, 0], [1, 0, 0]], axis=1)
        ext[:, 1, 0, 3] = BASELINE
        intr[:, 0, 2], intr[:, 1, 2] = -200.0, 400.0      # principal points beside the frame: no window wanders across them
        xs = [(80, 120), (8, 48)]
    boxes0 = np.array([[[x1, 24 + 2 * b, x2, 24 + 2 * b + (x2 - x1)] for x1, x2 in xs] for b in range(B)], np.int32)
    return intr, ext, boxes0


def _project_on_device(p3, fc, intr, ext):
    """hmv_project_joints per sample (its root_idx is one per call): the bits of the entry's joints_reproj."""
    from handmvnet_amd.camera import get_2d_joints_from_3d_joints
    return torch.cat([get_2d_joints_from_3d_joints(p3[b:b + 1], int(fc[b]), intr[b:b + 1], ext[b:b + 1]) for b in range(p3.shape[0])])


def _host_loop(m, cfg, frames, boxes0, intr, ext, margin, square, pose="fused", mask=None, ransac=None, confidence=None):
    """The step written from the public pieces: forward_frames, next_crop_boxes, (heatmap_peaks,) triangulate, hmv_project_joints and
    the numpy oracle.  The projections the oracle builds its windows on are hmv_project_joints' (`projected=`), so the comparison of
    joints_reproj with the tracker's is device against device, and the oracle supplies the sample and slot rules, the depth's sign,
    the integer box rule and the gap; what pins joints_reproj to the reference is the op-level fixture test above.  On these rigs the
    reprojected windows are a few pixels wide: the square rule and its odd pixel are exercised at op level, not here."""
    from handmvnet_amd import heatmap_peaks, next_crop_boxes, triangulate
    from handmvnet_amd.triangulation import parse_gate, parse_ransac
    B, V = boxes0.shape[:2]
    boxes, steps = boxes0.copy(), []
    cam = {"intrinsic": _dev(intr), "extrinsic": _dev(ext)}
    hmask = np.ones((B, V), bool) if mask is None else np.asarray(mask, bool)
    fc = hmask.argmax(axis=1).astype(np.int32)
    table, thr = parse_ransac(V, ransac)
    gate = parse_gate(confidence)
    for f in frames:
        out = m.forward_frames(_dev(f), _dev(boxes), cam, view_mask=mask)
        extra = {}
        if gate is not None:
            hm = out["heatmap"]
            conf = heatmap_peaks(hm.reshape(B, V, 21, hm.shape[-2], hm.shape[-1]))[0]
            extra = dict(confidences=conf, confidence_threshold=gate[0], confidence_step=gate[1], carry=gate[2])
        nb, _, img, st = next_crop_boxes(out["joints_crop_img"], _dev(boxes), cfg.image_size, margin, square,
                                         present=None if mask is None else _dev(hmask.astype(np.uint8)))
        present = _dev(hmask) & (st == 0)
        tri, tst = triangulate(img, cam["intrinsic"], cam["extrinsic"], present=present, subsets=table, threshold=thr,
                               refit=table is not None, frame_cam=fc, **extra)
        fused = out["joints_cam"] + tri[:, :1]
        p3 = fused if pose == "fused" else tri
        proj = _project_on_device(p3, fc, cam["intrinsic"], cam["extrinsic"]).cpu().numpy()
        r = ro.reproject_crop_boxes(p3.cpu().numpy(), intr, ext, nb.cpu().numpy(), st.cpu().numpy(), point_status=tst.cpu().numpy(),
                                    frame_cam=fc, joints_img=img.cpu().numpy(), margin=margin, square=square,
                                    require_all=pose != "fused", projected=proj)
        steps.append({"crop_boxes_used": boxes.copy(), "crop_boxes": r["crop_boxes"], "status": r["status"], "source": r["source"],
                      "joints_reproj": r["joints_reproj"], "reproj_gap": r["gap"], "joints_img": img.cpu().numpy(),
                      "joints_tri": tri.cpu().numpy(), "tri_status": tst.cpu().numpy(), "joints_abs": fused.cpu().numpy(),
                      "own_boxes": nb.cpu().numpy(), **{k: out[k].cpu().numpy() for k in ("joints_crop_img", "joints_cam", "heatmap")}})
        boxes = r["crop_boxes"]
    return steps


def _tracker_loop(m, frames, boxes0, intr, ext, margin, square, mask=None, **kw):
    from handmvnet_amd import SequenceTracker
    tr = SequenceTracker(m, torch.from_numpy(boxes0), {"intrinsic": _dev(intr), "extrinsic": _dev(ext)}, margin=margin, square=square, **kw)
    ptrs, steps = None, []
    for f in frames:
        out = tr.step(_dev(f), view_mask=mask)
        now = {k: v.data_ptr() for k, v in out.items()}
        assert ptrs is None or now == ptrs                  # the tracker's own buffers, the same at every step
        ptrs = now
        steps.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    return tr, steps


def _same(got, want, what):
    for t, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) - {"own_boxes"}, (what, set(g) ^ set(w))
        for k in g:
            assert g[k].shape == w[k].shape and g[k].dtype == w[k].dtype, (what, t, k, g[k].dtype, w[k].dtype)
            assert g[k].tobytes() == w[k].tobytes(), (what, t, k)


@pytest.mark.parametrize("mode,B,pose", [("f32", 1, "fused"), ("f32", 2, "fused"), ("f16", 1, "fused"), ("f16", 2, "fused"),
                                         ("f32", 2, "triangulated"), ("f16", 1, "triangulated")])
def test_closed_loop_equals_host_loop_and_follows_the_reprojection(mode, B, pose):
    m, cfg = _model(mode=mode)
    V, T = cfg.num_views, 4
    intr, ext, boxes0 = _rig(B, V, "follow")
    frames = _frames(V, B, T, seed=11)
    want = _host_loop(m, cfg, frames, boxes0, intr, ext, 4, True, pose=pose)
    tr, got = _tracker_loop(m, frames, boxes0, intr, ext, 4, True, windows="reprojected", pose=pose)
    _same(got, want, (mode, B, pose))
    for t, g in enumerate(got):
        print(f"step {t}: source {g['source'].tolist()} status {g['status'].tolist()} gap {g['reproj_gap'].tolist()}")
        assert (g["source"] == 1).any(), t                   # the path taken is the reprojection's, at every step
    assert any((w["crop_boxes"] != w["own_boxes"]).any() for w in want)      # and it is not the own-joints rule's windows
    assert tr._bbox is not None and tr._bbox.cpu().numpy().tobytes() == got[-1]["crop_boxes"].astype(np.float32).tobytes()


@pytest.mark.parametrize("kw", [dict(ransac=(2, 40.0)), dict(confidence=0.3), dict(ransac=(2, 40.0), confidence=(0.3, 0.1, True))],
                         ids=["ransac", "confidence", "both"])
def test_closed_loop_with_ransac_and_confidence_equals_host_loop(kw):
    """The tracker's ransac / refit / confidence arguments against the host loop that hands the same ones to triangulate(): whichever
    path the synthetic heat maps and the candidates' inliers lead to, every returned key has the host loop's bits."""
    m, cfg = _model()
    V = cfg.num_views
    intr, ext, boxes0 = _rig(2, V, "follow")
    frames = _frames(V, 2, 3, seed=17)
    want = _host_loop(m, cfg, frames, boxes0, intr, ext, 4, True, **kw)
    _, got = _tracker_loop(m, frames, boxes0, intr, ext, 4, True, windows="reprojected", **kw)
    _same(got, want, kw)
    for t, g in enumerate(got):
        print(f"step {t}: source {g['source'].tolist()} tri_status {g['tri_status'].tolist()}")


def test_reprojected_windows_need_the_rig():
    from handmvnet_amd import SequenceTracker
    m, cfg = _model()
    intr, ext, boxes0 = _rig(1, cfg.num_views, "follow")
    with pytest.raises(ValueError, match="extrinsic"):
        SequenceTracker(m, torch.from_numpy(boxes0), {"intrinsic": _dev(intr)}, windows="reprojected")
    with pytest.raises(ValueError, match="extrinsic"):
        SequenceTracker(m, torch.from_numpy(boxes0), {"intrinsic": _dev(intr), "extrinsic": _dev(ext[:, :1])}, windows="reprojected")


def test_cameras_that_look_away_fall_back_to_the_own_joints_windows():
    m, cfg = _model()
    intr, ext, boxes0 = _rig(2, cfg.num_views, "away")
    frames = _frames(cfg.num_views, 2, 4, seed=12)
    _, plain = _tracker_loop(m, frames, boxes0, intr, ext, 4, True)
    _, got = _tracker_loop(m, frames, boxes0, intr, ext, 4, True, windows="reprojected")
    for t, (g, p) in enumerate(zip(got, plain)):
        assert not g["source"].any(), (t, g["source"])
        for k in p:
            assert g[k].tobytes() == p[k].tobytes(), (t, k)


def test_graph_replay_equals_eager():
    T = 5
    m, cfg = _model()
    intr, ext, boxes0 = _rig(2, cfg.num_views, "follow")
    frames = _frames(cfg.num_views, 2, T, seed=13)
    m.set_graphs(False)
    _, eager = _tracker_loop(m, frames, boxes0, intr, ext, 4, True, windows="reprojected")
    m.set_graphs(True)
    _, got = _tracker_loop(m, frames, boxes0, intr, ext, 4, True, windows="reprojected")
    cached, replays = m.graph_stats()
    m.set_graphs(False)
    for t in range(T):
        for k in eager[t]:
            assert eager[t][k].tobytes() == got[t][k].tobytes(), (t, k)
    assert cached == 1 and replays >= T - 2
    assert all((g["source"] == 1).any() for g in got)


@pytest.mark.parametrize("model_case", ["r50_wocam_nn", "r50_lq"])
def test_ragged_sequence_moves_the_absent_view_s_window(model_case):
    """The mask of test_gpu_track.py::test_ragged_sequence, [[1, 1], [1, 0]], with a third camera in front: a sample needs two present
    views to be triangulated, so the models are three-view ones -- one without crop-FoV columns (the tracker keeps no bbox) and one
    with them, whose full fp32 copy of the windows must follow the launch that moved them last."""
    m, cfg = _model(model_case)
    V = cfg.num_views
    assert V == 3
    mask = [[1, 1, 1], [1, 1, 0]]
    intr, ext, boxes0 = _rig(2, V, "follow")
    frames = _frames(V, 2, 3, seed=14)
    want = _host_loop(m, cfg, frames, boxes0, intr, ext, 4, True, mask=mask)
    tr, got = _tracker_loop(m, frames, boxes0, intr, ext, 4, True, mask=mask, windows="reprojected")
    _same(got, want, "ragged")
    for g in got:
        assert g["status"][1, 2] == 1 and g["source"][1, 2] == 1 and (g["joints_img"][1, 2] == 0).all() and np.isnan(g["reproj_gap"][1, 2])
        assert (g["crop_boxes"][1, 2] != boxes0[1, 2]).any()              # absent, and its window moved all the same
    assert (tr._bbox is not None) == (model_case == "r50_lq")
    if tr._bbox is not None:
        assert tr._bbox.cpu().numpy().tobytes() == got[-1]["crop_boxes"].astype(np.float32).tobytes()
    moved_to = got[-1]["crop_boxes"][1, 2].copy()
    out = tr.step(_dev(frames[0]))                                        # the view returns and runs on the window it was given
    assert (out["crop_boxes_used"][1, 2].cpu().numpy() == moved_to).all() and int(out["status"][1, 2]) != 1


def test_a_tracker_without_the_new_arguments_is_the_parent_s():
    from handmvnet_amd import next_crop_boxes
    m, cfg = _model()
    intr, ext, boxes0 = _rig(2, cfg.num_views, "follow")
    frames = _frames(cfg.num_views, 2, 4, seed=15)
    _, got = _tracker_loop(m, frames, boxes0, intr, ext, 4, True)
    boxes, cam = _dev(boxes0), {"intrinsic": _dev(intr)}
    for t, f in enumerate(frames):
        assert set(got[t]) == {"joints_crop_img", "joints_cam", "heatmap", "joints_img", "status", "crop_boxes", "crop_boxes_used"}
        out = m.forward_frames(_dev(f), boxes, cam)
        assert (got[t]["crop_boxes_used"] == boxes.cpu().numpy()).all()
        boxes, _, img, st = next_crop_boxes(out["joints_crop_img"], boxes, cfg.image_size, 4, True)
        for k, w in (("crop_boxes", boxes), ("joints_img", img), ("status", st), ("joints_cam", out["joints_cam"]),
                     ("joints_crop_img", out["joints_crop_img"]), ("heatmap", out["heatmap"])):
            assert got[t][k].tobytes() == w.cpu().numpy().tobytes(), (t, k)


def test_an_evaluator_takes_a_reprojecting_tracker():
    from handmvnet_amd import SequenceEvaluator, SequenceTracker
    m, cfg = _model("r50_wocam_nn")
    V = cfg.num_views
    intr, ext, boxes0 = _rig(2, V, "follow")
    cam = {"intrinsic": _dev(intr), "extrinsic": _dev(ext)}
    ev = SequenceEvaluator(SequenceTracker(m, torch.from_numpy(boxes0), cam, margin=4, windows="reprojected"), cam)
    sources = []
    for f in _frames(V, 2, 3, seed=16):
        sources.append(ev.step(_dev(f), view_mask=[[1, 1, 1], [1, 1, 0]])["source"].cpu().numpy().copy())
    n = ev.compute()
    assert n["window_moved"] + n["window_absent"] + n["window_kept"] == 1.0
    assert n["window_absent"] == 1 / 6 and all(s[1, 2] == 1 for s in sources)      # the absent view is counted absent though its window moved
