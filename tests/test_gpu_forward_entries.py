"""Every way to call the forward describes its call by one value and keeps nothing of it in the engine handle (csrc/engine.hip
"ForwardCall"): forward, forward_frames, forward_views, forward_frames(view_mask=), forward_subsets and a SequenceTracker step, uniform
and ragged, on tiny_r18 at B = 2 with 96 x 128 frames (the seven calls of tests/golden/make_forward_entry_launches.py).
  (1) interleaved on one model, every plain entry directly behind a tracking one, each gives the bits it gives alone on a fresh model,
      and the tracking buffers of the step before stay as that step left them; f32 and f16, eager and with hipGraph replay, where the
      three uniform entries are captured and replayed each on its own key;
  (2) a tracking call refused in the middle leaves nothing behind either;
  (3) each entry enqueues the number of device operations the commit before this structure enqueued (forward_entry_launches.json).
Everything is compared with == : the forward is deterministic in every arithmetic mode."""
import ctypes
import json

import numpy as np
import pytest
import torch

from handmvnet_amd.spec import heatmap_size_of
from make_forward_entry_launches import B, ENTRIES, FH, FW, MARGIN, OUT, UNIFORM, Rig

pytestmark = pytest.mark.gpu

with open(OUT) as _f:
    LAUNCHES = json.load(_f)["launches"]
# every plain entry directly behind a tracking one, both kinds of tail in front of both kinds of forward
ORDER = ("track", "forward", "track_views", "forward_frames", "track", "forward_views", "track_views", "forward_frames_views", "track",
         "forward_subsets", "track_views", "forward")
TRACKING = ("joints_img", "status", "crop_boxes")   # what a tracking tail writes besides the forward's outputs
_SOLO = {}


def _snap(out):
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert (got[k].view(np.uint8) == want[k].view(np.uint8)).all(), (what, k)


def solo(mode):
    """Per entry (outputs, launch count) of the call alone on a fresh eager model: computed once per mode, shared, never changed."""
    if mode not in _SOLO:
        res = {}
        for name in ENTRIES:
            rig = Rig(mode)
            res[name] = (_snap(rig.call(name)), rig.m.launch_count())
        _SOLO[mode] = res
    return _SOLO[mode]


def _fixed_buffers(rig):
    """Caller-owned outputs for the two plain uniform entries, so that a repeated call presents the same addresses (a graph key)."""
    m, d = rig.m, rig.dev
    size = rig.cfg.image_size
    bb, it = d["bbox"].reshape(-1, 4).contiguous().float(), d["intr"].reshape(-1, 4).contiguous().float()
    boxes = d["boxes"].reshape(-1, 4).contiguous()
    windows = boxes.float()
    mean, std = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    outs = {n: dict(zip(("joints_crop_img", "joints_cam", "heatmap"), m._outputs(d["x"].device, (B, m.num_views), (B,), heatmap_size_of(rig.cfg, size, size))))
            for n in ("forward", "forward_frames")}

    def call(name):
        o = outs[name]
        if name == "forward":
            m._call("hmv_forward", size, size, d["x"].device, B, d["x"], bb, it, *o.values())
        else:
            m._call("hmv_forward_frames", size, size, d["x"].device, B, d["frames"], FH, FW, boxes, mean, std, windows, it, *o.values())
        return o
    keep = (bb, it, boxes, windows)   # the graph replays read these addresses
    return call, keep


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_interleaved_entries_give_their_solo_bits(mode, graphs):
    want = solo(mode)
    rig = Rig(mode, graphs=graphs)
    fixed, keep = _fixed_buffers(rig)
    for name in ("forward_subsets", "forward_views"):   # (the workspace takes its final size before anything is captured)
        _same(_snap(rig.call(name)), want[name][0], ("first", name))
    tracked = {}   # tracking entry -> the dict of its last step: views of the tracker's own buffers
    order = ORDER * 3 if graphs else ORDER   # with graphs: every uniform entry at least three times on the same buffers
    for i, name in enumerate(order):
        out = fixed(name) if graphs and name in ("forward", "forward_frames") else rig.call(name)
        _same(_snap(out), want[name][0], (i, name))
        if not graphs and mode == "f32":
            assert rig.m.launch_count() == LAUNCHES[name], (i, name)
        if name in ("track", "track_views"):
            tracked[name] = out
        else:   # a plain entry: the buffers of the tracking steps before it are as those steps left them
            for tname, tout in tracked.items():
                for k in TRACKING:
                    assert (tout[k].cpu().numpy() == want[tname][0][k]).all(), (i, name, "touched", tname, k)
    if graphs:
        cached, replays = rig.m.graph_stats()
        assert cached == len(UNIFORM), (cached, replays)   # forward, forward_frames and the tracking step: one graph each
        assert replays == sum(order.count(n) - 2 for n in UNIFORM)   # a key runs eagerly once, is captured on its second use
    del keep


def test_a_refused_tracking_call_leaves_nothing_behind():
    from handmvnet_amd import _lib
    lib, want = _lib.load(), solo("f32")
    rig = Rig("f32")
    m, d, size = rig.m, rig.dev, rig.cfg.image_size
    dev = d["x"].device
    tracked = rig.call("track")
    h = m._engine(size, size, 0)
    launches = lib.hmv_launch_count(h)
    it = d["intr"].reshape(-1, 4).contiguous().float()
    boxes = d["boxes"].reshape(-1, 4).contiguous().clone()
    bbox = boxes.float()
    crop, cam, hm = m._outputs(dev, (B, m.num_views), (B,), heatmap_size_of(rig.cfg, size, size))
    canary_img = torch.full((B, m.num_views, 21, 2), 7.5, device=dev)
    canary_status = torch.full((B, m.num_views), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    mean, std = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: t.data_ptr()   # noqa: E731
    table = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    rc = lib.hmv_forward_frames_track(h, B, p(d["frames"]), FH, FW, p(boxes), mean, (ctypes.c_float * 3)(0.2, 0.0, 0.2), p(bbox), p(it),
                                      p(crop), p(cam), p(hm), MARGIN, 1, p(canary_img), p(canary_status), stream)
    assert rc == 1 and b"std must be positive" in lib.hmv_last_error(h)          # HMV_ERR_ARG
    assert lib.hmv_launch_count(h) == launches
    rc = lib.hmv_forward_frames_views_track(h, B, (ctypes.c_int32 * B)(2, 0), p(d["frames"]), FH, FW, p(boxes), p(table), mean, std, p(bbox),
                                            p(it), p(crop), p(cam), p(hm), MARGIN, 1, p(canary_img), p(canary_status), stream)
    assert rc == 1 and b"view_counts[1] = 0" in lib.hmv_last_error(h)
    assert lib.hmv_launch_count(h) == launches
    # the next plain call: its solo bits, the plain forward's launches, no tail
    rc = lib.hmv_forward_frames(h, B, p(d["frames"]), FH, FW, p(boxes), mean, std, p(bbox), p(it), p(crop), p(cam), p(hm), stream)
    assert rc == 0
    assert lib.hmv_launch_count(h) == LAUNCHES["forward_frames"]
    _same(_snap({"joints_crop_img": crop, "joints_cam": cam, "heatmap": hm}), want["forward_frames"][0], "forward_frames")
    assert (canary_img == 7.5).all() and (canary_status == 0x5A5A5A5A).all()
    assert torch.equal(boxes, d["boxes"].reshape(-1, 4)) and torch.equal(bbox, boxes.float())
    for k in TRACKING:
        assert (tracked[k].cpu().numpy() == want["track"][0][k]).all(), k


def test_every_entry_enqueues_what_it_enqueued_before():
    """Exact equality with tests/golden/forward_entry_launches.json, which the commit before this structure wrote."""
    assert set(LAUNCHES) == set(ENTRIES)
    got = {name: n for name, (_, n) in solo("f32").items()}
    assert got == LAUNCHES
