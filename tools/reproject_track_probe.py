#!/usr/bin/env python3
"""Timing record of a sequence whose windows follow the reprojected 3D pose: milliseconds per time step of

  (a) reprojected  SequenceTracker(windows="reprojected").step: the call of (b), then, eager on the same stream, the triangulation of
                   the views' 2D joints, the pose and hmv_op_reproject_crop_boxes in place on the windows;
  (b) joints       SequenceTracker(windows="joints").step: ONE call (hmv_forward_frames_track), one replayed hipGraph

on the eval_fps shape -- ResNet50-paper at 256 x 256, batch 1 x 8 views -- fp32 and fp16, graphs on, synthetic 480 x 640 frames
resident on the device (the same frames at every step).  The rig is eight near-parallel cameras BASELINE apart along x, each
later view's first window strictly to the left of the earlier one's, so that every joint has a positive disparity and the windows do
come from the reprojection (the record holds the fraction of slot-steps with source == 1).  What (a) adds is never captured into the
graph: the difference is what the extra launches and the torch ops between them cost per step.

Both loops run in the one process in alternating blocks of --block steps; a block is timed with the host clock from its first enqueue
to a device synchronisation behind its last step; the figure is the median over blocks.

A record, not a gate.    python tools/reproject_track_probe.py [--blocks 5] [--block 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from handmvnet_amd import HandMvNet, SequenceTracker  # noqa: E402
from handmvnet_amd.spec import config_from_params  # noqa: E402
from handmvnet_amd.synth import synth_state_dict  # noqa: E402

B, V, SIZE, FH, FW, MARGIN = 1, 8, 256, 480, 640, 20
BASELINE = 1000.0   # far above the extent of the synthetic weights' joints_cam: the fused pose stays in front of every camera


def build(dtype, dev):
    tp = {"debug": False, "root_relative": True}
    mp = {"num_views": V, "backbone": "resnet", "backbone_type": "50_paper", "backbone_channels": [1024], "backbone_pretrained": False,
          "backbone_early_return": 3, "pos_enc": ["pos2d", "crop", "sin"], "fusion": "cross_attn", "fusion_layers": 5, "use_gcn": True}
    dp = {"batch_size": B, "image_size": SIZE, "heatmap_size": SIZE // 8, "name": "dexycb"}
    cfg = config_from_params(tp, mp, dp)
    model = HandMvNet(tp, mp, dp)
    model.load_state_dict(synth_state_dict(cfg, 1), strict=True)
    model.to(dev).eval()
    if dtype == "f16":
        model.half()
    model.reserve(B, SIZE, SIZE, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    frames = torch.randint(0, 256, (B, V, FH // 8, FW // 8, 3), dtype=torch.uint8, device=dev, generator=g)
    frames = frames.repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()       # blocky content: not flat, not white noise
    boxes0 = np.array([[[565 - 80 * v, 200, 635 - 80 * v, 270] for v in range(V)]] * B, np.int32)
    intr = np.tile(np.array([500, 500, 320, 240], np.float32), (B, V, 1))
    ext = np.tile(np.eye(4, dtype=np.float32), (B, V, 1, 1))
    for v in range(V):
        a = 0.005 * v
        ext[:, v, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        ext[:, v, 0, 3] = BASELINE * v
    cam = {"intrinsic": torch.from_numpy(intr).to(dev), "extrinsic": torch.from_numpy(ext).to(dev)}
    return model, frames, boxes0, cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="f32,f16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for dtype in a.dtypes.split(","):
        model, frames, boxes0, cam = build(dtype, dev)
        first = torch.from_numpy(boxes0)
        model.set_graphs(True)
        trackers = {"reprojected": SequenceTracker(model, first, cam, margin=MARGIN, square=True, device=dev, windows="reprojected"),
                    "joints": SequenceTracker(model, first, cam, margin=MARGIN, square=True, device=dev)}
        moved = {"slots": 0, "reprojected": 0}

        def run(name, n):
            tr = trackers[name]
            tr.reset(first)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = tr.step(frames)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if name == "reprojected":      # (read after the clock stopped: the last step's sources stand for the block)
                moved["slots"] += B * V
                moved["reprojected"] += int((out["source"] == 1).sum())
            return dt

        for name in trackers:
            run(name, a.warmup)
        moved.update(slots=0, reprojected=0)
        ms = {k: [] for k in trackers}
        for _ in range(a.blocks):
            for name in trackers:
                ms[name].append(1000.0 * run(name, a.block) / a.block)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        cached, replays = model.graph_stats()
        rows.append({"B": B, "V": V, "size": SIZE, "frame": [FH, FW], "dtype": dtype, "steps_per_loop": a.blocks * a.block,
                     "ms_per_step_median": {k: round(v, 3) for k, v in med.items()},
                     "extra_ms_per_step": round(med["reprojected"] - med["joints"], 3),
                     "reprojected_over_joints": round(med["reprojected"] / med["joints"], 4),
                     "ms_per_step_blocks": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                     "spread": {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in ms.items()},
                     "graphs_cached": cached, "graph_replays": replays,
                     "source_1_fraction_at_block_ends": round(moved["reprojected"] / max(moved["slots"], 1), 4)})
        del trackers, model
        torch.cuda.empty_cache()
    print(json.dumps({"probe": "reproject_track", "rows": rows}))


if __name__ == "__main__":
    main()
