#!/usr/bin/env python3
"""Timing record of a sequence whose crop windows follow the hand: milliseconds per time step of

  (a) tracker   SequenceTracker.step with hipGraph replay on: the frames are copied into the tracker's staging buffer, then ONE call
                (hmv_forward_frames_track) runs the forward and moves the windows on the device;
  (b) host      what a caller had before: forward_frames, joints_crop_img to the host (.cpu()), the windows in numpy
                (tests/track_oracle.py: batch_cropped_joints_to_joints_img + points2d_to_bbox per slot), the new windows uploaded

on ResNet50-paper at 256 x 256, 8 views, batch 1 and batch 32, fp32 and fp16, synthetic 480 x 640 frames resident on the device (the
same frames at every step).  Every block starts from the same first windows, so both loops walk the same window trajectory.

Both loops run in the one process in alternating blocks of --block steps; a block is timed with the host clock from its first enqueue
to a device synchronisation behind its last step; the figure is the median over blocks.

A record, not a gate.    python tools/track_probe.py [--blocks 5] [--block 20] [--warmup 3]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import track_oracle  # noqa: E402
from handmvnet_amd import HandMvNet, SequenceTracker  # noqa: E402
from handmvnet_amd.spec import config_from_params  # noqa: E402
from handmvnet_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

V, SIZE, FH, FW, MARGIN = 8, 256, 480, 640, 20


def build(dtype, B, dev):
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
    rng = np.random.default_rng(5)
    side = rng.integers(150, 260, (B, V))
    x1, y1 = rng.integers(0, FW - 150, (B, V)), rng.integers(0, FH - 150, (B, V))
    boxes0 = np.stack([x1, y1, x1 + side, y1 + side], -1).astype(np.int32)
    intr = torch.from_numpy(synth_inputs(cfg, B, 1000, SIZE)[2]).to(dev)
    return model, cfg, frames, boxes0, {"intrinsic": intr}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--batches", default="1,32")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for dtype in a.dtypes.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            model, cfg, frames, boxes0, cam = build(dtype, B, dev)
            first = torch.from_numpy(boxes0)
            model.set_graphs(True)
            tracker = SequenceTracker(model, first, cam, margin=MARGIN, square=True, device=dev)
            last = {}

            def run_tracker(n):
                tracker.reset(first)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    tracker.step(frames)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                last["tracker"] = tracker.crop_boxes.cpu().numpy().copy()
                return dt

            def run_host(n):
                boxes = boxes0.copy()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    out = model.forward_frames(frames, torch.from_numpy(boxes).to(dev), cam)
                    jc = out["joints_crop_img"].cpu().numpy()
                    boxes = track_oracle.next_crop_boxes(jc.reshape(-1, 21, 2), boxes.reshape(-1, 4), SIZE, MARGIN, True)[0].reshape(B, V, 4)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                last["host"] = boxes
                return dt

            loops = {"tracker": run_tracker, "host": run_host}
            for f in loops.values():
                f(a.warmup)
            ms = {k: [] for k in loops}
            for _ in range(a.blocks):
                for k, f in loops.items():
                    ms[k].append(1000.0 * f(a.block) / a.block)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            cached, replays = model.graph_stats()
            rows.append({"B": B, "V": V, "size": SIZE, "frame": [FH, FW], "dtype": dtype, "steps_per_loop": a.blocks * a.block,
                         "ms_per_step_median": {k: round(v, 3) for k, v in med.items()},
                         "tracker_over_host": round(med["tracker"] / med["host"], 4),
                         "ms_per_step_blocks": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                         "spread": {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in ms.items()},
                         "graphs_cached": cached, "graph_replays": replays,
                         "same_windows_after_block": bool((last["tracker"] == last["host"]).all())})
            del tracker, model
            torch.cuda.empty_cache()
    print(json.dumps({"probe": "track", "rows": rows}))


if __name__ == "__main__":
    main()
