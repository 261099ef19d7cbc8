#!/usr/bin/env python3
"""Timing record of evaluating a followed sequence: time steps per second of

  (a) evaluator  SequenceEvaluator.step: the tracker's step, the labels into its windows on the device (hmv_op_labels_to_windows),
                 EpochEvaluator.add and one hmv_seq_eval_add; nothing reaches the host until compute();
  (b) host       the loop a caller writes today from the public pieces: tracker.step, crop_boxes_used to the host (.cpu()), the labels
                 mapped in numpy (tests/seq_eval_oracle.py), upload, EpochEvaluator.add -- and no jitter, which nothing computed

on ResNet50-paper at 256 x 256, batch 1 x 8 views (the eval_fps shape), fp16 by default, synthetic 480 x 640 frames and labels resident
on the device (the same at every step), hipGraph replay on for the tracker's step in both loops, model.heatmap_targets = "joints" so
that both loops compute the loss terms.  Every block starts from the same first windows.

Both loops run in the one process in alternating blocks of --block steps after --warmup steps of each; a block is timed with the host
clock from its first enqueue to the end of compute()'s readback; the figure is the median over blocks.  The device's name, its
maximum engine clock and, where the driver shows it, the engine clock level in use before and after are part of the record.

A record, not a gate.    python tools/seq_eval_probe.py [--blocks 5] [--block 40] [--warmup 10] [--dtypes f16]
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seq_eval_oracle  # noqa: E402
from handmvnet_amd import HandMvNet, SequenceEvaluator, SequenceTracker  # noqa: E402
from handmvnet_amd.evaluation import EpochEvaluator  # noqa: E402
from handmvnet_amd.spec import config_from_params  # noqa: E402
from handmvnet_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

B, V, SIZE, FH, FW, MARGIN = 1, 8, 256, 480, 640, 20
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0}


def engine_clock():
    """The engine clock level in use, as the driver shows it (read only); None where it does not."""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            active = [ln.strip() for ln in open(path) if ln.rstrip().endswith("*")]
        except OSError:
            continue
        if active:
            return active[0]
    return None


def build(dtype, dev):
    tp = {"debug": False, "root_relative": True, "loss_weights": WEIGHTS, "mask_invisible_joints": True}
    mp = {"num_views": V, "backbone": "resnet", "backbone_type": "50_paper", "backbone_channels": [1024], "backbone_pretrained": False,
          "backbone_early_return": 3, "pos_enc": ["pos2d", "crop", "sin"], "fusion": "cross_attn", "fusion_layers": 5, "use_gcn": True}
    dp = {"batch_size": B, "image_size": SIZE, "heatmap_size": SIZE // 8, "name": "dexycb"}
    cfg = config_from_params(tp, mp, dp)
    model = HandMvNet(tp, mp, dp)
    model.load_state_dict(synth_state_dict(cfg, 1), strict=True)
    model.to(dev).eval()
    if dtype == "f16":
        model.half()
    model.heatmap_targets = "joints"
    model.reserve(B, SIZE, SIZE, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    frames = torch.randint(0, 256, (B, V, FH // 8, FW // 8, 3), dtype=torch.uint8, device=dev, generator=g)
    frames = frames.repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()       # blocky content: not flat, not white noise
    rng = np.random.default_rng(5)
    side = rng.integers(150, 260, (B, V))
    x1, y1 = rng.integers(0, FW - 150, (B, V)), rng.integers(0, FH - 150, (B, V))
    boxes0 = np.stack([x1, y1, x1 + side, y1 + side], -1).astype(np.int32)
    intr = torch.from_numpy(synth_inputs(cfg, B, 1000, SIZE)[2]).to(dev)
    joints_img = (boxes0[:, :, None, :2] + rng.uniform(0, 1, (B, V, 21, 2)) * side[:, :, None, None]).astype(np.float32)
    labels = {"joints_img": joints_img, "joints_cam": (rng.standard_normal((B, 21, 3)) * 40).astype(np.float32),
              "joints_img_mask": rng.random((B, V, 21)) < 0.2}
    return model, frames, boxes0, {"intrinsic": intr}, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtypes", default="f16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(dev)
    record = {"probe": "seq_eval", "device": props.name, "max_engine_clock_mhz": getattr(props, "clock_rate", 0) / 1000,
              "engine_clock_before": engine_clock(), "rows": []}
    for dtype in a.dtypes.split(","):
        model, frames, boxes0, cam, labels = build(dtype, dev)
        first = torch.from_numpy(boxes0)
        on_dev = {k: torch.from_numpy(v).to(dev) for k, v in labels.items()}
        model.set_graphs(True)
        tracker = SequenceTracker(model, first, cam, margin=MARGIN, square=True, device=dev)
        evaluator = SequenceEvaluator(tracker, cam)
        last = {}

        def run_evaluator(n):
            evaluator.reset()
            evaluator.restart(first)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                evaluator.step(frames, on_dev)
            last["evaluator"] = evaluator.compute()
            return time.perf_counter() - t0

        def run_host(n):
            tracker.reset(first)
            epoch = EpochEvaluator(model, "test")
            gt_m = on_dev["joints_cam"] / 1000
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = tracker.step(frames)
                used = out["crop_boxes_used"].cpu().numpy()
                crop, hidden, _ = seq_eval_oracle.labels_to_windows(labels["joints_img"].reshape(-1, 21, 2), used.reshape(-1, 4), SIZE,
                                                                    labels["joints_img_mask"].reshape(-1, 21))
                inputs = {"joints_crop_img": torch.from_numpy(crop.reshape(B, V, 21, 2)).to(dev), "joints_cam": gt_m,
                          "joints_img_mask": torch.from_numpy(hidden.reshape(B, V, 21)).to(dev),
                          "bboxes": torch.from_numpy(used.astype(np.float32)).to(dev)}
                epoch.add(out, inputs, cam)
            last["host"] = epoch.compute()
            return time.perf_counter() - t0

        loops = {"evaluator": run_evaluator, "host": run_host}
        for f in loops.values():
            f(a.warmup)
        sec = {k: [] for k in loops}
        for _ in range(a.blocks):
            for k, f in loops.items():
                sec[k].append(f(a.block) / a.block)
        rate = {k: 1.0 / float(np.median(v)) for k, v in sec.items()}
        same = all(last["evaluator"][k] == v for k, v in last["host"].items())
        record["rows"].append({"B": B, "V": V, "size": SIZE, "frame": [FH, FW], "dtype": dtype, "steps_per_loop": a.blocks * a.block,
                               "steps_per_s_median": {k: round(v, 1) for k, v in rate.items()},
                               "evaluator_over_host": round(rate["evaluator"] / rate["host"], 4),
                               "ms_per_step_blocks": {k: [round(1000 * x, 3) for x in v] for k, v in sec.items()},
                               "spread": {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in sec.items()},
                               "same_epoch_numbers": bool(same), "test_mka": last["evaluator"]["test_mka"],
                               "labels_outside_window": last["evaluator"]["labels_outside_window"]})
        del evaluator, tracker, model
        torch.cuda.empty_cache()
    record["engine_clock_after"] = engine_clock()
    print(json.dumps(record))


if __name__ == "__main__":
    main()
