#!/usr/bin/env python3
"""Timing record of an evaluation epoch: steps per second of

  1. test_step   the loop a user writes around HandMvNet.test_step(batch): every step ends in a device->host copy of the metrics
                 (PoseMetrics.all_metrics), i.e. one stream synchronisation per step;
  2. evaluator   EpochEvaluator.step(batch): forward, loss and one accumulation launch per step, nothing copied to the host, one
                 readback (compute()) at the end of the timed block

on the same device-resident batches, at batch 1 x 8 views of 256 x 256 on ResNet50-paper in fp16 and in fp32 (the shape the
reference's eval_fps.py times) and at cfg1 (batch 1 x 4 views of 128 x 128, fp32).  Every batch carries loss labels; the heat-map
targets are rebuilt in the loss kernel from the label joints (heatmap_targets = "joints").

Both loops run in the one process in alternating blocks of --block steps; a block is timed with the host clock from its first
enqueue to the end of a stream synchronisation (loop 2: after compute()'s readback), and the figure is the median over blocks of
steps / second.  Both loops clone the millimetre labels per step (the step converts them to metres in place): one small copy
kernel on either side.  Launches per step: the engine's own count (model.launch_count()) plus the launches of the evaluation
tail's library entries (hmv_pose_losses: 2, hmv_pose_metrics: 1 per call, hmv_eval_add: 1), counted by wrapping the entries for one
step; the small torch kernels around them (label conversion, mask) are not counted.

A record, not a gate.    python tools/eval_probe.py [--blocks 8] [--block 50] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from handmvnet_amd import HandMvNet, _lib  # noqa: E402
from handmvnet_amd.evaluation import EpochEvaluator  # noqa: E402
from handmvnet_amd.spec import config_from_params  # noqa: E402
from handmvnet_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

SHAPES = {   # name: (views, batch, size, dtypes)
    "b1_v8_256": (8, 1, 256, ("f16", "f32")),
    "cfg1": (4, 1, 128, ("f32",)),
}
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}
TAIL_LAUNCHES = {"hmv_pose_losses": 2, "hmv_pose_metrics": 1, "hmv_eval_add": 1}


def build(V, B, size, dtype, dev):
    tp = {"debug": False, "root_relative": True, "loss_weights": WEIGHTS, "mask_invisible_joints": True}
    mp = {"num_views": V, "backbone": "resnet", "backbone_type": "50_paper", "backbone_channels": [1024], "backbone_pretrained": False,
          "backbone_early_return": 3, "pos_enc": ["pos2d", "crop", "sin"], "fusion": "cross_attn", "fusion_layers": 5, "use_gcn": True}
    dp = {"batch_size": B, "image_size": size, "heatmap_size": size // 8, "name": "dexycb"}
    cfg = config_from_params(tp, mp, dp)
    model = HandMvNet(tp, mp, dp)
    model.load_state_dict(synth_state_dict(cfg, 1), strict=True)
    model.to(dev).eval()
    if dtype == "f16":
        model.half()
    model.heatmap_targets = "joints"
    x, bbox, intr = synth_inputs(cfg, B, 1000, size)
    xt, bt, it = (torch.from_numpy(a).to(dev) for a in (x, bbox, intr))
    model.reserve(B, size, size, dev)
    out = model(xt, bt, {"intrinsic": it})
    g = torch.Generator().manual_seed(3)
    extr = torch.eye(4).repeat(B, V, 1, 1)
    for i in range(V):   # cameras on a ring around the hand, looking at it (tools/loss_probe.py)
        ang = 2 * np.pi * i / V
        pos = torch.tensor([0.8 * np.cos(ang), 0.8 * np.sin(ang), 0.1], dtype=torch.float32)
        z = -pos / pos.norm()
        xa = torch.linalg.cross(z, torch.tensor([0.0, 0.0, 1.0]))
        xa = xa / xa.norm()
        extr[:, i, :3, 0], extr[:, i, :3, 1], extr[:, i, :3, 2], extr[:, i, :3, 3] = xa, torch.linalg.cross(z, xa), z, pos
    labels = {"gt_cam_mm": (out["joints_cam"] + torch.randn(B, 21, 3, generator=g).to(dev) * 0.006) * 1000,
              "root_mm": torch.tensor([0.0, 0.0, 800.0]).repeat(B, 1).to(dev),
              "gt_crop": (out["joints_crop_img"] + torch.randn(B, V, 21, 2, generator=g).to(dev) * 2).clamp(-5, size + 5),
              "mask": (torch.rand(B, V, 21, generator=g) < 0.2).to(dev)}
    cam = {"intrinsic": it, "extrinsic": extr.to(dev)}

    def batch():
        return {"data": {"rgb": xt, "bboxes": bt, "joints_cam": labels["gt_cam_mm"].clone(), "root_joint": labels["root_mm"].clone(),
                         "joints_crop_img": labels["gt_crop"], "joints_img_mask": labels["mask"], "root_idx": 0}, "cam_params": cam}
    return model, batch


def count_tail_launches(fn):
    """Launches of the evaluation tail's library entries during one call of fn()."""
    lib, n = _lib.load(), {"launches": 0}
    real = {name: getattr(lib, name) for name in TAIL_LAUNCHES}

    def wrap(name):
        def f(*a):
            n["launches"] += TAIL_LAUNCHES[name]
            return real[name](*a)
        return f
    try:
        for name in TAIL_LAUNCHES:
            setattr(lib, name, wrap(name))
        fn()
    finally:
        for name, f in real.items():
            setattr(lib, name, f)
    return n["launches"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if a.blocks * a.block < 200:
        ap.error("the record is the median over at least 200 steps per loop")
    dev = torch.device("cuda:0")
    rows = []
    for name, (V, B, size, dtypes) in SHAPES.items():
        for dtype in dtypes:
            model, batch = build(V, B, size, dtype, dev)
            ev = EpochEvaluator(model, "test")

            def loop_test_step(n):
                for _ in range(n):
                    model.test_step(batch(), 0)
                torch.cuda.synchronize()

            def loop_evaluator(n):
                ev.reset()
                for _ in range(n):
                    ev.step(batch())
                return ev.compute()

            loops = {"test_step": loop_test_step, "evaluator": loop_evaluator}
            for f in loops.values():
                f(a.warmup)
            torch.cuda.synchronize()
            rate = {k: [] for k in loops}
            for _ in range(a.blocks):
                for k, f in loops.items():
                    t0 = time.perf_counter()
                    f(a.block)
                    rate[k].append(a.block / (time.perf_counter() - t0))
            launches = {"test_step": count_tail_launches(lambda: model.test_step(batch(), 0)),
                        "evaluator": count_tail_launches(lambda: ev.step(batch()))}
            torch.cuda.synchronize()
            engine = model.launch_count()
            med = {k: float(np.median(v)) for k, v in rate.items()}
            rows.append({"shape": name, "B": B, "V": V, "size": size, "dtype": dtype, "steps_per_loop": a.blocks * a.block,
                         "steps_per_s_median": {k: round(v, 2) for k, v in med.items()},
                         "ms_per_step_median": {k: round(1000.0 / v, 4) for k, v in med.items()},
                         "evaluator_over_test_step": round(med["evaluator"] / med["test_step"], 4),
                         "steps_per_s_blocks": {k: [round(x, 1) for x in v] for k, v in rate.items()},
                         "launches_per_step": {"engine": engine, "tail_test_step": launches["test_step"], "tail_evaluator": launches["evaluator"]},
                         "host_readbacks_per_step": {"test_step": 1, "evaluator": 0}})
            del model, ev
    print(json.dumps({"probe": "eval_epoch", "rows": rows}))


if __name__ == "__main__":
    main()
