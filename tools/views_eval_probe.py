#!/usr/bin/env python3
"""Timing record of an evaluation epoch over a RAGGED split: milliseconds per step of HandMvNet.evaluate

  (a) ragged    on batches that carry batch["view_mask"]: forward_views on the present frames, the ragged loss
                (hmv_pose_losses_views) and the ragged accumulation (hmv_eval_add_views);
  (b) blacked   on the same batches without the mask and with the absent views blacked out (zero images): the only way a caller had
                before -- forward on every frame, the uniform loss and accumulation (whose numbers the black frames pollute)

at the benchmarked shape, batch 32 x 8 views of 256 x 256 on ResNet50-paper, in fp32 and in fp16, every sample keeping 4 random views.
Every batch carries loss labels; the heat-map targets are rebuilt in the loss kernel from the label joints.

Both loops run in the one process in alternating blocks of --block steps; a block is one evaluate() call over `block` batches, timed
with the host clock from its first enqueue to the end of compute()'s readback; the figure is the median over blocks.  Both loops
clone the millimetre labels per step (the step converts them to metres in place).

A record, not a gate.    python tools/views_eval_probe.py [--blocks 5] [--block 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from handmvnet_amd import HandMvNet  # noqa: E402
from handmvnet_amd.spec import config_from_params  # noqa: E402
from handmvnet_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

V, B, SIZE, KEEP = 8, 32, 256, 4
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}


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
    x, bbox, intr = synth_inputs(cfg, B, 1000, SIZE)
    rng = np.random.default_rng(5)
    mask = np.zeros((B, V), bool)
    for b in range(B):
        mask[b, rng.choice(V, KEEP, replace=False)] = True
    xt, bt, it = (torch.from_numpy(a).to(dev) for a in (x, bbox, intr))
    black = xt * torch.from_numpy(mask).to(dev).view(B, V, 1, 1, 1)      # the absent views as zero images
    view_mask = torch.from_numpy(mask)                                   # on the host, where forward_views reads it
    model.reserve(B, SIZE, SIZE, dev)
    out = model.forward_views(xt, view_mask, bt, {"intrinsic": it})
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
              "gt_crop": (out["joints_crop_img"] + torch.randn(B, V, 21, 2, generator=g).to(dev) * 2).clamp(-5, SIZE + 5),
              "mask": (torch.rand(B, V, 21, generator=g) < 0.2).to(dev)}
    cam = {"intrinsic": it, "extrinsic": extr.to(dev)}

    def batch(ragged):
        b = {"data": {"rgb": xt if ragged else black, "bboxes": bt, "joints_cam": labels["gt_cam_mm"].clone(),
                      "root_joint": labels["root_mm"].clone(), "joints_crop_img": labels["gt_crop"], "joints_img_mask": labels["mask"],
                      "root_idx": 0}, "cam_params": cam}
        if ragged:
            b["view_mask"] = view_mask
        return b
    return model, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="f32,f16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for dtype in a.dtypes.split(","):
        model, batch = build(dtype, dev)
        loops = {"ragged": lambda n: model.evaluate((batch(True) for _ in range(n))),
                 "blacked": lambda n: model.evaluate((batch(False) for _ in range(n)))}
        numbers = {k: f(a.warmup) for k, f in loops.items()}
        torch.cuda.synchronize()
        ms = {k: [] for k in loops}
        for _ in range(a.blocks):
            for k, f in loops.items():
                t0 = time.perf_counter()
                f(a.block)
                ms[k].append(1000.0 * (time.perf_counter() - t0) / a.block)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rows.append({"B": B, "V": V, "size": SIZE, "kept_views": KEEP, "dtype": dtype, "steps_per_loop": a.blocks * a.block,
                     "ms_per_step_median": {k: round(v, 3) for k, v in med.items()},
                     "ragged_over_blacked": round(med["ragged"] / med["blacked"], 4),
                     "ms_per_step_blocks": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                     "spread": {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in ms.items()},
                     "test_mpjpe2d": {k: round(numbers[k]["test_mpjpe2d"], 4) for k in loops},
                     "test/loss": {k: round(numbers[k]["test/loss"], 4) for k in loops}})
        del model
    print(json.dumps({"probe": "views_eval", "rows": rows}))


if __name__ == "__main__":
    main()
