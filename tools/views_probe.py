#!/usr/bin/env python3
"""Timing record: what does a ragged batch cost against the same batch padded with black views?

Workload: the benchmarked shape (BASELINE configs[2]: r50-paper, B = 32, 8 views, 256 x 256), every sample keeping 4 random views.

  1. views    forward_views(x, mask): the backbone runs on the 128 present frames, the fusion over 84 tokens per sample;
  2. padded   forward(x with the absent views blacked out): what the reference's data loader does (datasets/ho3d.py:138-140) --
              256 backbone passes and 168 tokens per sample, 84 of them junk.

Device events around each block of iterations, the two variants alternating within the one process; prints one JSON line.
A record, not a gate.    python tools/views_probe.py [--rounds 5] [--iters 10] [--warmup 3] [--dtype f32] [--keep 4]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from handmvnet_amd import HandMvNet  # noqa: E402
from handmvnet_amd.synth import synth_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16", "f32x3"])
    ap.add_argument("--keep", type=int, default=4, help="present views per sample")
    args = ap.parse_args()
    B, V, S = 32, 8, 256
    tp = {"debug": False, "root_relative": True}
    mp = {"num_views": V, "backbone": "resnet", "backbone_type": "50_paper", "backbone_channels": [1024], "backbone_pretrained": False,
          "backbone_early_return": 3, "pos_enc": ["pos2d", "crop", "sin"], "fusion": "cross_attn", "fusion_layers": 5, "use_gcn": True}
    dp = {"batch_size": B, "image_size": S, "heatmap_size": S // 8, "name": "dexycb"}
    m = HandMvNet(tp, mp, dp).to("cuda").eval()
    if args.dtype == "f16":
        m.half()
    elif args.dtype == "f32x3":
        m.float32x3()
    dev = torch.device("cuda:0")
    x, bbox, intr = (torch.from_numpy(a).to(dev) for a in synth_inputs(m.cfg, B, 7, S))
    rng = np.random.Generator(np.random.PCG64(11))
    mask = np.zeros((B, V), dtype=bool)
    for b in range(B):
        mask[b, rng.choice(V, args.keep, replace=False)] = True
    black = x * torch.from_numpy(mask).to(dev)[:, :, None, None, None]
    cam = {"intrinsic": intr}
    variants = {"views": lambda: m.forward_views(x, mask, bbox, cam), "padded": lambda: m(black, bbox, cam)}
    for f in variants.values():
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.iters)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps({"probe": "views", "dtype": args.dtype, "B": B, "V": V, "size": S, "present_views_per_sample": args.keep,
                      "views_ms": round(med["views"], 3), "padded_ms": round(med["padded"], 3),
                      "ratio_views_over_padded": round(med["views"] / med["padded"], 4),
                      "rounds_ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
