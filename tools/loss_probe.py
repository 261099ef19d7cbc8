#!/usr/bin/env python3
"""Timing record of the evaluation-step loss at the benchmarked shape (B=32, V=8, 32x32 heat maps from 256-pixel crops):

  1. torch     the five terms composed from torch ops on the device, the reprojection as a loop over batch x views with one
               torch.inverse per turn -- what a user of the reference's functions would run today;
  2. tensor    hmv_pose_losses with a target tensor;
  3. synth     hmv_pose_losses with the targets synthesised from the label joints.

Device events around each block of iterations, the three variants alternating within the one process; prints one JSON line.
A record, not a gate.    python tools/loss_probe.py [--rounds 5] [--iters 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from handmvnet_amd.losses import pose_losses, target_heatmaps  # noqa: E402

W = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}


def make_inputs(B, V, S, hs, dev):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    extr = torch.eye(4).repeat(B, V, 1, 1)
    for b in range(B):
        for i in range(V):   # cameras on a ring around the hand, looking at it
            ang = 2 * np.pi * i / V
            pos = torch.tensor([0.8 * np.cos(ang), 0.8 * np.sin(ang), 0.1], dtype=torch.float32)
            z = -pos / pos.norm()
            x = torch.linalg.cross(z, torch.tensor([0.0, 0.0, 1.0]))
            x = x / x.norm()
            extr[b, i, :3, 0], extr[b, i, :3, 1], extr[b, i, :3, 2], extr[b, i, :3, 3] = x, torch.linalg.cross(z, x), z, pos
    d = dict(extr=extr, intr=torch.tensor([600.0, 600.0, 320.0, 240.0]).repeat(B, V, 1), gt_2d=r(B, V, 21, 2) * S,
             gt_cam=(r(B, 21, 3) - 0.5) * 0.1, root=torch.tensor([0.0, 0.0, 0.8]).repeat(B, 1, 1), mask=r(B, V, 21) < 0.2,
             bbox=torch.tensor([220.0, 140.0, 420.0, 340.0]).repeat(B, V, 1))
    d["pred_2d"] = d["gt_2d"] + (r(B, V, 21, 2) - 0.5) * 4
    d["pred_cam"] = d["gt_cam"] + (r(B, 21, 3) - 0.5) * 0.01
    d = {k: v.to(dev) for k, v in d.items()}
    d["target"] = target_heatmaps(d["gt_2d"], S, hs)
    d["pred_hm"] = 0.8 * d["target"] + 0.05 * (torch.rand(d["target"].shape, device=dev) - 0.5)
    return d


def torch_losses(d, V):
    """Variant 1: torch ops only."""
    keep = (~d["mask"]).unsqueeze(-1)
    terms = [torch.nn.functional.mse_loss(d["pred_hm"], d["target"]) * W["heatmap"],
             torch.nn.functional.l1_loss(d["pred_2d"] * keep, d["gt_2d"] * keep) * W["joints_2d"],
             torch.nn.functional.l1_loss(d["pred_cam"], d["gt_cam"]) * W["joints_3d"]]
    joints = d["pred_cam"] + d["root"]
    B = joints.shape[0]
    proj = torch.zeros(B, V, 21, 2, device=joints.device)
    ones = torch.ones(21, 1, device=joints.device)
    for i in range(V):
        for b in range(B):
            world = d["extr"][b, 0] @ torch.cat((joints[b], ones), dim=1).T
            cam = (torch.inverse(d["extr"][b, i]) @ world).T[:, :3] * 1000
            z = cam[:, 2] + 1e-6
            k = d["intr"][b, i]
            proj[b, i] = torch.stack((cam[:, 0] * k[0] / z + k[2], cam[:, 1] * k[1] / z + k[3]), dim=1)
    bb = d["bbox"]
    proj = (proj - bb[:, :, None, :2]) * (256.0 / (bb[:, :, None, 2:] - bb[:, :, None, :2]))
    terms += [torch.nn.functional.l1_loss(proj, d["gt_2d"]) * W["g2d"], torch.nn.functional.l1_loss(proj, d["pred_2d"]) * W["p2d"]]
    return sum(terms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    B, V, S, hs = 32, 8, 256, 32
    dev = torch.device("cuda:0")
    d = make_inputs(B, V, S, hs, dev)
    common = dict(weights=W, joints_mask=d["mask"], mask_invisible_joints=True, root_joint=d["root"], root_idx=0, intrinsic=d["intr"],
                  extrinsic=d["extr"], bbox=d["bbox"])
    args = (d["pred_hm"], d["pred_2d"], d["pred_cam"], d["gt_2d"], d["gt_cam"])
    variants = {"torch": lambda: torch_losses(d, V), "tensor": lambda: pose_losses(*args, target_heatmap=d["target"], **common)[0][5],
                "synth": lambda: pose_losses(*args, image_size=S, sigma=2, **common)[0][5]}
    values = {k: float(f()) for k, f in variants.items()}
    for f in variants.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.iters)
    hm_bytes = d["pred_hm"].numel() * 4
    small = sum(d[k].numel() * d[k].element_size() for k in ("pred_2d", "gt_2d", "pred_cam", "gt_cam", "root", "mask", "intr", "extr", "bbox"))
    print(json.dumps({"shape": {"B": B, "V": V, "heatmap": hs, "image_size": S}, "iters_per_variant": a.rounds * a.iters,
                      "loss": values,
                      "ms_per_call_median": {k: float(np.median(v)) for k, v in ms.items()},
                      "ms_per_call_rounds": {k: [round(x, 5) for x in v] for k, v in ms.items()},
                      "bytes_read": {"torch": 2 * hm_bytes + small, "tensor": 2 * hm_bytes + small, "synth": hm_bytes + small}}))


if __name__ == "__main__":
    main()
