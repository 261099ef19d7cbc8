#!/usr/bin/env python3
"""Timing record of the evaluation breakdown: steps per second of

  1. on         EpochEvaluator(breakdown=True, records=...).step(batch): the pooled launch and the breakdown launch per step,
                nothing copied to the host; compute() and records() at the end of the timed block;
  2. off        the same loop without the switch -- what the evaluator did before the breakdown existed, the yardstick;
  3. readback   what gives these tables without the breakdown: forward and loss, the predictions copied to the host every step
                (one stream synchronisation), the per-joint / per-camera / per-sample numbers in numpy

on the same device-resident batches of tools/eval_probe.py (ResNet50-paper, 8 views of 256 x 256, loss labels on every batch), at
batch 1 and batch 32, in fp32 and fp16.  tools/eval_probe.py's protocol: the loops alternate in one process in blocks of --block
steps; a block is timed with the host clock from its first enqueue to the end of its last readback; the figure is the median over
blocks of steps / second.  The shader clock is read before and after (rocm-smi, when it is there) and reported as found.

A record, not a gate.    python tools/breakdown_probe.py [--blocks 8] [--block 50] [--warmup 20] [--out profiles/breakdown.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eval_probe import build  # noqa: E402
from handmvnet_amd.evaluation import EpochEvaluator  # noqa: E402

SHAPES = {"b1_v8_256": (8, 1, 256), "b32_v8_256": (8, 32, 256)}   # name: (views, batch, size)
DTYPES = ("f32", "f16")


def clock_level():
    """The current shader clock as rocm-smi prints it, or None."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=20)
        m = re.search(r"sclk clock level:?\s*(\w+):?\s*\((\d+)Mhz\)", r.stdout)
        return {"level": m.group(1), "mhz": int(m.group(2))} if m else None
    except (OSError, subprocess.SubprocessError):
        return None


def numpy_breakdown(pred_cam, gt_cam, pred_2d, gt_2d, mask, thr):
    """The tables from one step's arrays on the host, as a user writes them today: fp32 distances, Procrustes per pose."""
    d3 = np.linalg.norm(pred_cam - gt_cam, axis=-1)                                     # [B, 21]
    mu1, mu2 = pred_cam.mean(1, keepdims=True), gt_cam.mean(1, keepdims=True)
    x1, x2 = (pred_cam - mu1).astype(np.float64), (gt_cam - mu2).astype(np.float64)
    K = x1.transpose(0, 2, 1) @ x2
    U, _, Vh = np.linalg.svd(K)
    Z = np.tile(np.eye(3), (K.shape[0], 1, 1))
    Z[:, 2, 2] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.transpose(0, 2, 1) @ Z @ U.transpose(0, 2, 1)
    scale = np.trace(R @ K, axis1=1, axis2=2) / (x1 ** 2).sum((1, 2))
    dpa = np.linalg.norm(scale[:, None, None] * (x1 @ R.transpose(0, 2, 1)) - x2, axis=-1)
    keep = ~mask[..., None]
    d2 = np.linalg.norm(pred_2d * keep - gt_2d * keep, axis=-1)                         # [B, V, 21]
    hist = np.stack([np.searchsorted(thr, d3[:, j], side="left") for j in range(21)])
    return {"J3": d3.sum(0), "JPA": dpa.sum(0), "H": np.stack([np.bincount(h, minlength=thr.size + 1) for h in hist]),
            "C2": d2.sum(0), "CV": (~mask).sum(0), "rows": np.concatenate([d3.mean(1, keepdims=True), dpa.mean(1, keepdims=True),
                                                                            d2.mean((1, 2))[:, None], d2.mean(2)], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    thr = torch.linspace(0.0, 0.02, 20).numpy()
    rows, clock_before = [], clock_level()
    for name, (V, B, size) in SHAPES.items():
        for dtype in DTYPES:
            model, batch = build(V, B, size, dtype, dev)
            on = EpochEvaluator(model, "test", breakdown=True, records=a.block * B)
            off = EpochEvaluator(model, "test")

            def loop_on(n):
                on.reset()
                for _ in range(n):
                    on.step(batch())
                return on.compute(), on.records()

            def loop_off(n):
                off.reset()
                for _ in range(n):
                    off.step(batch())
                return off.compute()

            def loop_readback(n):
                for _ in range(n):
                    b = batch()
                    data = b["data"]
                    out = model(data["rgb"], data["bboxes"], b["cam_params"])
                    data["joints_cam"] /= 1000
                    data["root_joint"] /= 1000
                    model._calculate_loss(out, data, b["cam_params"], mode="test")
                    host = [t.float().cpu().numpy() for t in (out["joints_cam"], data["joints_cam"], out["joints_crop_img"], data["joints_crop_img"])]
                    numpy_breakdown(*host, data["joints_img_mask"].cpu().numpy(), thr)

            loops = {"on": loop_on, "off": loop_off, "readback": loop_readback}
            for f in loops.values():
                f(a.warmup)
            torch.cuda.synchronize()
            rate = {k: [] for k in loops}
            for _ in range(a.blocks):
                for k, f in loops.items():
                    t0 = time.perf_counter()
                    f(a.block)
                    rate[k].append(a.block / (time.perf_counter() - t0))
            med = {k: float(np.median(v)) for k, v in rate.items()}
            us = {k: 1e6 / v for k, v in med.items()}
            rows.append({"shape": name, "B": B, "V": V, "size": size, "dtype": dtype, "steps_per_loop": a.blocks * a.block,
                         "steps_per_s_median": {k: round(v, 2) for k, v in med.items()},
                         "us_per_step_median": {k: round(v, 1) for k, v in us.items()},
                         "on_minus_off_us": round(us["on"] - us["off"], 1), "readback_minus_off_us": round(us["readback"] - us["off"], 1),
                         "steps_per_s_blocks": {k: [round(x, 1) for x in v] for k, v in rate.items()}})
            print(json.dumps(rows[-1]), flush=True)
            del model, on, off
    record = {"probe": "eval_breakdown", "clock_before": clock_before, "clock_after": clock_level(), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
