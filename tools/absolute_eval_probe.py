#!/usr/bin/env python3
"""Timing record of the absolute evaluation: steps per second of

  1. epoch   HandMvNet.evaluate(batches, absolute=True): per step forward_absolute, the loss, the pooled accumulation launch and
             hmv_eval_absolute_add, nothing copied to the host per step; one readback at the end;
  2. steps   the loop a user writes without it: test_step with absolute_root = "triangulate" per batch and a float() of
             test_w_mpjpe and test_root_err per step

on the device-resident batches of tools/eval_probe.py (ResNet50-paper, 8 views of 256 x 256, loss labels on every batch), at batch 1
and batch 32, in fp32 and fp16.  tools/breakdown_probe.py's protocol: the loops alternate in one process in blocks of --block steps; a
block is timed with the host clock from its first enqueue to the end of its last readback; the figure is the median over blocks of
steps / second.  The shader clock is read before and after (rocm-smi, when it is there) and reported as found.

A record, not a gate.    python tools/absolute_eval_probe.py [--blocks 8] [--block 50] [--warmup 20] [--out profiles/absolute_eval.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from breakdown_probe import DTYPES, SHAPES, clock_level  # noqa: E402
from eval_probe import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="profiles/absolute_eval.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, clock_before = [], clock_level()
    for name, (V, B, size) in SHAPES.items():
        for dtype in DTYPES:
            model, plain_batch = build(V, B, size, dtype, dev)

            def batch():
                b = plain_batch()
                b["data"]["root_joint"] = b["data"]["root_joint"].reshape(B, 1, 3)   # the reference's layout, what test_step compares with
                return b

            last = {}

            def loop_epoch(n):
                last["epoch"] = model.evaluate((batch() for _ in range(n)), absolute=True)

            def loop_steps(n):
                model.absolute_root = "triangulate"
                try:
                    for _ in range(n):
                        m = model.test_step(batch())["metrics"]
                        last["steps"] = (float(m["test_w_mpjpe"]), float(m["test_root_err"]))
                finally:
                    model.absolute_root = None

            loops = {"epoch": loop_epoch, "steps": loop_steps}
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
                         "epoch_minus_steps_us": round(us["epoch"] - us["steps"], 1),
                         "located": last["epoch"]["located"], "lost": last["epoch"]["lost"],
                         "w_mpjpe": {"epoch": last["epoch"]["test_w_mpjpe"], "last_step": last["steps"][0]},
                         "steps_per_s_blocks": {k: [round(x, 1) for x in v] for k, v in rate.items()}})
            print(json.dumps(rows[-1]), flush=True)
            del model
    record = {"probe": "absolute_eval", "clock_before": clock_before, "clock_after": clock_level(), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
