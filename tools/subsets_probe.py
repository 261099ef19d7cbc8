#!/usr/bin/env python3
"""Timing record of a camera-subset sweep: all 70 subsets of 4 of the 8 cameras at the benchmarked shape (batch 32 x 8 views of
256 x 256 on ResNet50-paper, labels with the heat-map targets rebuilt in the loss kernel), in fp32 and in fp16.

  (a) sweep   HandMvNet.evaluate_subsets: per step one backbone pass and 70 fusion tails;
  (b) loop    what a caller had before: one HandMvNet.evaluate per subset over the same batches, each carrying that subset's mask.

Both run in the one process in alternating blocks; a block is the whole sweep over --block batches, timed with the host clock from
its first enqueue to the end of the (last) readback; the figure is the median over --blocks blocks, the spread (max - min) / median
over the blocks.  The condition: (a) is faster than (b) by more than the larger spread of the two.  Also recorded: (a)'s split into
the per-frame stage and the tails (the bracketing profiling records of one profiled step), and (a) with ONE subset against a plain
ragged evaluate with that mask -- what retaining and expanding the rows costs when there is nothing to share.

Each dtype runs in a child process of its own under a time limit (--limit seconds, sized to the (b) loop); the first failure ends
the probe.    python tools/subsets_probe.py [--blocks 5] [--block 2] [--warmup 1] [--out profiles/subsets_sweep.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, B, SIZE, KEEP = 8, 32, 256, 4
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}


def build(dtype, dev):
    import torch
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.spec import config_from_params
    from handmvnet_amd.synth import synth_inputs, synth_state_dict
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
    xt, bt, it = (torch.from_numpy(a).to(dev) for a in (x, bbox, intr))
    model.reserve(B, SIZE, SIZE, dev)
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
              "gt_crop": (out["joints_crop_img"] + torch.randn(B, V, 21, 2, generator=g).to(dev) * 2).clamp(-5, SIZE + 5),
              "mask": (torch.rand(B, V, 21, generator=g) < 0.2).to(dev)}
    cam = {"intrinsic": it, "extrinsic": extr.to(dev)}

    def batch(view_mask=None):
        b = {"data": {"rgb": xt, "bboxes": bt, "joints_cam": labels["gt_cam_mm"].clone(), "root_joint": labels["root_mm"].clone(),
                      "joints_crop_img": labels["gt_crop"], "joints_img_mask": labels["mask"], "root_idx": 0}, "cam_params": cam}
        if view_mask is not None:
            b["view_mask"] = view_mask
        return b
    return model, batch, (xt, bt, it)


def one(dtype, a):
    import torch
    from handmvnet_amd.subsets import as_subset_table, k_of_n
    dev = torch.device("cuda:0")
    model, batch, (xt, bt, it) = build(dtype, dev)
    subsets = k_of_n(V, KEEP)
    masks = [torch.from_numpy(np.broadcast_to(row.astype(bool), (B, V)).copy()) for row in as_subset_table(subsets, V)]   # on the host

    def sweep(subs, n):
        return model.evaluate_subsets((batch() for _ in range(n)), subs)

    def loop(ms, n):
        return [model.evaluate(batch(m) for _ in range(n)) for m in ms]

    def timed(loops):
        for f in loops.values():
            f(a.warmup)
        torch.cuda.synchronize()
        ms = {k: [] for k in loops}
        for _ in range(a.blocks):
            for k, f in loops.items():
                t0 = time.perf_counter()
                f(a.block)
                ms[k].append(1000.0 * (time.perf_counter() - t0) / a.block)
        return {k: {"ms_per_step_median": round(float(np.median(v)), 3), "ms_per_step_blocks": [round(x, 3) for x in v],
                    "spread": round((max(v) - min(v)) / float(np.median(v)), 4)} for k, v in ms.items()}

    numbers = sweep(subsets, 1)
    ref = loop(masks[:2], 1)
    same = all(numbers["per_subset"][s] == ref[s] for s in range(2))      # (the test suite pins this; the record says so too)
    full = timed({"sweep": lambda n: sweep(subsets, n), "loop": lambda n: loop(masks, n)})
    single = timed({"sweep_S1": lambda n: sweep(subsets[:1], n), "ragged_evaluate": lambda n: loop(masks[:1], n)})
    # (a)'s split: the bracketing records of one profiled step
    model.set_profiling(True)
    model.forward_subsets(xt, subsets, bt, {"intrinsic": it})
    torch.cuda.synchronize()
    recs = model.profile_records()
    model.set_profiling(False)
    frames_ms = sum(r["ms"] for r in recs if r["kernel"] == "subsets_frames")
    tails = [r["ms"] for r in recs if r["kernel"] == "subsets_tail"]
    a_ms, b_ms = full["sweep"]["ms_per_step_median"], full["loop"]["ms_per_step_median"]
    spread = max(full["sweep"]["spread"], full["loop"]["spread"])
    return {"B": B, "V": V, "size": SIZE, "subsets": len(subsets), "kept_views": KEEP, "dtype": dtype, "blocks": a.blocks, "steps_per_block": a.block,
            "sweep_vs_loop": full, "loop_over_sweep": round(b_ms / a_ms, 3), "larger_spread": spread,
            "sweep_faster_by_more_than_the_spread": bool(a_ms < b_ms * (1.0 - spread)),
            "one_subset": single, "sweep_S1_over_ragged_evaluate": round(single["sweep_S1"]["ms_per_step_median"] / single["ragged_evaluate"]["ms_per_step_median"], 4),
            "profiled_step_ms": {"per_frame_stage": round(frames_ms, 3), "tails_total": round(sum(tails), 3), "passes": len(tails),
                                 "per_subset_tail": round(sum(tails) / len(subsets), 4)},
            "per_subset_equal_to_evaluate": bool(same), "by_count": {str(k): v["test_mpjpe"] for k, v in numbers["by_count"].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--limit", type=int, default=300, help="seconds per dtype (a child process each)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print("ROW " + json.dumps(one(a.one, a)), flush=True)
        return 0
    rows = []
    for dtype in a.dtypes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", dtype, "--blocks", str(a.blocks), "--block", str(a.block), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{dtype}: no result within {a.limit} s; the probe ends here", file=sys.stderr)
            return 124
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"{dtype}: exit status {r.returncode}; the probe ends here", file=sys.stderr)
            return r.returncode
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:]))
    text = json.dumps({"probe": "subsets_sweep", "rows": rows}, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
