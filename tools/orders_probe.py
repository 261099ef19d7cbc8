#!/usr/bin/env python3
"""Timing record of a reference-view sweep: every one of the 8 cameras as the reference view (each_reference(8)) at batch 4 on the
cfg3 model (ResNet50-paper, 8 views of 256 x 256, cross-attention fusion), in fp32 and in fp16.

  (a) consensus  HandMvNet.forward_consensus: one backbone pass over the 32 frames, 8 fusion tails, one pose_consensus launch;
  (b) loop       what a caller had before: 8 forward() calls on the batch permuted by each order (256 backbone frames), the 8 results
                 copied to the host, rotated into camera 0's frame and averaged there with numpy.

Both run in the one process in alternating blocks of --block steps; a step is timed with the host clock from its first enqueue to
the end of a device synchronise (a) or of the host arithmetic (b); the figure is the median over --blocks blocks, the spread
(max - min) / median over the blocks.  Also recorded: (a)'s split into the per-frame stage and the tails (the bracketing profiling
records of one profiled step) and the largest difference between the two consensus poses.  A record, not a gate.

Each dtype runs in a child process of its own under a time limit (--limit seconds); the first failure ends the probe.
    python tools/orders_probe.py [--blocks 5] [--block 10] [--warmup 3] [--out profiles/orders.json]
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

V, B, SIZE = 8, 4, 256


def build(dtype, dev):
    import torch
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.spec import config_from_params
    from handmvnet_amd.synth import synth_inputs, synth_state_dict
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
    x, bbox, intr = synth_inputs(cfg, B, 1000, SIZE)
    xt, bt, it = (torch.from_numpy(a).to(dev) for a in (x, bbox, intr))
    model.reserve(B, SIZE, SIZE, dev)
    extr = torch.eye(4).repeat(B, V, 1, 1)
    for i in range(V):   # cameras on a ring around the hand, looking at it (tools/loss_probe.py)
        ang = 2 * np.pi * i / V
        pos = torch.tensor([0.8 * np.cos(ang), 0.8 * np.sin(ang), 0.1], dtype=torch.float32)
        z = -pos / pos.norm()
        xa = torch.linalg.cross(z, torch.tensor([0.0, 0.0, 1.0]))
        xa = xa / xa.norm()
        extr[:, i, :3, 0], extr[:, i, :3, 1], extr[:, i, :3, 2], extr[:, i, :3, 3] = xa, torch.linalg.cross(z, xa), z, pos
    return model, (xt, bt, it), extr


def one(dtype, a):
    import torch
    from handmvnet_amd.orders import each_reference
    dev = torch.device("cuda:0")
    model, (xt, bt, it), extr = build(dtype, dev)
    orders = each_reference(V)
    cam = {"intrinsic": it, "extrinsic": extr.to(dev)}
    # (b)'s inputs, permuted once outside the timed region, and the host rotations inverse(E_0) E_c [:3, :3]
    permuted = [(xt[:, o].contiguous(), bt[:, o].contiguous(), {"intrinsic": it[:, o].contiguous()}) for o in orders]
    E = extr.numpy().astype(np.float64)
    rot = np.stack([np.linalg.inv(E[:, 0]) @ E[:, o[0]] for o in orders])[:, :, :3, :3]      # [S, B, 3, 3]
    last = {}

    def consensus(n):
        for _ in range(n):
            last["a"] = model.forward_consensus(xt, bt, cam, orders=orders, target=0, mode="mean")["joints_cam"]
            torch.cuda.synchronize()

    def loop(n):
        for _ in range(n):
            poses = np.stack([model(*p)["joints_cam"].cpu().numpy() for p in permuted]).astype(np.float64)      # [S, B, 21, 3]
            last["b"] = np.einsum("sbrc,sbjc->sbjr", rot, poses).mean(axis=0)

    loops = {"consensus": consensus, "loop": loop}
    for f in loops.values():
        f(a.warmup)
    torch.cuda.synchronize()
    ms = {k: [] for k in loops}
    for _ in range(a.blocks):
        for k, f in loops.items():
            t0 = time.perf_counter()
            f(a.block)
            ms[k].append(1000.0 * (time.perf_counter() - t0) / a.block)
    full = {k: {"ms_per_step_median": round(float(np.median(v)), 3), "ms_per_step_blocks": [round(x, 3) for x in v],
                "spread": round((max(v) - min(v)) / float(np.median(v)), 4)} for k, v in ms.items()}
    diff = float(np.abs(last["a"].cpu().numpy().astype(np.float64) - last["b"]).max())
    model.set_profiling(True)
    model.forward_orders(xt, orders, bt, cam)
    torch.cuda.synchronize()
    recs = model.profile_records()
    model.set_profiling(False)
    frames_ms = sum(r["ms"] for r in recs if r["kernel"] == "subsets_frames")
    tails = [r["ms"] for r in recs if r["kernel"] == "subsets_tail"]
    a_ms, b_ms = full["consensus"]["ms_per_step_median"], full["loop"]["ms_per_step_median"]
    return {"B": B, "V": V, "size": SIZE, "orders": len(orders), "dtype": dtype, "blocks": a.blocks, "steps_per_block": a.block,
            "backbone_frames": {"consensus": B * V, "loop": B * V * len(orders)},
            "consensus_vs_loop": full, "loop_over_consensus": round(b_ms / a_ms, 3),
            "larger_spread": max(full["consensus"]["spread"], full["loop"]["spread"]),
            "profiled_step_ms": {"per_frame_stage": round(frames_ms, 3), "tails_total": round(sum(tails), 3), "passes": len(tails)},
            "max_abs_difference_of_the_two_consensus_poses": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--limit", type=int, default=240, help="seconds per dtype (a child process each)")
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
    text = json.dumps({"probe": "orders", "rows": rows}, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
