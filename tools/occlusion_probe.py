#!/usr/bin/env python3
"""Timing record of an occlusion sweep from raw frames: a 4 x 4 occluder grid on every camera of the headline rig (batch 4 x 8 views,
480 x 640 frames, 256 x 256 windows on ResNet50-paper) = 128 variants, in fp32 and in fp16.

  (a) sweep   HandMvNet.forward_frames_occlusions: one clean per-frame pass (B V frames), one occluded frame per (variant, sample)
              (n_occ B frames), the fusion tail per variant;
  (b) loop    what a caller had before: per variant copy the frames, zero the rectangle in that camera's frames, call forward_frames
              -- n_occ full forwards of B V frames each.

Both run in the one process in alternating blocks; a block is one whole sweep over the batch, timed with the host clock from its first
enqueue to a device synchronise; the figure is the median over --blocks blocks, the spread (max - min) / median over the blocks.  Also
recorded: the two backbone-frame counts and their ratio n_occ V / (V + n_occ), (a)'s split into the frame stages and the tails (the
bracketing profiling records of one profiled call), and whether the first variants of (a) have the bits of (b).

Each dtype runs in a child process of its own under a time limit (--limit seconds, sized to the (b) loop); the first failure ends the
probe.    python tools/occlusion_probe.py [--blocks 5] [--warmup 1] [--out profiles/occlusions.json]
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

V, B, SIZE, GRID, FH, FW = 8, 4, 256, 4, 480, 640


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
    intr = torch.from_numpy(synth_inputs(cfg, B, 1000, SIZE)[2]).to(dev)
    g = torch.Generator().manual_seed(7)
    frames = torch.randint(0, 256, (B, V, FH, FW, 3), dtype=torch.uint8, generator=g)
    frames = ((frames.float() + frames.roll(1, 2) + frames.roll(1, 3)) / 3).to(torch.uint8)      # a little smoothing: no flat heat maps
    side = torch.randint(150, 400, (B, V, 1), generator=g)
    org = torch.cat([torch.randint(-40, FW - 200, (B, V, 1), generator=g), torch.randint(-40, FH - 200, (B, V, 1), generator=g)], dim=-1)
    boxes = torch.cat([org, org + side], dim=-1).int()
    model.reserve(B, SIZE, SIZE, dev)
    return model, frames.to(dev), boxes, {"intrinsic": intr}


def one(dtype, a):
    import torch
    from handmvnet_amd.occlusion import cell_rects, grid_variants
    dev = torch.device("cuda:0")
    model, frames, boxes_host, cam = build(dtype, dev)
    boxes = boxes_host.to(dev)
    variants = grid_variants(V, GRID)
    view = np.array([c for c, _, _ in variants], dtype=np.int32)
    rects = torch.stack([cell_rects(boxes, GRID, r, k)[:, c] for c, r, k in variants])               # device [n_occ, B, 4]
    # the loop's rectangles in frame pixels, on the host (its caller has the windows there): [n_occ, B, 4], clipped to the frame
    win = torch.stack([cell_rects(boxes_host, GRID, r, k)[:, c] + boxes_host[:, c, :2].repeat(1, 2) for c, r, k in variants])
    win[..., 0::2].clamp_(0, FW)
    win[..., 1::2].clamp_(0, FH)
    win = win.tolist()

    def sweep():
        return model.forward_frames_occlusions(frames, boxes, view, rects, cam)

    def loop(n=len(variants)):
        outs = []
        for o, (c, _, _) in enumerate(variants[:n]):
            z = frames.clone()
            for b in range(B):
                x1, y1, x2, y2 = win[o][b]
                z[b, c, y1:y2, x1:x2] = 0
            outs.append(model.forward_frames(z, boxes, cam))
        return outs

    got = sweep()
    ref = loop(4)
    torch.cuda.synchronize()
    same = all(torch.equal(got["joints_cam"][1 + o], ref[o]["joints_cam"]) and
               torch.equal(got["heatmap_occ"][o], ref[o]["heatmap"][:, variants[o][0]]) for o in range(4))
    loops = {"sweep": sweep, "loop": loop}
    for f in loops.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in loops}
    for _ in range(a.blocks):
        for k, f in loops.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[k].append(1000.0 * (time.perf_counter() - t0))
    full = {k: {"ms_median": round(float(np.median(v)), 3), "ms_blocks": [round(x, 3) for x in v],
                "spread": round((max(v) - min(v)) / float(np.median(v)), 4)} for k, v in ms.items()}
    # (a)'s split: the bracketing records of one profiled call
    model.set_profiling(True)
    sweep()
    torch.cuda.synchronize()
    recs = model.profile_records()
    model.set_profiling(False)
    stages = [r["ms"] for r in recs if r["kernel"] == "occlusions_frames"]
    tails = [r["ms"] for r in recs if r["kernel"] == "occlusions_tail"]
    n = len(variants)
    a_ms, b_ms = full["sweep"]["ms_median"], full["loop"]["ms_median"]
    spread = max(full["sweep"]["spread"], full["loop"]["spread"])
    return {"B": B, "V": V, "size": SIZE, "frame": [FH, FW], "grid": GRID, "variants": n, "dtype": dtype, "blocks": a.blocks,
            "sweep_vs_loop": full, "loop_over_sweep": round(b_ms / a_ms, 3), "larger_spread": spread,
            "sweep_faster_by_more_than_the_spread": bool(a_ms < b_ms * (1.0 - spread)),
            "backbone_frames": {"sweep": (V + n) * B, "loop": n * V * B, "ratio": round(n * V / (V + n), 3)},
            "profiled_call_ms": {"clean_frame_stage": round(stages[0], 3), "occluded_frame_passes": [round(x, 3) for x in stages[1:]],
                                 "tails_total": round(sum(tails), 3), "tail_passes": len(tails)},
            "first_variants_equal_to_the_loop": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
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
        cmd = [sys.executable, os.path.abspath(__file__), "--one", dtype, "--blocks", str(a.blocks), "--warmup", str(a.warmup)]
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
    text = json.dumps({"probe": "occlusion_sweep", "rows": rows}, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
