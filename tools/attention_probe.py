#!/usr/bin/env python3
"""Timing record of the attention maps: what capturing the cross block costs at the benchmarked model (ResNet50-paper, 8 views of
256 x 256, cross_attn with 5 blocks), batch 1 and batch 32, in fp32 and in fp16.

  (a) plain    HandMvNet.forward, nothing captured;
  (b) capture  capture_attention("cross"): the forward plus the map and view-share launches, then read_attention of the cross block;
  (c) rebuild  the only route there was before: capture_stages, forward, read_stage("tokens"), then the fusion up to the cross block's
               softmax in torch on the device (fp32, weights resident), which is what a user had to write by hand.

All three run in the one process in alternating blocks; a block is --block steps timed with the host clock from its first enqueue to
the end of a device synchronisation; the figure is the median over --blocks blocks, the spread (max - min) / median.  A record, not a
gate.  Each (dtype, batch) runs in a child process of its own under a time limit; the first failure ends the probe.
    python tools/attention_probe.py [--blocks 7] [--block 5] [--warmup 2] [--out profiles/attention_maps.json]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, SIZE, LAYERS = 8, 256, 5


def torch_cross_maps(tokens, w, pe, cross):
    """CrossAttentionFusion (fusion.py:26-30, layers.py:202-237) from the fusion's input up to the cross block's attn, fp32 torch ops."""
    import torch
    import torch.nn.functional as F

    def heads(t):
        b, i, hd = t.shape
        return t.reshape(b, i, 8, hd // 8).permute(0, 2, 1, 3)
    x = tokens + pe
    for l in range(cross + 1):
        p = w[l]
        _q, _k = (x[:, :21], x[:, 21:]) if l == cross else (x, x)
        q, k = heads(_q @ p["to_q"].T), heads(_k @ p["to_k"].T)
        attn = torch.softmax(q @ k.transpose(-1, -2) * 128 ** -0.5, dim=-1)
        if l == cross:
            return attn
        out = (attn @ heads(_k @ p["to_v"].T)).permute(0, 2, 1, 3).reshape(x.shape[0], -1, 1024) @ p["to_out"].T + p["to_out_b"]
        out = F.layer_norm(out + _q, (x.shape[-1],), p["n1w"], p["n1b"])
        f = F.layer_norm(out, (x.shape[-1],), p["f0w"], p["f0b"])
        f = F.gelu(f @ p["f1w"].T + p["f1b"]) @ p["f4w"].T + p["f4b"]
        x = F.layer_norm(f + out, (x.shape[-1],), p["n2w"], p["n2b"])


def one(dtype, B, a):
    import torch
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.spec import config_from_params
    from handmvnet_amd.synth import synth_inputs, synth_state_dict
    dev = torch.device("cuda:0")
    tp = {"debug": False, "root_relative": True}
    mp = {"num_views": V, "backbone": "resnet", "backbone_type": "50_paper", "backbone_channels": [1024], "backbone_pretrained": False,
          "backbone_early_return": 3, "pos_enc": ["pos2d", "crop", "sin"], "fusion": "cross_attn", "fusion_layers": LAYERS, "use_gcn": True}
    dp = {"batch_size": B, "image_size": SIZE, "heatmap_size": SIZE // 8, "name": "dexycb"}
    cfg = config_from_params(tp, mp, dp)
    sd = synth_state_dict(cfg, 1)
    model = HandMvNet(tp, mp, dp)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    if dtype == "f16":
        model.half()
    x, bbox, intr = (torch.from_numpy(t).to(dev) for t in synth_inputs(cfg, B, 1000, SIZE))
    cam = {"intrinsic": intr}
    cross = model.cross_block
    d = cfg.feat_dim
    names = {"to_q": "to_q.weight", "to_k": "to_k.weight", "to_v": "to_v.weight", "to_out": "to_out.weight", "to_out_b": "to_out.bias",
             "n1w": "norm1.weight", "n1b": "norm1.bias", "n2w": "norm2.weight", "n2b": "norm2.bias", "f0w": "ff.net.0.weight",
             "f0b": "ff.net.0.bias", "f1w": "ff.net.1.weight", "f1b": "ff.net.1.bias", "f4w": "ff.net.4.weight", "f4b": "ff.net.4.bias"}
    w = [{k: torch.from_numpy(np.asarray(sd[f"joints_late_fusion.attn_fusion.{l}.{v}"], dtype=np.float32)).to(dev) for k, v in names.items()}
         for l in range(cross + 1)]
    pos = torch.arange(V * 21).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2) * (-math.log(10000.0) / d))
    pe = torch.zeros(V * 21, d)
    pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
    pe = pe.to(dev)

    def plain(n):
        model.capture_stages(False)
        model.capture_attention(None)
        for _ in range(n):
            model(x, bbox, cam)

    def capture(n):
        model.capture_stages(False)
        model.capture_attention("cross")
        for _ in range(n):
            model(x, bbox, cam)
            model.read_attention(cross)

    def rebuild(n):
        model.capture_attention(None)
        model.capture_stages(True)
        for _ in range(n):
            model(x, bbox, cam)
            torch_cross_maps(model.read_stage("tokens"), w, pe, cross)

    loops = {"plain": plain, "capture": capture, "rebuild": rebuild}
    # the two routes give the same map (the record says how close)
    capture(1)
    got = model.read_attention(cross)[0]
    rebuild(1)
    diff = float((got - torch_cross_maps(model.read_stage("tokens"), w, pe, cross)).abs().max())
    for f in loops.values():
        f(a.warmup)
    torch.cuda.synchronize()
    ms = {k: [] for k in loops}
    for _ in range(a.blocks):
        for k, f in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(a.block)
            torch.cuda.synchronize()
            ms[k].append(1000.0 * (time.perf_counter() - t0) / a.block)
    res = {k: {"ms_per_step_median": round(float(np.median(v)), 4), "ms_per_step_blocks": [round(t, 4) for t in v],
               "spread": round((max(v) - min(v)) / float(np.median(v)), 4)} for k, v in ms.items()}
    p = res["plain"]["ms_per_step_median"]
    return {"B": B, "V": V, "size": SIZE, "dtype": dtype, "block": cross, "map_shape": list(got.shape), "blocks": a.blocks, "steps_per_block": a.block,
            "routes": res, "capture_minus_plain_ms": round(res["capture"]["ms_per_step_median"] - p, 4),
            "rebuild_minus_plain_ms": round(res["rebuild"]["ms_per_step_median"] - p, 4), "max_abs_capture_vs_rebuild": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--limit", type=int, default=150, help="seconds per (dtype, batch) (a child process each)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        dtype, B = a.one.split(":")
        print("ROW " + json.dumps(one(dtype, int(B), a)), flush=True)
        return 0
    rows = []
    for dtype in a.dtypes.split(","):
        for B in a.batches.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{dtype}:{B}", "--blocks", str(a.blocks), "--block", str(a.block),
                   "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"{dtype} B={B}: no result within {a.limit} s; the probe ends here", file=sys.stderr)
                return 124
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                print(f"{dtype} B={B}: exit status {r.returncode}; the probe ends here", file=sys.stderr)
                return r.returncode
            rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:]))
    text = json.dumps({"probe": "attention_maps", "rows": rows}, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
