#!/usr/bin/env python3
"""Timing record of the confidence-gated absolute position: V = 8 cameras, B = 1 and B = 32, the cfg3 model of bench.py.

  (a) gated    model.forward_absolute(x, bbox, cam, confidence=0.5): forward + peaks + select + triangulate, all on the device;
  (b) plain    model.forward_absolute(x, bbox, cam): forward + triangulate, every view trusted alike;
  (c) host     (b), then what a caller had before for the gate: the heat map and the 2D joints read back, the maximum of every map
               (torch.max on the host, the algorithm of the reference's heatmaps_to_coordinates) and, per sample, the algorithm of the
               reference's triangulate_dlt written out below: the threshold walk over the joints and one numpy SVD per joint.

All run in the one process in alternating blocks of --block steps; a step is timed with the host clock from its first enqueue to the
end of a device synchronise; the figure is the median over --blocks blocks, the spread (max - min) / median over the blocks.  Also
recorded: the peaks launch alone (the library entry, outputs allocated once), timed with device events over --peak-calls back-to-back
calls, as bytes of heat map per second and as a fraction of the read rate of profiles/r04_probe_copy.txt -- once on the step's one
heat map, which the 256 MB last-level cache holds after the first call, and once walking over copies of it that together exceed
twice that cache, so that every call reads from HBM.  A record, not a gate: nothing was promised; the one expectation is that the peaks launch is bound by one read of
the heat map.

Each batch size runs in a child process of its own under a time limit (--limit seconds); the first failure ends the probe.
    python tools/confidence_probe.py [--blocks 5] [--block 5] [--warmup 2] [--out profiles/confidence.json]
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

V, SIZE, THRESHOLD = 8, 256, 0.5
CACHE_BYTES = 256 << 20          # the last-level (Infinity) cache of one MI355X
COPY_PROBE_READ_TBS = 5.9        # profiles/r04_probe_copy.txt: reads alone, 5.89-5.95 TB/s


def rig(B, rng):
    """Camera-to-world extrinsics of V cameras on a ring around the hand, in metres."""
    ext = np.zeros((B, V, 4, 4), dtype=np.float32)
    for b in range(B):
        for v in range(V):
            ang = 2 * np.pi * (v + rng.uniform(-0.2, 0.2)) / V
            pos = np.array([1.2 * np.cos(ang), rng.uniform(-0.3, 0.3), 1.2 * np.sin(ang)])
            z = -pos / np.linalg.norm(pos)
            x = np.cross([0.0, 1.0, 0.0], z)
            x /= np.linalg.norm(x)
            ext[b, v] = np.eye(4)
            ext[b, v, :3, :3], ext[b, v, :3, 3] = np.stack([x, np.cross(z, x), z], axis=1), pos
    return ext


def host_gate(pts, conf, M, thres):
    """One sample on the host: pts [V, J, 2], conf [V, J], M [V, 3, 4] -> [J, 3].  The threshold is lowered by 0.05 until two cameras
    pass and is never reset between the joints; each joint is one SVD of its selected cameras' DLT rows."""
    out = np.full((pts.shape[1], 3), np.nan)
    for j in range(pts.shape[1]):
        while True:
            sel = np.where(conf[:, j] > thres)[0]
            if thres <= 0 or len(sel) > 1:
                break
            thres -= 0.05
        if len(sel) < 2:
            continue
        rows = pts[sel, j, :, None] * M[sel, 2:3, :] - M[sel, :2, :]
        vt = np.linalg.svd(rows.reshape(-1, 4))[2]
        out[j] = vt[-1, :3] / vt[-1, 3]
    return out


def one(B, a):
    import torch
    import bench
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.confidence import heatmap_peaks
    from handmvnet_amd.spec import config_from_params
    from handmvnet_amd.synth import synth_inputs, synth_state_dict
    dev = torch.device("cuda:0")
    bt, ch, _, _, _ = bench.WORKLOADS["cfg3"]
    tp, mp, dp = bench.params(bt, ch, V, B, SIZE)
    cfg = config_from_params(tp, mp, dp)
    model = HandMvNet(tp, mp, dp)
    model.load_state_dict(synth_state_dict(cfg, 1), strict=True)
    model.to(dev).eval()
    x, bbox, intr = (torch.from_numpy(t).to(dev) for t in synth_inputs(cfg, B, 1000, SIZE))
    E = rig(B, np.random.default_rng(B))
    cam = {"intrinsic": intr, "extrinsic": torch.from_numpy(E).to(dev)}
    W = np.linalg.inv(E.astype(np.float64))[:, :, :3]
    K = np.zeros((B, V, 3, 3))
    k4 = intr.cpu().numpy().reshape(B, V, 4)
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = k4[..., 0], k4[..., 1], k4[..., 2], k4[..., 3], 1.0
    M = K @ W
    boxes = bbox.cpu().numpy().astype(np.float64).reshape(B, V, 1, 4)
    last = {}

    def gated():
        last["gated"] = model.forward_absolute(x, bbox, cam, confidence=THRESHOLD)

    def plain():
        last["plain"] = model.forward_absolute(x, bbox, cam)

    def host():
        out = model.forward_absolute(x, bbox, cam)
        hm = out["heatmap"].cpu()
        crop = out["joints_crop_img"].cpu().numpy().astype(np.float64)
        pts = crop * ((boxes[..., 2:] - boxes[..., :2]) / SIZE) + boxes[..., :2]      # crop pixels to frame pixels
        conf = torch.max(hm.reshape(B, V, 21, -1), 3)[0].numpy()
        last["host"] = np.stack([host_gate(pts[b], conf[b], M[b], THRESHOLD) for b in range(B)])

    loops = {"gated": gated, "plain": plain, "host": host}

    def run(f, n):
        for _ in range(n):
            f()
            torch.cuda.synchronize()

    for f in loops.values():
        run(f, a.warmup)
    ms = {k: [] for k in loops}
    for _ in range(a.blocks):
        for k, f in loops.items():
            t0 = time.perf_counter()
            run(f, a.block)
            ms[k].append(1000.0 * (time.perf_counter() - t0) / a.block)
    full = {k: {"ms_per_step_median": round(float(np.median(v)), 4), "ms_per_step_blocks": [round(t, 4) for t in v],
                "spread": round((max(v) - min(v)) / float(np.median(v)), 4)} for k, v in ms.items()}

    # the peaks launch alone: the library entry on outputs allocated once, so a call is one enqueue and nothing else
    import ctypes
    from handmvnet_amd import _lib
    hm = last["plain"]["heatmap"].contiguous()
    mv, ix, pr = heatmap_peaks(hm)
    pa = _lib.HmvPeaksArgs()
    pa.struct_size = ctypes.sizeof(_lib.HmvPeaksArgs)
    pa.N, pa.J, pa.h, pa.w = B * V, 21, int(hm.shape[-2]), int(hm.shape[-1])
    pa.heatmap, pa.maxval, pa.index, pa.preds = hm.data_ptr(), mv.data_ptr(), ix.data_ptr(), pr.data_ptr()
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nbytes = hm.numel() * 4
    # "rotating": the calls walk over copies of the map that together exceed twice the 256 MB last-level cache, so every call
    # reads its map from HBM; "same": every call reads the one map, which the cache holds after the first
    copies = hm.unsqueeze(0).repeat(-(-(2 * CACHE_BYTES) // nbytes) + 1, *([1] * hm.dim()))
    ptrs = {"same": [hm.data_ptr()], "rotating": [copies[i].data_ptr() for i in range(copies.shape[0])]}
    torch.cuda.synchronize()
    launch = {}
    for kind, where in ptrs.items():
        per_call = []
        for _ in range(a.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.peak_calls):
                pa.heatmap = where[i % len(where)]
                _lib.check(lib.hmv_op_heatmap_peaks(0, ctypes.byref(pa), stream))
            e1.record()
            torch.cuda.synchronize()
            per_call.append(e0.elapsed_time(e1) * 1000.0 / a.peak_calls)
        us = float(np.median(per_call))
        rate = nbytes / (us * 1e-6) / 1e12
        launch[kind] = {"maps_walked": len(where), "us_per_call_median": round(us, 3), "us_per_call_blocks": [round(t, 3) for t in per_call],
                        "heatmap_TB_per_s": round(rate, 4), "fraction_of_copy_probe_read_rate": round(rate / COPY_PROBE_READ_TBS, 4)}
    g, p = full["gated"]["ms_per_step_median"], full["plain"]["ms_per_step_median"]
    return {"B": B, "V": V, "image_size": SIZE, "heatmap": list(hm.shape), "threshold": THRESHOLD, "blocks": a.blocks,
            "steps_per_block": a.block, "timings": full, "gate_adds_ms": round(g - p, 4),
            "host_gate_adds_ms": round(full["host"]["ms_per_step_median"] - p, 4),
            "larger_spread": max(v["spread"] for v in full.values()),
            "peaks_launch": dict(launch, heatmap_bytes=nbytes, calls_per_block=a.peak_calls, copy_probe_read_TB_per_s=COPY_PROBE_READ_TBS,
                                 note="back-to-back library calls, outputs allocated once, device events around each block of calls; "
                                      "a small map is bound by the enqueue, not by its bytes"),
            "views_kept_histogram": np.bincount(last["gated"]["tri_views"].cpu().numpy().reshape(-1), minlength=V + 1).tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-calls", type=int, default=50)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--limit", type=int, default=200, help="seconds per batch size (a child process each)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print("ROW " + json.dumps(one(a.one, a)), flush=True)
        return 0
    rows = []
    for B in a.batches.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", B, "--blocks", str(a.blocks), "--block", str(a.block),
               "--warmup", str(a.warmup), "--peak-calls", str(a.peak_calls)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"B = {B}: no result within {a.limit} s; the probe ends here", file=sys.stderr)
            return 124
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"B = {B}: exit status {r.returncode}; the probe ends here", file=sys.stderr)
            return r.returncode
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:]))
    text = json.dumps({"probe": "confidence", "rows": rows}, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
