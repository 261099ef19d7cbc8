#!/usr/bin/env python3
"""Timing record of the triangulation launch: V = 8 cameras, 21 joints, B = 1 and B = 32, all 56 candidates of 3 cameras.

  (a) device   one handmvnet_amd.triangulation.triangulate call (hmv_op_triangulate): plain DLT, and DLT + RANSAC with refit;
  (b) torch    what a caller had before, on the same device tensors: the algorithm of the reference's batch_triangulate_dlt_torch (one
               batched torch.linalg.svd of the [B * 21, 2 V, 4] DLT matrices) and of its batch_triangulate_dlt_ransac_torch (a Python
               loop over the candidates with one such SVD and one reprojection each), written out below with torch ops.

Both run in the one process in alternating blocks of --block steps; a step is timed with the host clock from its first enqueue to the
end of a device synchronise; the figure is the median over --blocks blocks, the spread (max - min) / median over the blocks.  Also
recorded: the largest difference between the two results.  A record, not a gate: no speed-up is promised.

Each batch size runs in a child process of its own under a time limit (--limit seconds); the first failure ends the probe.
    python tools/triangulation_probe.py [--blocks 5] [--block 5] [--warmup 2] [--out profiles/triangulation.json]
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

V, J, N_CAMS, THRESHOLD = 8, 21, 3, 10.0


def rig(B, rng):
    """World-to-camera extrinsics of cameras on a ring around the hand, intrinsics, and fp32 pixels with 2 px of noise."""
    ext = np.zeros((B, V, 4, 4))
    for b in range(B):
        for v in range(V):
            ang = 2 * np.pi * (v + rng.uniform(-0.2, 0.2)) / V
            pos = np.array([1.2 * np.cos(ang), rng.uniform(-0.3, 0.3), 1.2 * np.sin(ang)])
            z = -pos / np.linalg.norm(pos)
            x = np.cross([0.0, 1.0, 0.0], z)
            x /= np.linalg.norm(x)
            c2w = np.eye(4)
            c2w[:3, :3], c2w[:3, 3] = np.stack([x, np.cross(z, x), z], axis=1), pos
            ext[b, v] = np.linalg.inv(c2w)
    intr = np.stack([rng.uniform(550, 650, (B, V)), rng.uniform(550, 650, (B, V)), rng.uniform(300, 340, (B, V)),
                     rng.uniform(220, 260, (B, V))], axis=-1)
    X = np.concatenate([rng.uniform(-0.1, 0.1, (B, J, 3)), np.ones((B, J, 1))], axis=-1)
    K = np.zeros((B, V, 3, 3))
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = intr[..., 0], intr[..., 1], intr[..., 2], intr[..., 3], 1.0
    h = np.einsum("bvik,bjk->bvji", K @ ext[:, :, :3], X)
    pts = h[..., :2] / h[..., 2:3] + rng.standard_normal((B, V, J, 2)) * 2
    return pts.astype(np.float32), intr.astype(np.float32), K.astype(np.float32), ext.astype(np.float32)


def torch_dlt(pts, M):
    """pts [B, n, J, 2], M [B, n, 3, 4] -> [B, J, 3]: the smallest right singular vector of each point's DLT matrix."""
    import torch
    B, n, Jn = pts.shape[:3]
    p = pts.permute(0, 2, 1, 3)                                                    # [B, J, n, 2]
    rows = p.unsqueeze(-1) * M[:, None, :, 2:3, :] - M[:, None, :, :2, :]         # [B, J, n, 2, 4]
    vt = torch.linalg.svd(rows.reshape(B * Jn, 2 * n, 4))[2]
    return (vt[:, -1, :3] / vt[:, -1, 3:]).reshape(B, Jn, 3)


def torch_ransac(pts, M, table, threshold):
    """The candidate loop: the first candidate with the most inliers keeps its point."""
    import torch
    B, _, Jn = pts.shape[:3]
    best = torch.zeros(B, Jn, 3, device=pts.device)
    best_n = torch.zeros(B, Jn, device=pts.device, dtype=torch.long)
    ones = torch.ones(B, Jn, 1, device=pts.device)
    for cams in table:
        X = torch_dlt(pts[:, cams], M[:, cams])
        h = torch.einsum("bvik,bjk->bvji", M, torch.cat([X, ones], dim=-1))
        n = ((pts - h[..., :2] / h[..., 2:3]).norm(dim=-1) < threshold).sum(dim=1)
        better = n > best_n
        best[better], best_n[better] = X[better], n[better]
    return best


def one(B, a):
    import torch
    from handmvnet_amd.triangulation import candidate_table, triangulate
    dev = torch.device("cuda:0")
    pts, intr, K, ext = (torch.from_numpy(x).to(dev) for x in rig(B, np.random.default_rng(B)))
    M = K @ ext[:, :, :3]
    table = candidate_table(V, N_CAMS)
    table_dev, table_list = torch.from_numpy(table).to(dev), [list(map(int, c)) for c in table]
    last = {}

    def device_plain():
        last["device_plain"] = triangulate(pts, intr, ext, extrinsic_kind="world_to_cam")[0]

    def torch_plain():
        last["torch_plain"] = torch_dlt(pts, M)

    def device_ransac():
        last["device_ransac"] = triangulate(pts, intr, ext, subsets=table_dev, threshold=THRESHOLD, extrinsic_kind="world_to_cam")[0]

    def device_ransac_refit():
        last["device_ransac_refit"] = triangulate(pts, intr, ext, subsets=table_dev, threshold=THRESHOLD, refit=True,
                                                  extrinsic_kind="world_to_cam")[0]

    def torch_ransac_loop():
        last["torch_ransac"] = torch_ransac(pts, M, table_list, THRESHOLD)

    loops = {"device_plain": device_plain, "torch_plain": torch_plain, "device_ransac": device_ransac,
             "device_ransac_refit": device_ransac_refit, "torch_ransac": torch_ransac_loop}

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
    full = {k: {"ms_per_call_median": round(float(np.median(v)), 4), "ms_per_call_blocks": [round(x, 4) for x in v],
                "spread": round((max(v) - min(v)) / float(np.median(v)), 4)} for k, v in ms.items()}
    diff = {k: float((last["device_" + k] - last["torch_" + k]).abs().max()) for k in ("plain", "ransac")}
    return {"B": B, "V": V, "J": J, "candidates": len(table), "n_cams": N_CAMS, "threshold_px": THRESHOLD, "blocks": a.blocks,
            "calls_per_block": a.block, "timings": full,
            "torch_over_device": {"plain": round(full["torch_plain"]["ms_per_call_median"] / full["device_plain"]["ms_per_call_median"], 2),
                                  "ransac": round(full["torch_ransac"]["ms_per_call_median"] / full["device_ransac"]["ms_per_call_median"], 2)},
            "larger_spread": max(v["spread"] for v in full.values()),
            "max_abs_difference_m": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
        cmd = [sys.executable, os.path.abspath(__file__), "--one", B, "--blocks", str(a.blocks), "--block", str(a.block), "--warmup", str(a.warmup)]
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
    text = json.dumps({"probe": "triangulation", "rows": rows}, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
