#!/usr/bin/env python3
"""Timing record of the vertex path of an evaluation step (get_vertices): milliseconds per step of

  (a) device   handmvnet_amd.ik.JointsToVertices.__call__ on a [B, 21, 3] device tensor: the IK launch (hmv_op_hand_ik), the layer,
               the un-alignment launch (hmv_op_rigid_unapply); nothing crosses to the host;
  (b) host     what the reference does per step (handmvnet.py:395-398): per sample, joints to the host (.cpu().numpy()), the numpy
               alignment + adaptive_IK (tests/ik_oracle.py), the layer on that sample's rotations, the un-alignment in numpy, and the
               vertices uploaded into the step's [B, 778, 3] device tensor

at batch 1 and batch 32.  The layer is a stand-in in ManoLayer's calling convention (a fixed linear map from pose_R - I to 778
vertices: one small fp32 GEMM), run in torch on the device by BOTH loops, as the reference runs its ManoLayer on the device in both.
The joints are the fixture's posed hands with seeded noise, resident on the device.

Both loops run in the one process in alternating blocks; a loop's block is at least --block steps and at least --seconds long (sized
from one calibration block after the warm-up: the device loop's steps are some 0.06 ms, and a block of a millisecond would measure the
host clock); a block is timed with the host clock from its first enqueue to a device synchronisation behind its last step; the figure
is the median over blocks, with the spread (max - min) / median.

A record, not a gate.    python tools/ik_probe.py [--blocks 7] [--block 20] [--seconds 0.4] [--warmup 3] [--out profiles/ik.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ik_oracle  # noqa: E402
from handmvnet_amd.ik import JointsToVertices  # noqa: E402

NV = 778


class LinearHand(torch.nn.Module):
    def __init__(self, template, dev):
        super().__init__()
        g = torch.Generator().manual_seed(778)
        self.W = (torch.randn(144, NV * 3, generator=g) * 12.0).to(dev)
        self.base = (torch.rand(NV, 3, generator=g) * 180.0 - 90.0).to(dev)
        self.eye = torch.eye(3, device=dev).repeat(16, 1, 1)
        self.template = torch.as_tensor(template).to(dev)

    def forward(self, pose_R):
        b = pose_R.shape[0]
        return ((pose_R - self.eye).reshape(b, 144) @ self.W).reshape(b, NV, 3) + self.base, self.template.expand(b, 21, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.4, help="least duration of a timed block")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    fix = np.load(os.path.join(ROOT, "tests", "golden", "ik_cases.npz"))
    template = fix["template_std"]
    layer = LinearHand(template, dev)
    j2v = JointsToVertices(layer, device=dev)
    rng = np.random.default_rng(9)
    rows = []
    for B in (int(b) for b in a.batches.split(",")):
        base = np.stack([fix[f"posed_{i % 3}.joints"] for i in range(B)])
        joints = torch.from_numpy((base + rng.normal(scale=1.0, size=base.shape)).astype(np.float32)).to(dev)
        last = {}

        def run_device(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                v = j2v(joints)
            torch.cuda.synchronize()
            last["device"] = v
            return time.perf_counter() - t0

        def run_host(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                v = torch.zeros((B, NV, 3), device=dev, dtype=torch.float32)
                for s in range(B):
                    j = joints[s].detach().cpu().numpy()
                    ret_R, ret_t, _, pose_R = ik_oracle.align_and_ik(j, template)
                    verts = layer(torch.from_numpy(pose_R[None]).float().to(dev))[0].cpu().numpy()[0]
                    verts = (np.linalg.inv(ret_R) @ (verts.T - ret_t)).T
                    v[s] = torch.from_numpy(verts).float().to(dev)
            torch.cuda.synchronize()
            last["host"] = v
            return time.perf_counter() - t0

        loops = {"device": run_device, "host": run_host}
        steps = {}
        for k, f in loops.items():   # warm up, then size the loop's blocks: at least --block steps and at least --seconds of work
            f(a.warmup)
            steps[k] = max(a.block, int(np.ceil(a.seconds / (f(a.block) / a.block))))
        ms = {k: [] for k in loops}
        for _ in range(a.blocks):
            for k, f in loops.items():
                ms[k].append(1000.0 * f(steps[k]) / steps[k])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rows.append({"B": B, "n_vertices": NV, "blocks": a.blocks, "steps_per_block": steps,
                     "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
                     "device_over_host": round(med["device"] / med["host"], 4),
                     "ms_per_step_blocks": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                     "spread": {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in ms.items()},
                     "max_abs_difference_mm": float((last["device"] - last["host"]).abs().max()),
                     "status_nonzero": int((j2v.last_status != 0).sum())})
    text = json.dumps({"probe": "ik", "rows": rows})
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
