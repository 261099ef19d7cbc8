#!/usr/bin/env python3
"""Timing record of the vertex path with this package's own MANO layer: milliseconds per step of

  (a) skin    handmvnet_amd.ik.JointsToVertices(ManoSkin) on a [B, 21, 3] device tensor: the IK launch (hmv_op_hand_ik) and the skin
              launch (hmv_op_mano_skin, with the un-alignment inside it);
  (b) torch   JointsToVertices around a torch fp32 transcription of the same rule on the device -- the projection as one batched
              torch.linalg.svd, the blends and the chain as einsums and small matmuls -- followed by the un-alignment launch
              (hmv_op_rigid_unapply)

at batch 1 and batch 32, 778 vertices, seeded MANO-shaped parameters (synth.mano_like).  The joints are the hand's own joints under
seeded rotations, moved rigidly, with seeded noise, resident on the device.  Nothing crosses to the host in either loop.

Both loops run in the one process in alternating blocks; a loop's block is at least --block steps and at least --seconds long (sized
from one calibration block after the warm-up); a block is timed with the host clock from its first enqueue to a device synchronisation
behind its last step; the figure is the median over blocks, with the spread (max - min) / median.

A record, not a gate.    python tools/mano_probe.py [--blocks 7] [--block 20] [--seconds 0.4] [--warmup 3] [--out profiles/mano.json]
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
from handmvnet_amd.ik import JointsToVertices  # noqa: E402
from handmvnet_amd.mano import JOINT_ORDER, PARENTS, ManoSkin  # noqa: E402
from handmvnet_amd.synth import mano_like  # noqa: E402

NV = 778


class TorchMano(torch.nn.Module):
    """The rule of include/handmv.h "MANO skinning" in torch fp32, batched, in ManoLayer's calling convention."""

    def __init__(self, p, dev):
        super().__init__()
        t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(dev)   # noqa: E731
        self.vt, self.sd, self.pd, self.reg, self.w = t(p.v_template), t(p.shapedirs), t(p.posedirs), t(p.J_regressor), t(p.weights)
        self.J = self.reg @ self.vt                    # zero betas: the joints of the template, once
        self.tips, self.order = list(p.tips), list(JOINT_ORDER)
        self.eye = torch.eye(3, device=dev)

    def forward(self, rot):
        n = rot.shape[0]
        U, _, Vh = torch.linalg.svd(rot)
        Q = U @ Vh
        flip = torch.where(torch.linalg.det(Q) < 0, -1.0, 1.0)
        rot = torch.cat([Q[..., :2], Q[..., 2:] * flip[..., None, None]], -1)
        v_posed = self.vt + torch.einsum("vcq,nq->nvc", self.pd, (rot[:, 1:] - self.eye).reshape(n, 135))
        J = self.J.expand(n, 16, 3)
        GR, Gt = [rot[:, 0]], [J[:, 0]]
        for k in range(1, 16):
            pa = PARENTS[k]
            Gt.append(torch.einsum("nij,nj->ni", GR[pa], J[:, k] - J[:, pa]) + Gt[pa])
            GR.append(GR[pa] @ rot[:, k])
        GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
        A = torch.cat([GR, (Gt - torch.einsum("nkij,nkj->nki", GR, J))[..., None]], -1)
        T = torch.einsum("vk,nkij->nvij", self.w, A)
        verts = torch.einsum("nvij,nvj->nvi", T[..., :3], v_posed) + T[..., 3]
        joints = torch.cat([Gt, verts[:, self.tips]], 1)[:, self.order]
        return verts * 1000, joints * 1000


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
    params = mano_like(7, NV)
    skin = ManoSkin(params, device=dev)
    j2v = {"skin": JointsToVertices(skin, device=dev), "torch": JointsToVertices(TorchMano(params, dev), device=dev)}
    rng = np.random.default_rng(9)
    rows = []
    for B in (int(b) for b in a.batches.split(",")):
        rot = np.zeros((B, 16, 3, 3), np.float32)
        for i in range(B):
            for k in range(16):
                ax, ang = rng.standard_normal(3), np.deg2rad(rng.uniform(0, 60))
                ax = ax / np.linalg.norm(ax)
                K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
                rot[i, k] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        posed = skin(torch.from_numpy(rot).to(dev), vertices=False)[1].cpu().numpy()
        joints = torch.from_numpy((posed + [0, 0, 600] + rng.normal(scale=1.0, size=posed.shape)).astype(np.float32)).to(dev)
        last = {}

        def runner(name):
            def run(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    v = j2v[name](joints)
                torch.cuda.synchronize()
                last[name] = v
                return time.perf_counter() - t0
            return run

        loops = {"skin": runner("skin"), "torch": runner("torch")}
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
                     "skin_over_torch": round(med["skin"] / med["torch"], 4),
                     "ms_per_step_blocks": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                     "spread": {k: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in ms.items()},
                     "max_abs_difference_mm": float((last["skin"] - last["torch"]).abs().max()),
                     "status_nonzero": int((j2v["skin"].last_status != 0).sum()) + int((skin.last_status != 0).sum())})
    text = json.dumps({"probe": "mano", "rows": rows})
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
