#!/usr/bin/env python3
"""Timing record of the vertex evaluation.  Two comparisons:

  epoch    steps per second of
             on         EpochEvaluator(vertices=True).step(batch): forward, loss, the pooled launch, joints -> mesh and
                        hmv_eval_vertices_add per step, nothing copied to the host; compute() at the end of the timed block;
             test_step  the loop that gave these numbers before: model.test_step(batch) with get_vertices and a float() of every value
                        it returns (one stream synchronisation per step)
           on the device-resident batches of tools/eval_probe.py (ResNet50-paper, 8 views of 256 x 256) with a 778-vertex
           synth.mano_like hand, at batch 1 and batch 32, in fp32 and fp16;
  entry    microseconds per call of hmv_eval_vertices_add alone against what test_step runs on the same [B, 778, 3] meshes: the two
           `/ 1000.` and one hmv_pose_metrics with the alignment, at batch 1 and batch 32; a block of --calls calls is timed with the
           host clock from its first enqueue to a device synchronise.

tools/eval_probe.py's protocol: the loops alternate in one process in blocks; the figure is the median over blocks.  The shader
clock is read before and after (rocm-smi, when it is there) and reported as found.

A record, not a gate.    python tools/vertices_eval_probe.py [--blocks 5] [--block 40] [--calls 200] [--warmup 10] [--out profiles/vertices_eval.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from breakdown_probe import clock_level  # noqa: E402
from eval_probe import build  # noqa: E402
from handmvnet_amd import _lib  # noqa: E402
from handmvnet_amd.evaluation import STEPS, EpochEvaluator, vertices_doubles  # noqa: E402
from handmvnet_amd.ik import JointsToVertices  # noqa: E402
from handmvnet_amd.mano import ManoSkin  # noqa: E402
from handmvnet_amd.synth import mano_like  # noqa: E402

SHAPES = {"b1_v8_256": (8, 1, 256), "b32_v8_256": (8, 32, 256)}   # name: (views, batch, size)
DTYPES = ("f32", "f16")
NV = 778


def median_rates(loops, blocks, block, warmup):
    for f in loops.values():
        f(warmup)
    torch.cuda.synchronize()
    rate = {k: [] for k in loops}
    for _ in range(blocks):
        for k, f in loops.items():
            t0 = time.perf_counter()
            f(block)
            rate[k].append(block / (time.perf_counter() - t0))
    return {k: float(np.median(v)) for k, v in rate.items()}, rate


def epoch_rows(a, dev):
    rows = []
    for name, (V, B, size) in SHAPES.items():
        for dtype in DTYPES:
            model, plain_batch = build(V, B, size, dtype, dev)
            model.joints_to_vertices = JointsToVertices(ManoSkin(mano_like(7, NV), device=dev), device=dev)
            first = plain_batch()
            own = model(first["data"]["rgb"], first["data"]["bboxes"], first["cam_params"])["joints_cam"].float()
            g = torch.Generator().manual_seed(5)
            gt_v = model.joints_to_vertices(own * 1000) + torch.randn(B, NV, 3, generator=g).to(dev) * 6.0

            def batch():
                b = plain_batch()
                b["data"]["vertices"] = gt_v
                return b

            on = EpochEvaluator(model, "test", vertices=True)

            def loop_on(n):
                on.reset()
                for _ in range(n):
                    on.step(batch())
                return on.compute()

            def loop_test_step(n):
                model.get_vertices = True
                try:
                    for _ in range(n):
                        res = model.test_step(batch())
                        [float(v) for v in res["metrics"].values() if not isinstance(v, list)]
                        float(res["loss"])
                finally:
                    model.get_vertices = False

            med, rate = median_rates({"on": loop_on, "test_step": loop_test_step}, a.blocks, a.block, a.warmup)
            us = {k: 1e6 / v for k, v in med.items()}
            rows.append({"shape": name, "B": B, "V": V, "size": size, "dtype": dtype, "n_verts": NV, "steps_per_loop": a.blocks * a.block,
                         "steps_per_s_median": {k: round(v, 2) for k, v in med.items()},
                         "us_per_step_median": {k: round(v, 1) for k, v in us.items()},
                         "test_step_minus_on_us": round(us["test_step"] - us["on"], 1),
                         "steps_per_s_blocks": {k: [round(x, 1) for x in v] for k, v in rate.items()}})
            print(json.dumps(rows[-1]), flush=True)
            del model, on
    return rows


def entry_rows(a, dev):
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rows = []
    for B in (1, 32):
        g = torch.Generator().manual_seed(B)
        gt = (torch.randn(B, NV, 3, generator=g) * 40 + 300).to(dev)
        pred = gt + torch.randn(B, NV, 3, generator=g).to(dev) * 6.0
        state = torch.zeros(vertices_doubles(NV, STEPS), device=dev, dtype=torch.float64)
        scratch = torch.empty(int(lib.hmv_eval_vertices_scratch_bytes(B, NV, STEPS)) // 8, device=dev, dtype=torch.float64)
        m = _lib.HmvEvalVerticesArgs()
        m.struct_size = ctypes.sizeof(_lib.HmvEvalVerticesArgs)
        m.B, m.n_verts, m.steps, m.thr_min, m.thr_max, m.unit_div = B, NV, STEPS, 0.0, 0.02, 1000.0
        m.pred_vertices, m.gt_vertices = pred.data_ptr(), gt.data_ptr()
        m.state, m.state_doubles, m.scratch, m.scratch_bytes = state.data_ptr(), state.numel(), scratch.data_ptr(), scratch.numel() * 8
        result = torch.empty(4 + 2 * STEPS, device=dev)

        def loop_entry(n):
            for _ in range(n):
                _lib.check(lib.hmv_eval_vertices_add(0, ctypes.byref(m), stream))
            torch.cuda.synchronize()

        def loop_pose_metrics(n):
            for _ in range(n):
                p, t = pred / 1000., gt / 1000.
                rc = lib.hmv_pose_metrics(0, p.data_ptr(), t.data_ptr(), B, NV, 3, 0.0, 0.02, STEPS, 1, None, result.data_ptr(), stream)
                assert rc == 0
            torch.cuda.synchronize()

        med, rate = median_rates({"vertices_add": loop_entry, "pose_metrics": loop_pose_metrics}, a.blocks, a.calls, a.warmup)
        us = {k: 1e6 / v for k, v in med.items()}
        # the two routes on the same meshes: the per-step values agree
        state.zero_()
        loop_entry(1)
        loop_pose_metrics(1)
        s, r = state.cpu().numpy(), result.cpu().numpy()
        rows.append({"B": B, "n_verts": NV, "calls_per_block": a.calls, "us_per_call_median": {k: round(v, 2) for k, v in us.items()},
                     "pose_metrics_over_vertices_add": round(us["pose_metrics"] / us["vertices_add"], 2),
                     "mpvpe_mm": {"vertices_add": float(s[6] / s[5] * 1000), "pose_metrics": float(r[0]) * 1000},
                     "pa_mpvpe_mm": {"vertices_add": float(s[7] / s[5] * 1000), "pose_metrics": float(r[1]) * 1000},
                     "us_per_call_blocks": {k: [round(1e6 / x, 2) for x in v] for k, v in rate.items()}})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("epoch", "entry"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vertices_eval_probe measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    record = {"probe": "vertices_eval", "clock_before": clock_level()}
    if a.only != "epoch":
        record["entry"] = entry_rows(a, dev)
    if a.only != "entry":
        record["epoch"] = epoch_rows(a, dev)
    record["clock_after"] = clock_level()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
