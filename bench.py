#!/usr/bin/env python3
"""Throughput benchmark of the HandMvNet hot path on MI355X (the eval_fps.py protocol,
/root/reference/src/eval_fps.py:68-108, re-stated: synthetic frames resident on the device,
warm-up, K timed forwards, frames/s = K*B*V / t -- without eval_fps's uninitialised
intrinsics, its hard-coded 8 views and the CPU MANO step).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the headline.  --full adds what takes runs or passes of its
own: the per-launch hipEvent timings behind `roofline` / `kernels` / `forward` (--instrument-every, --per-layer), the CPU
oracle baseline with its parity check, and the fp16 (BASELINE configs[4]) leg.  --dump-outputs DIR writes the last timed
step's outputs as DIR/<name>.npy (float32, seeded inputs: two builds can be compared output for output).

Workload = BASELINE.json configs[2] (the configuration the metric is quoted on): B=32
multi-view samples x V=8 views of 256x256 per GPU, ResNet50-paper backbone, cross-attention
fusion (5 layers), GCN decoder, fp32 on the fp32 matrix cores.  N GPUs = N independent
shards of 32 samples (weak scaling) + one RCCL all-gather of the results.

Prints ONE JSON line (rank 0).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from handmvnet_amd import HandMvNet  # noqa: E402
from handmvnet_amd.dist import gatherer_for  # noqa: E402
from handmvnet_amd.spec import config_from_params, conv_flops_per_image  # noqa: E402
from handmvnet_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_F16_MFMA_TFLOPS = 2500.0  # same guide, "Peak BF16/FP16 MFMA ~2.5 PF dense"
PEAK_HBM_GBS = 8000.0          # same guide, "HBM3E peak BW 8.0 TB/s spec" (6.29 TB/s measured with a float4 copy)

WORKLOADS = {
    # name: (backbone_type, channels, V, B per GPU, size)
    "cfg1": ("50_paper", [1024], 4, 1, 128),       # BASELINE.json configs[0]: HO3D_HandMvNet.yaml, batch 1, 4 views, 128x128 (its CPU plumbing case)
    "cfg3": ("50_paper", [1024], 8, 32, 256),      # BASELINE.json configs[2]
    "cfg2": ("18", [256, 128, 64], 4, 8, 256),     # BASELINE.json configs[1]
    "hr40": ("w40", [40, 80, 160, 320], 8, 32, 256),   # the *_HR release configs' backbone at the headline shape
}


def params(bt, ch, V, B, size, fusion="cross_attn"):
    tp = {"debug": False, "root_relative": True}
    lq = fusion == "cross_attn_learnable_query"   # (its blocks add their own PE: no 'sin' in pos_enc, spec.py warns otherwise)
    mp = {"num_views": V, "backbone": "hrnet" if bt.startswith("w") else "resnet", "backbone_type": bt, "backbone_channels": ch, "backbone_pretrained": False,
          "backbone_early_return": 3, "pos_enc": ["pos2d", "crop"] if lq else ["pos2d", "crop", "sin"], "fusion": fusion, "fusion_layers": 5,
          "use_gcn": True}
    dp = {"batch_size": B, "image_size": size, "heatmap_size": size // 8, "name": "dexycb"}
    return tp, mp, dp


def forward_flops(cfg, B, size):
    """Dense algorithmic FLOPs of one forward (SURVEY.md section 8(d) convention)."""
    f = conv_flops_per_image(cfg, size)
    per_frame = sum(f.values())
    V, d, T = cfg.num_views, cfg.feat_dim, cfg.num_views * 21
    def block(tq, tk):
        proj = 2 * d * 1024 * (tq + 2 * tk) + 2 * 1024 * d * tq
        att = 2 * 2 * tq * tk * 128 * 8
        ff = 2 * 2 * d * 128 * tq
        return proj + att + ff
    half = (cfg.fusion_layers - 1) // 2
    fusion = half * block(T, T) + block(21, T - 21) + half * block(21, 21)
    dec = 2 * 21 * 3 * (d * 256 + 256 * 64 + 64 * 3)
    return B * (V * per_frame + fusion + dec)


def forward_block(dtype, total_flops, ms_step, fam, n_instr):
    """Whole-forward figures.  fp32: dense algorithmic TFLOP/s against the fp32 MFMA peak (the north-star fraction).  fp16 /
    f32x3: the step's own floors -- MFMA time of the algorithmic FLOPs at the fp16 peak (x3 executed for f32x3) and HBM time of
    the algorithmic bytes of every conv / GEMM launch at 8 TB/s -- and the step time as a fraction of the higher one."""
    tf = total_flops / (ms_step * 1e-3) / 1e12
    fwd = {"algorithmic_gflop": round(total_flops / 1e9, 1), "tflops": round(tf, 2)}
    if dtype == "f32":
        fwd["frac_of_f32_mfma_peak"] = round(tf / PEAK_F32_MFMA_TFLOPS, 4)
        return fwd
    bytes_step = sum(v["bytes"] for v in fam.values()) / max(n_instr, 1)
    t_mfma = (3.0 if dtype == "f32x3" else 1.0) * total_flops / (PEAK_F16_MFMA_TFLOPS * 1e12) * 1e3
    t_hbm = bytes_step / (PEAK_HBM_GBS * 1e9) * 1e3
    per_launch = sum(max(v["t_hbm"], v["t_mfma"]) for v in fam.values()) / max(n_instr, 1) * 1e3
    fwd["algorithmic_gbytes"] = round(bytes_step / 1e9, 2)
    fwd["step_floor_ms"] = {"mfma": round(t_mfma, 3), "hbm@8TB/s": round(t_hbm, 3), "sum_of_per_launch_floors": round(per_launch, 3)}
    fwd["frac_of_step_floor"] = round(max(t_mfma, t_hbm) / ms_step, 4)
    return fwd


DUMP_BYTES = 64 << 20   # --dump-outputs: at most this much in all


def dump_outputs(out, dirname):
    """Writes each output tensor as DIR/<name>.npy in float32.  Arrays that do not fit their share of DUMP_BYTES (the smaller
    ones are written whole first) are replaced by a fixed, seeded sample of their flattened elements, in index order."""
    os.makedirs(dirname, exist_ok=True)
    arrs = sorted(((k, v.detach().float().cpu().numpy()) for k, v in out.items()), key=lambda kv: kv[1].nbytes)
    left = DUMP_BYTES - 4096 * len(arrs)   # room for the .npy headers
    for i, (k, a) in enumerate(arrs):
        share = left // (len(arrs) - i)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, f"{k}.npy"), a)
        left -= a.nbytes


def cpu_baseline(cfg, sd, size, model, dev, min_seconds=10.0):
    """The CPU oracle (fp32 port of the reference, OpenMP over the host cores) timed on a
    bounded sample of the same workload; also re-checks GPU-vs-oracle parity on it."""
    from oracle.oracle import Oracle
    orc = Oracle(cfg, sd, "f32")
    x, bbox, intr = synth_inputs(cfg, 1, 4242, size)
    ref = orc.forward(x, bbox, intr)                      # warm-up + parity reference
    t0, n = time.perf_counter(), 0
    while True:
        orc.forward(x, bbox, intr)
        n += 1
        el = time.perf_counter() - t0
        if el >= min_seconds or n >= 5000:   # a bounded sample: ~min_seconds of CPU work, whatever the shape
            break
    out = model(torch.from_numpy(x).to(dev), torch.from_numpy(bbox).to(dev), {"intrinsic": torch.from_numpy(intr).to(dev)})
    torch.cuda.synchronize()
    got = out["joints_cam"].cpu().numpy()
    rel = float(np.linalg.norm(got - ref["joints_cam"]) / np.linalg.norm(ref["joints_cam"]))
    frames = n * cfg.num_views
    cb = {"value": round(frames / el, 3), "unit": "frames/s", "cores": orc.num_threads, "kind": "port",
          "sample": f"{n} forwards of B=1 x V={cfg.num_views} x {size}x{size} ({frames} frames, {el:.1f} s) "
                    f"through oracle/hmv_oracle.c (fp32, OpenMP)"}
    try:   # the REAL reference (PyTorch CPU) timed in the build container on the same shape: it cannot travel to this box
        with open(os.path.join(ROOT, "profiles", "ref_pytorch_cpu.json")) as f:
            ref_cpu = json.load(f)
        key = f"{cfg.backbone_type}_B1_V{cfg.num_views}_{size}"
        if key in ref_cpu.get("shapes", {}):
            cb["reference_pytorch_cpu"] = dict(ref_cpu["shapes"][key], where=ref_cpu["where"], note=ref_cpu["note"])
    except (OSError, ValueError, KeyError):
        pass
    return cb, rel


def launch_command(n_ranks: int, argv, port: int):
    """The torchrun command line the parent uses to start `n_ranks` ranks of this script (one process per GPU)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def self_launch(n_ranks: int, argv) -> int:
    """`python bench.py --gpus N` with no torchrun around it: start the N ranks as CHILD processes (the parent has made no
    GPU call -- importing torch does not initialise HIP -- and never execs), relay rank 0's JSON line, return the
    children's status."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this pool (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", "1")
    proc = subprocess.Popen(launch_command(n_ranks, argv, port), stdout=subprocess.PIPE, text=True, env=env)
    for line in proc.stdout:          # rank 0 prints the one JSON line; anything else the children say goes to stderr
        line = line.rstrip("\n")
        is_json = False
        if line.startswith("{"):
            try:
                json.loads(line)
                is_json = True
            except ValueError:
                pass
        print(line, file=sys.stdout if is_json else sys.stderr, flush=True)
    return proc.wait()


def launch_check(world: int, rank: int):
    """--launch-check: the multi-rank control flow without the GPU work (CPU test of the launcher): rendezvous over gloo,
    one all-reduce, barrier, rank 0 prints the JSON line."""
    if os.environ.get("HMV_BENCH_FAIL_RANK") == str(rank):   # test hook: a dying rank must fail the whole launch
        raise SystemExit(3)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([float(rank + 1)], dtype=torch.float64)
        dist.all_reduce(t)
        dist.barrier()
        total = float(t.item())
        dist.destroy_process_group()
    else:
        total = 1.0
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "rank_sum": total}), flush=True)


def measure(args, world, rank, dev):
    """One workload in one arithmetic mode: W warm-up steps, K timed steps (barrier + synchronize on both sides, max over
    ranks), the last step's outputs to --dump-outputs, then (--full) the roofline of the dominant kernel family.  Returns
    (JSON line dict on rank 0 else None, context)."""
    bt, ch, V, B, size = WORKLOADS[args.workload]
    if args.batch:
        B = args.batch
    tp, mp, dp = params(bt, ch, V, B, size, args.fusion)
    cfg = config_from_params(tp, mp, dp)
    sd = synth_state_dict(cfg, 1)
    model = HandMvNet(tp, mp, dp)
    model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    model.freeze()
    if args.dtype == "f16":
        model.half()
    elif args.dtype == "f32x3":
        model.float32x3()

    # synthetic frames of this rank's shard, resident in HBM before the timed region
    x, bbox, intr = synth_inputs(cfg, B, 1000 + rank, size)
    xt, bt_, it = torch.from_numpy(x).to(dev), torch.from_numpy(bbox).to(dev), torch.from_numpy(intr).to(dev)
    cam = {"intrinsic": it}
    model.reserve(B, size, size, dev)

    if args.input == "frames":   # ho3d.py:26 camera resolution; windows like batch_center_scale_to_box makes them
        g = torch.Generator(device=dev).manual_seed(2000 + rank)
        raw = torch.randint(0, 256, (B, V, 480, 640, 3), dtype=torch.uint8, device=dev, generator=g)
        side = torch.randint(150, 400, (B, V, 1), device=dev, generator=g)
        org = torch.randint(-40, 300, (B, V, 2), device=dev, generator=g)
        crop_boxes = torch.cat([org, org + side], dim=-1).int()

    # one packed all-gather of (joints_cam | joints_crop_img) per step; its buffers exist before the timed loop
    gat = gatherer_for(B, V, dev) if world > 1 else None

    def step():
        out = model.forward_frames(raw, crop_boxes, cam, image_size=size) if args.input == "frames" else model(xt, bt_, cam)
        return gat.gather(out) if gat is not None else out

    for _ in range(args.warmup):
        step()
    if args.no_hr_fusion or args.hr_mode >= 0:   # A/B: HRNet fuse-layer fusion (bit 0) / branch overlap (bit 1) off (the engine exists after the first step)
        model.set_hr_fusion(0 if args.no_hr_fusion else args.hr_mode)
        step()
    if args.graphs:
        model.use_graphs(True)
    every = args.instrument_every if args.full else 0
    if args.full:
        model.set_profiling(True)      # fresh record list ...
        model.set_profiling(False)     # ... paused until an instrumented step resumes it
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    n_instr = 0
    for i in range(args.steps):
        instr = every > 0 and i % every == 0
        if instr:                      # hipEvent pairs around every conv/GEMM launch of this timed step
            model.set_profiling(2)
            n_instr += 1
        out = step()
        if instr:
            model.set_profiling(False)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if rank == 0 and args.dump_outputs:   # before anything else runs: gathered outputs are views of a reused buffer
        dump_outputs(out, args.dump_outputs)
    graph_stats = model.graph_stats()
    recs = []
    if args.full:
        if n_instr == 0:               # the roofline pass: same K steps, instrumented, not part of `value`
            model.set_profiling(2)
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            n_instr = args.steps
        recs = model.profile_records()
        model.set_profiling(False)
    launches = model.launch_count()
    # what the communicator itself saw: its size, and from every rank its device and its own clock over the timed steps
    props = torch.cuda.get_device_properties(dev)
    mine = {"rank": rank, "device": str(dev), "name": props.name, "uuid": str(getattr(props, "uuid", "")),
            "pci_bus_id": int(getattr(props, "pci_bus_id", -1)), "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "collectives": gat.collectives if gat is not None else 0}
    ranks = [mine]
    ranks_seen = 1
    if world > 1:
        ranks_seen = dist.get_world_size()
        ranks = [None] * ranks_seen
        dist.all_gather_object(ranks, mine)
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0 and args.full and args.per_layer:
        lay = {}
        for r in recs:
            e = lay.setdefault(r["layer"], {"kernel": r["kernel"], "ms": 0.0, "flops": r["flops"], "bytes": r["bytes"], "n": 0})
            e["ms"] += r["ms"]; e["n"] += 1
        rows = [{"layer": k, "kernel": v["kernel"], "avg_ms": v["ms"] / v["n"], "gflop": v["flops"] / 1e9,
                 "tflops": v["flops"] / (v["ms"] / v["n"] * 1e-3) / 1e12, "mbytes": v["bytes"] / 1e6,
                 "gbs": v["bytes"] / (v["ms"] / v["n"] * 1e-3) / 1e9} for k, v in lay.items()]
        with open(args.per_layer, "w") as f:
            json.dump(rows, f, indent=1)
    if rank != 0:
        return None, (cfg, sd, size, model)
    ms_step = elapsed / args.steps * 1e3
    line = {
        "metric": "samples/sec (BxV frames) eval_fps.py, 8-view 256x256; 21-kpt L2 vs reference",
        "value": round(args.steps * B * V * world / elapsed, 2), "unit": "frames/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": args.dtype,
        "data": "synthetic" if args.input == "nchw" else "synthetic uint8 480x640 frames + crop windows (prepared on the device)",
        "config": {"workload": f"{ {'cfg3': 'BASELINE configs[2]', 'cfg2': 'BASELINE configs[1]', 'cfg1': 'BASELINE configs[0] (HO3D_HandMvNet.yaml shape)'}.get(args.workload, 'HRNet release-config backbone') }: B={B}/GPU x V={V} x {size}x{size}, "
                               f"{'hrnet_' if cfg.is_hrnet else 'resnet'}{bt} backbone, d={cfg.feat_dim}, {args.fusion} x{cfg.fusion_layers}, GCN decoder",
                   "global_batch": B * world, "views": V, "frame": size, "parallelism": f"sample-shard x{world}"},
        "communicator": {"ranks_seen": ranks_seen, "backend": dist.get_backend() if world > 1 else None,
                         "distinct_devices": len({(r["uuid"], r["pci_bus_id"], r["device"]) for r in ranks}),
                         "collectives_per_step": (ranks[0]["collectives"] // max(args.warmup + args.steps + (args.steps if args.full and every == 0 else 0), 1)) if world > 1 else 0,
                         "ranks": ranks},
        "launches_per_forward": launches,
        "timed_region": {"instrumented_steps": n_instr if every > 0 else 0,
                         "note": "hipEvent pair around every conv/GEMM launch on the instrumented steps" if every > 0
                                 else "no events in the timed region; roofline from a separate instrumented pass of the same steps"
                                 if args.full else "no events in the timed region",
                         "hipgraph": {"enabled": bool(args.graphs), "cached": graph_stats[0], "replays": graph_stats[1]}},
    }
    if args.full:
        # ---- roofline of the dominant kernel family from the live per-launch event timings.  Each launch carries its
        # algorithmic FLOPs (2*M*N*K over the real channels) and algorithmic HBM bytes (input pixels, weights, residual and
        # output rows moved once in the mode's storage type); the family's bound is whichever floor is higher:
        # bytes / 8 TB/s (HBM) or FLOPs / the MFMA peak of the dtype it multiplies in (min(MFMA, HBM)).
        fam = {}
        for r in recs:
            f = fam.setdefault(r["kernel"], {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "n": 0})
            f["ms"] += r["ms"]; f["flops"] += r["flops"]; f["bytes"] += r["bytes"]; f["n"] += 1
        for k, v in fam.items():
            v["peak_tflops"] = PEAK_F16_MFMA_TFLOPS if "f16" in k else PEAK_F32_MFMA_TFLOPS
            mult = 3.0 if (args.dtype == "f32x3" and "f16" in k) else 1.0      # executed MFMA work per algorithmic FLOP
            v["t_mfma"] = mult * v["flops"] / (v["peak_tflops"] * 1e12)
            v["t_hbm"] = v["bytes"] / (PEAK_HBM_GBS * 1e9)
            v["bound"] = "hbm" if v["t_hbm"] > v["t_mfma"] else "mfma"
            v["frac"] = max(v["t_hbm"], v["t_mfma"]) / (v["ms"] * 1e-3)
        dom = max(fam, key=lambda k: fam[k]["ms"])
        d = fam[dom]
        traffic, traffic_src = None, None
        try:   # HBM bytes per launch of that kernel from the committed rocprofv3 PMC passes (tools/pmc_summary.py)
            with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
                pt = json.load(f)
            pt = pt.get(args.dtype, pt if "kernels" in pt else {})
            if dom in pt.get("kernels", {}) and args.workload == "cfg3" and B == 32 and pt.get("dtype", "f32") == args.dtype:
                traffic, traffic_src = round(pt["kernels"][dom]), pt["source"]
        except (OSError, ValueError, KeyError):
            pass
        if d["bound"] == "hbm":
            achieved, peak, unit = d["bytes"] / (d["ms"] * 1e-3) / 1e9, PEAK_HBM_GBS, "GB/s"
        else:
            achieved, peak, unit = d["flops"] / (d["ms"] * 1e-3) / 1e12, d["peak_tflops"], "TFLOP/s"
        roofline = {"bound": d["bound"], "kernel": dom, "achieved": round(achieved, 2), "peak": peak,
                    "unit": unit, "frac": round(achieved / peak, 4), "traffic": traffic,
                    "traffic_unit": "bytes/launch", "traffic_source": traffic_src,
                    "launches_per_step": d["n"] // max(n_instr, 1), "avg_launch_ms": round(d["ms"] / d["n"], 4),
                    "flops_per_launch": d["flops"] / d["n"], "bytes_per_launch": d["bytes"] / d["n"],
                    "floor_ms_per_launch": {"hbm@8TB/s": round(d["t_hbm"] / d["n"] * 1e3, 4),
                                            "mfma": round(d["t_mfma"] / d["n"] * 1e3, 4)}}
        if args.dtype == "f32x3" and "f16" in dom:   # three fp16 MFMAs per algorithmic multiply-add
            tf = d["flops"] / (d["ms"] * 1e-3) / 1e12
            roofline["executed_tflops"] = round(3 * tf, 2)
            roofline["executed_frac"] = round(3 * tf / d["peak_tflops"], 4)
            roofline["note"] = "algorithmic fp32 FLOPs; the fp16 matrix cores execute 3x that (hi*hi + lo*hi + hi*lo)"
        # dense algorithmic count for the ResNet workloads; for HRNet the executed FLOPs of the
        # conv/GEMM launches of one step (the engine's own 2*M*N*K accounting)
        total_flops = (sum(r["flops"] for r in recs) / max(n_instr, 1) if (cfg.is_hrnet or cfg.learnable_query)
                       else forward_flops(cfg, B, size))
        line["roofline"] = roofline
        line["forward"] = forward_block(args.dtype, total_flops, ms_step, fam, n_instr)
        line["kernels"] = {k: {"ms_per_step": round(v["ms"] / n_instr, 3), "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2),
                               "gbs": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1), "bound": v["bound"], "frac": round(v["frac"], 4)}
                           for k, v in fam.items()}
    return line, (cfg, sd, size, model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="cfg3", choices=list(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="override samples per GPU")
    ap.add_argument("--fusion", default="cross_attn", choices=["cross_attn", "cross_attn_learnable_query"],
                    help="model.fusion (every release config: cross_attn; the learnable-query module is SURVEY 8(f) row 2)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16", "f32x3"],
                    help="f16 = BASELINE configs[4] (fp16 conv stack); f32x3 = fp32-equivalent (hi, lo) fp16 pairs, three fp16 MFMAs per "
                         "product (HMV_F32X3, ResNet50-paper)")
    ap.add_argument("--input", default="nchw", choices=["nchw", "frames"],
                    help="nchw = prepared fp32 batch (eval_fps.py protocol, the headline); frames = raw uint8 480x640 camera "
                         "frames + crop windows through hmv_forward_frames (SURVEY 8(f) row 4)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline / per-kernel figures from hipEvent-timed "
                         "launches, the CPU oracle baseline and parity check, the fp16 (BASELINE configs[4]) leg")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's outputs as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--instrument-every", type=int, default=None,
                    help="--full: bracket every conv/GEMM launch with a hipEvent pair on every Nth timed step (default 4; N=1: "
                         "every step; the events cost ~0.5 ms per instrumented cfg-3 step); 0: none in the timed region, "
                         "roofline from a separate instrumented pass afterwards")
    ap.add_argument("--graphs", action="store_true", help="opt into hipGraph replay for the un-instrumented steps")
    ap.add_argument("--per-layer", default="", help="--full: write per-layer launch timings (JSON) to this file")
    ap.add_argument("--no-hr-fusion", action="store_true", help="A/B: HRNet fuse layers as one conv launch per term, one stream")
    ap.add_argument("--hr-mode", type=int, default=-1, help="A/B: hmv_set_hr_fusion mode (bit 0: fused fuse layers, bit 1: branch overlap)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the fp16 (BASELINE configs[4]) leg that a --full run appends as `configs4_fp16`")
    ap.add_argument("--launch-check", action="store_true",
                    help="only exercise the rank launch / rendezvous / relay path (gloo, no GPU work): CPU test of --gpus N")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full and (args.per_layer or args.instrument_every is not None):
        ap.error("--per-layer and --instrument-every need --full")
    if args.instrument_every is None:
        args.instrument_every = 4

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # not under torchrun: this process becomes the launcher.  Nothing here has touched the GPU yet.
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE={world}")
    if args.launch_check:
        launch_check(world, rank)
        return
    # rehearsal switches for a one-GPU box: HMV_BENCH_SAME_DEVICE=1 maps every rank to cuda:0 and
    # HMV_BENCH_BACKEND=gloo replaces RCCL (which refuses two ranks on one GPU); never set by the driver
    same_dev = os.environ.get("HMV_BENCH_SAME_DEVICE") == "1"
    backend = os.environ.get("HMV_BENCH_BACKEND", "nccl")
    dev = torch.device("cuda:0" if same_dev else f"cuda:{local_rank}")
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    line, (cfg, sd, size, model) = measure(args, world, rank, dev)
    if rank == 0 and args.full:
        if world == 1 and not args.no_cpu_baseline:
            cb, rel = cpu_baseline(cfg, sd, size, model, dev, args.cpu_seconds)
            line["cpu_baseline"] = cb
            line["parity_rel_l2_vs_oracle"] = float(f"{rel:.3e}")
        else:
            line["cpu_baseline"] = None
        # BASELINE configs[4] (the fp16 path) in the same --full run, so that the record of `python bench.py --full` carries a
        # number for it too: same workload, same K / W, no events in its timed region.  Not `value`.
        if (world == 1 and args.dtype == "f32" and args.workload == "cfg3" and not args.batch and args.input == "nchw"
                and not args.no_cpu_baseline and not args.no_secondary):
            a2 = argparse.Namespace(**vars(args))
            a2.dtype, a2.per_layer, a2.instrument_every, a2.dump_outputs = "f16", "", 0, ""
            x1, b1, i1 = synth_inputs(cfg, 1, 4242, size)
            probe = (torch.from_numpy(x1).to(dev), torch.from_numpy(b1).to(dev), {"intrinsic": torch.from_numpy(i1).to(dev)})
            ref32 = model(*probe)["joints_cam"].float().cpu().numpy()
            l2, (_, _, _, m16) = measure(a2, world, rank, dev)
            got16 = m16(*probe)["joints_cam"].float().cpu().numpy()
            sec = {k: l2[k] for k in ("value", "unit", "ms_per_step", "dtype", "steps", "warmup", "roofline", "forward", "timed_region")}
            sec["joints_cam_rel_l2_vs_fp32_engine"] = float(f"{np.linalg.norm(got16 - ref32) / np.linalg.norm(ref32):.3e}")
            try:   # the fp16-STORAGE noise floor of this shape measured on the real reference (tests/golden/make_fp16_noise.py)
                with open(os.path.join(ROOT, "tests", "golden", "fp16_noise.json")) as f:
                    fl = json.load(f)["cases"]["cfg3s_r50_v8_256"]
                sec["reference_fp16_storage_noise_floor"] = {"joints_cam_rel_l2": float(f"{fl['joints_cam_rel_l2']:.3e}"),
                                                             "coord_flip_frac": float(f"{fl['coord_flip_frac']:.3e}")}
            except (OSError, ValueError, KeyError):
                pass
            sec["note"] = ("BASELINE configs[4]: conv stack in fp16 storage + fp16 MFMA, fp32 accumulation.  Its error is that of fp16 "
                           "STORAGE (x1000 soft-argmax flips near-tied heat-map peaks): the reference itself, with only its activations "
                           "rounded to fp16, lands the noise floor above away from its fp32 run; tests hold the engine to 3x that floor "
                           "(DESIGN.md section 4, tests/test_gpu_parity.py)")
            line["configs4_fp16"] = sec
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
