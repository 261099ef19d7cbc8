#!/usr/bin/env python3
"""The launch ledger: which kernel the engine runs for every conv / GEMM launch of the benchmarked forwards, and the FLOPs and
bytes that launch reports about itself (needs an MI355X; reads the engine's own profiling records, nothing else).

For every workload bench.py publishes numbers for -- cfg1, cfg2, cfg3, hr40 at their B, V and frame size, restated below as data
so that no test depends on bench.py internals -- plus the batch-1, 8-view r50 shape of profiles/r04_bench_b1.json, and for each
arithmetic mode (f32, f16, f32x3), it builds the model on synthetic weights, runs ONE eager profiled forward and records the
ordered list of {layer, kernel, flops, bytes} (HandMvNet.profile_records()), and under "plans" the workspace plan of that
forward: the bytes reserve() sizes for its batch and the device operations the forward enqueued (launch_count()).

tests/test_gpu_launch_ledger.py holds every later build to this list: a forward whose (layer, kernel) sequence, workspace bytes or launch count differs
fails.  A
DELIBERATE routing change regenerates the ledger with this script and comes with a measurement that justifies it; the ledger is
always generated from the library of the commit BEFORE the change under test, never from the tree a test is about to judge.

    python tests/golden/make_launch_ledger.py                  # writes tests/golden/launch_ledger.json
    python tests/golden/make_launch_ledger.py cfg3 hr40        # these workloads only, merged into the existing file
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for q in (ROOT, HERE):
    if q not in sys.path:
        sys.path.insert(0, q)

LEDGER = os.path.join(HERE, "launch_ledger.json")
MODES = ("f32", "f16", "f32x3")
WSEED, ISEED = 1, 1000   # synthetic weights / frames: routing, FLOPs and bytes depend on neither
# name: backbone_type, backbone_channels, views, samples per forward, frame size
WORKLOADS = {
    "cfg1": {"backbone_type": "50_paper", "channels": [1024], "V": 4, "B": 1, "size": 128},
    "cfg2": {"backbone_type": "18", "channels": [256, 128, 64], "V": 4, "B": 8, "size": 256},
    "cfg3": {"backbone_type": "50_paper", "channels": [1024], "V": 8, "B": 32, "size": 256},
    "hr40": {"backbone_type": "w40", "channels": [40, 80, 160, 320], "V": 8, "B": 32, "size": 256},
    "cfg3_b1": {"backbone_type": "50_paper", "channels": [1024], "V": 8, "B": 1, "size": 256},
}


def workload_params(w):
    """The reference's three constructor dicts for a workload row (cross_attn x 5, GCN decoder, pos2d + crop + sin)."""
    bt = w["backbone_type"]
    tp = {"debug": False, "root_relative": True}
    mp = {"num_views": w["V"], "backbone": "hrnet" if bt.startswith("w") else "resnet", "backbone_type": bt,
          "backbone_channels": list(w["channels"]), "backbone_pretrained": False, "backbone_early_return": 3,
          "pos_enc": ["pos2d", "crop", "sin"], "fusion": "cross_attn", "fusion_layers": 5, "use_gcn": True}
    dp = {"batch_size": w["B"], "image_size": w["size"], "heatmap_size": w["size"] // 8, "name": "dexycb"}
    return tp, mp, dp


def profiled_forward(w, mode):
    """-> (model, cfg, state_dict, records, plan) of ONE eager profiled forward of workload row `w` in `mode`; plan =
    {"workspace_bytes": what reserve() sizes for the batch, "launches": device operations the forward enqueued}."""
    import torch
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.spec import config_from_params
    from handmvnet_amd.synth import synth_inputs, synth_state_dict
    tp, mp, dp = workload_params(w)
    cfg = config_from_params(tp, mp, dp)
    sd = synth_state_dict(cfg, WSEED)
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    if mode == "f16":
        m.half()
    elif mode == "f32x3":
        m.float32x3()
    dev = torch.device("cuda:0")
    x, bbox, intr = synth_inputs(cfg, w["B"], ISEED, w["size"])
    xt, bt, it = torch.from_numpy(x).to(dev), torch.from_numpy(bbox).to(dev), torch.from_numpy(intr).to(dev)
    m.use_graphs(False)
    m.set_profiling(True)
    out = m(xt, bt, {"intrinsic": it})
    torch.cuda.synchronize()
    recs = m.profile_records()
    plan = {"launches": m.launch_count()}
    m.set_profiling(False)
    plan["workspace_bytes"] = m.reserve(w["B"], w["size"], w["size"])
    assert torch.isfinite(out["joints_cam"]).all()
    return m, cfg, sd, recs, {k: plan[k] for k in ("workspace_bytes", "launches")}


def main():
    import torch
    from handmvnet_amd import _lib
    only = set(sys.argv[1:])
    led = {"what": "per workload and arithmetic mode: the ordered conv / GEMM launches of one eager forward "
                   "(tests/golden/make_launch_ledger.py)", "workloads": WORKLOADS, "forwards": {}, "plans": {}}
    if only:
        with open(LEDGER) as f:
            old = json.load(f)
        led["forwards"], led["plans"] = old["forwards"], old.get("plans", {})
    led["library"] = _lib.load().hmv_version().decode()
    for name, w in WORKLOADS.items():
        if only and name not in only:
            continue
        for mode in MODES:
            m, _, _, recs, plan = profiled_forward(w, mode)
            led["plans"].setdefault(name, {})[mode] = plan
            led["forwards"].setdefault(name, {})[mode] = [{"layer": r["layer"], "kernel": r["kernel"], "flops": r["flops"],
                                                            "bytes": r["bytes"]} for r in recs]
            print(name, mode, len(recs), "launches", flush=True)
            del m
            torch.cuda.empty_cache()
    with open(LEDGER, "w") as f:
        f.write("{\n")
        f.write(' "what": %s,\n "library": %s,\n "workloads": %s,\n "forwards": {\n' % (
            json.dumps(led["what"]), json.dumps(led["library"]), json.dumps(led["workloads"])))
        names = list(led["forwards"])
        for i, name in enumerate(names):
            f.write('  %s: {\n' % json.dumps(name))
            modes = list(led["forwards"][name])
            for j, mode in enumerate(modes):
                rows = ",\n".join("    " + json.dumps(r) for r in led["forwards"][name][mode])
                f.write('   %s: [\n%s\n   ]%s\n' % (json.dumps(mode), rows, "," if j + 1 < len(modes) else ""))
            f.write("  }%s\n" % ("," if i + 1 < len(names) else ""))
        f.write(' },\n "plans": {\n%s\n }\n}\n' % ",\n".join("  %s: %s" % (json.dumps(n), json.dumps(p)) for n, p in led["plans"].items()))


if __name__ == "__main__":
    main()
