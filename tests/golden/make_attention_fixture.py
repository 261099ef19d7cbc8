"""Generate tests/golden/attention_cases.npz from the REAL reference (run in the build container only).

    python tests/golden/make_attention_fixture.py

For every case below the script builds the reference's HandMvNet (ref_harness.build_reference_model) with the synthesised weights of
cases.py, runs its forward on the synthesised inputs, takes the fusion module's input with a forward pre-hook, and walks
`joints_late_fusion.attn_fusion` layer by layer with return_attention=True (layers.py:202-237, 267-301) -- once as the module stands
(fp32) and once on a .double() copy -- on the FIRST sample of the case's batch (the fusion treats samples independently; the file
stays below the largest committed fixture that way).  Stored per case: that sample's tokens, the reference's fp32 maps of the listed blocks, every block's shape,
and per block the scalar n32 = max |p32 - p64|, the reference's own distance from its float64 run.  Data only: weights and inputs are
regenerated from the seeds of cases.py.
"""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import torch  # noqa: E402

import ref_harness  # noqa: E402
from cases import CASES, case_params  # noqa: E402
from handmvnet_amd.attention import cross_block_index  # noqa: E402
from handmvnet_amd.spec import config_from_params  # noqa: E402
from handmvnet_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

# case -> the blocks whose maps are stored: "all", "cross" (the cross block only), or a list of indices
ATTENTION_CASES = {
    "tiny_r18": "all",
    "r18_frozen_nosin": "all",          # 3 blocks; the cross block is block 1
    "r18_lq_wocam": "all",
    "r50_wocam_nn": "cross",
    "r50_lq": "cross",
    "cfg1_r50_v4_128": "cross",
    "r18_single_view": [0],             # one view: the cross block has no keys; its (empty) shape is stored like every block's
}
OUT = os.path.join(HERE, "attention_cases.npz")


def walk(fusion, tokens, add_pos):
    """The fusion module layer by layer: every block's attn."""
    x = tokens
    if add_pos and hasattr(fusion, "pos_encoding"):
        x = fusion.pos_encoding(x)
    maps = []
    for layer in fusion.attn_fusion:
        x, attn = layer(x, return_attention=True)
        maps.append(attn)
    return maps, x


def run_case(name: str, which) -> dict:
    spec = CASES[name]
    tp, mp, dp = case_params(spec)
    cfg = config_from_params(tp, mp, dp)
    sd = synth_state_dict(cfg, spec["wseed"])
    model = ref_harness.build_reference_model(tp, mp, dp, sd)
    x, bbox, intr = synth_inputs(cfg, spec["B"], spec["iseed"], spec["size"])
    got = {}
    hook = model.joints_late_fusion.register_forward_pre_hook(lambda m, i: got.__setitem__("tokens", i[0].detach().clone()))
    try:
        with torch.no_grad():
            model(torch.from_numpy(x), torch.from_numpy(bbox), {"intrinsic": torch.from_numpy(intr)})
    finally:
        hook.remove()
    tokens = got["tokens"][:1].clone()   # the first sample: the fusion treats samples independently, and the file has a size limit
    fusion = model.joints_late_fusion
    add_pos = bool(getattr(model, "sinusoidal_pos", "sin" in mp["pos_enc"]))
    with torch.no_grad():
        maps32, fused32 = walk(fusion, tokens, add_pos)
        maps64, _ = walk(copy.deepcopy(fusion).double(), tokens.double(), add_pos)
    cross = cross_block_index(mp)
    keep = list(range(len(maps32))) if which == "all" else ([cross] if which == "cross" else list(which))
    fx = {f"{name}.spec": np.array(json.dumps(spec)), f"{name}.tokens": tokens.numpy(), f"{name}.blocks": np.array(keep, dtype=np.int64),
          f"{name}.shapes": np.array([list(m.shape) for m in maps32], dtype=np.int64),
          f"{name}.n32": np.array([float((a.double() - b).abs().max()) if a.numel() else 0.0 for a, b in zip(maps32, maps64)])}
    for l in keep:
        fx[f"{name}.attn{l}"] = maps32[l].numpy()
    print(f"{name}: blocks {len(maps32)}, cross {cross}, stored {keep}, n32 " + " ".join(f"{v:.1e}" for v in fx[f'{name}.n32']))
    return fx


def main():
    if not ref_harness.reference_available():
        raise SystemExit("the reference is not available here")
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    fx = {}
    for name, which in ATTENTION_CASES.items():
        fx.update(run_case(name, which))
    np.savez_compressed(OUT, **fx)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
