"""Generate tests/golden/views_cases.npz from the REAL reference (run in the build container only, like make_fixtures.py).

    python tests/golden/make_views_fixture.py

For every case of views_cases.py: ONE synthetic state_dict (handmvnet_amd.synth keys its tensors by name and seed, not by the view
count -- asserted below), the full-view input batch, and per sample the reference built with num_views = that sample's number of
present views, run on the sample's present views in camera order.  Stored per sample: joints_cam, joints_crop_img, heatmap.
"""
from __future__ import annotations

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
from cases import case_params  # noqa: E402
from views_cases import VIEWS_CASES, sample_spec  # noqa: E402
from handmvnet_amd.spec import config_from_params  # noqa: E402
from handmvnet_amd.synth import synth_inputs, synth_state_dict  # noqa: E402


def run_case(name: str, spec: dict) -> dict:
    full = {k: v for k, v in spec.items() if k != "views"}
    cfg = config_from_params(*case_params(full))
    sd = synth_state_dict(cfg, spec["wseed"])
    x, bbox, intr = synth_inputs(cfg, spec["B"], spec["iseed"], spec["size"])
    fx = {name + "/spec": np.array(json.dumps(spec))}
    for b, views in enumerate(spec["views"]):
        tp, mp, dp = case_params(sample_spec(spec, b))
        sd_b = synth_state_dict(config_from_params(tp, mp, dp), spec["wseed"])
        assert list(sd_b) == list(sd) and all(np.array_equal(sd_b[k], sd[k]) for k in sd), "the weights depend on the view count"
        model = ref_harness.build_reference_model(tp, mp, dp, sd)
        with torch.no_grad():
            out = model(torch.from_numpy(x[b:b + 1, views].copy()), torch.from_numpy(bbox[b:b + 1, views].copy()),
                        {"intrinsic": torch.from_numpy(intr[b:b + 1, views].copy())})
        for k in ("joints_cam", "joints_crop_img", "heatmap"):
            fx[f"{name}/{b}/{k}"] = out[k].numpy().astype(np.float32)
        print(f"{name} sample {b}: views {views}  joints_cam |max| {np.abs(fx[f'{name}/{b}/joints_cam']).max():.4f}")
    return fx


if __name__ == "__main__":
    torch.set_num_threads(8)
    fx = {}
    for name, spec in VIEWS_CASES.items():
        fx.update(run_case(name, spec))
    np.savez_compressed(os.path.join(HERE, "views_cases.npz"), **fx)
