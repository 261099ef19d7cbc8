"""Generate tests/golden/orders_cases.npz from the REAL reference (run in the build container only, like make_views_fixture.py).

    python tests/golden/make_orders_fixture.py

For every case of orders_cases.py: the views_cases.py case's synthetic state_dict and full-view input batch, and per order the
reference built with num_views = len(order), run on the whole batch with its views permuted by that order -- x[:, order],
bbox[:, order], intrinsic[:, order].  Stored per order: joints_cam, joints_crop_img, heatmap.
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
from orders_cases import ORDERS_CASES  # noqa: E402
from views_cases import VIEWS_CASES  # noqa: E402
from handmvnet_amd.spec import config_from_params  # noqa: E402
from handmvnet_amd.synth import synth_inputs, synth_state_dict  # noqa: E402


def run_case(name: str, orders) -> dict:
    spec = VIEWS_CASES[name]
    full = {k: v for k, v in spec.items() if k != "views"}
    cfg = config_from_params(*case_params(full))
    sd = synth_state_dict(cfg, spec["wseed"])
    x, bbox, intr = synth_inputs(cfg, spec["B"], spec["iseed"], spec["size"])
    fx = {name + "/orders": np.array(json.dumps(orders))}
    for s, order in enumerate(orders):
        tp, mp, dp = case_params(dict(full, V=len(order)))
        sd_s = synth_state_dict(config_from_params(tp, mp, dp), spec["wseed"])
        assert list(sd_s) == list(sd) and all(np.array_equal(sd_s[k], sd[k]) for k in sd), "the weights depend on the view count"
        model = ref_harness.build_reference_model(tp, mp, dp, sd)
        with torch.no_grad():
            out = model(torch.from_numpy(x[:, order].copy()), torch.from_numpy(bbox[:, order].copy()),
                        {"intrinsic": torch.from_numpy(intr[:, order].copy())})
        for k in ("joints_cam", "joints_crop_img", "heatmap"):
            fx[f"{name}/{s}/{k}"] = out[k].numpy().astype(np.float32)
        print(f"{name} order {s}: {order}  joints_cam |max| {np.abs(fx[f'{name}/{s}/joints_cam']).max():.4f}")
    return fx


if __name__ == "__main__":
    torch.set_num_threads(8)
    fx = {}
    for name, orders in ORDERS_CASES.items():
        fx.update(run_case(name, orders))
    np.savez_compressed(os.path.join(HERE, "orders_cases.npz"), **fx)
