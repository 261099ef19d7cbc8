"""Shared by the ragged view-set tests (test_views_cpu.py, test_gpu_views.py): the cases of golden/views_cases.py with their
fixture, and the f64 oracle per sample -- computed once per process and handed out unchanged."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from cases import case_params
from helpers import GOLDEN
from views_cases import VIEWS_CASES, sample_spec, view_mask
from handmvnet_amd.spec import config_from_params
from handmvnet_amd.synth import synth_inputs, synth_state_dict

OUT_KEYS = ("joints_cam", "joints_crop_img", "heatmap")


@functools.lru_cache(maxsize=None)
def load_views_case(name: str) -> dict:
    """spec, params / cfg / weights of the full-view model, the full-view inputs, the mask and per sample: the present cameras, the
    params of the model that defines its result, and a helpers.check_against_fixture-style fixture dict."""
    spec = VIEWS_CASES[name]
    z = np.load(os.path.join(GOLDEN, "views_cases.npz"), allow_pickle=False)
    assert json.loads(str(z[name + "/spec"])) == json.loads(json.dumps(spec)), "fixture is stale: regenerate with make_views_fixture.py"
    full = {k: v for k, v in spec.items() if k != "views"}
    params = case_params(full)
    cfg = config_from_params(*params)
    samples = []
    for b, views in enumerate(spec["views"]):
        hm = z[f"{name}/{b}/heatmap"]
        fx = {"joints_cam": z[f"{name}/{b}/joints_cam"], "joints_crop_img": z[f"{name}/{b}/joints_crop_img"], "heatmap": hm,
              "heatmap_idx": np.arange(hm.size), "heatmap_val": hm.reshape(-1), "heatmap_shape": np.array(hm.shape)}
        p = case_params(sample_spec(spec, b))
        samples.append({"views": list(views), "params": p, "cfg": config_from_params(*p), "fx": fx})
    return {"spec": spec, "params": params, "cfg": cfg, "sd": synth_state_dict(cfg, spec["wseed"]),
            "inputs": synth_inputs(cfg, spec["B"], spec["iseed"], spec["size"]), "mask": np.array(view_mask(spec), dtype=bool),
            "samples": samples}


def sample_inputs(case: dict, b: int):
    """Sample b's present views as a batch of one for the model with num_views = its view count."""
    v = case["samples"][b]["views"]
    return tuple(a[b:b + 1, v] for a in case["inputs"])


@functools.lru_cache(maxsize=None)
def oracle_per_sample(name: str):
    """Per sample, the f64 oracle built with num_views = that sample's count on its present views (read-only dicts)."""
    from oracle.oracle import Oracle
    case = load_views_case(name)
    outs = []
    for b, s in enumerate(case["samples"]):
        o = Oracle(s["cfg"], case["sd"], "f64").forward(*sample_inputs(case, b))
        for a in o.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        outs.append(o)
    return outs


def per_sample(out: dict, case: dict, b: int) -> dict:
    """Sample b of a full-shape result dict (numpy) in the shapes of its own model: present views only, batch 1."""
    v = case["samples"][b]["views"]
    return {"joints_cam": out["joints_cam"][b:b + 1], "joints_crop_img": out["joints_crop_img"][b:b + 1, v],
            "heatmap": out["heatmap"][b:b + 1, v]}
