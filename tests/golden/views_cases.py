"""Ragged view-set cases shared by make_views_fixture.py and the tests (data only).

A case is a cases.py-style model configuration with `V` cameras plus, per sample, the cameras that are present (`views`, in camera
order).  Weights and the FULL-view input batch are regenerated from the two seeds (handmvnet_amd.synth: tensors are keyed by name and
seed, never by the view count); the fixture holds, per sample, what the reference built with num_views = len(views[b]) computes from
that sample's present views.
"""
from __future__ import annotations

from cases import ALL_POS

VIEWS_CASES = {
    # counts 7, 1, 2, 3, 5 -- token ranges 147 (five 32-key chunks: one wave takes two), 21 (NO keys in the cross block), 42 (two
    # chunks, one partial; 21 cross keys), 63 and 105 (idle waves); none of the partial sets is a prefix of the cameras
    "views_r18_v7": dict(bt="18", ch=[256, 128, 64], V=7, B=5, size=64, pos=ALL_POS, gcn=True, wseed=41, iseed=51,
                         views=[[0, 1, 2, 3, 4, 5, 6], [4], [1, 5], [0, 3, 6], [0, 2, 3, 5, 6]]),
    # the learnable-query fusion (the generator calls the module as ref_harness.py does for r50_lq)
    "views_r50_lq_v3": dict(bt="50_paper", ch=[1024], V=3, B=3, size=64, pos=ALL_POS, gcn=True, wseed=42, iseed=52,
                            fusion="cross_attn_learnable_query", views=[[0, 1, 2], [2], [0, 2]]),
}


def sample_spec(spec: dict, b: int) -> dict:
    """The cases.py-style spec of the model that sample b's result is defined by: num_views = its number of present views, batch 1."""
    s = {k: v for k, v in spec.items() if k != "views"}
    s.update(V=len(spec["views"][b]), B=1)
    return s


def view_mask(spec: dict):
    """bool [B][V] nested list, True = present."""
    return [[v in views for v in range(spec["V"])] for views in spec["views"]]
