"""Reference-view sweep cases shared by make_orders_fixture.py and the tests (data only).

A case names a ragged view-set case of views_cases.py (its model, weights and FULL-view input batch) and a few camera orders; the fixture
holds, per order, what the reference built with num_views = len(order) computes from the whole batch with its views permuted by that
order, x[:, order]."""
from __future__ import annotations

ORDERS_CASES = {
    # cross_attn: an unsorted three-camera order, the reversed rig, one camera, an unsorted five-camera order
    "views_r18_v7": [[3, 0, 6], [6, 5, 4, 3, 2, 1, 0], [2], [1, 4, 0, 5, 2]],
    # the learnable-query fusion
    "views_r50_lq_v3": [[2, 0, 1], [1], [2, 0], [0, 1, 2]],
}
