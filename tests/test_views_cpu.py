"""Ragged view sets, the part that needs no GPU: the entry is exported, the weights really carry across view counts (the oracle built
with num_views = v_b reproduces the reference built with num_views = v_b from ONE state_dict), and forward_views' argument checks."""
import numpy as np
import pytest
import torch

from helpers import check_against_fixture
from views_cases import VIEWS_CASES
from views_helpers import load_views_case, oracle_per_sample


def test_forward_views_is_exported():
    from handmvnet_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "hmv_forward_views") and hasattr(lib, "hmv_op_attention_views")
    assert "hmv_forward_views" in _lib.SYMBOLS


@pytest.mark.parametrize("name", list(VIEWS_CASES))
def test_oracle_with_the_samples_view_count_matches_the_reference(name):
    """One state_dict, the model rebuilt with num_views = each sample's count: the f64 oracle against the real reference's outputs
    at the bars of test_oracle_golden.py (joints_cam 3e-4 rel-L2, coordinates 0.05 px, heat map 1e-4 rel-L2)."""
    case = load_views_case(name)
    for b, (s, o) in enumerate(zip(case["samples"], oracle_per_sample(name))):
        rep = check_against_fixture(o, s["fx"], tol_cam=3e-4, tol_coord_px=0.05, tol_stage=1e-4)
        print(name, b, s["views"], rep)


def _model():
    from handmvnet_amd import HandMvNet
    return HandMvNet(*load_views_case("views_r18_v7")["params"])


def test_forward_views_argument_checks():
    from handmvnet_amd import _lib
    m = _model()
    x = torch.zeros(2, 7, 3, 64, 64)
    full = np.ones((2, 7), dtype=bool)
    with pytest.raises(ValueError, match="view_mask must have shape"):
        m.forward_views(x, np.ones((2, 6), dtype=bool))
    with pytest.raises(ValueError, match="view_mask must have shape"):
        m.forward_views(x, [True] * 7)
    none = full.copy()
    none[1] = False
    for mask in (none, torch.from_numpy(none), none.tolist()):
        with pytest.raises(ValueError, match="at least one present view.*sample 1"):
            m.forward_views(x, mask)
    with pytest.raises(ValueError, match="all 7 views"):
        m.forward_views(torch.zeros(2, 5, 3, 64, 64), np.ones((2, 5), dtype=bool))
    with pytest.raises(ValueError, match=r"\[b, v, 3, h, w\]"):
        m.forward_views(torch.zeros(14, 3, 64, 64), full)
    with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
        m.forward_views(x, full)
