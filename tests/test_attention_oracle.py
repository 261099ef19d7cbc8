"""Attention maps without a GPU: the torch oracle (tests/attention_oracle.py) against the maps of the REAL reference
(tests/golden/attention_cases.npz, written by tests/golden/make_attention_fixture.py), the per-camera helpers of
handmvnet_amd/attention.py on CPU tensors, and the argument checks of the new C entries that happen before any HIP call."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import attention_oracle as ao
from cases import CASES, case_params
from handmvnet_amd import _lib
from handmvnet_amd.attention import ViewAttentionMeter, cross_block_index, share_to_cameras
from handmvnet_amd.spec import config_from_params
from handmvnet_amd.synth import synth_state_dict

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_cases.npz"), allow_pickle=False)
NAMES = sorted({k.split(".")[0] for k in FIX.files})


def _case(name):
    spec = json.loads(str(FIX[f"{name}.spec"]))
    assert spec == json.loads(json.dumps(CASES[name])), "fixture is stale: regenerate with make_attention_fixture.py"
    tp, mp, dp = case_params(spec)
    cfg = config_from_params(tp, mp, dp)
    return cfg, mp, synth_state_dict(cfg, spec["wseed"])


def test_fixture_holds_the_cases_and_stays_small():
    assert NAMES == sorted(["tiny_r18", "r18_frozen_nosin", "r18_lq_wocam", "r50_wocam_nn", "r50_lq", "cfg1_r50_v4_128", "r18_single_view"])
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(golden, "attention_cases.npz")) <= os.path.getsize(os.path.join(golden, "frames_cases.npz"))
    assert [int(l) for l in FIX["tiny_r18.blocks"]] == [0, 1, 2, 3, 4]
    assert [int(l) for l in FIX["r18_frozen_nosin.blocks"]] == [0, 1, 2]
    assert [int(l) for l in FIX["r50_lq.blocks"]] == [2]
    assert list(FIX["r18_single_view.shapes"][2]) == [1, 8, 21, 0]      # one view: the cross block has no keys


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_maps(name):
    """The float64 oracle on the fixture's tokens against the reference's fp32 maps.  The oracle equals the reference's own float64 run up
    to float64 rounding, and n32 is the reference's own distance from that run: the bar per block is n32 + 1e-10."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg, mp, sd = _case(name)
    maps, _ = ao.fusion_attention(FIX[f"{name}.tokens"], sd, cfg, torch.float64)
    shapes = FIX[f"{name}.shapes"]
    assert len(maps) == len(shapes) and all(list(m.shape) == list(s) for m, s in zip(maps, shapes))
    for l in FIX[f"{name}.blocks"]:
        ref = torch.from_numpy(FIX[f"{name}.attn{int(l)}"]).double()
        err = float((maps[int(l)] - ref).abs().max())
        bar = float(FIX[f"{name}.n32"][int(l)]) + 1e-10
        print(name, int(l), err, bar)
        assert err <= bar, (name, int(l), err, bar)
    # the share of the oracle's maps: per view, the sum over its 21 keys
    cx = cross_block_index(mp)
    for l in range(cx + 1):
        m = maps[l]
        if m.shape[-1] == 0:
            continue
        sh = ao.view_share(m)
        assert torch.equal(sh, m.reshape(*m.shape[:3], m.shape[-1] // 21, 21).sum(-1))
        assert float((sh.sum(-1) - 1).abs().max()) < 1e-12


def test_oracle_runs_in_fp32_too():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg, mp, sd = _case("tiny_r18")
    m64, _ = ao.fusion_attention(FIX["tiny_r18.tokens"], sd, cfg, torch.float64)
    m32, _ = ao.fusion_attention(FIX["tiny_r18.tokens"], sd, cfg, torch.float32)
    assert all(m.dtype == torch.float32 for m in m32)
    assert max(float((a.double() - b).abs().max()) for a, b in zip(m32, m64)) < 1e-5


def test_cross_block_index():
    assert cross_block_index({"fusion": "cross_attn", "fusion_layers": 5}) == 2
    assert cross_block_index({"fusion": "cross_attn", "fusion_layers": 3}) == 1
    assert cross_block_index({"fusion": "cross_attn", "fusion_layers": 1}) == 0
    assert cross_block_index({"fusion": "cross_attn"}) == 2
    assert cross_block_index({"fusion": "cross_attn_learnable_query", "fusion_layers": 3}) == 2
    with pytest.raises(ValueError):
        cross_block_index({"fusion": "cross_attn", "fusion_layers": 4})


def test_share_to_cameras():
    g = torch.Generator().manual_seed(3)
    share = torch.rand(2, 8, 21, 3, generator=g)
    share[0, :, :, 2] = 0                                     # sample 0 has two present views
    mask = [[False, True, False, True], [True, True, False, True]]
    cam = share_to_cameras(share, mask)
    assert cam.shape == (2, 8, 21, 4)
    assert torch.equal(cam[0, :, :, 1], share[0, :, :, 0]) and torch.equal(cam[0, :, :, 3], share[0, :, :, 1])
    assert torch.equal(cam[1, :, :, 0], share[1, :, :, 0]) and torch.equal(cam[1, :, :, 1], share[1, :, :, 1])
    assert torch.equal(cam[1, :, :, 3], share[1, :, :, 2])
    assert float(cam[0, :, :, 0].abs().max()) == 0 and float(cam[:, :, :, 2].abs().max()) == 0
    assert torch.equal(share_to_cameras(share, torch.tensor(mask)), cam)
    full = share_to_cameras(share, None)
    assert torch.equal(full, share)
    assert share_to_cameras(share, None, num_views=5).shape == (2, 8, 21, 5)
    with pytest.raises(ValueError):
        share_to_cameras(share, [[True, True, True, True], [True, False, False, False]])


def test_view_attention_meter():
    V = 3
    a = torch.zeros(2, 21, V)
    a[0, :, 1], a[0, :, 2] = 0.25, 0.75                       # sample 0: all cameras, camera 0 supplies the queries
    a[1, :, 2] = 1.0                                          # sample 1: cameras 1 and 2, camera 1 supplies the queries
    meter = ViewAttentionMeter(V)
    meter.add({"view_attention": a[:1]})
    meter.add({"view_attention": a[1:]}, view_mask=[[False, True, True]])
    res = meter.compute()
    assert res["samples"] == 2 and list(res["present"]) == [1, 2, 2]
    assert np.allclose(res["per_joint_camera"], np.tile([[0.0, 0.125, 0.875]], (21, 1)))
    assert np.allclose(res["per_camera"], [0.0, 0.125, 0.875])
    assert np.allclose(res["query_view_fraction"], [0.5, 0.5, 0.0])
    m2 = ViewAttentionMeter(V, query_view=False)
    m2.add(a)
    assert "query_view_fraction" not in m2.compute()
    with pytest.raises(ValueError):
        meter.add({"view_attention": torch.zeros(1, 21, V + 1)})
    with pytest.raises(RuntimeError):
        ViewAttentionMeter(V).compute()


def test_new_entries_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    ci = ctypes.c_int32
    B, Tq, Tk, views = ci(), ci(), ci(), ci()
    assert lib.hmv_set_attention_capture(None, 1) == _lib.HMV_ERR_ARG
    assert lib.hmv_attention_shape(None, 0, ctypes.byref(B), ctypes.byref(Tq), ctypes.byref(Tk), ctypes.byref(views)) == _lib.HMV_ERR_ARG
    assert lib.hmv_read_attention(None, 0, None, 0, None, 0, None) == _lib.HMV_ERR_ARG
    fake = 0x1000   # never dereferenced: every call below is refused by its argument checks
    op = lib.hmv_op_attention_probs
    seg = lambda *v: (ci * len(v))(*v)   # noqa: E731

    def refused(*args, word):
        assert op(*args) == _lib.HMV_ERR_ARG, args
        assert word in lib.hmv_last_error(None).decode(), lib.hmv_last_error(None)

    refused(0, 0, None, None, 1, 21, 21, 0, 21, None, fake, None, 0, None, word="bad argument")          # NULL input
    refused(0, 0, fake, None, 1, 21, 21, 0, 21, None, None, None, 0, None, word="bad argument")          # NULL output
    refused(0, 3, fake, None, 1, 21, 21, 0, 21, None, fake, None, 0, None, word="bad argument")          # unknown kind
    refused(0, 0, fake, None, 0, 21, 21, 0, 21, None, fake, None, 0, None, word="bad argument")          # empty batch
    refused(0, 0, fake, fake, 1, 21, 21, 0, 21, None, fake, None, 0, None, word="probe")                 # probe with 128-wide heads
    refused(0, 0, fake, None, 1, 42, 43, 0, 42, None, fake, None, 0, None, word="Tq > T")                # queries outside the sample
    refused(0, 0, fake, None, 1, 42, 21, 21, 22, None, fake, None, 0, None, word="koff + Tk > T")        # keys outside the sample
    refused(0, 1, fake, None, 1, 42, 21, -1, 21, None, fake, None, 0, None, word="negative")
    refused(0, 2, fake, None, 2, 0, 21, 0, 21, None, fake, None, 0, None, word="positive")
    refused(0, 0, fake, None, 2, 0, 21, 21, 0, seg(0, 42, 52), fake, None, 0, None, word="fewer rows than koff")
    refused(0, 0, fake, None, 2, 0, 21, 0, 0, seg(0, 42, 52), fake, None, 0, None, word="fewer rows than Tq")
    refused(0, 0, fake, None, 2, 0, 0, 0, 0, seg(1, 42, 84), fake, None, 0, None, word="seg[0]")
    refused(0, 0, fake, None, 2, 0, 0, 0, 0, seg(0, 42, 42), fake, None, 0, None, word="at least one row")
    refused(0, 0, fake, None, 1, 42, 21, 20, 21, None, fake, fake, 2, None, word="view share")           # keys that start inside a view
    refused(0, 0, fake, None, 1, 42, 21, 21, 21, None, fake, fake, 1, None, word="view share")           # more views than columns
    refused(0, 0, fake, None, 1, 33, 33, 0, 33, None, fake, fake, 2, None, word="view share")            # key range of no whole views
