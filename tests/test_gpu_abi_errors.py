"""Status codes and messages of the raw C ABI (include/handmv.h) on a real device: every misuse comes back as an
integer status + hmv_last_error text, nothing throws and nothing falls back."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import load_case

pytestmark = pytest.mark.gpu

OK, ARG, STATE, MISSING, SHAPE, HIP, UNSUPPORTED = range(7)


def _cfg(lib_mod, cfg, hh, ww, **over):
    from handmvnet_amd.spec import BACKBONE_IDS
    c = lib_mod.HmvConfig()
    c.struct_size = ctypes.sizeof(lib_mod.HmvConfig)
    c.backbone = BACKBONE_IDS[cfg.backbone_type]
    c.n_levels = len(cfg.backbone_channels)
    for i, ch in enumerate(cfg.backbone_channels):
        c.channels[i] = ch
    c.num_views, c.height, c.width = cfg.num_views, hh, ww
    c.image_size, c.heatmap_size = cfg.image_size, cfg.heatmap_size
    c.pos_enc, c.fusion_layers, c.decoder, c.dtype, c.device = cfg.pos_mask, cfg.fusion_layers, int(cfg.use_gcn), 0, 0
    c.fusion = int(cfg.learnable_query)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _set(lib, h, key, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
    return lib.hmv_set_tensor(h, key.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim)


def test_create_rejects_bad_configurations():
    from handmvnet_amd import _lib
    lib = _lib.load()
    cfg, _, sd, _, _ = load_case("tiny_r18")
    h = ctypes.c_void_p()
    for over, code, text in [({"struct_size": 8}, ARG, b"struct_size"), ({"backbone": 9}, ARG, b"Supports only"),
                             ({"fusion_layers": 4}, ARG, b"odd number"), ({"height": 16}, ARG, b"at least 32"),
                             ({"fusion": 7}, ARG, b"Invalid fusion type"), ({"backbone": 3, "height": 100}, ARG, b"multiples of 32"),
                             ({"num_views": 0}, ARG, b"num_views"), ({"dtype": 7}, UNSUPPORTED, b"dtype"),
                             ({"device": 99}, ARG, b"device ordinal")]:
        rc = lib.hmv_create(ctypes.byref(_cfg(_lib, cfg, 64, 64, **over)), ctypes.byref(h))
        assert rc == code, (over, rc, lib.hmv_last_error(None))
        assert text in lib.hmv_last_error(None), (over, lib.hmv_last_error(None))
    assert lib.hmv_create(None, ctypes.byref(h)) == ARG


def test_weight_loading_and_forward_state_machine():
    from handmvnet_amd import _lib
    from handmvnet_amd.spec import executed_keys
    lib = _lib.load()
    cfg, _, sd, (x, bbox, intr), fx = load_case("tiny_r18")
    h = ctypes.c_void_p()
    assert lib.hmv_create(ctypes.byref(_cfg(_lib, cfg, 64, 64)), ctypes.byref(h)) == OK
    try:
        dev = torch.device("cuda:0")
        xt, bt, it = torch.from_numpy(x).to(dev), torch.from_numpy(bbox).to(dev), torch.from_numpy(intr).to(dev)
        b, v = x.shape[:2]
        crop, cam = torch.empty(b, v, 21, 2, device=dev), torch.empty(b, 21, 3, device=dev)
        fwd = lambda xp=xt.data_ptr(), bp=bt.data_ptr(), ip=it.data_ptr(), batch=b: lib.hmv_forward(
            h, batch, xp, bp, ip, crop.data_ptr(), cam.data_ptr(), None, None)
        assert fwd() == STATE and b"finalize" in lib.hmv_last_error(h)          # no weights yet
        keys = executed_keys(cfg)
        for k in keys[:-1]:
            assert _set(lib, h, k, sd[k]) == OK
        assert lib.hmv_finalize_weights(h) == MISSING and keys[-1].encode() in lib.hmv_last_error(h)
        assert _set(lib, h, keys[-1], np.zeros(5)) == OK                        # stored; the shape is checked at finalize
        assert lib.hmv_finalize_weights(h) == SHAPE and b"size mismatch" in lib.hmv_last_error(h)
        assert _set(lib, h, keys[-1], sd[keys[-1]]) == OK
        assert _set(lib, h, "backbone.layer4.0.conv1.weight", np.zeros((4, 4))) == OK   # unread keys are accepted and ignored
        assert lib.hmv_finalize_weights(h) == OK
        assert fwd(xp=None) == ARG and fwd(batch=0) == ARG
        assert fwd(bp=None) == ARG and b"crop" in lib.hmv_last_error(h)         # pos_enc has 'crop': bbox / intrinsic required
        assert lib.hmv_reserve(h, 0) == ARG
        assert lib.hmv_workspace_bytes(h, 2) > lib.hmv_workspace_bytes(h, 1) > 0
        assert fwd() == OK                                                       # heatmap output is optional (NULL)
        torch.cuda.synchronize()
        assert np.abs(cam.cpu().numpy() - fx["joints_cam"]).max() <= 1e-3 * np.abs(fx["joints_cam"]).max()
        assert lib.hmv_read_stage(h, b"no_such_stage", crop.data_ptr(), 4, None) != OK
        assert lib.hmv_profile_get(h, 10 ** 6, None, None, None, None) == ARG
    finally:
        lib.hmv_destroy(h)
    assert lib.hmv_forward(None, 1, None, None, None, None, None, None, None) == ARG
    assert lib.hmv_version().startswith(b"handmv")


def test_op_attention_argument_errors():
    """hmv_op_attention (op-level test entry): ranges that would read outside [B][T][3072] are refused before any launch."""
    import torch
    from handmvnet_amd import _lib
    lib = _lib.load()
    qkv = torch.zeros(2, 42, 3072, device="cuda:0")
    out = torch.zeros(2, 42, 1024, device="cuda:0")
    ok = lib.hmv_op_attention(0, qkv.data_ptr(), 2, 42, 21, 21, 21, out.data_ptr(), None)
    assert ok == 0
    for args in ((2, 42, 43, 0, 42), (2, 42, 21, 30, 21), (2, 42, 21, 0, 0), (0, 42, 21, 0, 21), (2, 42, 0, 0, 21), (2, 42, 21, -1, 21)):
        assert lib.hmv_op_attention(0, qkv.data_ptr(), *args, out.data_ptr(), None) != 0, args
    assert lib.hmv_op_attention(0, None, 2, 42, 21, 0, 42, out.data_ptr(), None) != 0
    # hmv_op_attention_pairs: the same ranges, x3 outside {0, 1} and null operands -- HMV_ERR_ARG with the entry's name, nothing launched
    pairs = torch.full((2 * 42, 2048), 7.0, dtype=torch.float16, device="cuda:0")
    sat = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    for x3 in (0, 1):
        for args in ((2, 42, 43, 0, 42), (2, 42, 21, 30, 21), (2, 42, 21, 0, 0), (0, 42, 21, 0, 21), (2, 42, 0, 0, 21), (2, 42, 21, -1, 21),
                     (2, 0, 21, 0, 21)):
            assert lib.hmv_op_attention_pairs(0, x3, qkv.data_ptr(), *args, pairs.data_ptr(), sat.data_ptr(), None) == ARG, (x3, args)
            assert b"hmv_op_attention_pairs" in lib.hmv_last_error(None)
        assert lib.hmv_op_attention_pairs(0, x3, None, 2, 42, 21, 21, 21, pairs.data_ptr(), sat.data_ptr(), None) == ARG
        assert lib.hmv_op_attention_pairs(0, x3, qkv.data_ptr(), 2, 42, 21, 21, 21, None, sat.data_ptr(), None) == ARG
    for x3 in (2, -1):
        assert lib.hmv_op_attention_pairs(0, x3, qkv.data_ptr(), 2, 42, 21, 21, 21, pairs.data_ptr(), sat.data_ptr(), None) == ARG
    torch.cuda.synchronize()
    assert bool((pairs == 7.0).all()) and int(sat.item()) == 7
    # ... and the good calls run: zero rows in, zero pairs out for the 21 query rows of both samples, the range word left alone (NULL is accepted)
    for x3 in (0, 1):
        pairs.fill_(7.0)
        assert lib.hmv_op_attention_pairs(0, x3, qkv.data_ptr(), 2, 42, 21, 21, 21, pairs.data_ptr(), sat.data_ptr() if x3 else None, None) == OK
        assert not pairs[:2 * 21].any() and bool((pairs[2 * 21:] == 7.0).all()) and int(sat.item()) == 7     # out_pairs is [B][Tq][2048]


def test_non_gemm_op_entries_refuse_bad_arguments():
    """The hmv_op_* entries of the non-GEMM kernels (tests/test_gpu_ops_f64.py): HMV_ERR_ARG with the entry's name in hmv_last_error(NULL),
    before any launch -- the output keeps its bytes."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    a = torch.zeros(1 << 16, device=dev)
    out = torch.full((1 << 16,), 7.0, device=dev)
    idx = torch.zeros(64, dtype=torch.int32, device=dev)
    A, O, I = a.data_ptr(), out.data_ptr(), idx.data_ptr()
    bad = [
        ("hmv_op_input_layout", (0, 0, 0, None, 1, 4, 4, O, None, None)),
        ("hmv_op_input_layout", (0, 2, 0, A, 1, 4, 4, O, None, None)),
        ("hmv_op_input_layout", (0, 0, 3, A, 1, 4, 4, O, None, None)),
        ("hmv_op_input_layout", (0, 1, 0, A, 1, 0, 4, O, None, None)),
        ("hmv_op_maxpool", (0, 3, A, 1, 4, 4, 8, O, None)),
        ("hmv_op_maxpool", (0, 0, A, 1, 4, 4, 6, O, None)),
        ("hmv_op_maxpool", (0, 1, A, 1, 4, 4, 12, O, None)),
        ("hmv_op_maxpool", (0, 0, A, 1, 4, 4, 8, None, None)),
        ("hmv_op_soft_argmax", (0, A, 20, 1, 4, 4, O, O, 64.0, 16.0, None, None)),
        ("hmv_op_soft_argmax", (0, A, 32, 1, 4, 4, O, None, 64.0, 16.0, None, None)),
        ("hmv_op_soft_argmax", (0, A, 32, 1, 0, 4, O, O, 64.0, 16.0, None, None)),
        ("hmv_op_soft_argmax", (0, A, 32, 1, 4, 4, O, O, 64.0, 0.0, None, None)),
        ("hmv_op_sample_gather", (0, A, 1, 1, 4, 16, 4, A, O, None)),
        ("hmv_op_sample_gather", (0, A, 1, 4, 4, 16, 3, A, O, None)),
        ("hmv_op_sample_gather", (0, A, 1, 4, 4, 4, 2, A, O, None)),
        ("hmv_op_sample_gather", (0, A, 1, 4, 4, 16, 4, None, O, None)),
        ("hmv_op_sample_blend", (0, A, 8, 16, 1, 4, 4, A, O, 32, 0, None)),
        ("hmv_op_sample_blend", (0, A, 16, 16, 1, 4, 4, A, O, 32, 17, None)),
        ("hmv_op_sample_blend", (0, A, 16, 16, 1, 4, 4, A, O, 32, -1, None)),
        ("hmv_op_sample_blend", (0, A, 16, 16, 1, 4, 1, A, O, 32, 0, None)),
        ("hmv_op_tokens_finalize", (0, O, 48, 44, 32, 1, 1, None, A, A, A, 4, None, None, None, None, None)),
        ("hmv_op_tokens_finalize", (0, O, 48, 43, 32, 1, 1, None, A, A, A, 3, None, None, None, None, None)),
        ("hmv_op_tokens_finalize", (0, O, 40, 44, 32, 1, 1, None, A, A, A, 3, None, None, None, None, None)),
        ("hmv_op_tokens_finalize", (0, O, 48, 44, 32, 1, 1, None, A, None, A, 3, None, None, None, None, None)),
        ("hmv_op_tokens_finalize", (0, O, 48, 34, 32, 1, 1, None, None, A, A, 1, None, None, None, None, None)),
        ("hmv_op_tokens_finalize", (0, O, 48, 44, 32, 1, 0, None, A, A, A, 3, None, None, None, None, None)),
        ("hmv_op_tokens_finalize", (0, O, 48, 44, 32, 1, 1, I, A, A, A, 3, None, A, None, None, None)),
        ("hmv_op_layernorm", (0, A, 44, 2, 44, A, A, O, 40, None, None, None, None)),
        ("hmv_op_layernorm", (0, A, 40, 2, 44, A, A, O, 44, None, None, None, None)),
        ("hmv_op_layernorm", (0, A, 1028, 2, 1028, A, A, O, 1028, None, None, None, None)),
        ("hmv_op_layernorm", (0, A, 44, 2, 44, A, A, O, 44, A, A, None, None)),
        ("hmv_op_layernorm", (0, A, 44, 2, 44, A, None, O, 44, None, None, None, None)),
        ("hmv_op_splitk_reduce", (0, A, 0, 5, 44, 44, A, None, 0, 0, 0, 0, O, 44, None)),
        ("hmv_op_splitk_reduce", (0, A, 4, 5, 40, 44, A, None, 0, 0, 0, 0, O, 44, None)),
        ("hmv_op_splitk_reduce", (0, A, 4, 5, 44, 44, A, A, 40, 0, 0, 0, O, 44, None)),
        ("hmv_op_splitk_reduce", (0, A, 4, 5, 44, 44, A, None, 0, 0, 0, 4, O, 44, None)),
        ("hmv_op_splitk_reduce", (0, A, 4, 5, 44, 44, A, A, 44, 21, 20, 0, O, 44, None)),
        ("hmv_op_splitk_reduce", (0, A, 4, 5, 44, 44, None, None, 0, 0, 0, 0, O, 44, None)),
        ("hmv_op_splitk_layernorm", (0, A, 2, 5, 44, 44, A, None, 0, 0, 0, A, A, O, 44, None, None, None, None)),
        ("hmv_op_splitk_layernorm", (0, A, 4, 5, 1028, 1028, A, None, 0, 0, 0, A, A, O, 1028, None, None, None, None)),
        ("hmv_op_splitk_layernorm", (0, A, 4, 5, 44, 44, A, None, 0, 0, 0, None, A, O, 44, None, None, None, None)),
        ("hmv_op_add_pe", (0, A, 44, 42, 0, None, 44, A, O, 48, None)),
        ("hmv_op_add_pe", (0, A, 44, 40, 42, I, 44, A, O, 48, None)),
        ("hmv_op_add_pe", (0, A, 44, 42, 42, None, 44, A, O, 40, None)),
        ("hmv_op_add_pe", (0, A, 44, 42, 42, None, 44, None, O, 48, None)),
        ("hmv_op_cheb_mix", (0, A, 47, 1, 16, A, A, 0, O, 16, None)),
        ("hmv_op_cheb_mix", (0, A, 48, 1, 16, A, A, 0, O, 12, None)),
        ("hmv_op_cheb_mix", (0, A, 48, 0, 16, A, A, 0, O, 16, None)),
        ("hmv_op_cheb_mix", (0, A, 48, 1, 16, None, A, 0, O, 16, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == ARG, (name, args)
        assert name.encode() in lib.hmv_last_error(None), (name, args, lib.hmv_last_error(None))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # ... and the smallest good call of one of them still runs
    assert lib.hmv_op_add_pe(0, A, 44, 42, 42, None, 44, A, O, 48, None) == OK
    assert not out[:42 * 48].any() and bool((out[42 * 48:] == 7.0).all())


def test_fused_tail_op_entries_refuse_bad_arguments():
    """hmv_op_ff_block and hmv_op_cheb_fused (tests/test_gpu_tail_f64.py): HMV_ERR_ARG with the entry's name in hmv_last_error(NULL), before
    any launch -- the outputs keep their bytes -- for everything launch_ff_block / cheb_fusable refuse, null operands, and a forced 32-row
    tile that does not fit LDS."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    a = torch.zeros(1 << 18, device=dev)
    out = torch.full((1 << 16,), 7.0, device=dev)
    A, O = a.data_ptr(), out.data_ptr()

    def ff(**over):
        s = _lib.HmvFfBlockArgs()
        s.struct_size = ctypes.sizeof(_lib.HmvFfBlockArgs)
        s.rows, s.d, s.ld, s.ldo, s.hid = 5, 44, 48, 48, 128
        s.S, s.lds, s.slice, s.ldr, s.ldx, s.ldw1, s.ldw2 = 4, 48, 5 * 48, 48, 48, 48, 128
        s.slab = s.bias0 = s.res = s.n1g = s.n1b = s.fg = s.fb = s.w1 = s.b1 = s.w2 = s.b2 = s.n2g = s.n2b = A
        s.out = O
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def cheb(**over):
        s = _lib.HmvChebFusedArgs()
        s.struct_size = ctypes.sizeof(_lib.HmvChebFusedArgs)
        s.B, s.K, s.ldx, s.c1, s.ldw1, s.c2, s.ldw2, s.c3, s.ldw3, s.ldo = 1, 96, 96, 32, 96, 16, 32, 1, 16, 4
        s.x = s.w1 = s.bias1 = s.w2 = s.bias2 = s.w3 = s.bias3 = s.tk = A
        s.scratch = s.out = O
        for k, v in over.items():
            setattr(s, k, v)
        return s

    bad_ff = [{"struct_size": 8}, {"rows": 0}, {"d": 0}, {"out": None}, {"w1": None}, {"w2": None}, {"b1": None}, {"b2": None}, {"fg": None},
              {"fb": None}, {"n1b": None}, {"n2g": None}, {"slab": None}, {"x": A}, {"bias0": None}, {"S": 0}, {"S": 5}, {"tile_rows": 8},
              {"ld": 40, "ldo": 40}, {"ld": 56, "ldo": 56, "ldw1": 56}, {"ldo": 64}, {"d": 580, "ld": 592, "ldo": 592, "ldw1": 592, "lds": 592, "ldr": 592},
              {"lds": 46}, {"ldr": 50}, {"ldw1": 50}, {"ldw2": 130}, {"hid": 64}, {"ldw1": 44}, {"ldw2": 124}, {"lds": 40}, {"ldr": 40},
              {"slice": 100}, {"rg_out": -1}, {"rg_out": 21, "rg_in": 20}, {"slab": None, "x": A, "ldx": 46}, {"slab": None, "x": A, "ldx": 40},
              {"d": 560, "ld": 560, "ldo": 560, "ldw1": 560, "lds": 560, "ldr": 560, "slice": 5 * 560, "tile_rows": 32},
              {"d": 496, "ld": 496, "ldo": 496, "ldw1": 496, "lds": 496, "ldr": 496, "slice": 5 * 496, "hid": 256, "ldw2": 256, "tile_rows": 32}]
    for over in bad_ff:
        assert lib.hmv_op_ff_block(0, ctypes.byref(ff(**over)), None) == ARG, over
        assert b"hmv_op_ff_block" in lib.hmv_last_error(None), (over, lib.hmv_last_error(None))
    assert lib.hmv_op_ff_block(0, None, None) == ARG and b"hmv_op_ff_block" in lib.hmv_last_error(None)
    bad_cheb = [{"struct_size": 8}, {"B": 0}, {"K": 0}, {"c3": 0}, {"K": 592, "ldx": 592, "ldw1": 592}, {"K": 100, "ldx": 100, "ldw1": 100},
                {"ldx": 92}, {"ldw1": 92}, {"ldx": 98}, {"c1": 24}, {"c1": 272, "ldw2": 272}, {"c2": 80, "ldw3": 80}, {"c2": 8}, {"c3": 6, "ldo": 8},
                {"ldw2": 28}, {"ldw3": 12}, {"ldo": 0}, {"x": None}, {"w1": None}, {"bias1": None}, {"w2": None}, {"bias2": None}, {"w3": None},
                {"bias3": None}, {"tk": None}, {"scratch": None}, {"out": None}]
    for over in bad_cheb:
        assert lib.hmv_op_cheb_fused(0, ctypes.byref(cheb(**over)), None) == ARG, over
        assert b"hmv_op_cheb_fused" in lib.hmv_last_error(None), (over, lib.hmv_last_error(None))
    assert lib.hmv_op_cheb_fused(0, None, None) == ARG and b"hmv_op_cheb_fused" in lib.hmv_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # ... and the good calls run: zeros in, LayerNorm2's beta (0) out; tile_rows_used says what was launched
    good = ff(tile_rows=32)
    assert lib.hmv_op_ff_block(0, ctypes.byref(good), None) == OK, lib.hmv_last_error(None)
    assert good.tile_rows_used == 32
    torch.cuda.synchronize()
    assert not out[:5 * 48].any() and bool((out[5 * 48:] == 7.0).all())
    out.fill_(7.0)
    assert lib.hmv_op_cheb_fused(0, ctypes.byref(cheb()), None) == OK, lib.hmv_last_error(None)
    torch.cuda.synchronize()
    assert not out[:21 * 32].any()      # scratch and out alias here: zeros either way


def test_conv_form_entry_refuses_what_the_engine_never_issues():
    """hmv_op_conv2d_form (tests/test_gpu_conv_forms.py): a non-zero code with the entry's name in hmv_last_error(NULL) and the outputs
    untouched -- HMV_ERR_ARG before any launch for a NULL args, another struct_size, null operands, forms that do not meet, a second
    source sampled outside its map, a chain or a pool the engine's own rule (conv_stream_chain_ok, conv_hs_supported) would not issue, a
    slice count splitk_slices never gives -- and the good call runs."""
    import numpy as np
    from handmvnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    ARG, OK = 1, 0
    N, H, W = 1, 4, 4
    x = torch.zeros(N * H * W * 64, device=dev)
    x2 = torch.zeros(N * 8 * 8 * 64, device=dev)
    out = torch.full((N * 8 * 8 * 256,), 7.0, device=dev)
    nxt = torch.full((N * H * W * 128,), 7.0, device=dev)
    w = np.zeros(256 * 64 * 16, dtype=np.float32)
    wp = w.ctypes.data_as(ctypes.c_void_p)

    def form(**over):
        a = _lib.HmvConvFormArgs()
        a.struct_size = ctypes.sizeof(_lib.HmvConvFormArgs)
        a.dtype, a.form, a.N, a.H, a.W, a.Cin, a.Cout, a.R, a.S, a.stride, a.pad, a.relu = 1, _lib.HMV_FORM_DUAL, N, H, W, 64, 256, 1, 1, 1, 0, 1
        a.in_, a.out, a.w, a.in2, a.w2 = x.data_ptr(), out.data_ptr(), wp, x2.data_ptr(), wp
        a.Cin2, a.H2, a.W2, a.stride2 = 64, 7, 7, 2
        for k, v in over.items():
            setattr(a, k, v)
        return a

    F = _lib
    res = x2.data_ptr()
    bad = [({"struct_size": 8}, ARG), ({"in_": None}, ARG), ({"w": None}, ARG), ({"out": None}, ARG), ({"N": 0}, ARG), ({"dtype": 3}, ARG),
           ({"form": 64}, ARG), ({"in2": None}, ARG), ({"w2": None}, ARG), ({"stride2": 0}, ARG),
           ({"H2": 6}, ARG),                                    # row (H - 1) * stride2 = 6 lies outside a 6-row map
           ({"W2": 4, "stride2": 2}, ARG),
           ({"ld_in2": 60}, ARG), ({"ld_in": 72}, ARG),        # the first source of a dual launch has no stride of its own
           ({"dtype": 2}, ARG),                                 # the pair mode never fuses the downsample
           ({"Cin": 32, "dtype": 1}, ARG),                      # half a 64-channel chunk before the seam
           ({"form": F.HMV_FORM_DUAL | F.HMV_FORM_POOL}, ARG), ({"form": F.HMV_FORM_DUAL | F.HMV_FORM_SPLITK, "dtype": 0}, ARG),
           ({"form": F.HMV_FORM_PAIR_OUT}, ARG),                # pairs out of an fp16 layer
           ({"form": F.HMV_FORM_CHAIN, "residual": res, "next_w": wp, "next_out": nxt.data_ptr(), "next_cout": 96}, ARG),   # no 96-channel chain
           ({"form": F.HMV_FORM_CHAIN, "next_w": wp, "next_out": nxt.data_ptr(), "next_cout": 64}, ARG),    # conv3 without a residual
           ({"form": F.HMV_FORM_CHAIN, "dtype": 0, "residual": res, "next_w": wp, "next_out": nxt.data_ptr(), "next_cout": 64}, ARG),
           ({"form": F.HMV_FORM_POOL, "pool_h": 2, "pool_w": 2}, ARG),                                      # a 1x1 conv is no stem
           ({"form": F.HMV_FORM_POOL, "Cin": 12, "ld_in": 16, "Cout": 64, "R": 4, "S": 4, "pad": 2, "Ho": 4, "Wo": 4, "pool_h": 3, "pool_w": 2}, ARG),
           ({"form": F.HMV_FORM_SPLITK, "dtype": 0, "H": 1, "W": 1, "relu": 0, "slices": 4}, ARG),         # K = 64: the rule never slices it
           ({"form": F.HMV_FORM_SPLITK, "dtype": 0, "relu": 0, "slices": 1}, ARG),                          # a map, not GEMM rows
           ({"form": F.HMV_FORM_PHASES, "R": 4, "S": 4, "stride": 2, "pad": 1, "merged": 2}, ARG),
           ({"form": F.HMV_FORM_PHASES, "R": 3, "S": 3, "stride": 2, "pad": 1}, ARG),
           ({"form": F.HMV_FORM_PHASES, "dtype": 2, "R": 4, "S": 4, "stride": 2, "pad": 1, "merged": 1}, ARG),   # the pair mode never merges
           ({"route_stream": 3}, ARG), ({"gemm8_persist": -1}, ARG)]
    for over, want in bad:
        rc = lib.hmv_op_conv2d_form(0, ctypes.byref(form(**over)), None)
        assert rc == want, (over, rc, lib.hmv_last_error(None))
        assert b"hmv_op_conv2d_form" in lib.hmv_last_error(None), (over, lib.hmv_last_error(None))
    assert lib.hmv_op_conv2d_form(0, None, None) == ARG and b"hmv_op_conv2d_form" in lib.hmv_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((nxt == 7.0).all())
    good = form()
    assert lib.hmv_op_conv2d_form(0, ctypes.byref(good), None) == OK, lib.hmv_last_error(None)
    assert good.kernel_name and good.kernel_name.startswith(b"conv_")
    torch.cuda.synchronize()
    o = out.view(torch.float16)
    assert not o[:N * H * W * 256].any() and bool((out[N * H * W * 128:] == 7.0).all())   # zeros in, zeros out (fp16 rows); nothing beyond
