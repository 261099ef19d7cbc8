"""Attention maps of the fusion blocks on the device (run with -m gpu on an MI355X): the kernels of attention_probs.hip through the
op-level entry against torch float64, and hmv_set_attention_capture / hmv_read_attention through handmvnet_amd.HandMvNet against the
float64 oracle of tests/attention_oracle.py run on the engine's OWN captured tokens (the pattern of test_fusion_tail_on_engine_tokens).
Every test needs entries the library did not have before this feature."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import attention_oracle as ao
from cases import ALL_POS, CASES, case_params
from guards import Guards
from helpers import load_case

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23

# (B, T, Tq, koff, Tk)
SHAPES = [(2, 21, 21, 0, 21),        # one partial chunk
          (2, 42, 21, 21, 21),       # the cross block at V = 2
          (1, 33, 33, 0, 33),        # one key and one query past a block edge
          (2, 64, 64, 0, 64),        # exact chunks
          (2, 84, 21, 21, 63),
          (1, 129, 129, 0, 129),     # five chunks on four waves, the last holding 1 key
          (1, 273, 21, 21, 252)]
# (B, T, Tq, probe queries)
LQ_SHAPES = [(2, 42, 42, False), (3, 63, 21, True), (1, 273, 21, True)]
OP_CASES = [("f32", s) for s in SHAPES] + [("pairs", s) for s in SHAPES] + [("lq", s) for s in LQ_SHAPES]
OP_IDS = [f"{k}-{'x'.join(str(int(v)) for v in s)}" for k, s in OP_CASES]


def _guards_hold(gd):
    try:
        gd.check()
    except AssertionError as e:
        print(e)
        return False
    return True


@functools.lru_cache(maxsize=None)
def _op_run(kind, shape):
    """One op-level case, computed once and shared by the tests below (read-only): the float64 reference, the kernel's map and share for
    the whole batch, the map of sample 0 run alone, and whether the guard bands survived."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    if kind == "lq":
        B, T, Tq, probe = shape
        koff, Tk, D = 0, T, 256
        g = torch.Generator().manual_seed(B * 1000 + T)
        if probe:
            q = torch.randn(Tq, 8, 256, generator=g) * 3.0
            kv = torch.randn(B, T, 2, 8, 256, generator=g)
            rows, pq = kv.reshape(B, T, 4096), q.reshape(Tq, 2048)
            q64 = q.double().permute(1, 0, 2)[None].expand(B, -1, -1, -1)
            k64 = kv[:, :, 0].double().permute(0, 2, 1, 3)
        else:
            qkv = torch.randn(B, T, 3, 8, 256, generator=g)
            qkv[:, :, 0] *= 3.0
            rows, pq = qkv.reshape(B, T, 6144), None
            q64 = qkv[:, :Tq, 0].double().permute(0, 2, 1, 3)
            k64 = qkv[:, :, 1].double().permute(0, 2, 1, 3)
        code = 2
    else:
        B, T, Tq, koff, Tk = shape
        D = 128
        g = torch.Generator().manual_seed(B * 1000 + T)
        qkv = torch.randn(B, T, 3, 8, 128, generator=g)
        qkv[:, :, 0] *= 3.0                                   # logits of std ~3: sharp rows
        rows, pq = qkv.reshape(B, T, 3072), None
        q64 = qkv[:, :Tq, 0].double().permute(0, 2, 1, 3)
        k64 = qkv[:, koff:koff + Tk, 1].double().permute(0, 2, 1, 3)
        code = 0 if kind == "f32" else 1
    ref = torch.softmax(q64 @ k64.transpose(-1, -2) * D ** -0.5, dim=-1)      # [B, 8, Tq, Tk]
    views = (koff + Tk) // 21 if (koff % 21 == 0 and Tk % 21 == 0) else 0

    def run(nb):
        gd = Guards(dev)                    # 0xFF bands (tests/guards.py) around the rows, the probe and both outputs, which start as NaN
        rd = gd.inp(rows[:nb])
        pd = gd.inp(pq) if pq is not None else None
        pout = gd.out((nb, 8, Tq, Tk))
        sout = gd.out((nb, 8, Tq, views)) if views else None
        rc = lib.hmv_op_attention_probs(0, code, rd.data_ptr(), pd.data_ptr() if pd is not None else None, nb, T, Tq, koff,
                                        Tk, None, pout.data_ptr(), sout.data_ptr() if views else None, views, None)
        assert rc == 0, lib.hmv_last_error(None)
        torch.cuda.synchronize()
        return pout.cpu(), sout.cpu() if views else None, _guards_hold(gd)

    probs, share, ok = run(B)
    alone, _, ok1 = run(1)
    return {"ref": ref, "probs": probs, "share": share, "alone": alone, "guards": ok and ok1, "views": views, "rank0": koff // 21, "Tk": Tk}


@pytest.mark.parametrize("kind,shape", OP_CASES, ids=OP_IDS)
def test_probs_kernel_vs_torch(kind, shape):
    """Op level against torch float64 softmax, inputs as test_attention_kernel_vs_torch builds them (randn, q x 3).  Bar 4e-6 absolute: the bar
    that test holds softmax . V to for these inputs -- probabilities are <= 1 and the same ~1e-6 logit rounding applies.  The outputs were
    pre-filled with NaN and framed by guard bands; sample 0 alone gives the same bits."""
    r = _op_run(kind, shape)
    assert r["guards"], "a guard band around the output was written"
    assert torch.isfinite(r["probs"]).all()
    err = float((r["probs"].double() - r["ref"]).abs().max())
    print(kind, shape, "max |p - p64|", err)
    assert err <= 4e-6, err
    assert torch.equal(r["alone"][0], r["probs"][0])


@pytest.mark.parametrize("kind,shape", OP_CASES, ids=OP_IDS)
def test_probs_rows_sum_to_one(kind, shape):
    """|sum_j p - 1| <= (Tk + 32) 2^-23: Tk roundings of the sum, plus a handful for the rescaling, the reciprocal and the product."""
    r = _op_run(kind, shape)
    dev = float((r["probs"].double().sum(-1) - 1).abs().max())
    print(kind, shape, "max |sum - 1|", dev, "bar", (r["Tk"] + 32) * EPS)
    assert dev <= (r["Tk"] + 32) * EPS


@pytest.mark.parametrize("kind,shape", [(k, s) for k, s in OP_CASES if (k == "lq" or (s[3] % 21 == 0 and s[4] % 21 == 0))],
                         ids=[i for i, (k, s) in zip(OP_IDS, OP_CASES) if (k == "lq" or (s[3] % 21 == 0 and s[4] % 21 == 0))])
def test_view_share_kernel(kind, shape):
    """The share against the float64 sum of the returned 21 probabilities: <= 21 2^-23; where the keys start at the second view (the cross
    block of cross_attn) the rank-0 column is exactly 0."""
    r = _op_run(kind, shape)
    assert r["views"] > 0 and torch.isfinite(r["share"]).all()
    p = r["probs"].double()
    want = torch.zeros(*p.shape[:3], r["views"], dtype=torch.float64)
    want[..., r["rank0"]:] = p.reshape(*p.shape[:3], -1, 21).sum(-1)
    err = float((r["share"].double() - want).abs().max())
    print(kind, shape, "share err", err)
    assert err <= 21 * EPS
    if r["rank0"]:
        assert float(r["share"][..., :r["rank0"]].abs().max()) == 0.0


def test_probs_kernel_ragged_op():
    """The ragged form on its own: samples of 42, 21 and 63 rows in the cross block of the 128-wide heads (the second has no keys) equal,
    bit for bit, their own uniform runs; everything beyond a sample's extent is the zero the call filled in; guards untouched."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    seg = [0, 42, 63, 126]
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(126, 3, 8, 128, generator=g)
    qkv[:, 0] *= 3.0
    for code in (0, 1):
        gd = Guards(dev)
        rows = gd.inp(qkv.reshape(126, 3072))
        probs, share = gd.out((3, 8, 21, 42)), gd.out((3, 8, 21, 3))
        rc = lib.hmv_op_attention_probs(0, code, rows.data_ptr(), None, 3, 0, 21, 21, 0, (ctypes.c_int32 * 4)(*seg), probs.data_ptr(),
                                        share.data_ptr(), 3, None)
        assert rc == 0, lib.hmv_last_error(None)
        torch.cuda.synchronize()
        gd.check()
        assert torch.isfinite(probs).all() and torch.isfinite(share).all()
        for b in range(3):
            T = seg[b + 1] - seg[b]
            Tk = T - 21
            assert float(probs[b, :, :, Tk:].abs().max()) == 0.0 if Tk < 42 else True
            assert float(share[b, :, :, 0].abs().max()) == 0.0 and float(share[b, :, :, 1 + Tk // 21:].abs().sum()) == 0.0
            if Tk == 0:
                assert float(probs[b].abs().max()) == 0.0 and float(share[b].abs().max()) == 0.0
                continue
            one = gd.out((8, 21, Tk))
            rc = lib.hmv_op_attention_probs(0, code, gd.inp(qkv[seg[b]:seg[b + 1]].reshape(T, 3072)).data_ptr(), None, 1, T, 21, 21, Tk, None,
                                            one.data_ptr(), None, 0, None)
            assert rc == 0, lib.hmv_last_error(None)
            torch.cuda.synchronize()
            gd.check()
            assert torch.equal(probs[b, :, :, :Tk], one)


# ------------------------------------------------------------------ through the engine
def _model(name):
    from handmvnet_amd import HandMvNet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg, (tp, mp, dp), sd, inputs, fx = load_case(name)
        m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    return m, cfg, sd, inputs


def _set_mode(m, mode):
    if mode == "f16":
        m.half()
    elif mode == "f32x3":
        m.float32x3()


def _dev_inputs(inputs):
    dev = torch.device("cuda:0")
    x, bbox, intr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in inputs)
    return x, bbox, {"intrinsic": intr}


E2E_CASES = ["tiny_r18", "r18_frozen_nosin", "r50_wocam_nn", "cfg1_r50_v4_128", "r18_lq_wocam", "r50_lq"]
assert not any(CASES[n].get("cond") for n in E2E_CASES)   # (the cond=True case, hr40_lq, is left out)


@pytest.mark.parametrize("mode", ["f32", "f32x3", "f16"])
@pytest.mark.parametrize("name", E2E_CASES)
def test_engine_maps_on_engine_tokens(name, mode):
    """End to end: every block captured together with the `tokens` stage; the engine's maps against the float64 oracle on the engine's own
    tokens.  Bar per block max(4e-6, 4 n32'), n32' = the oracle chain in fp32 against float64 on those same tokens, measured here (4 x: the
    margin test_gpu_parity gives a differently ordered fp32 evaluation).  In the two (hi, lo) modes also 2 x what a 2^-19 relative
    perturbation of those tokens does to the float64 maps, as test_fusion_tail_on_engine_tokens allows.
    Measured on MI355X (max |p - p64| over the blocks, f32 / f32x3 / f16): see DESIGN.md section 4, "Attention maps"."""
    m, cfg, sd, inputs = _model(name)
    _set_mode(m, mode)
    x, bbox, cam = _dev_inputs(inputs)
    m.capture_stages(True)
    m.capture_attention("all")
    out = m(x, bbox, cam)
    torch.cuda.synchronize()
    tokens = m.read_stage("tokens").cpu().numpy()
    got = [m.read_attention(l) for l in range(m.fusion_blocks)]
    torch.cuda.synchronize()
    ref, _ = ao.fusion_attention(tokens, sd, cfg, torch.float64)
    r32, _ = ao.fusion_attention(tokens, sd, cfg, torch.float32)
    moved = None
    if mode != "f32":
        rng = np.random.default_rng(1234)
        tk = tokens.astype(np.float64)
        moved, _ = ao.fusion_attention((tk * (1.0 + 2.0 ** -19 * rng.standard_normal(tk.shape))).astype(np.float32), sd, cfg, torch.float64)
    cx = m.cross_block
    for l, (probs, share) in enumerate(got):
        p = probs.cpu()
        assert tuple(p.shape) == tuple(ref[l].shape), (l, p.shape, ref[l].shape)
        assert torch.isfinite(p).all()
        n32 = float((r32[l].double() - ref[l]).abs().max()) if p.numel() else 0.0
        bar = max(4e-6, 4 * n32)
        if moved is not None and p.numel():
            bar = max(bar, 2.0 * float((moved[l] - ref[l]).abs().max()))
        err = float((p.double() - ref[l]).abs().max()) if p.numel() else 0.0
        print(name, mode, "block", l, "err", err, "n32'", n32, "bar", bar)
        assert err <= bar, (name, mode, l, err, bar)
        if l <= cx:
            V = cfg.num_views
            assert share is not None and tuple(share.shape) == (p.shape[0], 8, p.shape[2], V)
            r0 = 1 if (l == cx and not cfg.learnable_query) else 0
            want = torch.zeros(share.shape, dtype=torch.float64)
            if p.numel():
                want[..., r0:] = p.double().reshape(*p.shape[:3], -1, 21).sum(-1)
            assert float((share.cpu().double() - want).abs().max()) <= 21 * EPS
            if r0:
                assert float(share[..., 0].abs().max()) == 0.0     # the view of rank 0 supplies the queries
        else:
            assert share is None
    assert torch.isfinite(out["joints_cam"]).all()


@pytest.mark.parametrize("name,mode", [("tiny_r18", "f32"), ("tiny_r18", "f16"), ("r18_lq_wocam", "f32"), ("r50_lq", "f32x3")])
def test_capture_does_not_disturb_the_forward(name, mode):
    """With any mask set, joints_cam / joints_crop_img / heatmap equal the bits of a run without it; with the mask back at 0 the forward
    enqueues what it enqueued before capture was first enabled (hmv_launch_count)."""
    m, cfg, sd, inputs = _model(name)
    _set_mode(m, mode)
    x, bbox, cam = _dev_inputs(inputs)
    base = {k: v.clone() for k, v in m(x, bbox, cam).items()}
    torch.cuda.synchronize()
    n0 = m.launch_count()
    for blocks in ("cross", "all", [0]):
        m.capture_attention(blocks)
        out = m(x, bbox, cam)
        torch.cuda.synchronize()
        assert m.launch_count() > n0
        for k in base:
            assert torch.equal(out[k], base[k]), (blocks, k)
    fa = m.forward_attention(x, bbox, cam, blocks="cross")
    for k in base:
        assert torch.equal(fa[k], base[k]), k
    assert fa["view_attention"].shape == (x.shape[0], 21, cfg.num_views)
    assert float((fa["view_attention"].sum(-1) - 1).abs().max()) <= (21 * cfg.num_views + 32) * EPS
    m.capture_attention(None)
    out = m(x, bbox, cam)
    torch.cuda.synchronize()
    assert m.launch_count() == n0
    for k in base:
        assert torch.equal(out[k], base[k]), k


RAGGED_VIEWS = [[1, 3], [0, 2, 3]]


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
@pytest.mark.parametrize("fusion", ["cross_attn", "cross_attn_learnable_query"])
def test_ragged_maps_equal_the_uniform_ones(fusion, mode):
    """A two-sample forward_views batch with 2 and 3 present views of a 4-view model: per sample the maps equal the bits of the uniform
    forward_attention of a second model object built with num_views = v_b; the padding is zeros; the camera-slot scatter puts zeros at
    absent cameras; a full mask equals the uniform bits."""
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.spec import config_from_params
    from handmvnet_amd.synth import synth_inputs, synth_state_dict
    spec = dict(bt="18", ch=[256, 128, 64], V=4, B=2, size=64, pos=ALL_POS, gcn=True, wseed=61, iseed=71, fusion=fusion)

    def build(V):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            params = case_params(dict(spec, V=V))
            mm = HandMvNet(*params)
            cfg = config_from_params(*params)
        mm.load_state_dict(synth_state_dict(cfg, spec["wseed"]), strict=True)
        mm.to("cuda").eval()
        _set_mode(mm, mode)
        return mm, cfg
    m4, cfg4 = build(4)
    inputs = synth_inputs(cfg4, spec["B"], spec["iseed"], spec["size"])
    x, bbox, cam = _dev_inputs(inputs)
    mask = np.zeros((2, 4), dtype=bool)
    for b, v in enumerate(RAGGED_VIEWS):
        mask[b, v] = True
    out = m4.forward_attention(x, bbox, cam, view_mask=mask, blocks="all")
    torch.cuda.synchronize()
    cx, nb = m4.cross_block, m4.fusion_blocks
    lq = fusion != "cross_attn"
    for b, views in enumerate(RAGGED_VIEWS):
        mb, _ = build(len(views))
        ob = mb.forward_attention(x[b:b + 1, views].contiguous(), bbox[b:b + 1, views].contiguous(),
                                  {"intrinsic": cam["intrinsic"][b:b + 1, views].contiguous()}, blocks="all")
        torch.cuda.synchronize()
        assert torch.equal(ob["joints_cam"][0], out["joints_cam"][b])
        for l in range(nb):
            one, full = ob["attention"][l][0], out["attention"][l][b]
            tq, tk = one.shape[1], one.shape[2]
            assert torch.equal(full[:, :tq, :tk], one), (b, l)
            assert float(full[:, tq:].abs().sum()) == 0.0 and float(full[:, :, tk:].abs().sum()) == 0.0, (b, l)
            if l <= cx:
                sh = out["view_share"][l][b]                       # [8, Tq_max, 4] by camera slot
                assert torch.equal(sh[:, :tq][..., views], ob["view_share"][l][0]), (b, l)
                absent = [v for v in range(4) if v not in views]
                assert float(sh[..., absent].abs().sum()) == 0.0 and float(sh[:, tq:].abs().sum()) == 0.0
            else:
                assert l not in out["view_share"]
        va = out["view_attention"][b]
        assert torch.equal(va[:, views], ob["view_attention"][0])
        if not lq:
            assert float(va[:, views[0]].abs().max()) == 0.0      # the first present camera supplies the queries
    uni = m4.forward_attention(x, bbox, cam, blocks="all")
    ful = m4.forward_attention(x, bbox, cam, view_mask=np.ones((2, 4), dtype=bool), blocks="all")
    torch.cuda.synchronize()
    for l in range(nb):
        assert torch.equal(uni["attention"][l], ful["attention"][l]), l
        if l <= cx:
            assert torch.equal(uni["view_share"][l], ful["view_share"][l]), l
    assert torch.equal(uni["view_attention"], ful["view_attention"])


def test_single_view_cross_block_has_no_keys():
    """r18_single_view: the cross block has Tk = 0.  read_attention succeeds, the share is zeros, and the block adds one device operation
    (the share's memset), no launch on an empty grid."""
    m, cfg, sd, inputs = _model("r18_single_view")
    x, bbox, cam = _dev_inputs(inputs)
    m(x, bbox, cam)
    torch.cuda.synchronize()
    n0 = m.launch_count()
    m.capture_attention("cross")
    m(x, bbox, cam)
    torch.cuda.synchronize()
    assert m.launch_count() == n0 + 1
    probs, share = m.read_attention(m.cross_block)
    torch.cuda.synchronize()
    assert tuple(probs.shape) == (x.shape[0], 8, 21, 0)
    assert tuple(share.shape) == (x.shape[0], 8, 21, 1) and float(share.abs().max()) == 0.0
    out = m.forward_attention(x, bbox, cam, blocks="all")
    assert tuple(out["attention"][0].shape) == (x.shape[0], 8, 21, 21)
    assert float(out["view_attention"].abs().max()) == 0.0


def test_errors_leave_the_handle_usable():
    from handmvnet_amd import _lib
    lib = _lib.load()
    m, cfg, sd, inputs = _model("tiny_r18")
    x, bbox, cam = _dev_inputs(inputs)
    base = m(x, bbox, cam)["joints_cam"].clone()
    torch.cuda.synchronize()
    hh, ww, idx, _, dt = m._last_key
    h = m._engines[(hh, ww, idx, dt)]
    buf = torch.empty(8 * 42 * 42, device="cuda:0")

    def usable():
        assert torch.equal(m(x, bbox, cam)["joints_cam"], base)
        torch.cuda.synchronize()

    # read without capture
    assert lib.hmv_read_attention(h, 2, buf.data_ptr(), buf.numel(), None, 0, None) == _lib.HMV_ERR_STATE
    assert b"hmv_set_attention_capture" in lib.hmv_last_error(h)
    usable()
    # bad mask bit
    assert lib.hmv_set_attention_capture(h, 1 << m.fusion_blocks) == _lib.HMV_ERR_ARG
    usable()
    m.capture_attention("all")
    usable()
    # block out of range; share of a block behind the cross block; short capacities
    assert lib.hmv_read_attention(h, m.fusion_blocks, buf.data_ptr(), buf.numel(), None, 0, None) == _lib.HMV_ERR_ARG
    assert lib.hmv_read_attention(h, 3, buf.data_ptr(), buf.numel(), buf.data_ptr(), buf.numel(), None) == _lib.HMV_ERR_ARG
    assert b"no view share" in lib.hmv_last_error(h)
    assert lib.hmv_read_attention(h, 0, buf.data_ptr(), 8 * 42 * 42 - 1, None, 0, None) == _lib.HMV_ERR_ARG
    assert lib.hmv_read_attention(h, 0, None, 0, buf.data_ptr(), 8 * 42 * 2 - 1, None) == _lib.HMV_ERR_ARG
    assert lib.hmv_read_attention(h, 0, buf.data_ptr(), buf.numel(), None, 0, None) == 0
    usable()
    # read after a sweep
    m.forward_subsets(x, [[0], [0, 1]], bbox, cam)
    torch.cuda.synchronize()
    assert lib.hmv_read_attention(h, 2, buf.data_ptr(), buf.numel(), None, 0, None) == _lib.HMV_ERR_STATE
    usable()
    probs, share = m.read_attention(2)
    torch.cuda.synchronize()
    assert tuple(probs.shape) == (1, 8, 21, 21) and float((probs.sum(-1) - 1).abs().max()) <= 53 * EPS
