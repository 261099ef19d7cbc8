"""The k-step schedule of conv_igemm's fp32 main loop, at the smallest shapes where it can still go wrong (run with -m gpu).

Within one k-step the fp32 kernels issue the last MFMA group right behind the barrier and place the DMA pieces of tile t+2 and the
fragment reads of tile t+1 between its MFMAs.  What can break is the loop's edges (one, two, three ... k-steps; both buffer parities),
the cursor that advances once per k-step (taps, stride), ragged last tiles, and each instantiation's own piece counts.  Every case
goes through hmv_op_conv2d_sel with kernel_sel = 1 (conv_igemm only), must report the expected family, writes every element of a
NaN-filled output, and stays under the project's fp32 bar against a float64 reference computed on the device (unfold + matmul):
max |got - ref| / max |ref| < 4e-6 (BARS["f32"] of tests/test_gpu_launch_ledger.py).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAR_F32 = 4e-6


def _down(n, k, s, p):
    return (n + 2 * p - k) // s + 1


_DATA = {}   # (n, h, w, cin, cout, k, res) -> inputs, made once and left unchanged


def _data(n, h, w, cin, cout, k, stride, pad, res):
    key = (n, h, w, cin, cout, k, stride, pad, res)
    if key not in _DATA:
        dev = torch.device("cuda:0")
        g = torch.Generator(device=dev).manual_seed(h + 3 * w + 7 * cin + 11 * cout + k)
        gc = torch.Generator().manual_seed(cin * 1000 + cout + k)
        x = torch.randn(n, h, w, cin, generator=g, device=dev)
        wt = torch.randn(cout, cin, k, k, generator=gc) / (cin * k * k) ** 0.5
        b = torch.randn(cout, generator=gc)
        r = torch.randn(n, _down(h, k, stride, pad), _down(w, k, stride, pad), cout, generator=g, device=dev) if res else None
        _DATA[key] = (x, wt, b, r)
    return _DATA[key]


def _launch(x, wt, b, res, k, stride, pad, relu):
    """One conv_igemm launch into a NaN-filled buffer: (output, family name)."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    vp = ctypes.c_void_p
    n, h, w, cin = x.shape
    cout = wt.shape[0]
    out = torch.full((n, _down(h, k, stride, pad), _down(w, k, stride, pad), cout), float("nan"), device=x.device)
    wc, bc = np.ascontiguousarray(wt.numpy()), np.ascontiguousarray(b.numpy())
    name = ctypes.c_char_p()
    rc = lib.hmv_op_conv2d_sel(0, vp(x.data_ptr()), n, h, w, cin, wc.ctypes.data_as(vp), bc.ctypes.data_as(vp), cout, k, k, stride, pad,
                               vp(res.data_ptr()) if res is not None else None, int(relu), vp(out.data_ptr()), 1, ctypes.byref(name), None)
    assert rc == 0, lib.hmv_last_error(None).decode()
    torch.cuda.synchronize()
    return out, name.value.decode()


def _reference_error(x, wt, b, res, k, stride, pad, relu, out):
    """max |got - ref| / max |ref| against float64 unfold + matmul on the device, a few frames at a time."""
    n, h, w, cin = x.shape
    cout = wt.shape[0]
    ho, wo = out.shape[1], out.shape[2]
    wmat = wt.permute(2, 3, 1, 0).reshape(-1, cout).double().to(x.device)
    bd = b.double().to(x.device)
    step = max(1, min(n, (64 << 20) // max(1, ho * wo * k * k * cin)))
    err = ref_max = 0.0
    for f0 in range(0, n, step):
        xs = x[f0:f0 + step].double()
        if k == 1 and pad == 0:
            a = xs[:, ::stride, ::stride, :].reshape(-1, cin)
        else:
            xp = torch.nn.functional.pad(xs, (0, 0, pad, pad, pad, pad))
            cols = [xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride, :] for r in range(k) for s in range(k)]
            a = torch.cat(cols, dim=3).reshape(-1, k * k * cin)
        y = torch.matmul(a, wmat) + bd
        if res is not None:
            y = y + res[f0:f0 + step].double().reshape(-1, cout)
        if relu:
            y = y.clamp_min(0)
        err = max(err, (out[f0:f0 + step].reshape(-1, cout).double() - y).abs().max().item())
        ref_max = max(ref_max, y.abs().max().item())
    return err / ref_max


def _check(want, n, h, w, cin, cout, k, stride, pad, res, relu):
    x, wt, b, r = _data(n, h, w, cin, cout, k, stride, pad, res)
    out, name = _launch(x, wt, b, r, k, stride, pad, relu)
    assert name == want, (name, want)
    assert torch.isfinite(out).all(), "an element was left unwritten (NaN poison)"
    rel = _reference_error(x, wt, b, r, k, stride, pad, relu, out)
    print(want, (n, h, w, cin, cout, k, stride, pad, res, relu), f"rel {rel:.3e}")
    assert rel < BAR_F32, rel
    return out


# ---- loop edges: 1x1 with 1 .. 5 k-steps of 32 (one k-step: nothing to fetch, nothing to read ahead; two: no further DMA; three and
# more: the steady state, ending on either buffer), on the 256 x 256 tile (32 frames: 512 tiles) and on a small one (2 frames)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("cin", [32, 64, 96, 128, 160])
@pytest.mark.parametrize("frames,want", [(32, "conv_igemm_f32<256x256,1x1>"), (2, "conv_igemm_f32<64x64,1x1>")])
def test_loop_edges_1x1(frames, want, cin, relu):
    _check(want, frames, 32, 32, cin, 1024, 1, 1, 0, False, relu)


# ---- taps: the cursor (tap column, tap row, channel chunk) advances once per k-step, behind the last DMA piece
@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("frames,want", [(32, "conv_igemm_f32<256x256,taps>"), (2, "conv_igemm_f32<64x64,taps>")])
def test_taps(frames, want, cin):
    _check(want, frames, 32, 32, cin, 1024, 3, 1, 1, False, 1)


def test_taps_stride2():
    _check("conv_igemm_f32<256x256,taps>", 32, 64, 64, 32, 1024, 3, 2, 1, False, 0)


# ---- ragged M: 37 * 31 * 29 = 33 263 pixels = 129 full 256-pixel tiles + 239 rows
@pytest.mark.parametrize("k,pad,want", [(1, 0, "conv_igemm_f32<256x256,1x1>"), (3, 1, "conv_igemm_f32<256x256,taps>")])
def test_ragged_m(k, pad, want):
    _check(want, 37, 31, 29, 64, 1024, k, 1, pad, False, 1)


# ---- the other fp32 families of the headline forwards: the shortest reduction each admits at the smallest pixel count that selects it
#      (family, frames, H, W, Cin, Cout, k, stride, pad, residual, relu)
FAMILIES = [
    ("conv_igemm_f32<256x128,taps>", 128, 32, 32, 32, 128, 3, 1, 1, False, 1),
    ("conv_igemm_f32<256x64,taps>", 512, 32, 32, 32, 64, 3, 1, 1, False, 1),            # 524 288 pixels: the launcher's own bound
    ("conv_igemm_f32<256x128,k16,w8,1x1>", 256, 32, 32, 256, 128, 1, 1, 0, False, 1),   # squeezing conv1: K >= 256, Cout = 128, 1 024 M-tiles
    ("conv_igemm_f32<256x128,k16,w8,1x1>", 128, 32, 32, 160, 512, 1, 1, 0, True, 1),    # residual form: 128 < K <= 256, 2 048 tiles
    ("conv_igemm_f32<128x128,k16,1x1>", 64, 32, 32, 32, 256, 1, 1, 0, True, 1),
    ("conv_igemm_f32<128x32,1x1>", 16, 32, 32, 32, 80, 1, 1, 0, False, 0),
    ("conv_igemm_f32<128x128,1x1>", 64, 32, 32, 32, 128, 1, 1, 0, False, 1),
    ("conv_igemm_f32<64x64,1x1>", 2, 32, 32, 32, 128, 1, 1, 0, True, 1),
    ("conv_igemm_f32<128x32,taps>", 16, 32, 32, 32, 80, 3, 1, 1, False, 1),
    ("conv_igemm_f32<128x32,dense>", 16, 32, 32, 40, 80, 3, 1, 1, False, 1),
    ("conv_igemm_f32<256x128,taps,skipN>", 128, 32, 32, 256, 80, 3, 1, 1, False, 1),    # K >= 2 048 keeps Cout = 80 off the 32-wide tiles
]


@pytest.mark.parametrize("case", FAMILIES, ids=[f"{c[0]}{'+res' if c[9] else ''}" for c in FAMILIES])
def test_headline_families(case):
    _check(*case)


# ---- a sample's bits never depend on its batch: frames 0 and 1 alone (small tile) against the same frames of the 32-frame launch
@pytest.mark.parametrize("k,pad,cin", [(1, 0, 32), (1, 0, 64), (1, 0, 96), (1, 0, 128), (1, 0, 160), (3, 1, 32), (3, 1, 64)])
def test_bits_do_not_depend_on_the_batch(k, pad, cin):
    x, wt, b, _ = _data(32, 32, 32, cin, 1024, k, 1, pad, False)
    mode = "1x1" if k == 1 else "taps"
    big, name_big = _launch(x, wt, b, None, k, 1, pad, 1)
    small, name_small = _launch(x[:2].contiguous(), wt, b, None, k, 1, pad, 1)
    assert name_big == f"conv_igemm_f32<256x256,{mode}>" and name_small == f"conv_igemm_f32<64x64,{mode}>", (name_big, name_small)
    assert torch.isfinite(big).all() and torch.isfinite(small).all()
    assert torch.equal(big[:2].view(torch.int32), small.view(torch.int32))
