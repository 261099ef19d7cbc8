"""conv_igemm's fp32 row drain (the staged epilogue of the fp32 kernels), op level on an MI355X.

The fp32 kernels write fp32 rows with an optional fp32 residual through a straight-line drain: no residual -> nothing loaded, the
stores of a staging pass back to back; fp32 residual -> the next rows' residual requested before this group's stores; rows past M
stored to a scratch slot.  Every other format keeps the general drain.  What is checked per shape: the kernel that ran, guard
bands / inputs / finiteness, torch float64 at the bar of test_stream32_kernel_is_bit_identical (4e-6 of the largest reference
value), the bits of conv_stream_f32 where that kernel has the shape, and the bits of values whose arithmetic is exact.

The shapes are the smallest that conv_pick_tile sends to each tile family (the name assertion keeps them honest).
"""
import ctypes

import pytest
import torch

from guards import Guards

pytestmark = pytest.mark.gpu

REL = 4e-6

# (N, H, W, Cin, Cout, k, residual, relu), expected kernel, does conv_stream_f32 have the shape
SHAPES = [
    # 256x256 1x1 with an fp32 residual: two staging passes, the residual ring crosses the pass boundary
    ((32, 32, 32, 64, 1024, 1, True, True), "conv_igemm_f32<256x256,1x1>", True),
    # ragged last M tile (33 759 = 131 * 256 + 223 rows), no residual, no ReLU
    ((33, 31, 33, 64, 1024, 1, False, False), "conv_igemm_f32<256x256,1x1>", False),
    # 256x256 taps, pad 1
    ((32, 32, 32, 32, 1024, 3, False, True), "conv_igemm_f32<256x256,taps>", False),
    # 256x128
    ((128, 32, 32, 32, 128, 3, False, True), "conv_igemm_f32<256x128,taps>", False),
    # small tiles with a residual and ragged rows
    ((3, 17, 19, 128, 512, 1, True, True), "conv_igemm_f32<64x64,1x1>", True),
    ((1, 8, 8, 64, 256, 1, True, False), "conv_igemm_f32<64x64,1x1>", True),
    # row stride 21: the general (non-vector) drain beside the new one
    ((4, 32, 32, 512, 21, 1, False, False), "conv_igemm_f32<128x32,1x1>", False),
]


def _reference(x, w, b, res, k, relu, dev):
    """float64 on the device: im2col (unfold) and one matmul; NHWC in, NHWC out."""
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    xd = x.to(dev).double().permute(0, 3, 1, 2)
    if k == 1:
        cols = xd.reshape(N, Cin, H * W)
    else:
        cols = torch.nn.functional.unfold(xd, k, padding=k // 2)          # [N, Cin*k*k, H*W], (c, r, s) order = w.reshape
    ref = torch.matmul(w.to(dev).double().reshape(Cout, -1), cols)       # [N, Cout, H*W]
    ref = ref.permute(0, 2, 1).reshape(N, H, W, Cout) + b.to(dev).double()
    if res is not None:
        ref = ref + res.to(dev).double()
    return ref.clamp_min(0) if relu else ref


def _conv(lib, gd, xin, w, b, rdev, shape, sel):
    N, H, W, Cin, Cout, k, use_res, relu = shape
    wc, bc = w.contiguous().numpy(), b.contiguous().numpy()
    out = gd.out((N, H, W, Cout))
    kname = ctypes.c_char_p()
    rc = lib.hmv_op_conv2d_sel(0, xin.data_ptr(), N, H, W, Cin, wc.ctypes.data_as(ctypes.c_void_p), bc.ctypes.data_as(ctypes.c_void_p),
                               Cout, k, k, 1, k // 2, rdev.data_ptr() if use_res else None, int(relu), out.data_ptr(), sel,
                               ctypes.byref(kname), None)
    assert rc == 0, lib.hmv_last_error(None)
    torch.cuda.synchronize()
    gd.check()
    return out, kname.value.decode()


@pytest.mark.parametrize("shape,kernel,stream", SHAPES, ids=[s[1][15:-1] + "-" + "x".join(map(str, s[0][:6])) for s in SHAPES])
def test_fp32_drain(shape, kernel, stream):
    from handmvnet_amd import _lib
    lib = _lib.load()
    N, H, W, Cin, Cout, k, use_res, relu = shape
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(sum(shape[:6]) + 3)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    res = torch.randn(N, H, W, Cout, generator=g) if use_res else None
    exact = {}
    if not use_res and not relu and Cout >= 8:
        # channels with zero weights: the accumulator is +0, so the output is (0 + bias) + 0 -- exact, sign of zero included
        # (-0.0 + 0.0 is +0.0: what the addition of an absent residual has always given)
        exact = {1: (-0.0, 0.0), 2: (-1.5, -1.5), 5: (0.0, 0.0), Cout - 1: (-0.0, 0.0)}
        for c, (bias, _) in exact.items():
            w[c] = 0
            b[c] = bias
    gd = Guards(dev)
    xin = gd.inp(x)
    rdev = gd.inp(res) if use_res else None
    out, name = _conv(lib, gd, xin, w, b, rdev, shape, 1)
    assert name == kernel, name
    assert torch.isfinite(out).all()
    ref = _reference(x, w, b, res, k, relu, dev)
    scale = ref.abs().max().item()
    err = (out.double() - ref).abs().max().item() / scale
    print(f"{name} {shape}: max error / max |ref| = {err:.3e}")
    assert err < REL, err
    if not relu:
        assert (out < 0).any()
    for c, (_, want) in exact.items():
        col = out[..., c].contiguous().view(torch.int32)
        bits = torch.tensor([want], dtype=torch.float32).view(torch.int32).item()
        assert bool((col == bits).all()), (c, want, out[..., c].flatten()[:4])
    if stream:
        out2, name2 = _conv(lib, gd, xin, w, b, rdev, shape, 2)
        assert name2.startswith("conv_stream_f32"), name2
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), (name, name2, (out - out2).abs().max())
