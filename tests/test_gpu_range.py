"""The fp16 range edges of the three arithmetic modes (include/handmv.h, "Range contract"), against torch fp64 on the CPU and the f64 oracle.

  fp32    no range limit: the op-level bars hold at every scale.
  f32x3   (hi, lo) fp16 pairs, hi = fp16(v), lo = fp16(v - hi).  In [2^-3, 65504) fp32-equivalent (the existing 3e-6 bars).  Below 2^-3
          lo is an fp16 subnormal (spacing 2^-24), so a converted value carries an ABSOLUTE error of at most 2^-25 (half that spacing; hi + lo
          together, also once hi itself is subnormal).  An output o = sum_k w_k x_k (+ r) then picks up at most
              FLOOR_o = 2^-25 * (sum_k |w_ok| + [residual]) * (1 + 2^-10)
          on top of the relative bar (the 2^-10: the weights' own pair rounding; the dropped lo * lo products are below 2^-44 |w x|).  Above
          65504 a pair cannot hold the value: the conversion clamps and REPORTS it -- HMV_ERR_RANGE from an hmv_op_* entry, the handle's
          range word after a forward (HandMvNet.check_range) -- and never returns rc 0 with a clamped result.
  f16     model.half(): round-to-nearest casts, |v| >= 65520 becomes +-inf; finite outputs meet the fp16 bar; the kernel families documented
          as giving the same bits still do at the range edge (inf positions included).  Folded weights fp16 cannot hold are refused."""
import ctypes
import re

import numpy as np
import pytest
import torch

from guards import Guards, bands_intact, guarded
from helpers import load_case, rel_l2

pytestmark = pytest.mark.gpu

HMV_ERR_RANGE = 7
F16_MAX = 65504.0
F16_INF_EDGE = 65520.0          # the smallest magnitude that rounds to inf (round to nearest even)
FLOOR_UNIT = 2.0 ** -25 * (1 + 2.0 ** -10)
TOL_CAM, TOL_STAGE = 1e-3, 2e-4  # test_gpu_parity.py's fp32 bars against the oracle
vp = ctypes.c_void_p

# (N, H, W, Cin, Cout, k, stride, pad, residual, relu): a 1x1, a 3x3, the stem's 7x7 s2, a residual 1x1, ragged M / N tails
SHAPES = {"1x1": (2, 9, 7, 64, 96, 1, 1, 0, False, True), "3x3": (1, 9, 7, 32, 40, 3, 1, 1, False, False),
          "stem": (1, 32, 32, 8, 64, 7, 2, 3, False, True), "residual": (2, 8, 8, 64, 128, 1, 1, 0, True, True),
          "ragged": (1, 9, 7, 24, 20, 3, 1, 1, True, False)}
# shapes with the special fp16 kernels' forms: tall-tile 3x3 (kernel_sel 3 .. 7), conv_gemm8 1x1 (2 / 8), conv_hs 64 -> 64 3x3 (2)
F16_SHAPES = dict(SHAPES, ragged=(1, 9, 7, 24, 24, 3, 1, 1, True, False),   # (fp16 rows: Cout % 8 == 0)
                  tall=(1, 16, 32, 64, 128, 3, 1, 1, False, True), gemm8=(2, 32, 32, 128, 256, 1, 1, 0, False, True),
                  hs=(4, 32, 32, 64, 64, 3, 1, 1, False, True))
KS = [-14, -10, -6, -3, 0, 4, 8, 12, 14, 15, 16, 18]
# kernel_sel groups documented as bit-identical (hmv_op_conv2d_f16 in include/handmv.h): conv_igemm and the round-3 kernels (0 / 1 / 2 / 8),
# the tall-tile packing on 16x16x32 (3 / 4 / 7) and on 32x32x16 (5 / 6)
F16_GROUPS = [(0, 1, 2, 8), (3, 4, 7), (5, 6)]


def _lib():
    from handmvnet_amd import _lib as L
    return L.load()


def _case(shape, k, which):
    N, H, W, Cin, Cout, ks, stride, pad, use_res, relu = shape
    g = torch.Generator().manual_seed(sum(shape[:8]))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
    b = torch.randn(Cout, generator=g)
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    res = torch.randn(N, Cout, Ho, Wo, generator=g) if use_res else None
    s = 2.0 ** k
    if which == "input":
        x = x * s
        res = res * s if use_res else None
    else:
        b = b * s
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
    if use_res:
        ref = ref + res.double()
    if relu:
        ref = ref.clamp_min(0)
    floor = FLOOR_UNIT * (w.double().abs().sum(dim=(1, 2, 3)) + (1.0 if use_res else 0.0))   # per output channel
    return x, w, b, res, ref, floor.view(1, Cout, 1, 1)


def _call(fn, shape, x, w, b, res, out, *extra):
    """One op-level conv call on guarded device buffers (tests/guards.py): whatever the return code, the bands around the inputs and the
    output (an _nhwc_out) are intact afterwards and the inputs hold their bits."""
    N, H, W, Cin, Cout, ks, stride, pad, use_res, relu = shape
    gd = Guards(torch.device("cuda:0"))
    xin = gd.inp(x.permute(0, 2, 3, 1))
    rdev = gd.inp(res.permute(0, 2, 3, 1)) if use_res else None
    wc, bc = w.contiguous().numpy(), b.contiguous().numpy()
    rc = fn(xin.data_ptr(), N, H, W, Cin, wc.ctypes.data_as(vp), bc.ctypes.data_as(vp), Cout, ks, ks, stride, pad,
            rdev.data_ptr() if use_res else None, int(relu), out.data_ptr(), *extra)
    torch.cuda.synchronize()
    gd.check()
    assert bands_intact(out.guard_buf, out), "a guard band around the output was written"
    return rc


def _nhwc_out(shape, ref, dtype=torch.float32):
    """The output rows as a guarded payload: every byte 0xFF (NaN), its whole buffer kept at .guard_buf for _call's band check."""
    N, Cout = shape[0], shape[4]
    buf, out = guarded((N, ref.shape[2], ref.shape[3], Cout), dtype, torch.device("cuda:0"))
    out.guard_buf = buf
    return out


def _conv_f32(shape, dtype, x, w, b, res, ref):
    lib = _lib()
    out = _nhwc_out(shape, ref)
    rc = _call(lambda *a: lib.hmv_op_conv2d_ex(0, dtype, *a, None), shape, x, w, b, res, out)
    return rc, out.cpu().permute(0, 3, 1, 2).double()


def _check_x3(rc, got, x, res, ref, floor, who):
    lib = _lib()
    over = x.abs().max().item() > F16_MAX or (res is not None and res.abs().max().item() > F16_MAX)
    if over:
        assert rc == HMV_ERR_RANGE, (who, rc)
        assert who.encode() in lib.hmv_last_error(None) and b"65504" in lib.hmv_last_error(None)
        return None
    assert rc == 0, lib.hmv_last_error(None)
    assert torch.isfinite(got).all()
    excess = ((got - ref).abs() - floor).max().item()
    assert excess <= 3e-6 * ref.abs().max().item(), (who, excess, ref.abs().max().item())
    return (got - ref).abs().max().item()


@pytest.mark.parametrize("which", ["input", "bias"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_conv_modes_across_the_fp16_range(name, which):
    """hmv_op_conv2d_ex in fp32 and f32x3 with the inputs (and residual) -- or the bias alone -- scaled by 2^k, k = -14 .. 18:
    fp32 meets 2e-6 at every k; f32x3 meets 3e-6 plus FLOOR_o (module docstring) while its inputs fit a pair, and returns HMV_ERR_RANGE
    naming the op once one does not (the bias is fp32 in every mode: a huge bias is no range problem, a huge output in fp32 rows neither)."""
    shape = SHAPES[name]
    for k in KS:
        x, w, b, res, ref, floor = _case(shape, k, which)
        rc, got = _conv_f32(shape, 0, x, w, b, res, ref)
        assert rc == 0, _lib().hmv_last_error(None)
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        assert err < 2e-6, (k, err)
        rc, got = _conv_f32(shape, 2, x, w, b, res, ref)
        _check_x3(rc, got, x, res, ref, floor, "hmv_op_conv2d_ex")


def test_split_pair_gemm_kernels_across_the_fp16_range():
    """hmv_op_conv2d_x3: conv_igemm's fused split loop (sel 1) and gemm_x3k16 (sel 2) keep giving the same bits, meet the f32x3 bound in range
    and both report HMV_ERR_RANGE above it."""
    lib = _lib()
    shape = (1, 1, 300, 256, 768, 1, 1, 0, False, False)
    for k in KS:
        x, w, b, res, ref, floor = _case(shape, k, "input")
        outs = []
        for sel in (1, 2):
            out = _nhwc_out(shape, ref)
            kname = ctypes.c_char_p()
            rc = _call(lambda *a: lib.hmv_op_conv2d_x3(0, *a, sel, ctypes.byref(kname), None), shape, x, w, b, res, out)
            got = out.cpu().permute(0, 3, 1, 2).double()
            _check_x3(rc, got, x, res, ref, floor, "hmv_op_conv2d_x3")
            outs.append((rc, out.cpu()))
        assert outs[0][0] == outs[1][0]
        if outs[0][0] == 0:
            assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), k


def test_split_pair_layers_with_huge_weights():
    """A split layer whose weights exceed 2^14 is packed scaled DOWN by a power of two (Loader::finish's acc_shift < 0 branch, "huge folded
    weights"): weights of 2^20 x the unit scale still meet the fp32-grade bar, their fp32 output rows far above 65504 included."""
    for name in ("1x1", "3x3", "residual"):
        shape = SHAPES[name]
        x, w, b, res, _, _ = _case(shape, 0, "input")
        w = w * 2.0 ** 20
        N, H, W, Cin, Cout, ks, stride, pad, use_res, relu = shape
        ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
        ref = (ref + res.double()) if use_res else ref
        ref = ref.clamp_min(0) if relu else ref
        assert w.abs().max().item() > 16384 and ref.abs().max().item() > F16_MAX
        rc, got = _conv_f32(shape, 2, x, w, b, res, ref)
        assert rc == 0, _lib().hmv_last_error(None)
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        assert err < 3e-6, (name, err)


def _f16_outputs(shape, x, w, b, res, ref):
    lib = _lib()
    outs = {}
    for sel in range(9):
        out = _nhwc_out(shape, ref, torch.float16)
        kname = ctypes.c_char_p()
        rc = _call(lambda *a: lib.hmv_op_conv2d_f16(0, *a, sel, ctypes.byref(kname), None), shape, x, w, b, res, out)
        if rc == 1 and 3 <= sel <= 7:
            continue   # no tall-tile form for this shape
        assert rc == 0, (sel, lib.hmv_last_error(None))
        outs[sel] = out.cpu()
    return outs


@pytest.mark.parametrize("which", ["input", "bias"])
@pytest.mark.parametrize("name", list(F16_SHAPES))
def test_fp16_rows_across_the_fp16_range(name, which):
    """hmv_op_conv2d_f16 (fp16 output rows) for every kernel_sel with a form for the shape: outputs whose fp64 value is >= 65520 in
    magnitude are +-inf like torch's .half(), the finite ones meet the fp16 bar, and the bit-identical families stay bit-identical --
    every inf included.  Inputs are scaled while they are finite in fp16 (k <= 12); the bias to 2^18."""
    shape = F16_SHAPES[name]
    ks = [k for k in KS if k >= -6 and (which == "bias" or k <= 12)]
    for k in ks:
        x, w, b, res, ref, _ = _case(shape, k, which)
        outs = _f16_outputs(shape, x, w, b, res, ref)
        for group in F16_GROUPS:
            present = [s for s in group if s in outs]
            for s in present[1:]:
                assert torch.equal(outs[present[0]].view(torch.int16), outs[s].view(torch.int16)), (k, present[0], s)
        refn = ref.permute(0, 2, 3, 1)
        big = refn.abs() >= F16_INF_EDGE * (1 + 2e-3)
        fin = refn.abs() < F16_MAX * (1 - 2e-3)
        scale = refn[fin].abs().max().item() if fin.any() else 1.0
        for sel, o in outs.items():
            o = o.double()
            assert torch.isinf(o[big]).all() and torch.equal(torch.sign(o[big]), torch.sign(refn[big])), (k, sel)
            assert torch.isfinite(o[fin]).all(), (k, sel)
            err = (o[fin] - refn[fin]).abs().max().item() / scale
            assert err < 2e-3, (k, sel, err)
        if which == "bias" and k >= 18:
            assert big.any()   # the sweep does reach the inf region


def test_fp16_conv_with_fp32_output_across_the_range():
    """hmv_op_conv2d_ex(HMV_F16): fp16 operands, fp32 output rows -- a bias far above 65504 is still added in fp32 (finite, fp16 bar)."""
    shape = SHAPES["residual"]
    for k in (0, 8, 14, 18):
        x, w, b, res, ref, _ = _case(shape, k, "bias")
        rc, got = _conv_f32(shape, 1, x, w, b, res, ref)
        assert rc == 0, _lib().hmv_last_error(None)
        assert torch.isfinite(got).all()
        assert (got - ref).abs().max().item() / ref.abs().max().item() < 2e-3


@pytest.mark.parametrize("shape", [(2, 84, 84, 0, 84), (2, 168, 21, 21, 147)])
def test_attention_across_the_fp16_range(shape):
    """hmv_op_attention_x3 next to hmv_op_attention with q, k, v scaled by 2^k.  Softmax is not scale-invariant (logits grow as 2^2k), so the
    fp64 comparison runs where the unit-scale bar of test_attention_kernel_vs_torch applies (k <= 0); below 2^-3 the pair operands add their
    absolute floor (P sums to one: <= 2^-25 per value row, 2^-24 with the logits'); above 65504 the x3 entry returns HMV_ERR_RANGE and the
    fp32 kernel stays finite."""
    lib = _lib()
    B, T, Tq, koff, Tk = shape
    g = torch.Generator().manual_seed(B * 1000 + T)
    base = torch.randn(B, T, 3, 8, 128, generator=g)
    dev = torch.device("cuda:0")
    for k in (-14, -6, -3, 0, 4, 15, 16, 18):
        qkv = base * 2.0 ** k
        gd = Guards(dev)
        qd = gd.inp(qkv.reshape(B, T, 3072))
        q = qkv[:, :Tq, 0].double().permute(0, 2, 1, 3)
        kk = qkv[:, koff:koff + Tk, 1].double().permute(0, 2, 1, 3)
        v = qkv[:, koff:koff + Tk, 2].double().permute(0, 2, 1, 3)
        ref = (torch.softmax(q @ kk.transpose(-1, -2) * 128 ** -0.5, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, Tq, 1024)
        for kernel, op in (("f32", lib.hmv_op_attention), ("x3", lib.hmv_op_attention_x3)):
            out = gd.out((B, Tq, 1024))
            rc = op(0, qd.data_ptr(), B, T, Tq, koff, Tk, out.data_ptr(), None)
            torch.cuda.synchronize()
            gd.check()
            if kernel == "x3" and qkv.abs().max().item() > F16_MAX:
                assert rc == HMV_ERR_RANGE and b"hmv_op_attention_x3" in lib.hmv_last_error(None), (k, rc)
                continue
            assert rc == 0, lib.hmv_last_error(None)
            got = out.cpu().double()
            assert torch.isfinite(got).all(), (kernel, k)
            if k <= 0:
                floor = 2.0 ** -24 if kernel == "x3" else 0.0
                err = ((got - ref).abs() - floor).max().item() / ref.abs().max().item()
                assert err < 4e-6, (kernel, k, err)


@pytest.mark.parametrize("shape", [(2, 16, 32, 40, ((80, 1), (160, 2)), True), (1, 32, 32, 64, ((128, 1),), False)])
def test_hr_fuse_up_fp16_across_the_range(shape):
    """hmv_op_hr_fuse_up(f16 = 1) with the maps scaled by 2^k while fp16 holds them, then the biases up to 2^18: fp16 rows, |ref| >= 65520
    -> +-inf, finite outputs within the fp16 bar of test_hr_fuse_up_vs_torch."""
    lib = _lib()
    N, H, W, C, srcs, relu = shape
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W + C)
    dev = torch.device("cuda:0")
    base0 = torch.randn(N, H, W, C, generator=g)
    xs0 = [torch.randn(N, H >> sh, W >> sh, cs, generator=g) for cs, sh in srcs]
    ws = [torch.randn(C, cs, generator=g) / cs ** 0.5 for cs, _ in srcs]
    bs0 = [torch.randn(C, generator=g) for _ in srcs]
    for which, k in [("input", k) for k in (-6, 0, 8, 12, 13)] + [("bias", k) for k in (14, 16, 18)]:
        si, sb = (2.0 ** k, 1.0) if which == "input" else (1.0, 2.0 ** k)
        base, xs, bs = base0 * si, [x * si for x in xs0], [b * sb for b in bs0]
        ref = base.half().double()
        for x, w, b, (_, sh) in zip(xs, ws, bs, srcs):
            gq = x.half().double() @ w.double().t() + b.double()
            ref = ref + gq.repeat_interleave(1 << sh, dim=1).repeat_interleave(1 << sh, dim=2)
        if relu:
            ref = ref.clamp_min(0)
        gd = Guards(dev)
        dbase = gd.inp(base)
        dxs = [gd.inp(x) for x in xs]
        out = gd.out((N, H, W, C), torch.float16)
        n = len(srcs)
        wn = [w.contiguous().numpy() for w in ws]
        bn = [b.contiguous().numpy() for b in bs]
        rc = lib.hmv_op_hr_fuse_up(0, 1, vp(dbase.data_ptr()), N, H, W, C, n, (vp * n)(*[vp(t.data_ptr()) for t in dxs]),
                                   (ctypes.c_int32 * n)(*[cs for cs, _ in srcs]), (ctypes.c_int32 * n)(*[sh for _, sh in srcs]),
                                   (vp * n)(*[a.ctypes.data_as(vp) for a in wn]), (vp * n)(*[a.ctypes.data_as(vp) for a in bn]), int(relu),
                                   vp(out.data_ptr()), None)
        assert rc == 0, lib.hmv_last_error(None)
        gd.check()
        got = out.cpu().double()
        big = ref.abs() >= F16_INF_EDGE * (1 + 1e-3)
        fin = ref.abs() < F16_MAX * (1 - 1e-3)
        assert torch.isinf(got[big]).all() and torch.equal(torch.sign(got[big]), torch.sign(ref[big])), (which, k)
        assert torch.isfinite(got[fin]).all(), (which, k)
        err = (got[fin] - ref[fin]).abs().max().item() / ref[fin].abs().max().item()
        assert err < 1e-3, (which, k, err)


# ------------------------------------------------------------------ weights

def _key(sd, pattern):
    return next(k for k in sd if re.search(pattern, k))


def test_fp16_refuses_folded_weights_it_cannot_hold():
    """HMV_F16: a folded weight >= 65520 would be packed as inf; hmv_finalize_weights returns HMV_ERR_RANGE naming the state_dict key
    (and hmv_op_conv2d_f16 refuses such a weight the same way).  fp32 and f32x3 take the same weights."""
    from handmvnet_amd import HandMvNet, _lib as L
    cfg, (tp, mp, dp), sd, (x, bbox, intr), _ = load_case("tiny_r50")
    key = _key(sd, r"layer1\.0\.conv2\.weight$")
    bn = key.replace("conv2.weight", "bn2")
    sd = dict(sd)
    wv = np.array(sd[key], dtype=np.float32, copy=True)
    scale = float(np.asarray(sd[bn + ".weight"])[0]) / np.sqrt(float(np.asarray(sd[bn + ".running_var"])[0]) + 1e-5)
    wv[0, 0, 0, 0] = 2.0 * F16_INF_EDGE / scale
    sd[key] = wv
    dev = torch.device("cuda:0")
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(bbox).to(dev), {"intrinsic": torch.from_numpy(intr).to(dev)})
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.half()
    with pytest.raises(L.HandMvError, match=r"error 7: .*" + re.escape(key)):
        m(*args)
    for mode in (m.float, m.float32x3):
        mode()
        m(*args)
        torch.cuda.synchronize()
    lib = _lib()
    shape = SHAPES["3x3"]
    xx, w, b, res, ref, _ = _case(shape, 0, "input")
    w[1, 2, 0, 0] = 70000.0
    out = _nhwc_out(shape, ref, torch.float16)
    rc = _call(lambda *a: lib.hmv_op_conv2d_f16(0, *a, 0, None, None), shape, xx, w, b, res, out)
    assert rc == HMV_ERR_RANGE and b"fp16 range" in lib.hmv_last_error(None)


def test_split_precision_to_out_weights_scaled_by_2_20():
    """f32x3 end to end with one layer's weights x 2^20: the first fusion block's to_out projection (a split-pair GEMM with fp32 output rows
    that LayerNorm folds back to unit scale, layers.py:224-226) is packed with a NEGATIVE acc_shift and tiny_r50 still meets the fp32 bars
    against the f64 oracle, with nothing clamped."""
    from handmvnet_amd import HandMvNet
    from oracle.oracle import Oracle
    cfg, (tp, mp, dp), sd, (x, bbox, intr), _ = load_case("tiny_r50")
    key = _key(sd, r"attn_fusion\.0\.to_out\.weight$")
    sd = dict(sd)
    sd[key] = np.asarray(sd[key], dtype=np.float32) * np.float32(2.0 ** 20)
    assert np.abs(sd[key]).max() > 16384
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.float32x3()
    got = _forward(m, x, bbox, intr)
    m.check_range()
    ref = Oracle(cfg, sd, "f64").forward(x, bbox, intr, stages=True)
    assert rel_l2(got["joints_cam"], ref["joints_cam"]) < TOL_CAM
    assert rel_l2(got["feat0"], ref["feat0"]) < TOL_STAGE


# ------------------------------------------------------------------ end to end

def _forward(m, x, bbox, intr):
    dev = torch.device("cuda:0")
    m.capture_stages(True)
    out = m(torch.from_numpy(x).to(dev), torch.from_numpy(bbox).to(dev), {"intrinsic": torch.from_numpy(intr).to(dev)})
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    for nm in ("feat0", "tokens"):
        res[nm] = m.read_stage(nm).cpu().numpy()
    torch.cuda.synchronize()
    return res


def _scaled(sd, key, factor):
    sd = dict(sd)
    sd[key] = np.asarray(sd[key], dtype=np.float32) * np.float32(factor)
    return sd


def _gamma_above_range(cfg, sd, x, bbox, intr, key):
    """The factor on BN gamma `key` for which the f64 oracle's backbone output (a stored activation) peaks 2 .. 4 x above 65504."""
    from oracle.oracle import Oracle
    f = 1.0
    for _ in range(8):
        peak = float(np.abs(Oracle(cfg, _scaled(sd, key, f), "f64").forward(x, bbox, intr, stages=True)["feat0"]).max())
        if 2.2 * F16_MAX <= peak <= 3.8 * F16_MAX:
            return f, peak
        f *= 3.0 * F16_MAX / peak
    raise AssertionError(f"no gamma factor found: peak {peak} at {f}")


@pytest.mark.parametrize("name", ["tiny_r50", "hr40_tiny"])
def test_activations_above_the_pair_range_end_to_end(name):
    """One BN gamma (layer1.0.bn3 in both backbones) scaled so that the oracle's feat0 peaks 2 .. 4 x above 65504: fp32 meets TOL_CAM /
    TOL_STAGE against the f64 oracle and reports nothing; f32x3 reports the clamp through check_range (FloatingPointError naming the mode);
    the report is sticky over forwards and cleared by the read."""
    from handmvnet_amd import HandMvNet
    from oracle.oracle import Oracle
    cfg, (tp, mp, dp), sd, (x, bbox, intr), _ = load_case(name)
    key = _key(sd, r"layer1\.0\.bn3\.weight$")
    f, peak = _gamma_above_range(cfg, sd, x, bbox, intr, key)
    sd2 = _scaled(sd, key, f)
    ref = Oracle(cfg, sd2, "f64").forward(x, bbox, intr, stages=True)
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd2, strict=True)
    got = _forward(m, x, bbox, intr)
    m.check_range()
    rep = {k: rel_l2(got[k], ref[k]) for k in ("joints_cam", "heatmap", "feat0")}
    assert rep["joints_cam"] < TOL_CAM and rep["heatmap"] < TOL_STAGE and rep["feat0"] < TOL_STAGE, (f, peak, rep)
    m.float32x3()
    _forward(m, x, bbox, intr)
    _forward(m, x, bbox, intr)
    with pytest.raises(FloatingPointError, match="float32x3"):
        m.check_range()
    m.check_range()   # read and cleared


@pytest.mark.parametrize("name", ["tiny_r50", "hr40_tiny"])
def test_activations_below_the_pair_floor_end_to_end(name):
    """The same gamma x 2^-12: that branch of layer1.0 then runs at ~2^-12 of its scale, deep in the region where lo is subnormal.  An
    activation a >= ~2^-12 carries at most 2^-25 / 2^-12 = 2^-13 relative error per conversion there, weighted by its share of each dot
    product; f32x3 stays within TOL_CAM / TOL_STAGE of the f64 oracle (where its in-range error is ~1e-6) and reports nothing."""
    from handmvnet_amd import HandMvNet
    from oracle.oracle import Oracle
    cfg, (tp, mp, dp), sd, (x, bbox, intr), _ = load_case(name)
    key = _key(sd, r"layer1\.0\.bn3\.weight$")
    sd2 = _scaled(sd, key, 2.0 ** -12)
    ref = Oracle(cfg, sd2, "f64").forward(x, bbox, intr, stages=True)
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd2, strict=True)
    m.float32x3()
    got = _forward(m, x, bbox, intr)
    m.check_range()
    rep = {k: rel_l2(got[k], ref[k]) for k in ("joints_cam", "heatmap", "feat0")}
    print(name, rep)
    assert rep["joints_cam"] < TOL_CAM and rep["heatmap"] < TOL_STAGE and rep["feat0"] < TOL_STAGE, rep


def test_tokens_above_the_pair_range_end_to_end():
    """The token features (sample_nets.0: conv + BN + ReLU, nets.py:24-31) shifted by their BN beta until the oracle's tokens peak 2 .. 4 x
    above 65504: the fusion transformer's (hi, lo) pairs clamp in half() and float32x3 alike, and both report it; fp32 reports nothing."""
    from handmvnet_amd import HandMvNet
    from oracle.oracle import Oracle
    cfg, (tp, mp, dp), sd, (x, bbox, intr), _ = load_case("tiny_r50")
    key = _key(sd, r"sample_nets\.0\.conv\.1\.bias$")
    sd2 = dict(sd)
    sd2[key] = np.full_like(np.asarray(sd[key], dtype=np.float32), 3.0 * F16_MAX)
    peak = float(np.abs(Oracle(cfg, sd2, "f64").forward(x, bbox, intr, stages=True)["tokens"]).max())
    assert 2 * F16_MAX <= peak <= 4 * F16_MAX, peak
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd2, strict=True)
    _forward(m, x, bbox, intr)
    m.check_range()
    for mode, label in ((m.half, "half"), (m.float32x3, "float32x3")):
        mode()
        _forward(m, x, bbox, intr)
        with pytest.raises(FloatingPointError, match=label):
            m.check_range()
