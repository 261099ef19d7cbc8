"""The conv launch forms that only a forward issues otherwise, one launch at a time through hmv_op_conv2d_form, against the float64
references of tests/conv_forms_oracle.py (run with -m gpu on an MI355X): dual source, chain +1x1, +maxpool, 4-phase transposed conv,
split-K, pair-output epilogue.  Inside a forward they are judged at 2e-4 rel-L2 on a stage tensor; here every launch is held to the
project's op-level bars (fp32 2e-6, pairs 3e-6, fp16 1e-3 on fp16-rounded operands: conv_forms_oracle.BAR, shown reachable on these
inputs by tests/test_conv_forms_oracle.py), and bit for bit to its unfused partner where the project claims that.

Every device buffer is framed by guard bands (tests/guards.py).  Pad columns of the second source and of the residual (ld > C) hold NaN;
the first source's pad channels are operands of the kernel (the loader gives them zero weights, the layout kernels write zeros), so
they hold zeros.  Outputs start as 0xFF; their columns [C, ld) hold a sentinel that must survive bit for bit.

COVERAGE maps every kernel name tests/golden/launch_ledger.json records on an engine-only record to the case of this file that
reports it, or to the reason no small launch reaches it; the table is checked against the ledger at collection time."""
import ctypes
import math
import re

import pytest
import torch

import conv_forms_oracle as co
from guards import Guards
from test_gpu_launch_ledger import MODES, WORKLOADS, _LEDGER, engine_only_form, reference_layers

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = math.nan
SENT = 1234.5            # exact in fp16 and fp32
F32, F16, X3 = 0, 1, 2
RULE, NEVER, FORCE = 0, 1, 2
OK, ERR_RANGE = 0, 7


def _mod():
    from handmvnet_amd import _lib as L
    return L


def _lib():
    return _mod().load()


def _report(what, text):
    print(f"\n[conv_forms] {what}: {text}")


def _bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _pad(t, ld, fill):
    """Rows of t [..., C] in a stride of ld: [..., ld] with `fill` in [C, ld)."""
    out = torch.full(tuple(t.shape[:-1]) + (ld,), fill, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def _host(t):
    a = t.detach().contiguous().float().numpy()
    return a, a.ctypes.data_as(ctypes.c_void_p)


class Out:
    """An output buffer under guard: 0xFF payload, the sentinel in columns [C, ld) of every plane."""

    def __init__(self, gd, lead, C, ld, dtype, planes=1):
        self.C, self.ld, self.planes = C, ld, planes
        self.t = gd.out(tuple(lead) + (planes * ld,), dtype)
        for p in range(planes):
            self.t[..., p * ld + C:(p + 1) * ld] = SENT
        self.before = self.t.clone()

    def ptr(self):
        return self.t.data_ptr()

    def take(self, touched=True):
        """-> the real columns on the CPU ([..., planes, C] when planes > 1); the sentinel columns must hold their bits."""
        torch.cuda.synchronize()
        ld, C = self.ld, self.C
        for p in range(self.planes):
            assert _bits(self.t[..., p * ld + C:(p + 1) * ld], self.before[..., p * ld + C:(p + 1) * ld]), "a pad column of an output row was written"
        if not touched:
            assert _bits(self.t, self.before), "a refused call wrote its output"
        got = torch.stack([self.t[..., p * ld:p * ld + C] for p in range(self.planes)], dim=-2) if self.planes > 1 else self.t[..., :C]
        got = got.cpu()
        if touched:
            assert not torch.isnan(got.float()).any(), "an output element was not written (or is NaN)"
        return got


def _form(keep, dtype, form, N, H, W, Cin, Cout, x, w, bias, out, ldc, R=1, S=1, stride=1, pad=0, relu=1, **kw):
    """hmv_conv_form_args for one call.  x: a guarded device tensor; w / bias: host tensors (kept alive in `keep`)."""
    L = _mod()
    a = L.HmvConvFormArgs()
    a.struct_size = ctypes.sizeof(L.HmvConvFormArgs)
    a.dtype, a.form, a.N, a.H, a.W, a.Cin, a.Cout, a.R, a.S, a.stride, a.pad, a.relu = dtype, form, N, H, W, Cin, Cout, R, S, stride, pad, relu
    a.in_, a.out, a.ldc = x.data_ptr(), out.ptr() if isinstance(out, Out) else out, ldc
    for name, t in (("w", w), ("bias", bias)) + tuple((k, kw.pop(k)) for k in ("w2", "bias2", "next_w", "next_bias") if k in kw):
        if t is not None:
            arr, p = _host(t)
            keep.append(arr)
            setattr(a, name, p)
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else (v.ptr() if isinstance(v, Out) else v))
    return a


def _call(a, gd, want=OK):
    rc = _lib().hmv_op_conv2d_form(0, ctypes.byref(a), None)
    assert rc == want, (rc, _lib().hmv_last_error(None))
    torch.cuda.synchronize()
    gd.check()
    return a.kernel_name.decode() if a.kernel_name else None


REPORTED = {}   # case id -> kernel names its launches reported


def _note(request, *names):
    REPORTED.setdefault(request.node.name, set()).update(names)
    missing = {k for k, v in COVERAGE.items() if v[0] == request.node.name} - REPORTED[request.node.name]
    return missing


# ------------------------------------------------------------------ dual source
def _run_dual(case, t, dtype, routes):
    planes, inpl, outc, s, _, N, Ho, Wo, H2, W2 = case
    gd, keep = Guards(DEV), []
    ld2, ldc = inpl + 8, outc + 8
    x = gd.inp(t["x"])
    x2 = gd.inp(_pad(t["x2"], ld2, NAN))
    out = Out(gd, (N, Ho, Wo), outc, ldc, torch.float16 if dtype == F16 else torch.float32)
    a = _form(keep, dtype, _mod().HMV_FORM_DUAL, N, Ho, Wo, planes, outc, x, t["w1"], t["b1"], out, ldc, w2=t["w2"], bias2=t["b2"],
              in2=x2, Cin2=inpl, H2=H2, W2=W2, stride2=s, ld_in2=ld2, **routes)
    name = _call(a, gd)
    return out.take(), name


DUAL_CASES = list(co.dual_cases())


@pytest.mark.parametrize("case", DUAL_CASES, ids=lambda c: f"{c[0]}+{c[1]}-{c[4]}")
def test_dual(case, request):
    """conv3 + downsample as one GEMM over [t2 | x(strided)], on every kernel that takes the shape, each against float64.
    Bit for bit (test_gpu_parity.py::test_stream_kernel_is_bit_identical: a special kernel keeps its small-launch partner's operand roles,
    accumulation order and epilogue; kernels.h says the same of every family): conv_stream_f16 == conv_gemm8_f16<..., dual> == conv_igemm_f16
    (K = 128, 384); conv_gemm8_f16<..., m16> == conv_m16_f16 (K = 768); conv_gemm8's persistent form == its plain form (include/handmv.h,
    kernel_sel 8); fp32: conv_stream_f32 == conv_igemm_f32 (K = 128)."""
    planes, inpl, outc, s = case[:4]
    t = co.dual_inputs(case)
    m16 = planes + inpl >= 768
    names = set()
    # fp32
    ref = co.dual_ref(t, s, "f32")
    got, k_ig = _run_dual(case, t, F32, dict(route_stream=NEVER))
    e = co.check(got, ref, co.BAR["f32"], f"dual f32 {k_ig}")
    assert k_ig == "conv_igemm_f32<64x64,1x1>", k_ig
    names.add(k_ig)
    if planes + inpl == 128:
        got_s, k_s = _run_dual(case, t, F32, dict(route_stream=FORCE))
        assert k_s == "conv_stream_f32<64x256,k128,dual>", k_s
        e = max(e, co.check(got_s, ref, co.BAR["f32"], f"dual f32 {k_s}"))
        names.add(k_s)
        assert _bits(got_s, got), (k_s, k_ig)
    # fp16
    ref16 = co.dual_ref(t, s, "f16")
    base, k_b = _run_dual(case, t, F16, dict(route_stream=NEVER, route_gemm8=NEVER))
    assert k_b == ("conv_m16_f16<64x64,1x1,dual>" if m16 else "conv_igemm_f16<64x64,1x1>"), k_b
    e16 = co.check(base, ref16, co.BAR["f16"], f"dual f16 {k_b}")
    names.add(k_b)
    if not m16:
        got_s, k_s = _run_dual(case, t, F16, dict(route_stream=FORCE))
        assert k_s == ("conv_stream_f16<128x256,k128,dual>" if planes + inpl == 128 else "conv_stream_f16<64x256,k384,dual>"), k_s
        e16 = max(e16, co.check(got_s, ref16, co.BAR["f16"], f"dual f16 {k_s}"))
        assert _bits(got_s, base), (k_s, k_b)
        names.add(k_s)
    g8, k_8 = _run_dual(case, t, F16, dict(route_stream=NEVER, route_gemm8=FORCE, gemm8_persist=NEVER))
    assert k_8.startswith("conv_gemm8_f16<") and "dual" in k_8 and "persistent" not in k_8 and ("m16" in k_8) == m16, k_8
    e16 = max(e16, co.check(g8, ref16, co.BAR["f16"], f"dual f16 {k_8}"))
    g8p, k_8p = _run_dual(case, t, F16, dict(route_stream=NEVER, route_gemm8=FORCE, gemm8_persist=FORCE))
    assert k_8p.startswith("conv_gemm8_f16<") and "dual" in k_8p, k_8p
    e16 = max(e16, co.check(g8p, ref16, co.BAR["f16"], f"dual f16 {k_8p}"))
    assert _bits(g8p, g8), (k_8p, k_8)
    if m16:
        assert _bits(g8, base), (k_8, k_b)
        assert k_8p == "conv_gemm8_f16<256x256,1x1,dual,m16,persistent>", k_8p
    else:
        assert k_8 == "conv_gemm8_f16<256x256,1x1,dual>" and _bits(g8, base), (k_8, k_b)
    names.update((k_8, k_8p))
    _report(f"dual {case[:5]} M {case[5] * case[6] * case[7]}", f"f32 {e:.3e} of {co.BAR['f32']:g}, f16 {e16:.3e} of {co.BAR['f16']:g}; {sorted(names)}")
    assert not _note(request, *names)


# ------------------------------------------------------------------ chain +1x1
def _conv_f16(x, N, H, W, Cin, w, b, Cout, res, relu, sel=1):
    """hmv_op_conv2d_f16 of one 1x1 conv (or the 4x4 pad-2 stem conv) -> (fp16 rows of its own output map on the CPU, kernel name)."""
    lib = _lib()
    gd = Guards(DEV)
    xin = gd.inp(x)
    rdev = gd.inp(res) if res is not None else None
    R = w.shape[2] if w.dim() == 4 else 1
    pad = 2 if R == 4 else 0
    out = gd.out((N, H + 2 * pad - R + 1, W + 2 * pad - R + 1, Cout), torch.float16)     # the conv's own map
    (wa, wp), (ba, bp) = _host(w), _host(b)
    k = ctypes.c_char_p()
    rc = lib.hmv_op_conv2d_f16(0, xin.data_ptr(), N, H, W, Cin, wp, bp, Cout, R, R, 1, pad, rdev.data_ptr() if res is not None else None,
                               int(relu), out.data_ptr(), sel, ctypes.byref(k), None)
    assert rc == 0, lib.hmv_last_error(None)
    torch.cuda.synchronize()
    gd.check()
    return out.cpu(), k.value.decode()


@pytest.mark.parametrize("size", co.CHAIN_SIZES, ids=lambda s: s[0])
@pytest.mark.parametrize("kind", co.CHAIN_KINDS, ids=lambda k: k[0])
def test_chain(kind, size, request):
    """A conv3 launch that also computes the next block's conv1: both outputs equal, bit for bit, hmv_op_conv2d_f16 of the first conv
    (the two-source one: the unchained dual launch on conv_igemm) followed by hmv_op_conv2d_f16 of the second on that output, and both
    meet float64 at the fp16 bar."""
    name, dual, ncout = kind
    _, N, H, W = size
    t = co.chain_inputs(kind, size)
    L = _mod()
    gd, keep = Guards(DEV), []
    ldc = 264
    x = gd.inp(t["x"])
    out = Out(gd, (N, H, W), 256, ldc, torch.float16)
    nxt = Out(gd, (N, H, W), ncout, ncout, torch.float16)
    kw = dict(next_w=t["wn"], next_bias=t["bn"], next_out=nxt, next_cout=ncout, route_stream=FORCE)
    if dual:
        x2 = gd.inp(_pad(t["x2"], 72, NAN))
        a = _form(keep, F16, L.HMV_FORM_DUAL | L.HMV_FORM_CHAIN, N, H, W, 64, 256, x, t["w1"], t["b1"], out, ldc, w2=t["w2"], bias2=t["b2"],
                  in2=x2, Cin2=64, H2=H, W2=W, stride2=1, ld_in2=72, **kw)
        want = "conv_stream_f16<128x256,k128,dual,+1x1:64>"
    else:
        res = gd.inp(_pad(t["res"], 264, NAN))
        a = _form(keep, F16, L.HMV_FORM_CHAIN, N, H, W, 64, 256, x, t["w1"], t["b1"], out, ldc, residual=res, ldr=264, **kw)
        want = f"conv_stream_f16<128x256,k64,res,+1x1:{ncout}>"
    kname = _call(a, gd)
    assert kname == want, kname
    y, z = out.take(), nxt.take()
    # the two launches.  (The two-source conv has no hmv_op_conv2d_f16 form: its bitwise partner is the same launch without the chain on
    # conv_igemm; the single conv over [x | x2] that hmv_op_conv2d_f16 can express is a 128 -> 256 layer of the 16x16x32-MFMA family, another
    # summation order, and is held to the same float64 reference instead)
    if dual:
        g2, keep2 = Guards(DEV), []
        o2 = Out(g2, (N, H, W), 256, ldc, torch.float16)
        a2 = _form(keep2, F16, L.HMV_FORM_DUAL, N, H, W, 64, 256, g2.inp(t["x"]), t["w1"], t["b1"], o2, ldc, w2=t["w2"], bias2=t["b2"],
                   in2=g2.inp(_pad(t["x2"], 72, NAN)), Cin2=64, H2=H, W2=W, stride2=1, ld_in2=72, route_stream=NEVER, route_gemm8=NEVER)
        k1 = _call(a2, g2)
        y2 = o2.take()
        xa, wa = torch.cat([t["x"], t["x2"]], dim=3), torch.cat([t["w1"], t["w2"]], dim=1)
        y3, k3 = _conv_f16(xa, N, H, W, 128, wa, (t["b1"].double() + t["b2"].double()).float(), 256, None, True)
        co.check(y3, co.chain_first_ref(t, dual), co.BAR["f16"], f"chain {name}: {k3} over [x | x2]")
    else:
        y2, k1 = _conv_f16(t["x"], N, H, W, 64, t["w1"], t["b1"], 256, t["res"], True)
    z2, k2 = _conv_f16(y2.float(), N, H, W, 256, t["wn"], t["bn"], ncout, None, True)
    assert k1.startswith("conv_igemm_f16") and k2.startswith("conv_igemm_f16"), (k1, k2)
    assert _bits(y, y2), (kname, k1)
    assert _bits(z, z2), (kname, k2)
    e1 = co.check(y, co.chain_first_ref(t, dual), co.BAR["f16"], f"chain {name} first output")
    e2 = co.check(z, co.chain_next_ref(y, t), co.BAR["f16"], f"chain {name} chained output")
    _report(f"chain {name} {size}", f"{kname}: first {e1:.3e}, chained {e2:.3e} of {co.BAR['f16']:g}; partners {k1}, {k2}")
    assert not _note(request, kname)


# ------------------------------------------------------------------ +maxpool
@pytest.mark.parametrize("size", co.POOL_MAPS, ids=lambda s: "x".join(map(str, s)))
def test_pool(size, request):
    """The fp16 space-to-depth stem with MaxPool2d(3, 2, 1) in the launch (conv_hs.hip): bit for bit hmv_op_conv2d_f16 followed by
    hmv_op_maxpool in fp16 mode; float64 at the fp16 bar (the conv map's reference pooled)."""
    N, H, W = size
    t = co.pool_inputs(size)
    L = _mod()
    gd, keep = Guards(DEV), []
    x = gd.inp(t["x"])
    hp, wp = H // 2, W // 2
    out = Out(gd, (N, hp, wp), 64, 64, torch.float16)
    a = _form(keep, F16, L.HMV_FORM_POOL, N, H, W, 12, 64, x, t["w"], t["b"], out, 64, R=4, S=4, pad=2, Ho=H, Wo=W, ld_in=16, pool_h=hp, pool_w=wp,
              route_hs=FORCE)
    kname = _call(a, gd)
    assert kname == "conv_hs_f16<4x4,16->64,+maxpool>", kname
    got = out.take()
    # the two launches: the same conv with its 4 pad channels as channels of zero weight, its map cut to H x W, then the pool
    w16 = torch.zeros(64, 16, 4, 4)
    w16[:, :12] = t["w"]
    full, k1 = _conv_f16(t["x"], N, H, W, 16, w16, t["b"], 64, None, True)
    assert tuple(full.shape) == (N, H + 1, W + 1, 64) and k1.startswith("conv_igemm_f16"), (full.shape, k1)
    cut = full[:, :H, :W, :].contiguous()
    g2 = Guards(DEV)
    cin, pout = g2.inp(cut), g2.out((N, hp, wp, 64), torch.float16)
    assert _lib().hmv_op_maxpool(0, 1, cin.data_ptr(), N, H, W, 64, pout.data_ptr(), None) == 0, _lib().hmv_last_error(None)
    torch.cuda.synchronize()
    g2.check()
    assert _bits(got, pout.cpu()), kname
    e0 = co.check(cut, co.stem_map_ref(t), co.BAR["f16"], "stem conv map")
    e = co.check(got, co.pool_ref(co.stem_map_ref(t)), co.BAR["f16"], f"pooled stem {size}")
    assert _bits(got, co.pool_ref(cut.float()).half())      # the pool of the rounded map, on the CPU
    _report(f"pool {size}", f"{kname}: {e:.3e} (conv map {e0:.3e}) of {co.BAR['f16']:g}")
    assert not _note(request, kname)


# ------------------------------------------------------------------ 4-phase transposed conv
@pytest.mark.parametrize("N", co.PHASE_N)
@pytest.mark.parametrize("hw", co.PHASE_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cin", co.PHASE_CIN)
@pytest.mark.parametrize("mode", ["f32", "f16", "x3"])
def test_phases(mode, cin, hw, N, request):
    """ConvTranspose2d(4, 2, 1) + ReLU as four sub-pixel 2x2 convs: the one merged launch == the four launches, bit for bit, and both
    against conv_transpose2d itself in float64; output rows of 136 columns keep their sentinel beyond the 128 channels.  Pairs: the four
    launches only, as the engine issues them, hi + lo against float64."""
    H, W = hw
    t = co.phase_inputs(cin, hw, N)
    L = _mod()
    dtype = {"f32": F32, "f16": F16, "x3": X3}[mode]
    ref = co.phase_ref(t, mode)
    ldc, C = 136, co.PHASE_COUT
    want = "conv_igemm_f32<64x64,taps>" if mode == "f32" else "conv_igemm_f16<64x64,taps>"
    outs = []
    for merged in ((0,) if mode == "x3" else (0, 1)):
        gd, keep = Guards(DEV), []
        x = gd.inp(t["x"])
        out = Out(gd, (N, 2 * H, 2 * W), C, ldc, torch.float32 if mode == "f32" else torch.float16, planes=2 if mode == "x3" else 1)
        form = L.HMV_FORM_PHASES | (L.HMV_FORM_PAIR_OUT if mode == "x3" else 0)
        a = _form(keep, dtype, form, N, H, W, cin, C, x, t["w"], t["b"], out, ldc, R=4, S=4, stride=2, pad=1, merged=merged)
        kname = _call(a, gd)
        assert kname == want, kname
        got = out.take()
        if mode == "x3":
            hi, lo = got[..., 0, :], got[..., 1, :]
            assert bool((lo.double().abs() <= co.ulp_f16(hi) / 2).all())
            got = hi.double() + lo.double()
        e = co.check(got, ref, co.BAR[mode], f"phases {mode} cin {cin} {hw} N {N} merged {merged}")
        outs.append(got)
    if len(outs) == 2:
        assert _bits(outs[0], outs[1]), "merged launch != four launches"
    _report(f"phases {mode} cin {cin} {hw} N {N}", f"{kname}: {e:.3e} of {co.BAR[mode]:g}")
    assert not _note(request, kname)


# ------------------------------------------------------------------ split-K
@pytest.mark.parametrize("rows", co.SPLITK_ROWS)
@pytest.mark.parametrize("cout", co.SPLITK_COUT)
@pytest.mark.parametrize("K", co.SPLITK_K)
def test_splitk(K, cout, rows, request):
    """Slices of a long fp32 reduction: S = 4, the one count the engine's rule (Runner::splitk_slices) gives these shapes -- Kpad >= 1024 in
    whole 128-column units, Kpad / S a multiple of 32.  Each slab slice against its float64 partial GEMM, hmv_op_splitk_reduce of the slab
    against the full GEMM, both at 2e-6; the pad columns between the rows of the slab hold their sentinel; a count the rule never gives
    is refused."""
    t = co.splitk_inputs(K, cout, rows)
    L = _mod()
    full = co.gemm_ref(t)
    ldc = (cout + 3) // 4 * 4 + 4
    for S in (4,):
        assert K % (128 * S) == 0 and (K // S) % 32 == 0
        gd, keep = Guards(DEV), []
        a_dev = gd.inp(t["a"])
        slab = Out(gd, (S, rows), cout, ldc, torch.float32)
        a = _form(keep, F32, L.HMV_FORM_SPLITK, rows, 1, 1, K, cout, a_dev, t["w"], t["b"], slab, ldc, relu=0, slices=S)
        kname = _call(a, gd)
        assert kname == "conv_igemm_f32<64x64,1x1>", kname
        got = slab.take()
        worst = max(co.check(got[i], co.splitk_slice_ref(t, S, i), co.BAR["f32"], f"split-K {K} -> {cout}, {rows} rows: slice {i} of {S}") for i in range(S))
        bias = gd.inp(_pad(t["b"], ldc, 0.0))
        red = Out(gd, (rows,), cout, ldc, torch.float32)
        rc = _lib().hmv_op_splitk_reduce(0, slab.ptr(), S, rows, ldc, cout, bias.data_ptr(), None, 0, 0, 0, 0, red.ptr(), ldc, None)
        assert rc == 0, _lib().hmv_last_error(None)
        gd.check()
        slab.take()
        e = co.check(red.take(), full, co.BAR["f32"], f"split-K {K} -> {cout}, {rows} rows, S {S}: reduced")
        _report(f"split-K {K} -> {cout}, {rows} rows, S {S}", f"{kname}: slices {worst:.3e}, reduced {e:.3e} of {co.BAR['f32']:g}")
    # a slice count the engine's rule never gives is refused, nothing written
    gd, keep = Guards(DEV), []
    a_dev = gd.inp(t["a"])
    slab = Out(gd, (2, rows), cout, ldc, torch.float32)
    a = _form(keep, F32, L.HMV_FORM_SPLITK, rows, 1, 1, K, cout, a_dev, t["w"], t["b"], slab, ldc, relu=0, slices=2)
    _call(a, gd, want=1)
    assert b"hmv_op_conv2d_form" in _lib().hmv_last_error(None)
    slab.take(touched=False)
    assert not _note(request, kname)


# ------------------------------------------------------------------ pair-output epilogue
def _run_pair(t, K, cout, rows, route, want_rc=OK):
    L = _mod()
    gd, keep = Guards(DEV), []
    ldc = cout + 16
    a_dev = gd.inp(t["a"])
    out = Out(gd, (rows,), cout, ldc, torch.float16, planes=2)
    a = _form(keep, X3, L.HMV_FORM_PAIR_OUT, rows, 1, 1, K, cout, a_dev, t["w"], t["b"], out, ldc, relu=0, route_x3k16=route)
    kname = _call(a, gd, want=want_rc)
    got = out.take()
    return got[..., 0, :], got[..., 1, :], kname


@pytest.mark.parametrize("rows", co.PAIR_ROWS)
@pytest.mark.parametrize("shape", co.PAIR_SHAPES, ids=lambda s: f"{s[0]}->{s[1]}")
def test_pair_out(shape, rows, request):
    """A split layer that writes (hi, lo) fp16 pairs, through conv_igemm's fused split loop and through gemm_x3k16: hi + lo within 3e-6 of
    float64, the same bits from both kernels (test_split_pair_gemm_large_tiles_by_kernel_sel claims that for their fp32 rows),
    |lo| <= ulp_fp16(hi) / 2 everywhere; HMV_OK -- and HMV_ERR_RANGE once a weight row is scaled so that an output leaves the fp16 range."""
    K, cout = shape
    t = co.pair_inputs(K, cout, rows)
    v = co.gemm_ref(t)
    hi1, lo1, k1 = _run_pair(t, K, cout, rows, NEVER)
    hi2, lo2, k2 = _run_pair(t, K, cout, rows, FORCE)
    assert k1 == "conv_igemm_f16<64x64,1x1>" and k2 == "gemm_x3k16_f16<256x256>", (k1, k2)
    assert _bits(hi1, hi2) and _bits(lo1, lo2), (k1, k2)
    e = co.check(hi1.double() + lo1.double(), v, co.BAR["x3"], f"pair-out {K} -> {cout}, {rows} rows")
    assert bool((lo1.double().abs() <= co.ulp_f16(hi1) / 2).all())
    big = dict(t)
    big["w"] = t["w"].clone()
    big["w"][3] *= 1e6
    assert float(co.gemm_ref(big)[:, 3].abs().max()) > co.F16_MAX
    for route in (NEVER, FORCE):
        bh, bl, _ = _run_pair(big, K, cout, rows, route, want_rc=ERR_RANGE)
        assert b"hmv_op_conv2d_form" in _lib().hmv_last_error(None)
        assert float(bh[:, 3].float().abs().max()) == co.F16_MAX and not bool(bl[bh[:, 3].float().abs() == co.F16_MAX, 3].any())
    _report(f"pair-out {K} -> {cout}, {rows} rows", f"{k1} == {k2}: hi + lo {e:.3e} of {co.BAR['x3']:g}")
    assert not _note(request, k1, k2)


# ------------------------------------------------------------------ completeness
# kernel name on an engine-only ledger record -> (case of this file that must report it, None) or (None, why no small launch reaches it)
_BY_M = "conv_igemm's tile is conv_pick_tile's choice from the pixel count: this one needs thousands of rows; the 64x64 case runs the same template"
COVERAGE = {
    "conv_hs_f16<4x4,16->64,+maxpool>": ("test_pool[2x16x16]", None),
    "conv_igemm_f16<64x64,taps>": ("test_phases[f16-256-4x4-1]", None),
    "conv_igemm_f32<64x64,taps>": ("test_phases[f32-256-4x4-1]", None),
    "conv_stream_f16<128x256,k64,res,+1x1:128>": ("test_chain[res128-m35]", None),
    "conv_stream_f16<128x256,k64,res,+1x1:64>": ("test_chain[res64-m35]", None),
    "conv_stream_f16<128x256,k128,dual,+1x1:64>": ("test_chain[dual64-m35]", None),
    "conv_gemm8_f16<256x256,1x1,dual,m16,persistent>": ("test_dual[256+512-a]", None),
    "conv_m16_f16<64x64,1x1,dual>": ("test_dual[256+512-a]", None),
    "conv_m16_f16<128x128,1x1,dual>": (None, "conv_m16's tile follows the pixel count like conv_igemm's; the 64x64 case runs the same template"),
    "conv_igemm_f16<64x64,1x1>": ("test_dual[64+64-a]", None),
    "conv_igemm_f16<128x128,1x1>": (None, _BY_M),
    "conv_igemm_f32<64x64,1x1>": ("test_dual[64+64-a]", None),
    "conv_igemm_f32<128x128,1x1>": (None, _BY_M),
    "conv_igemm_f32<256x256,1x1>": (None, _BY_M),
    "conv_stream_f16<64x256,k384,dual>": ("test_dual[128+256-a]", None),
    "conv_stream_f32<64x256,k128,dual>": ("test_dual[64+64-a]", None),
    "gemm_x3k16_f16<256x256>": ("test_pair_out[544->3072-21]", None),
}


def _ledger_names():
    from handmvnet_amd.spec import config_from_params, state_dict_layout
    from make_launch_ledger import workload_params
    names = {}
    for wl, w in WORKLOADS.items():
        cfg = config_from_params(*workload_params(w))
        layers = reference_layers(cfg, dict(state_dict_layout(cfg)), w["B"], w["size"])
        for mode in MODES:
            for rec in _LEDGER["forwards"][wl][mode]:
                parts = rec["layer"].split("+")
                if parts[-1] == "up":
                    continue
                form = engine_only_form(rec, layers[re.sub(r"\.phase\d$", "", parts[0])], mode)
                if form:
                    names.setdefault(rec["kernel"], set()).add(form)
    return names


LEDGER_NAMES = _ledger_names()
assert set(LEDGER_NAMES) == set(COVERAGE), (sorted(set(LEDGER_NAMES) - set(COVERAGE)), sorted(set(COVERAGE) - set(LEDGER_NAMES)))
assert all((case is None) != (why is None) for case, why in COVERAGE.values())


def test_every_engine_only_kernel_has_a_case(request):
    """Every kernel name the ledger records on an engine-only record is reported by the case COVERAGE names (each such case asserts that
    itself, from the names its launches reported), or is listed with the reason; the cases named exist in this collection."""
    ids = ({f"test_dual[{c[0]}+{c[1]}-{c[4]}]" for c in DUAL_CASES} | {f"test_chain[{k[0]}-{z[0]}]" for k in co.CHAIN_KINDS for z in co.CHAIN_SIZES} |
           {"test_pool[" + "x".join(map(str, z)) + "]" for z in co.POOL_MAPS} |
           {f"test_phases[{m}-{c}-{h}x{w}-{n}]" for m in ("f32", "f16", "x3") for c in co.PHASE_CIN for h, w in co.PHASE_MAPS for n in co.PHASE_N} |
           {f"test_pair_out[{k}->{c}-{r}]" for k, c in co.PAIR_SHAPES for r in co.PAIR_ROWS})
    collected = {item.name for item in request.session.items}
    assert len(collected) < 50 or ids <= collected, sorted(ids - collected)[:5]   # (a whole-file or whole-suite run: the ids above are the real ones)
    reached = {k: v[0] for k, v in COVERAGE.items() if v[0]}
    assert set(reached.values()) <= ids, sorted(set(reached.values()) - ids)
    unreached = {k: v[1] for k, v in COVERAGE.items() if not v[0]}
    print(f"\n[conv_forms] {len(reached)} of {len(COVERAGE)} engine-only kernel names are reported by a case; {len(unreached)} are not reachable at a small size:")
    for k, why in unreached.items():
        print(f"    {k} ({', '.join(sorted(LEDGER_NAMES[k]))}): {why}")
