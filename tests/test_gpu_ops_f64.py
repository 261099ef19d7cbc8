"""The non-GEMM kernels of a forward, each alone through its hmv_op_* entry, against the float64 references of tests/ops_oracle.py
(run with -m gpu on an MI355X).  Inside a forward these kernels are judged by 2e-4 rel-L2 on a stage tensor and 0.05 px on the
coordinates; here each is held to what fp32 arithmetic can do (bars and their derivations: ops_oracle.py, DESIGN.md "Op-level tests of the
non-GEMM kernels"; test_ops_oracle.py shows torch fp32 inside every bar on these very inputs), bit for bit where the operation is exact.

Every device buffer is framed by guard bands (tests/guards.py): inputs are NaN beyond their payload and in the pad columns of wide rows,
outputs start as 0xFF bytes, columns an op does not own hold a sentinel that must survive bit for bit, and Guards.check() runs after
every call.

Launcher (kernel)                                               test
  launch_nchw_to_nhwc4 / _nhwc8_f16 / _nhwc_split                 test_input_layout[kind 0], test_input_layout_over_the_grid_cap
  launch_nchw_to_s2d (nchw_to_s2d_kernel<0 | 1 | 2>)              test_input_layout[kind 1], test_input_layout_over_the_grid_cap
  launch_maxpool3s2 / _f16 / _split                               test_maxpool, test_maxpool_over_the_grid_cap
    (maxpool3s2_kernel, maxpool3s2_f16_kernel, maxpool3s2_split_kernel)
  launch_soft_argmax (soft_argmax_frame_kernel: h w <= 1024;      test_soft_argmax (4x4 .. 32x32: frame kernel; 33x32, 16x80: wave kernel)
                      soft_argmax_kernel: above)
  launch_sample_gather (sample_gather_kernel)                     test_sample_gather
  launch_sample_blend (sample_blend_kernel)                       test_sample_blend
  launch_tokens_finalize (tokens_finalize_kernel)                 test_tokens_finalize (uniform form)
  launch_tokens_finalize_views (tokens_finalize_views_kernel)     test_tokens_finalize (ragged form)
  launch_layernorm (layernorm_kernel<0>)                          test_layernorm, test_layernorm_refuses_rows_beyond_1024_columns
  launch_splitk_reduce (splitk_reduce_kernel)                     test_splitk_reduce
  launch_splitk_layernorm (layernorm_kernel<4>)                   test_splitk_layernorm_is_reduce_then_layernorm_bit_for_bit
  launch_add_pe (add_pe_kernel) / launch_add_pe_views (..._views) test_add_pe
  launch_cheb_mix (cheb_mix_kernel)                               test_cheb_mix
The fused tail kernels (fusion_kernels.hip) have float64 tests of their own: test_gpu_tail_f64.py."""
import math

import pytest
import torch

import ops_oracle as oo
from guards import Guards

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NJ = oo.NJ
SENT = 12345.678   # what columns outside an op's payload hold before the call
SAT_IDLE = 7       # a range word nobody raised keeps this


def _lib():
    from handmvnet_amd import _lib as L
    return L.load()


def _ok(rc):
    assert rc == 0, _lib().hmv_last_error(None)
    torch.cuda.synchronize()


def _p(t):
    return None if t is None else t.data_ptr()


def _wide(t, ld, fill=math.nan):
    """t [rows][c] -> [rows][ld] with `fill` in the columns from c on."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _prefilled(gd, host):
    """An output buffer that starts as `host` (sentinels where the op must not write)."""
    p = gd.out(host.shape, host.dtype)
    p.copy_(host)
    return p


def _sat(gd):
    s = gd.out((1,), torch.int32)
    s.fill_(SAT_IDLE)
    return s


def _bits(got, want, what=""):
    assert oo.bits_equal(got.cpu(), want), what


def _report(what, worst):
    print(f"\n[ops_f64] {what}: {worst}")


# ------------------------------------------------------------------ input layout
def _layout_ref(x, kind, mode):
    return oo.s2d_rows(x, mode) if kind else oo.nhwc_rows(x, mode)


def _run_layout(x, kind, mode):
    gd = Guards(DEV)
    want = _layout_ref(x, kind, mode)
    out, sat = gd.out(want.shape, want.dtype), _sat(gd)
    N, _, H, W = x.shape
    _ok(_lib().hmv_op_input_layout(0, kind, mode, _p(gd.inp(x)), N, H, W, _p(out), _p(sat), None))
    gd.check()
    return out.cpu(), want, int(sat.item())


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", oo.FRAME_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_input_layout(shape, kind, mode):
    """Bitwise against indexing on the CPU: fp16 round-to-nearest-even, pairs hi = fp16(clamp v), lo = fp16(v - hi), pad channels and the odd
    row / column of the space-to-depth image exactly 0; the range word rises for one value above 65504 in the pair modes and only then."""
    x = oo.frames(*shape)
    got, want, sat = _run_layout(x, kind, mode)
    assert oo.bits_equal(got, want) and sat == SAT_IDLE
    x = x.clone()
    x.view(-1)[x.numel() // 2] = 70000.0
    got, want, sat = _run_layout(x, kind, mode)
    assert oo.bits_equal(got, want)
    assert sat == (1 if mode == 2 else SAT_IDLE)


@pytest.mark.parametrize("kind,mode", [(0, 0), (0, 1), (0, 2), (1, 0)])
def test_input_layout_over_the_grid_cap(kind, mode):
    """One workgroup's worth of pixels more than the launcher's grid covers in one pass: the grid-stride loop takes a second trip."""
    N, H, W = oo.FRAME_SHAPE_OVER_CAP[kind]
    x = oo.frames(N, H, W)
    got, want, sat = _run_layout(x, kind, mode)
    assert oo.bits_equal(got, want) and sat == SAT_IDLE


# ------------------------------------------------------------------ max-pool
def _run_pool(rows, mode):
    gd = Guards(DEV)
    N, H, W, K = rows.shape
    C = K // 2 if mode == 2 else K
    Ho, Wo = oo.pool_out_hw(H, W)
    out = gd.out((N, Ho, Wo, K), rows.dtype)
    _ok(_lib().hmv_op_maxpool(0, mode, _p(gd.inp(rows)), N, H, W, C, _p(out), None))
    gd.check()
    return out.cpu()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", oo.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool(shape, mode):
    """maxpool3s2_kernel (0), maxpool3s2_f16_kernel (1), maxpool3s2_split_kernel (2): bitwise MaxPool2d(3, 2, 1) -- max is exact -- on all
    negative, mixed and all-equal finite values.  All negative: a pool that pads with 0 instead of -inf is wrong on every border pixel."""
    for kind in oo.POOL_KINDS:
        rows = oo.pool_rows(oo.pool_values(shape, kind), mode)
        want = oo.pool_ref(rows, mode)
        assert oo.bits_equal(_run_pool(rows, mode), want), kind
        if kind == "negative":
            assert float(want[..., :shape[3]].float().max()) < 0   # (the hi halves in pair rows)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_maxpool_over_the_grid_cap(mode):
    """Just more 16-byte channel groups of output than the grid covers in one pass (many tiny maps, so the buffers stay small)."""
    shape = oo.POOL_SHAPE_OVER_CAP[mode]
    rows = oo.pool_rows(oo.pool_values(shape, "negative"), mode)
    F = torch.nn.functional
    if mode == 2:
        v = rows[..., :shape[3]].float() + rows[..., shape[3]:].float()
        want = torch.cat(oo.split_f16(F.max_pool2d(v.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)), dim=-1)
    else:
        want = F.max_pool2d(rows.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(rows.dtype)
    assert oo.bits_equal(_run_pool(rows, mode), want.contiguous())


# ------------------------------------------------------------------ soft-argmax
@pytest.mark.parametrize("N", oo.SAM_BATCHES)
@pytest.mark.parametrize("hw", oo.SAM_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_soft_argmax(hw, N):
    """soft_argmax_frame_kernel up to 32 x 32 (9 x 13: pixel slots without a pixel), soft_argmax_kernel from 33 x 32 on (N = 3: 63 waves, a
    last workgroup that is not full).  Reference: z = fp32(raw * 1000), softmax and expectations in float64; bar max(8 e32, 8 ulp of the
    largest coordinate).  NaN in the pad channels changes nothing; hm_nchw is the logits transposed, bit for bit, and may be null."""
    h, w = hw
    worst = 0.0
    for scale in oo.SAM_SCALES:
        hm = oo.heatmap_logits(N, h, w, scale)
        ref = oo.soft_argmax_ref(hm)
        e32 = float((oo.soft_argmax_ref(hm, torch.float32).double() - ref).abs().max())
        bar = oo.soft_argmax_bar(e32, h, w)
        results = []
        for with_nchw in (True, False):
            gd = Guards(DEV)
            coords, crop = gd.out((N, NJ, 2)), gd.out((N, NJ, 2))
            nchw = gd.out((N, NJ, h, w)) if with_nchw else None
            _ok(_lib().hmv_op_soft_argmax(0, _p(gd.inp(hm.reshape(N * h * w, oo.SAM_LD))), oo.SAM_LD, N, h, w, _p(coords), _p(crop),
                                          oo.SAM_IMAGE, oo.SAM_HEAT, _p(nchw), None))
            gd.check()
            err = float((coords.cpu().double() - ref).abs().max())
            err_crop = float((crop.cpu().double() - ref * oo.SAM_IMAGE / oo.SAM_HEAT).abs().max())
            print(f"[ops_f64] soft_argmax N {N} {h}x{w} scale {scale:g}: err {err:.3e} px, e32 {e32:.3e}, bar {bar:.3e}")
            assert err <= bar, (scale, err, e32, bar)
            assert err_crop <= bar * oo.SAM_IMAGE / oo.SAM_HEAT, (scale, err_crop, bar)
            if with_nchw:
                _bits(nchw, hm[..., :NJ].permute(0, 3, 1, 2).contiguous(), "hm_nchw")
            results.append((coords.cpu(), crop.cpu()))
            worst = max(worst, err / bar)
        assert oo.bits_equal(results[0][0], results[1][0]) and oo.bits_equal(results[0][1], results[1][1])   # hm_nchw changes no coordinate
        # planted joints: the flat map's centre, the four corners, the midpoint of two equal peaks
        got = results[0][0].double()
        assert (got[:, 0] - torch.tensor([(w - 1) / 2, (h - 1) / 2])).abs().max() <= bar
        corners = torch.tensor([[0.0, 0.0], [w - 1.0, 0.0], [0.0, h - 1.0], [w - 1.0, h - 1.0]], dtype=torch.float64)
        assert (got[:, 1:5] - corners).abs().max() <= bar
        assert (got[:, 5] - torch.tensor([(w - 1) / 2, (h - 1) / 2])).abs().max() <= bar
    _report(f"soft_argmax N {N} {h}x{w} worst err / bar", f"{worst:.3f}")


# ------------------------------------------------------------------ SampleNet gather / blend
def _gather(rows, coords, C, elem_bytes):
    gd = Guards(DEV)
    N, H, W, K = rows.shape
    out = gd.out((N * NJ * 4, K), rows.dtype)
    _ok(_lib().hmv_op_sample_gather(0, _p(gd.inp(rows)), N, H, W, C, elem_bytes, _p(gd.inp(coords)), _p(out), None))
    gd.check()
    return out.cpu()


@pytest.mark.parametrize("fmt", ["f32", "f16", "pairs"])
@pytest.mark.parametrize("shape", oo.SAMPLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sample_gather(shape, fmt):
    """Bitwise the four neighbours by indexing; taps outside the map and every tap of a +-1e9, +-inf or NaN coordinate are zeros."""
    N, H, W, C = shape
    feat, coords = oo.sample_feat(N, H, W, C), oo.sample_coords(N, H, W)
    rows, eb = {"f32": (feat, 4), "f16": (feat.half(), 2), "pairs": (torch.cat(oo.split_f16(feat), dim=-1), 4)}[fmt]
    got = _gather(rows, coords, C, eb)
    assert oo.bits_equal(got, oo.gather_ref(rows, coords))
    dead = (~torch.isfinite(coords).all(dim=-1) | (coords.abs() >= 1e9).any(dim=-1)).reshape(-1)
    assert int(dead.sum()) == 6 * N and not got.reshape(N * NJ, -1)[dead].any()


@pytest.mark.parametrize("shape", oo.SAMPLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sample_blend(shape):
    """The gathered rows (identity conv) blended into columns [col0, col0 + C) of wider token rows, against float64 grid_sample; no other
    column is written, the pad of the gathered rows (NaN) is not read."""
    N, H, W, C = shape
    feat, coords = oo.sample_feat(N, H, W, C), oo.sample_coords(N, H, W)
    s4 = _gather(feat, coords, C, 4)
    col0, ldt, lds4 = 8, C + 24, C + 4
    gd = Guards(DEV)
    before = torch.full((N * NJ, ldt), SENT)
    tokens = _prefilled(gd, before)
    _ok(_lib().hmv_op_sample_blend(0, _p(gd.inp(_wide(s4, lds4))), lds4, C, N, H, W, _p(gd.inp(coords)), _p(tokens), ldt, col0, None))
    gd.check()
    got = tokens.cpu()
    ref, bar = oo.blend_ref(feat, coords), oo.blend_bar(feat, H, W)
    err = float((got[:, col0:col0 + C].double() - ref).abs().max())
    _report(f"sample_blend {shape} err / bar", f"{err:.3e} / {bar:.3e}")
    assert err <= bar
    assert oo.bits_equal(got[:, :col0], before[:, :col0]) and oo.bits_equal(got[:, col0 + C:], before[:, col0 + C:])
    dead = ~torch.isfinite(coords).all(dim=-1).reshape(-1)
    assert not got[dead, col0:col0 + C].any()


# ------------------------------------------------------------------ token finalise
def _finalize(B, V, fdim, ldt, pos_mask, with_pe, with_raw, with_pairs, ragged, plant):
    N, d = B * V, oo.token_d(fdim, pos_mask)
    R = N * NJ
    feat, coords, bbox, intr, pe = oo.token_inputs(B, V, fdim)
    if plant:
        feat = feat.clone()
        feat[R // 2, fdim // 3] = 70000.0
    pe_d = pe[:, :d].contiguous()
    fpos = oo.token_fpos(N) if ragged else None
    n = torch.arange(R) // NJ
    pos = (fpos.long()[n] if ragged else (n % V) * NJ) + torch.arange(R) % NJ
    gd = Guards(DEV)
    tokens = _prefilled(gd, _wide(feat, ldt, SENT))
    raw = gd.out((R, d)) if with_raw else None
    pairs = gd.out((R, 2 * ldt), torch.float16) if with_pairs else None
    sat = _sat(gd)
    _ok(_lib().hmv_op_tokens_finalize(0, _p(tokens), ldt, d, fdim, N, V, _p(gd.inp(fpos)) if ragged else None, _p(gd.inp(coords)),
                                      _p(gd.inp(bbox)), _p(gd.inp(intr)), pos_mask, _p(gd.inp(pe_d)) if with_pe else None, _p(raw), _p(pairs),
                                      _p(sat), None))
    gd.check()
    got = tokens.cpu()
    rows, fov, fcol = oo.token_rows_ref(feat, coords, bbox, intr, pos_mask, ldt)
    add = pe_d[pos] if with_pe else None
    want = rows.clone()
    if with_pe:
        want[:, :d] = rows[:, :d] + add
    exact = torch.ones(ldt, dtype=torch.bool)
    worst = 0.0
    if fov is not None:
        exact[fcol:fcol + 10] = False
        target = fov + add[:, fcol:fcol + 10].double() if with_pe else fov
        err = (got[:, fcol:fcol + 10].double() - target).abs()
        assert bool((err <= oo.FOV_BAR + (oo.U24 * target.abs() if with_pe else 0.0)).all()), float(err.max())   # + the rounding of the PE add
        worst = float(err.max())
    _bits(got[:, exact], want[:, exact], "feature + PE, pos2d and pad columns")
    assert not got[:, d:].any()
    if with_raw:
        r = raw.cpu()
        ex = exact[:d]
        _bits(r[:, ex], rows[:, :d][:, ex], "raw_copy")
        if fov is not None:
            assert float((r[:, fcol:fcol + 10].double() - fov).abs().max()) <= oo.FOV_BAR
            worst = max(worst, float((r[:, fcol:fcol + 10].double() - fov).abs().max()))
            _bits(got[:, fcol:fcol + 10], r[:, fcol:fcol + 10] + add[:, fcol:fcol + 10] if with_pe else r[:, fcol:fcol + 10], "FoV + PE is the fp32 sum")
    if with_pairs:
        pr = pairs.cpu()
        hi, lo = oo.split_f16(got[:, :d])
        _bits(pr[:, :d], hi, "pairs hi")
        _bits(pr[:, ldt:ldt + d], lo, "pairs lo")
        assert not pr[:, d:ldt].any() and not pr[:, ldt + d:].any()
        assert oo.bits_equal(pr[:, d:ldt], torch.zeros(R, ldt - d, dtype=torch.float16))
        if plant:
            assert float(pr[R // 2, fdim // 3]) == 65504.0
    assert int(sat.item()) == (1 if (plant and with_pairs) else SAT_IDLE)   # note_range: raised by a clamped pair, otherwise left alone
    return worst


@pytest.mark.parametrize("pos_mask", [0, 1, 2, 3])
@pytest.mark.parametrize("dims", oo.TOKEN_DIMS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("BV", oo.TOKEN_BATCHES, ids=lambda s: "x".join(map(str, s)))
def test_tokens_finalize(BV, dims, pos_mask):
    """tokens_finalize_kernel (uniform) and tokens_finalize_views_kernel (an fpos table that is not monotonic): feature + PE, pos2d, raw_copy
    and pairs bitwise, pad exactly 0, FoV columns against float64 atan((p - c) / f) within 8 ulp at pi / 2, the range word as note_range
    documents it."""
    (B, V), (fdim, ldt) = BV, dims
    worst = 0.0
    for with_pe in (True, False):
        for with_raw in (True, False):
            for with_pairs in (True, False):
                worst = max(worst, _finalize(B, V, fdim, ldt, pos_mask, with_pe, with_raw, with_pairs, False, False))
        for with_pairs in (True, False):
            worst = max(worst, _finalize(B, V, fdim, ldt, pos_mask, with_pe, False, with_pairs, True, False))
    for with_pairs in (True, False):
        for ragged in (False, True):
            _finalize(B, V, fdim, ldt, pos_mask, True, False, with_pairs, ragged, True)
    _report(f"tokens_finalize {BV} {dims} pos_mask {pos_mask} worst FoV error (bar {oo.FOV_BAR:.3e})", f"{worst:.3e}")


# ------------------------------------------------------------------ LayerNorm
def _layernorm(x, ldx, d, ldy, params, chain):
    g1, b1, g2, b2 = params
    rows = x.shape[0]
    gd = Guards(DEV)
    y = gd.out((rows, ldy))
    y2 = gd.out((rows, ldy)) if chain else None
    _ok(_lib().hmv_op_layernorm(0, _p(gd.inp(_wide(x, ldx))), ldx, rows, d, _p(gd.inp(g1)), _p(gd.inp(b1)), _p(y), ldy,
                                _p(gd.inp(g2)) if chain else None, _p(gd.inp(b2)) if chain else None, _p(y2), None))
    gd.check()
    return y.cpu(), (y2.cpu() if chain else None)


def _check_layernorm(x, kinds, y, y2, d, params):
    g1, b1, g2, b2 = params
    ref = oo.layernorm_ref(x, g1, b1)
    ratio = (y[:, :d].double() - ref).abs() / oo.layernorm_bar(x, g1, ref)
    worst = 0.0
    for i, k in enumerate(kinds):
        if k == "constant":
            assert oo.bits_equal(y[i, :d], b1), "a constant row gives exactly the bias"
        else:
            assert float(ratio[i].max()) <= 1.0, (k, d, float(ratio[i].max()))
            worst = max(worst, float(ratio[i].max()))
    assert oo.bits_equal(y[:, d:], torch.zeros_like(y[:, d:]))
    if y2 is not None:   # the second norm, judged on what the first one wrote
        ref2 = oo.layernorm_ref(y[:, :d], g2, b2)
        r2 = float(((y2[:, :d].double() - ref2).abs() / oo.layernorm_bar(y[:, :d], g2, ref2)).max())
        assert r2 <= 1.0, (d, r2)
        assert oo.bits_equal(y2[:, d:], torch.zeros_like(y2[:, d:]))
        worst = max(worst, r2)
    return worst


@pytest.mark.parametrize("d", oo.LN_DIMS)
@pytest.mark.parametrize("rows", oo.LN_ROWS)
def test_layernorm(rows, d):
    """layernorm_kernel<0>, plain and with the chained second norm, ldx > d, ldy = d and d rounded up to 8.  The mean-100 / std-0.1 row is
    what a one-pass variance fails (test_ops_oracle.py); a constant row must give exactly the bias."""
    params = oo.ln_params(d)
    worst = 0.0
    for ldy in sorted({d, (d + 7) // 8 * 8}):
        for chain in (False, True):
            for only in ([None] if rows > 1 else oo.LN_KINDS):
                x, kinds = oo.ln_rows(rows, d, only=only)
                y, y2 = _layernorm(x, d + 4, d, ldy, params, chain)
                worst = max(worst, _check_layernorm(x, kinds, y, y2, d, params))
    _report(f"layernorm rows {rows} d {d} worst err / bar", f"{worst:.3f}")


def test_layernorm_refuses_rows_beyond_1024_columns():
    lib = _lib()
    x = torch.zeros(2, 1040, device=DEV)
    y = torch.full((2, 1040), SENT, device=DEV)
    g = torch.ones(1040, device=DEV)
    for d, ldy in ((1028, 1028), (1000, 1032)):
        assert lib.hmv_op_layernorm(0, _p(x), 1040, 2, d, _p(g), _p(g), _p(y), ldy, None, None, None, None) == 1
        assert b"1024" in lib.hmv_last_error(None)
    torch.cuda.synchronize()
    assert bool((y == SENT).all())   # refused, not launched


# ------------------------------------------------------------------ split-K epilogues
def _splitk_buffers(gd, rows, N, with_res):
    slab, bias, res = oo.splitk_inputs(rows, N)
    lds, ldr = N + 4, N + 12
    d_slab = gd.inp(_wide(slab.reshape(-1, N), lds).reshape(oo.SPLITK_S, rows, lds))
    d_res = gd.inp(_wide(res, ldr)) if with_res else None
    return slab, bias, (res if with_res else None), d_slab, gd.inp(bias), d_res, lds, ldr


@pytest.mark.parametrize("N", oo.SPLITK_N)
@pytest.mark.parametrize("rows", oo.SPLITK_ROWS)
def test_splitk_reduce(rows, N):
    """Slices + bias (+ residual rows through the cross block's mapping 21 -> 63) and each of the four activations against float64 sums:
    8 ulp of the sum of |terms|, GELU 8 * 2^-24 * max(1, |v|); columns [N, ldc) keep their sentinel."""
    ldc = N + 8
    worst = {}
    for with_res in (False, True):
        for act in (oo.ACT_NONE, oo.ACT_RELU, oo.ACT_GELU, oo.ACT_LEAKY):
            gd = Guards(DEV)
            slab, bias, res, d_slab, d_bias, d_res, lds, ldr = _splitk_buffers(gd, rows, N, with_res)
            before = torch.full((rows, ldc), SENT)
            out = _prefilled(gd, before)
            _ok(_lib().hmv_op_splitk_reduce(0, _p(d_slab), oo.SPLITK_S, rows, lds, N, _p(d_bias), _p(d_res), ldr, *oo.SPLITK_RG, act, _p(out), ldc, None))
            gd.check()
            got = out.cpu()
            ref, v, mag = oo.splitk_ref(slab, bias, res, act)
            ratio = float(((got[:, :N].double() - ref).abs() / oo.splitk_bar(v, mag, act)).max())
            worst[act] = max(worst.get(act, 0.0), ratio)
            assert ratio <= 1.0, (with_res, act, ratio)
            assert oo.bits_equal(got[:, N:], before[:, N:])
    _report(f"splitk_reduce rows {rows} N {N} worst err / bar per act", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("N", oo.SPLITK_N)
@pytest.mark.parametrize("rows", oo.SPLITK_ROWS)
def test_splitk_layernorm_is_reduce_then_layernorm_bit_for_bit(rows, N):
    """layernorm_kernel<4> promises the arithmetic of splitk_reduce_kernel followed by layernorm_kernel<0>: the same bits, pads included."""
    lib = _lib()
    g1, b1, g2, b2 = oo.ln_params(N)
    ldc, ldy = N + 8, (N + 7) // 8 * 8
    for with_res in (False, True):
        for chain in (False, True):
            gd = Guards(DEV)
            slab, bias, res, d_slab, d_bias, d_res, lds, ldr = _splitk_buffers(gd, rows, N, with_res)
            dg1, db1 = gd.inp(g1), gd.inp(b1)
            dg2, db2 = (gd.inp(g2), gd.inp(b2)) if chain else (None, None)
            mid = _prefilled(gd, torch.full((rows, ldc), math.nan))
            ya, yb = gd.out((rows, ldy)), gd.out((rows, ldy))
            y2a, y2b = (gd.out((rows, ldy)), gd.out((rows, ldy))) if chain else (None, None)
            _ok(lib.hmv_op_splitk_reduce(0, _p(d_slab), oo.SPLITK_S, rows, lds, N, _p(d_bias), _p(d_res), ldr, *oo.SPLITK_RG, oo.ACT_NONE, _p(mid), ldc, None))
            _ok(lib.hmv_op_layernorm(0, _p(mid), ldc, rows, N, _p(dg1), _p(db1), _p(ya), ldy, _p(dg2), _p(db2), _p(y2a), None))
            _ok(lib.hmv_op_splitk_layernorm(0, _p(d_slab), oo.SPLITK_S, rows, lds, N, _p(d_bias), _p(d_res), ldr, *oo.SPLITK_RG, _p(dg1), _p(db1), _p(yb),
                                            ldy, _p(dg2), _p(db2), _p(y2b), None))
            gd.check()
            assert oo.bits_equal(ya.cpu(), yb.cpu()), (with_res, chain)
            assert not torch.isnan(yb).any() and not yb[:, N:].any()
            if chain:
                assert oo.bits_equal(y2a.cpu(), y2b.cpu()), (with_res, chain)
            # ... and the fused form against float64 on its own
            v = oo.splitk_ref(slab, bias, res, oo.ACT_NONE, torch.float32)[0]
            ref = oo.layernorm_ref(v, g1, b1)
            assert float(((yb.cpu()[:, :N].double() - ref).abs() / oo.layernorm_bar(v, g1, ref)).max()) <= 1.0
            # S != 4 has no fused form: refused, nothing written
            yb.fill_(SENT)
            assert lib.hmv_op_splitk_layernorm(0, _p(d_slab), 2, rows, lds, N, _p(d_bias), _p(d_res), ldr, *oo.SPLITK_RG, _p(dg1), _p(db1), _p(yb), ldy,
                                               _p(dg2), _p(db2), _p(y2b), None) == 1
            torch.cuda.synchronize()
            assert bool((yb == SENT).all())


# ------------------------------------------------------------------ add_pe
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "fpos"])
def test_add_pe(ragged):
    """add_pe_kernel (position r % T) and add_pe_views_kernel (position fpos[r / 21] + r % 21): bitwise the fp32 sum, pad exactly 0."""
    lib = _lib()
    x, pe, fpos = oo.add_pe_inputs()
    gd = Guards(DEV)
    y = gd.out((oo.PE_ROWS, oo.PE_LDY))
    dx, dpe, dfpos = gd.inp(_wide(x, oo.PE_LDX)), gd.inp(pe), (gd.inp(fpos) if ragged else None)
    _ok(lib.hmv_op_add_pe(0, _p(dx), oo.PE_LDX, oo.PE_ROWS, oo.PE_T, _p(dfpos), oo.PE_D, _p(dpe), _p(y), oo.PE_LDY, None))
    gd.check()
    got = y.cpu()
    _bits(got[:, :oo.PE_D], x + pe[oo.add_pe_positions(fpos if ragged else None)])
    assert oo.bits_equal(got[:, oo.PE_D:], torch.zeros(oo.PE_ROWS, oo.PE_LDY - oo.PE_D))
    if ragged:   # whole frames only
        y.fill_(SENT)
        assert lib.hmv_op_add_pe(0, _p(dx), oo.PE_LDX, 40, oo.PE_T, _p(dfpos), oo.PE_D, _p(dpe), _p(y), oo.PE_LDY, None) == 1
        assert b"21" in lib.hmv_last_error(None)
        torch.cuda.synchronize()
        assert bool((y == SENT).all())


# ------------------------------------------------------------------ ChebConv mix
@pytest.mark.parametrize("co", oo.CHEB_CO)
@pytest.mark.parametrize("B", oo.CHEB_B)
def test_cheb_mix(B, co):
    """co = 16 / 48: lanes of a 32-channel slice beyond co return early, 48: a second slice.  Against float64 within the rigorous bound of a
    63-term fp32 sum, 63 * 2^-24 * sum|T y| + 2^-23 |out|; columns [co, ldo) keep their sentinel, the pad of y (NaN) is not read."""
    ldy, ldo = 3 * co + 4, co + 4
    y, bias = oo.cheb_inputs(B, co)
    worst = 0.0
    for kind in ("hand", "dense"):
        tk = oo.cheb_stack(kind)
        for leaky in (0, 1):
            gd = Guards(DEV)
            before = torch.full((B * NJ, ldo), SENT)
            out = _prefilled(gd, before)
            _ok(_lib().hmv_op_cheb_mix(0, _p(gd.inp(_wide(y, ldy))), ldy, B, co, _p(gd.inp(tk)), _p(gd.inp(bias)), leaky, _p(out), ldo, None))
            gd.check()
            got = out.cpu()
            ref, mag = oo.cheb_ref(y, tk, bias, leaky)
            ratio = float(((got[:, :co].double() - ref).abs() / oo.cheb_bar(ref, mag)).max())
            assert ratio <= 1.0, (kind, leaky, ratio)
            assert oo.bits_equal(got[:, co:], before[:, co:])
            worst = max(worst, ratio)
    _report(f"cheb_mix B {B} co {co} worst err / bar", f"{worst:.3f}")
