"""tests/ops_oracle.py on the CPU: (a) its float64 references agree with torch's own float64 ops where one exists, (b) the same formulas
evaluated in torch fp32 on every input test_gpu_ops_f64.py uses land inside the bar that file applies -- a correct fp32 kernel passes --
and a one-pass LayerNorm variance lands outside it, (c) the seeded input generators are pinned."""
import math

import pytest
import torch
import torch.nn.functional as F

import ops_oracle as oo

NJ = oo.NJ


# ------------------------------------------------------------------ (a) the references against torch's float64 ops
@pytest.mark.parametrize("shape", oo.POOL_SHAPES)
@pytest.mark.parametrize("kind", oo.POOL_KINDS)
def test_maxpool_reference_is_torch_max_pool2d(shape, kind):
    v = oo.pool_values(shape, kind).double()
    want = F.max_pool2d(v.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert oo.bits_equal(oo.maxpool_ref(v), want.contiguous())
    assert tuple(want.shape[1:3]) == oo.pool_out_hw(shape[1], shape[2])
    if kind == "negative":   # the case is there for the padding: a pool that pads with 0 is wrong wherever the window leaves the map
        zero_pad = F.max_pool2d(F.pad(v.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2, 0).permute(0, 2, 3, 1)
        assert not torch.equal(zero_pad, want)


def test_soft_argmax_reference_is_torch_softmax():
    for (h, w) in oo.SAM_SIZES:
        for scale in oo.SAM_SCALES:
            hm = oo.heatmap_logits(3, h, w, scale)
            z = (hm[..., :NJ] * torch.tensor(1000.0)).double().reshape(3, h * w, NJ)
            p = torch.softmax(z, dim=1)
            pix = torch.arange(h * w)
            want = torch.stack([(p * (pix % w)[None, :, None]).sum(1), (p * (pix // w)[None, :, None]).sum(1)], dim=-1)
            assert (oo.soft_argmax_ref(hm) - want).abs().max() < 1e-12


def test_blend_reference_is_torch_grid_sample():
    for (N, H, W, C) in oo.SAMPLE_SHAPES:
        feat, coords = oo.sample_feat(N, H, W, C).double(), oo.sample_coords(N, H, W)
        fin = torch.isfinite(coords).all(dim=-1)
        c = torch.where(fin[..., None], coords, torch.full_like(coords, -100.0)).double()   # grid_sample on a NaN is undefined: far outside instead
        grid = c / torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64) * 2 - 1
        want = F.grid_sample(feat.permute(0, 3, 1, 2), grid[:, :, None, :], mode="bilinear", padding_mode="zeros", align_corners=True)
        want = want[..., 0].permute(0, 2, 1).reshape(N * NJ, C)
        got = oo.blend_ref(feat, coords)
        assert (got - want).abs().max() < 1e-12
        assert not got[(~fin).reshape(-1)].any()            # non-finite coordinates sample nothing
        x0, y0, _, valid = oo.sample_taps(coords, H, W)
        assert not valid[:, 9:17].any() and valid[:, 0].all()   # far outside, +-1e9, +-inf, NaN: no tap; the integer coordinate: all four
        assert valid[:, 2, 0].all() and not valid[:, 2, 1:].any()   # exactly (W - 1, H - 1): the first tap alone, the others outside with weight 0


def test_layernorm_and_gelu_references_are_torchs():
    for d in oo.LN_DIMS:
        x, _ = oo.ln_rows(5, d)
        g1, b1, _, _ = oo.ln_params(d)
        want = F.layer_norm(x.double(), (d,), g1.double(), b1.double(), eps=oo.LN_EPS)
        assert (oo.layernorm_ref(x, g1, b1) - want).abs().max() < 1e-9
    v = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    assert (oo.gelu_ref(v) - F.gelu(v)).abs().max() < 1e-15
    dv = (oo.gelu_ref(v + 1e-6) - oo.gelu_ref(v - 1e-6)) / 2e-6
    assert 1.12 < float(dv.abs().max()) < 1.13   # the slope an error of the sum passes through


def test_fov_reference_against_math_atan():
    _, _, bbox, intr, _ = oo.token_inputs(2, 3, 32)
    got = oo.fov_ref(bbox, intr)
    b, k = bbox.double().tolist(), intr.double().tolist()
    for n in range(6):
        x1, y1, x2, y2 = b[n]
        fx, fy, cx, cy = k[n]
        pts = [(x1, y1), (x1, y2), (x2, y1), (x2, y2), ((x1 + x2) / 2, (y1 + y2) / 2)]
        want = [f(p) for p in pts for f in (lambda p: math.atan((p[0] - cx) / fx), lambda p: math.atan((p[1] - cy) / fy))]
        assert max(abs(a - w) for a, w in zip(got[n].tolist(), want)) < 1e-15


def test_cheb_stack_is_the_chebyshev_recurrence_of_a_scaled_laplacian():
    tk = oo.cheb_stack("hand").double()
    assert torch.equal(tk[0], torch.eye(NJ, dtype=torch.float64))
    assert (tk[1] - tk[1].T).abs().max() == 0 and float(torch.linalg.eigvalsh(tk[1]).max()) == pytest.approx(1.0, abs=1e-6)
    assert float(torch.linalg.eigvalsh(tk[1]).min()) >= -1.0 - 1e-6
    assert (tk[2] - (2 * tk[1] @ tk[1] - tk[0])).abs().max() < 1e-6
    assert int((tk[1] != 0).sum()) == NJ + 2 * len(oo.HAND_EDGES)


# ------------------------------------------------------------------ (b) fp32 torch is inside every bar
def test_fp32_torch_is_inside_every_bar(capsys):
    worst = {}

    def note(op, e32, bar):
        e32, bar = float(e32), float(bar)
        assert e32 <= bar, (op, e32, bar)
        w = worst.get(op, (0.0, math.inf))
        worst[op] = (max(w[0], e32), min(w[1], bar))

    # soft-argmax: the bar follows e32 itself (8 e32) above a floor of 8 ulp of the largest coordinate; e32 stays within a few 1e-5 px
    for N in oo.SAM_BATCHES:
        for (h, w) in oo.SAM_SIZES:
            for scale in oo.SAM_SCALES:
                hm = oo.heatmap_logits(N, h, w, scale)
                e32 = (oo.soft_argmax_ref(hm, torch.float32).double() - oo.soft_argmax_ref(hm)).abs().max()
                assert float(e32) < 5e-5, (N, h, w, scale, float(e32))
                note("soft_argmax", e32, oo.soft_argmax_bar(float(e32), h, w))
    # blend: torch's fp32 grid_sample on the fp32 grid the model builds
    for (N, H, W, C) in oo.SAMPLE_SHAPES:
        feat, coords = oo.sample_feat(N, H, W, C), oo.sample_coords(N, H, W)
        fin = torch.isfinite(coords).all(dim=-1)
        c = torch.where(fin[..., None], coords, torch.full_like(coords, -100.0))
        grid = c / torch.tensor([W - 1.0, H - 1.0]) * 2 - 1
        got = F.grid_sample(feat.permute(0, 3, 1, 2), grid[:, :, None, :], mode="bilinear", padding_mode="zeros", align_corners=True)
        got = got[..., 0].permute(0, 2, 1).reshape(N * NJ, C).double()
        note("sample_blend", (got - oo.blend_ref(feat, coords)).abs().max(), oo.blend_bar(feat, H, W))
        note("sample_blend", (oo.blend_ref(feat, coords, torch.float32).double() - oo.blend_ref(feat, coords)).abs().max(), oo.blend_bar(feat, H, W))
    # FoV columns
    for (B, V) in oo.TOKEN_BATCHES:
        for (fdim, _) in oo.TOKEN_DIMS:
            _, _, bbox, intr, _ = oo.token_inputs(B, V, fdim)
            note("fov", (oo.fov_ref(bbox, intr, torch.float32).double() - oo.fov_ref(bbox, intr)).abs().max(), oo.FOV_BAR)
    # LayerNorm, and the second norm of a chain on the first one's fp32 output
    for rows in oo.LN_ROWS:
        for d in oo.LN_DIMS:
            g1, b1, g2, b2 = oo.ln_params(d)
            for only in ([None] if rows > 1 else oo.LN_KINDS):
                x, kinds = oo.ln_rows(rows, d, only=only)
                y32 = F.layer_norm(x, (d,), g1, b1, eps=oo.LN_EPS)
                ref = oo.layernorm_ref(x, g1, b1)
                live = torch.tensor([k != "constant" for k in kinds])
                if live.any():
                    note("layernorm", ((y32.double() - ref).abs() / oo.layernorm_bar(x, g1, ref))[live].max(), 1.0)
                ref2 = oo.layernorm_ref(y32, g2, b2)
                note("layernorm chained", ((F.layer_norm(y32, (d,), g2, b2, eps=oo.LN_EPS).double() - ref2).abs() / oo.layernorm_bar(y32, g2, ref2)).max(), 1.0)
    # split-K epilogues
    for rows in oo.SPLITK_ROWS:
        for N in oo.SPLITK_N:
            slab, bias, res = oo.splitk_inputs(rows, N)
            for r in (None, res):
                for act in (oo.ACT_NONE, oo.ACT_RELU, oo.ACT_GELU, oo.ACT_LEAKY):
                    ref, v, mag = oo.splitk_ref(slab, bias, r, act)
                    got, _, _ = oo.splitk_ref(slab, bias, r, act, torch.float32)
                    note("splitk act %d" % act, ((got.double() - ref).abs() / oo.splitk_bar(v, mag, act)).max(), 1.0)
    # ChebConv mix
    for kind in ("hand", "dense"):
        tk = oo.cheb_stack(kind)
        for B in oo.CHEB_B:
            for co in oo.CHEB_CO:
                y, bias = oo.cheb_inputs(B, co)
                for leaky in (0, 1):
                    ref, mag = oo.cheb_ref(y, tk, bias, leaky)
                    got, _ = oo.cheb_ref(y, tk, bias, leaky, torch.float32)
                    note("cheb_mix", ((got.double() - ref).abs() / oo.cheb_bar(ref, mag)).max(), 1.0)
    with capsys.disabled():
        print("\nfp32 torch is inside every bar (worst e32, smallest bar; ratios for the per-element bars):")
        for op, (e, b) in worst.items():
            print(f"  {op:20s} e32 {e:.3e}   bar {b:.3e}")


def test_one_pass_variance_is_outside_the_layernorm_bar(capsys):
    for d in oo.LN_DIMS:
        x, _ = oo.ln_rows(1, d, only="mean100")
        g1, b1, _, _ = oo.ln_params(d)
        ref = oo.layernorm_ref(x, g1, b1)
        ratio = float(((oo.layernorm_one_pass(x, g1, b1).double() - ref).abs() / oo.layernorm_bar(x, g1, ref)).max())
        two = float(((F.layer_norm(x, (d,), g1, b1, eps=oo.LN_EPS).double() - ref).abs() / oo.layernorm_bar(x, g1, ref)).max())
        with capsys.disabled():
            print(f"\none-pass variance is outside the bar: d {d}: {ratio:.1f} x the bar (two-pass fp32: {two:.3f} x)")
        assert ratio > 4.0 and two <= 1.0
        # ... while on a row with |mean| ~ std, which is what token rows look like, the two are indistinguishable
        x, _ = oo.ln_rows(1, d, only="randn")
        ref = oo.layernorm_ref(x, g1, b1)
        assert float(((oo.layernorm_one_pass(x, g1, b1).double() - ref).abs() / oo.layernorm_bar(x, g1, ref)).max()) <= 1.0


def test_constant_row_has_an_exact_mean_in_fp32():
    """Why 'exactly the bias' is a fair demand: every partial sum of d copies of the constant, and the mean from it, is exact."""
    c = torch.tensor(oo.LN_CONSTANT)
    for d in oo.LN_DIMS:
        for k in range(1, d + 1):
            assert float(c * k) == oo.LN_CONSTANT * k and float((c * k).float()) == oo.LN_CONSTANT * k
        s = (c * d).float()
        assert float(s / d) == oo.LN_CONSTANT and float(s * (torch.tensor(1.0) / d)) == oo.LN_CONSTANT
        x, kinds = oo.ln_rows(1, d, only="constant")
        g1, b1, _, _ = oo.ln_params(d)
        assert torch.equal(oo.layernorm_ref(x, g1, b1, torch.float32), b1[None])


# ------------------------------------------------------------------ (c) the generators are pinned
def _digest(t):
    t = t.contiguous()
    nan = torch.isnan(t) if t.is_floating_point() else torch.zeros_like(t, dtype=torch.bool)
    fin = torch.where(nan | torch.isinf(t), torch.zeros_like(t), t).double() if t.is_floating_point() else t.double()
    return (tuple(t.shape), int(nan.sum()), round(float(fin.sum()), 4), round(float(fin.abs().sum()), 4))


def test_generators_are_seeded_and_repeatable():
    pairs = [(lambda: oo.frames(2, 8, 8)), (lambda: oo.pool_values((2, 7, 9, 8), "negative")), (lambda: oo.heatmap_logits.__wrapped__(1, 9, 13, 1e-2)),
             (lambda: oo.sample_coords(2, 8, 8)), (lambda: oo.sample_feat(1, 5, 7, 16)), (lambda: oo.token_inputs.__wrapped__(2, 3, 32)[0]),
             (lambda: oo.ln_rows(5, 44)[0]), (lambda: oo.splitk_inputs.__wrapped__(21, 44)[0]), (lambda: oo.add_pe_inputs()[0]),
             (lambda: oo.cheb_inputs.__wrapped__(3, 48)[0]), (lambda: oo.cheb_stack("dense"))]
    for f in pairs:
        assert _digest(f()) == _digest(f())
    # a few values by hand: the first draw of torch's CPU generator for a seed is part of torch's reproducibility contract
    assert torch.equal(oo.frames(1, 1, 1), torch.randn(1, 3, 1, 1, generator=torch.Generator().manual_seed(1000 + 7 + 31 + 101)) * 2.0)
    hm = oo.heatmap_logits(1, 4, 4, 1.0)
    assert int(torch.isnan(hm).sum()) == 16 * 11 and bool((hm[..., 0] == 0.25).all())
    assert int(hm[0, :, :, 1].argmax()) == 0 and int(hm[0, :, :, 4].argmax()) == 15
    assert float(hm[0, 1, 1, 5]) == float(hm[0, 2, 2, 5]) == float(hm[0, :, :, 5].max())
    c = oo.sample_coords(1, 5, 7)
    assert c[0, 1].tolist() == [0.0, 0.0] and c[0, 2].tolist() == [6.0, 4.0] and math.isnan(float(c[0, 15, 0])) and math.isinf(float(c[0, 13, 0]))
    assert bool(((c[0, 17:] >= 0) & (c[0, 17:] <= torch.tensor([6.0, 4.0]))).all())
    x, kinds = oo.ln_rows(5, 44)
    assert kinds == oo.LN_KINDS and abs(float(x[1].mean()) - 100.0) < 0.1 and 0.05 < float(x[1].std()) < 0.2 and float(x[3].max()) == 1e4
    assert oo.token_fpos(6).tolist() == [21, 0, 42, 0, 42, 21] and oo.splitk_res_rows(42)[[0, 20, 21, 41]].tolist() == [0, 20, 63, 83]
    for kind, (N, H, W) in oo.FRAME_SHAPE_OVER_CAP.items():
        px = N * H * W if kind == 0 else N * ((H + 1) // 2) * ((W + 1) // 2)
        assert oo.GRID_CAP[kind] < px <= oo.GRID_CAP[kind] + 4096
    for mode, (N, H, W, C) in oo.POOL_SHAPE_OVER_CAP.items():
        Ho, Wo = oo.pool_out_hw(H, W)
        assert oo.POOL_GRID_CAP < N * Ho * Wo * (C // (4 if mode == 0 else 8)) <= oo.POOL_GRID_CAP + 8


def test_split_pairs_and_layout_references():
    v = torch.tensor([0.0, 1.0, 1.0009765625 + 2.0 ** -14, -3.3333333, 65504.0, 70000.0, -1e9, 6.1e-5, 1e-8])
    hi, lo = oo.split_f16(v)
    assert torch.equal(hi[:2], torch.tensor([0.0, 1.0]).half()) and float(hi[5]) == 65504.0 and float(lo[5]) == 0.0 and float(hi[6]) == -65504.0
    back = hi.float() + lo.float()
    assert (back[:5] - v[:5]).abs().max() <= 2.0 ** -22 * 4 and oo.out_of_pair_range(v) and not oo.out_of_pair_range(v[:5])
    x = oo.frames(1, 3, 3)
    r = oo.nhwc_rows(x, 0)
    assert float(r[0, 1, 2, 1]) == float(x[0, 1, 1, 2]) and not r[..., 3].any()
    s = oo.s2d_rows(x, 0)
    assert s.shape == (1, 2, 2, 12) and float(s[0, 0, 1, (1 * 2 + 0) * 3 + 2]) == float(x[0, 2, 1, 2])
    assert not s[0, 1, :, 6:].any() and not s[0, :, 1, 3:6].any() and not s[0, :, 1, 9:].any()   # the odd row / column is zeros
    assert not oo.s2d_rows(x, 1)[..., 12:].any() and not oo.s2d_rows(x, 2)[..., 12:16].any() and not oo.s2d_rows(x, 2)[..., 28:].any()
