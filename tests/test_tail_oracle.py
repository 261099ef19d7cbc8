"""tests/tail_oracle.py on the CPU: (a) its float64 references agree with torch's own float64 ops, (b) the same chain in torch fp32 on every
input test_gpu_tail_f64.py uses gives E32, which is inside the bar 8 E32 by construction and, for ChebConv layer 1, inside the rigorous
bound too, (c) the bar has teeth: nine wrong formulas land outside it on every case they apply to, (d) packers and generators."""
import pytest
import torch
import torch.nn.functional as F

import ops_oracle as oo
import tail_oracle as to

NJ = oo.NJ
FF_ALL = to.FF_CASES + to.FF_TILE_CASES


# ------------------------------------------------------------------ (a) the references against torch's float64 ops
@pytest.mark.parametrize("case", FF_ALL, ids=lambda c: c.name)
def test_ff_block_reference_is_torchs_float64_chain(case):
    t = to.ff_inputs(case.name)
    d64 = {k: v.double() for k, v in t.items()}
    d = case.d
    if case.S:
        tt = d64["slab"].sum(dim=0) + d64["bias0"]
        if case.res:
            tt = tt + d64["res"][to.ff_res_rows(case)]
    else:
        tt = d64["x"]
    n1 = F.layer_norm(tt, (d,), d64["n1g"], d64["n1b"], eps=1e-5) if case.n1 else tt
    f0 = F.layer_norm(n1, (d,), d64["fg"], d64["fb"], eps=1e-5)
    f2 = F.linear(F.gelu(F.linear(f0, d64["w1"], d64["b1"])), d64["w2"], d64["b2"]) + n1
    out = F.layer_norm(f2, (d,), d64["n2g"], d64["n2b"], eps=1e-5) if case.n2 else f2
    r_n1, r_f2, r_out = to.ff_block_ref(case, t)
    assert r_out.dtype == torch.float64 and tuple(r_out.shape) == (case.rows, d)
    for got, want in ((r_n1, n1), (r_f2, f2), (r_out, out)):
        assert float((got - want).abs().max()) < 1e-9 * max(1.0, float(want.abs().max()))


def test_ff_row_map_and_row_block_zero():
    c = to.FF_BY_NAME["row_map"]
    assert to.ff_res_rows(c)[[0, 20, 21, 41]].tolist() == [0, 20, 168, 188] and to.ff_inputs(c.name)["res"].shape[0] == 189
    t = to.ff_inputs("s4_res")
    head = to.ff_head(t, 16)
    c = to.FF_BY_NAME["s4_res"]
    assert float((to.ff_block_ref(c, head)[2] - to.ff_block_ref(c, t)[2][:16]).abs().max()) < 1e-12   # row-wise arithmetic


@pytest.mark.parametrize("case", to.CHEB_CASES, ids=lambda c: c.name)
def test_cheb_fused_reference_is_the_chebconv_arithmetic(case):
    """ChebConv.forward as the model writes it: matmul(T_k, x) first, then the weight, summed over k, + bias."""
    t = {k: v.double() for k, v in to.cheb_fused_inputs(case.name).items()}

    def conv(v, w, bias):
        r = torch.matmul(t["tk"].unsqueeze(1), v.reshape(case.B, NJ, -1))     # [3][B][21][ci]
        return (torch.matmul(r, w.unsqueeze(1)).sum(dim=0) + bias).reshape(case.B * NJ, -1)

    l1 = F.leaky_relu(conv(t["x"], t["w1"], t["bias1"]))
    l2 = F.leaky_relu(conv(l1, t["w2"], t["bias2"]))
    out = conv(l2, t["w3"], t["bias3"])
    r1, r_out, mag1, pre1, pre2 = to.cheb_fused_ref(to.cheb_fused_inputs(case.name))
    assert float((r1 - l1).abs().max()) < 1e-9 * float(l1.abs().max()) and float((r_out - out).abs().max()) < 1e-9 * max(1.0, float(out.abs().max()))
    assert tuple(r1.shape) == (case.B * NJ, case.c1) and tuple(r_out.shape) == (case.B * NJ, case.c3) and bool((mag1 >= (pre1 - t["bias1"]).abs() * (1 - 1e-12)).all())
    if case.negative:
        assert float(pre1.max()) < 0 and float(pre2.max()) < 0
    else:   # both branches of LeakyReLU are taken
        assert float(pre1.max()) > 0 > float(pre1.min()) and float(pre2.max()) > 0 > float(pre2.min())
    assert not torch.equal(t["tk"][1], t["tk"][1].T)   # a symmetric stack could not tell T_k from its transpose


# ------------------------------------------------------------------ (b) E32, (c) the mutants
@pytest.mark.parametrize("case", FF_ALL, ids=lambda c: c.name)
def test_ff_block_mutants_are_outside_the_bar(case, capsys):
    t = to.ff_inputs(case.name)
    e32, ref = to.ff_e32(case, t)
    bar = to.BAR_FACTOR * e32
    assert 0.0 < e32 < 1e-4 * float(ref.abs().max())      # a sane fp32 evaluation: five digits at least
    lines = []
    for m in to.ff_mutants_of(case):
        dtype = torch.float32 if m == "one_pass_variance" else torch.float64   # that one is a loss of precision, not another formula
        err = float((to.ff_block_ref(case, t, dtype, m)[2].double() - ref).abs().max())
        lines.append(f"{m} {err / bar:.1f}")
        assert err > bar, (case.name, m, err, bar)
    with capsys.disabled():
        print(f"\n[tail] ff {case.name}: E32 {e32:.3e}, bar {bar:.3e}; mutants / bar: " + ", ".join(lines))


def test_every_ff_mutant_is_exercised():
    seen = {m for c in FF_ALL for m in to.ff_mutants_of(c)}
    assert seen == set(to.FF_MUTANTS)


@pytest.mark.parametrize("case", to.CHEB_CASES, ids=lambda c: c.name)
def test_cheb_fused_mutants_are_outside_the_bar(case, capsys):
    t = to.cheb_fused_inputs(case.name)
    e1, eo, l1, out, mag1 = to.cheb_e32(t)
    assert 0.0 < e1 < 1e-4 * float(l1.abs().max()) and 0.0 < eo < 1e-4 * float(out.abs().max())
    # torch fp32 is inside the rigorous bound of layer 1
    l1_32 = to.cheb_fused_ref(t, torch.float32)[0]
    rig = float(((l1_32.double() - l1).abs() / to.cheb_layer1_bar(case.K, l1, mag1)).max())
    assert rig <= 1.0, rig
    lines = []
    for m in to.CHEB_MUTANTS:
        m1, mo, _, _, _ = to.cheb_fused_ref(t, torch.float64, m)
        r1, ro = float((m1 - l1).abs().max()) / (to.BAR_FACTOR * e1), float((mo - out).abs().max()) / (to.BAR_FACTOR * eo)
        lines.append(f"{m} {r1:.0f} / {ro:.0f}")
        assert r1 > 1.0 and ro > 1.0, (case.name, m, r1, ro)
        assert bool(((m1 - l1).abs() > to.cheb_layer1_bar(case.K, l1, mag1)).any())
    with capsys.disabled():
        print(f"\n[tail] cheb {case.name}: E32 layer 1 {e1:.3e}, out {eo:.3e}; fp32 / rigorous layer-1 bound {rig:.3f}; mutants / bar (layer 1 / out): " + ", ".join(lines))


# ------------------------------------------------------------------ (d) packers, generators, the exact rows
def test_packers_lay_weights_out_as_the_kernels_take_them():
    w1, w2 = torch.randn(128, 130), torch.randn(130, 128)
    p1, p2 = to.pack_w1(w1, 164), to.pack_w2(w2, 160, 132)
    assert p1.shape == (128, 164) and torch.equal(p1[:, :130], w1) and not p1[:, 130:].any()
    assert p2.shape == (160, 132) and torch.equal(p2[:130, :128], w2) and not p2[130:].any() and not p2[:, 128:].any()
    x = torch.randn(5, 130)
    h = torch.randn(5, 128)
    assert torch.allclose(to.pad_cols(x, 164) @ p1.T, F.linear(x, w1), atol=1e-5)
    assert torch.allclose((h @ p2[:, :128].T)[:, :130], F.linear(h, w2), atol=1e-5) and not (h @ p2[:, :128].T)[:, 130:].any()
    w = torch.randn(3, 64, 5)
    p = to.pack_cheb(w, 68, rows16=True)
    assert p.shape == (16, 68) and not p[15].any() and not p[:, 64:].any()
    assert torch.equal(p[1 * 5 + 2, :64], w[1, :, 2])          # row k * co + o = column o of order k
    xx = torch.randn(21, 64)
    assert torch.allclose(xx @ p[:15, :64].T, torch.cat([xx @ w[k] for k in range(3)], dim=1), atol=1e-5)
    assert to.pack_cheb(torch.randn(3, 96, 32), 100).shape == (96, 100)
    nan = to.pad_cols(torch.ones(2, 3), 5, float("nan"))
    assert torch.isnan(nan[:, 3:]).all() and bool((nan[:, :3] == 1).all()) and to.round4(130) == 132 and to.round4(524) == 524


def test_inputs_are_seeded_and_shaped():
    for c in FF_ALL:
        t = to.ff_inputs(c.name)
        again = to.ff_inputs.__wrapped__(c.name)
        assert all(torch.equal(t[k], again[k]) for k in t)
        assert ("x" in t) == (c.S == 0) and ("res" in t) == bool(c.res) and ("n1g" in t) == c.n1 and ("n2g" in t) == c.n2
        assert c.ld % 16 == 0 and c.d <= c.ld <= 576 and t["w1"].shape == (c.hid, c.d) and t["w2"].shape == (c.d, c.hid)
        rows = to.ff_assemble(c, t)
        assert 7.0 < float(rows.mean()) < 9.0 and float(rows.std(dim=-1).max()) < 0.5
    # which instantiations 32-row tiles fit: hid 128 up to ld 544, hid 256 up to ld 480 (160 KB of LDS)
    lds = lambda ld, hid, rows: 4 * (2 * rows * (ld + 4) + max(rows * (hid + 4), 4 * ld) + 2 * ld)
    assert lds(544, 128, 32) <= 160 * 1024 < lds(560, 128, 32) and lds(480, 256, 32) <= 160 * 1024 < lds(496, 256, 32)
    assert lds(576, 128, 16) <= 160 * 1024 and lds(576, 256, 16) <= 160 * 1024
    for c in to.CHEB_CASES:
        t = to.cheb_fused_inputs(c.name)
        assert t["x"].shape == (c.B * NJ, c.K) and t["w3"].shape == (3, c.c2, c.c3) and 3 * c.c3 <= 16


def test_a_constant_assembled_row_is_exact_in_fp32():
    """Four slices of -1, bias0 0.25, residual 0.5: every partial sum is exact and the row is -3.25 everywhere, ops_oracle's LN_CONSTANT, whose
    mean is exact at the widths of oo.LN_DIMS (test_ops_oracle.py) -- LayerNorm1 of it is exactly beta1 in float64 and in fp32."""
    assert ((-1.0 - 1.0) - 1.0) - 1.0 + 0.25 + 0.5 == oo.LN_CONSTANT
    for d in (44, 268):
        assert d in oo.LN_DIMS
        g1, b1, _, _ = oo.ln_params(d)
        x = torch.full((3, d), oo.LN_CONSTANT)
        assert torch.equal(F.layer_norm(x, (d,), g1, b1, 1e-5), b1.expand(3, d)) and torch.equal(oo.layernorm_ref(x, g1, b1), b1.double().expand(3, d))
