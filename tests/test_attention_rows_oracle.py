"""tests/attention_rows_oracle.py on the CPU: (a) its float64 reference agrees with torch's float64 scaled_dot_product_attention and its
chunk-by-chunk evaluation (the kernels' order) with the reference, (b) E32n of every case test_gpu_attention_rows.py uses -- printed, and
never above 1e-3: a case where fp32 itself fails would be ill-posed, (c) the bar 8 E32n has teeth: eight wrong evaluations land outside it,
each on the case it names, (d) the x3 body's (ph, pl) carrier of P against E32n on the flat-tail and spread cases, (e) the builders."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_rows_oracle as ao
import ops_oracle as oo

# (head width, operands as the pair kernels multiply them)
FORMS = [(128, False), (128, True), (256, False)]
FORM_IDS = ["d128", "d128_x3", "d256"]


def _operands(name, D, x3):
    t = ao.inputs(name, D)
    return ao.x3_operands(t) if x3 else t


# ------------------------------------------------------------------ (a) the reference
@pytest.mark.parametrize("D", [128, 256])
def test_reference_is_torchs_float64_attention(D):
    for c in ao.CASES:
        t = ao.inputs(c.name, D)
        ref, p, rs = ao.attention_ref(t["q"], t["k"], t["v"], ao.scale_of(D))
        q, k, v = (t[n].double().permute(0, 2, 1, 3) for n in "qkv")
        want = F.scaled_dot_product_attention(q, k, v)     # its default scale is D ** -0.5
        assert ref.dtype == torch.float64 and tuple(ref.shape) == (c.B, ao.HEADS, c.Tq, D) and tuple(p.shape) == (c.B, ao.HEADS, c.Tq, c.Tk)
        assert float((ref - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), c.name
        assert float((p.sum(dim=-1) - 1).abs().max()) < 1e-13
        assert bool((rs >= ref.abs().max(dim=-1).values * (1 - 1e-12)).all()) and float(rs.min()) > 0
        # the kernels' order of evaluation is the same function
        fl = ao.flash(t["q"], t["k"], t["v"], ao.scale_of(D))
        assert float(ao.row_ratio(fl, ref, rs).max()) < 1e-13, c.name


def test_rowscale_is_the_rows_own_size():
    """spread_v: the rows' scales span decades, so a whole-tensor bar cannot see a small row; constant_v: rowscale is the constant's size."""
    t = ao.inputs("spread_v")
    _, _, rs = ao.attention_ref(t["q"], t["k"], t["v"], ao.scale_of(128))
    assert float(rs.max() / rs.min()) > 1e4
    t = ao.inputs("constant_v")
    ref, _, rs = ao.attention_ref(t["q"], t["k"], t["v"], ao.scale_of(128))
    want = t["v"][:, :1].double().permute(0, 2, 1, 3).expand_as(ref)
    assert float((ref - want).abs().max()) < 1e-14 and float((rs - want.abs().max(dim=-1).values).abs().max()) < 1e-14


# ------------------------------------------------------------------ (b) E32n
@pytest.mark.parametrize("D,x3", FORMS, ids=FORM_IDS)
def test_no_case_is_ill_posed(D, x3, capsys):
    lines = []
    for c in ao.CASES:
        _, _, e = ao.reference(_operands(c.name, D, x3), D)
        lines.append(f"{c.name} {e:.2e}")
        assert ao.E32N_FLOOR <= e <= ao.E32N_ILL_POSED, (c.name, e)
    with capsys.disabled():
        print(f"\n[attention_rows] E32n, D {D}{' x3 operands' if x3 else ''}: " + ", ".join(lines))


# ------------------------------------------------------------------ (c) the mutants
@pytest.mark.parametrize("D,x3", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("mutant", list(ao.MUTANTS))
def test_mutant_is_outside_the_bar_on_the_case_it_names(mutant, D, x3, capsys):
    fn, name = ao.MUTANTS[mutant]
    t = _operands(name, D, x3)
    ref, rs, e = ao.reference(t, D)
    worst = float(ao.row_ratio(fn(t, D), ref, rs).max())
    with capsys.disabled():
        print(f"\n[attention_rows] {mutant} on {name}, D {D}{' x3' if x3 else ''}: r / (8 E32n) = {worst / (ao.BAR_FACTOR * e):.3g}")
    assert worst > ao.BAR_FACTOR * e, (mutant, name, worst, e)


def test_mutants_name_cases_and_apply_widely():
    """Every mutant names an existing case; over all cases (D = 128) each is caught by many, not by one lucky draw."""
    caught = {m: 0 for m in ao.MUTANTS}
    for c in ao.CASES:
        t = ao.inputs(c.name)
        ref, rs, e = ao.reference(t, 128)
        for m, (fn, name) in ao.MUTANTS.items():
            assert name in ao.BY_NAME
            if m in ao.MUTANT_SKIPS and ao.MUTANT_SKIPS[m](c):
                continue
            caught[m] += float(ao.row_ratio(fn(t, 128), ref, rs).max()) > ao.BAR_FACTOR * e
    assert all(n >= 5 for n in caught.values()), caught


# ------------------------------------------------------------------ (d) the x3 body's carrier of P
@pytest.mark.parametrize("name", [c.name for c in ao.FLAT_CASES] + ["spread_v"])
def test_p_split_against_e32n(name, capsys):
    """P as ph = fp16(pe), pl = fp16(pe - ph) has an ABSOLUTE quantum of 2^-25 (the fp16 subnormal spacing, halved by rounding); with
    pe scaled by 2^14 first it is 2^-39.  Emulated in the kernels' order of evaluation, everything else in float64, on the pair operands.
    The flat-tail rows stay inside the bar either way (torch fp32 loses the tail's mass in its own sum); spread_v, where a key with P below
    2^-25 carries a value 10^5 times the row's size, is 20 times outside it without the scale and far inside with it."""
    t = ao.x3_operands(ao.inputs(name))
    ref, rs, e = ao.reference(t, 128)
    r0 = float(ao.row_ratio(ao.flash(t["q"], t["k"], t["v"], ao.scale_of(128), p_hook=ao.p_split), ref, rs).max())
    r14 = float(ao.row_ratio(ao.flash(t["q"], t["k"], t["v"], ao.scale_of(128), p_hook=lambda p: ao.p_split(p, 14)), ref, rs).max())
    with capsys.disabled():
        print(f"\n[attention_rows] {name}: E32n {e:.2e}; (ph, pl) split r / E32n = {r0 / e:.3g}, with P scaled by 2^14 = {r14 / e:.3g}")
    assert r14 <= ao.BAR_FACTOR * e
    if name == "spread_v":
        assert r0 > ao.BAR_FACTOR * e
    else:
        assert r0 <= ao.BAR_FACTOR * e


def test_p_split_quantum():
    p = torch.tensor([1.0, 0.3, 2.0 ** -14, 1e-5, 2.0 ** -25 * 0.98, 1e-9, 0.0]).double()      # fp32 values, as pe is
    assert bool(((ao.p_split(p) - p).abs() <= torch.clamp(2.0 ** -22 * p, min=2.0 ** -25)).all()) and float(ao.p_split(p)[4]) == 0.0
    assert bool(((ao.p_split(p, 14) - p).abs() <= torch.clamp(2.0 ** -22 * p, min=2.0 ** -39)).all()) and float(ao.p_split(p, 14)[0]) == 1.0
    assert float((ao.p_split(p, 14) - p).abs()[3:].max()) < 2.0 ** -39 < float((ao.p_split(p) - p).abs()[3:].max())
    assert float(ao.p_hi_only(p)[1]) != 0.3 and abs(float(ao.p_hi_only(p)[1]) - 0.3) < 2.0 ** -12


# ------------------------------------------------------------------ (e) builders
def test_cases_cover_the_edges_and_are_seeded():
    rand = [c for c in ao.CASES if c.kind == "random"]
    assert {c.Tk for c in rand} == {1, 31, 32, 33, 96, 97, 128, 129, 160, 161}
    for tq in (1, 21, 32, 33):
        assert {c.koff == 0 for c in rand if c.Tq == tq} == {True, False}
    assert all(c.B <= 2 and (c.Tk <= 161 or c.name.endswith("tk1008")) for c in ao.CASES)
    for c in ao.CASES:
        for D in (128, 256):
            t, again = ao.inputs(c.name, D), ao.inputs.__wrapped__(c.name, D)
            assert all(oo.bits_equal(t[n], again[n]) for n in t)
            assert tuple(t["q"].shape) == (c.B, c.Tq, 8, D) and tuple(t["k"].shape) == tuple(t["v"].shape) == (c.B, c.Tk, 8, D)
            assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) < 65504 for v in t.values())


def test_placed_logits_sit_where_the_cases_say():
    D = 128
    for name in ("max_walk", "gap100", "flat17_tk161", "offset_m60", "ascending"):
        c = ao.BY_NAME[name]
        t = ao.inputs(name, D)
        s = (t["q"].double().permute(0, 2, 1, 3) @ t["k"].double().permute(0, 2, 3, 1)) * ao.scale_of(D)
        top = s.argmax(dim=-1)
        if name in ("max_walk", "flat17_tk161"):
            assert all(bool((top[:, :, i] == ao.dominant_key(c, i)).all()) for i in range(c.Tq))
        if name == "max_walk":   # chunks 0..4, both halves of a chunk, all four quarters
            keys = [ao.dominant_key(c, i) for i in range(c.Tq)]
            assert {k // 32 for k in keys} == {0, 1, 2, 3, 4} and {(k >> 2) & 1 for k in keys} == {0, 1} and {(k >> 3) & 3 for k in keys} == {0, 1, 2, 3}
        if name == "gap100":
            assert all(bool((top[:, :, i] // 32 == ao.GAP_CHUNKS[i % 6]).all()) for i in range(c.Tq))
            gap = s.max(dim=-1).values - s.sort(dim=-1).values[..., c.Tk - 33]     # (a raised chunk has at most 32 keys)
            assert float(gap.min()) > 97 and math.exp(-97) < 2.0 ** -126              # alpha and the merge weights are below fp32's normal range
        if name == "flat17_tk161":
            assert float((s.sort(dim=-1).values[..., -2] + 17.4).abs().max()) < 1e-5
        if name == "offset_m60":
            assert -75 < float(s.min()) and float(s.max()) < -45
        if name == "ascending":
            m = torch.stack([s[..., 32 * kc:32 * kc + 32].max(dim=-1).values for kc in range(6)])
            assert bool((m[1:] > m[:-1] + 1).all())


def test_pack_qkv_places_rows_and_poison():
    c = ao.BY_NAME["rand_tk33_tq21_k7"]
    t = ao.inputs(c.name)
    T = ao.rows_T(c)
    assert T == 42
    m, n = ao.pack_qkv(t, c, "random"), ao.pack_qkv(t, c, "nan")
    for x in (m, n):
        assert tuple(x.shape) == (c.B, T, 3, 8, 128)
        assert oo.bits_equal(x[:, :21, 0], t["q"]) and oo.bits_equal(x[:, 7:40, 1], t["k"]) and oo.bits_equal(x[:, 7:40, 2], t["v"])
    assert oo.bits_equal(m[:, 40, 1], t["kx"][:, 0]) and oo.bits_equal(m[:, 40, 2], t["vx"][:, 0]) and bool(torch.isfinite(m).all())
    assert bool(torch.isnan(n[:, 21:, 0]).all()) and bool(torch.isnan(n[:, :7, 1:]).all()) and bool(torch.isnan(n[:, 40:, 1:]).all())
    ops = ao.x3_operands(t)
    assert all(float((ops[k] - t[k]).abs().max()) <= 2.0 ** -21 * float(t[k].abs().max()) for k in t)
